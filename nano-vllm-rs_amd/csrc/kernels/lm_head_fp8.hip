// lm_head_fp8.hip — the LM head of decode-sized steps over an FP8 (OCP e4m3fn) weight stream: logits[T,N] f32 = x[T,K] · (scales[n] · e4m3(Wq[n,k]))^T
// for T <= 64, with the greedy arg-max partials of lm_head.hip in the epilogue.
// reference: ParallelLMHead::compute_logits src/layers/embed_head.rs:292-306, Sampler::sample greedy branch src/layers/sampler.rs:126-151; the byte stream
// itself is an extension (the reference has 16-bit weights only).
//
// Operand.  Exactly what weight_quantize_fp8 (linear_fp8.hip) writes: Wq [N/16][K/64][64 lanes][16 B] and one power-of-two f32 scale per vocabulary row.
// One 1-KiB wave request (global_load_dwordx4, nontemporal) is one 16-row x 64-column block: after v_cvt_scalef32_pk_f16_fp8 / _bf16_fp8 at scale 1.0
// (exact) the A fragments of two v_mfma_f32_16x16x32.  Activations are not quantised.
//
// Work split (the LM head's, not the projection GEMMs').  Persistent workgroups of 8 waves, one per CU; every WAVE owns whole 16-row vocabulary tiles
// (tile j -> wave j % all_waves, ascending) and runs the K loop alone: H8_U requests of 1 KiB in flight per wave, no cross-wave reduction and no barrier
// inside the weight stream; every weight byte is read once per launch.  The B operand comes from an XOR-swizzled 16-bit activation image in LDS, rows
// padded to 16·MT (MT = 1..4) by repeating row T-1 (never stored, never part of a partial):
//   * resident form (T <= 32, K <= 2048): the whole image (<= 128 KiB) is written once and a wave walks any number of tiles;
//   * chunked form (more rows, or K > 2048): the image passes through LDS in chunks of KC = 1024 / 512 / 512 columns (MT = 2 / 3 / 4; <= 16 rows run the
//     MT = 2 instance on a 32-row image: its own instance kept all eight tiles' addresses live and spilled, and the stream is HBM-bound either way), double
//     buffered and filled by LDS-DMA (chunk c+1 is requested right behind the barrier that opens chunk c); every wave keeps the f32 accumulators of ALL
//     its tiles (at most H8_TPW) across the chunks, as lm_head_kchunk_kernel does.
// Epilogue: the row scale multiplies the finished f32 sums first (a power of two: exact; a lane's 4 C values are 4 consecutive vocabulary rows of one
// token: one 16-byte scale load per tile), then the f32 logit stores (on demand) and (max, lowest index) per lane -> wave -> workgroup.  The stores are
// the only thing the logits pointer gates, so the partials of a launch without logits are those of a launch with them, bit for bit.
// Roofline: HBM, algorithmic bytes N·K + 4·N (+ 4·T·N logits on demand).
#include <algorithm>
#include "kernels.h"
#include "device_utils.h"
#include "../common.h"

namespace nvr { namespace NVR_DT_NS {

typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));

constexpr int H8_WAVES = 8, H8_WGS = 256, H8_U = 8, H8_TPW = 8;            // waves per workgroup, workgroups, requests in flight, tiles per wave (chunked form)
constexpr int H8_RES_ROWS = 32, H8_RES_K = 2048;                            // the resident form's largest image

struct LmFp8 {
    const half_t *x; int64_t ldx;
    const uint8_t *Wq; const float *scales;
    int32_t T, K, N;
    float *y;                          // f32 logits [T, N], or null: partials only
    float *pval; int32_t *pidx;        // [gridDim.x][T]
};

// blocks 0 .. nkb-1 (64 columns, 1 KiB each, from the wave-uniform wq on: a scalar base and the lane's 32-bit offset, no 64-bit address registers per
// request) of one tile against the image columns that start at img (rowb bytes per row): H8_U requests in flight, the ragged rest of a K that is no
// multiple of 64·H8_U one by one
template <int MT>
__device__ __forceinline__ void h8_blocks(const uint8_t *__restrict__ wq, unsigned lane16, int nkb, const char *img, int rowb, int r, int q, float4_t (&acc)[MT]) {
    auto use = [&](const uint4_t w, int kb) {
        const half8_t a0 = fp8x8_to_half8(w[0], w[1]), a1 = fp8x8_to_half8(w[2], w[3]);
        const int ch = kb * 8 + q;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const char *row = img + (j * 16 + r) * rowb;
            const half8_t b0 = *reinterpret_cast<const half8_t *>(row + (ch ^ (r & 7)) * 16);
            const half8_t b1 = *reinterpret_cast<const half8_t *>(row + ((ch + 4) ^ (r & 7)) * 16);
            acc[j] = mfma16(a0, b0, acc[j]);
            acc[j] = mfma16(a1, b1, acc[j]);
        }
    };
    int kb = 0;
    for (; kb + H8_U <= nkb; kb += H8_U) {
        uint4_t w[H8_U];
#pragma unroll
        for (int u = 0; u < H8_U; ++u) w[u] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(wq + (int64_t)kb * 1024 + (lane16 + u * 1024u)));
#pragma unroll
        for (int u = 0; u < H8_U; ++u) use(w[u], kb + u);
    }
    for (; kb < nkb; ++kb) use(__builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(wq + (int64_t)kb * 1024 + lane16)), kb);
}

// a finished tile: scale, logit stores on demand, the lane's running (max, lowest index).  C layout: rows n = q*4 + e, column = token r
template <int MT>
__device__ __forceinline__ void h8_finish_tile(const LmFp8 &p, int tile, int r, int q, const float4_t (&acc)[MT], float (&best)[MT], int (&besti)[MT]) {
    const int n0 = tile * 16 + q * 4;
    const float4_t sc = *reinterpret_cast<const float4_t *>(p.scales + n0);
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const float4_t v = acc[j] * sc;
        const int m = j * 16 + r;
        if (m < p.T && p.y) *reinterpret_cast<float4_t *>(p.y + (int64_t)m * p.N + n0) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] > best[j]) { best[j] = v[e]; besti[j] = n0 + e; }            // tiles ascend: the first maximum is kept
    }
}

__device__ __forceinline__ void h8_better(float &bv, int &bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// lanes r, r+16, r+32, r+48 hold the same token; then the waves through LDS (the image is dead: behind a barrier); rows >= T are dropped here
template <int MT>
__device__ __forceinline__ void h8_merge(const LmFp8 &p, char *smem, int tid, float (&best)[MT], int (&besti)[MT]) {
    constexpr int ROWS = MT * 16;
    const int wave = tid >> 6, r = tid & 15, q = (tid & 63) >> 4;
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const float v = __shfl_xor(best[j], o, 64);
            const int i = __shfl_xor(besti[j], o, 64);
            h8_better(best[j], besti[j], v, i);
        }
    __syncthreads();
    float *sv = reinterpret_cast<float *>(smem);
    int *si = reinterpret_cast<int *>(smem + H8_WAVES * ROWS * 4);
    if (q == 0) {
#pragma unroll
        for (int j = 0; j < MT; ++j) { sv[wave * ROWS + j * 16 + r] = best[j]; si[wave * ROWS + j * 16 + r] = besti[j]; }
    }
    __syncthreads();
    if (tid < p.T) {
        float bv = sv[tid]; int bi = si[tid];
        for (int w2 = 1; w2 < H8_WAVES; ++w2) h8_better(bv, bi, sv[w2 * ROWS + tid], si[w2 * ROWS + tid]);
        p.pval[(int64_t)blockIdx.x * p.T + tid] = bv;
        p.pidx[(int64_t)blockIdx.x * p.T + tid] = bi;
    }
}

// ---- resident form ---------------------------------------------------------------------------------------------------------------
template <int MT>
__global__ __launch_bounds__(H8_WAVES * 64) void lm_head_fp8_kernel(LmFp8 p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int cpr = p.K / 8, kbt = p.K / 64;                                // 16-byte chunks per image row, 64-column blocks per tile
    fill_x_image<MT * 16, H8_WAVES * 64, 8>(smem, p.x, p.ldx, 0, cpr, p.T, tid);
    __syncthreads();
    const int ntiles = p.N / 16, nw = gridDim.x * H8_WAVES;
    float best[MT]; int besti[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) { best[j] = -INFINITY; besti[j] = 0x7fffffff; }
    for (int tile = blockIdx.x * H8_WAVES + wave; tile < ntiles; tile += nw) {
        float4_t acc[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[j] = (float4_t){0.f, 0.f, 0.f, 0.f};
        h8_blocks<MT>(p.Wq + (int64_t)tile * kbt * 1024, lane * 16u, kbt, smem, cpr * 16, r, q, acc);
        h8_finish_tile<MT>(p, tile, r, q, acc, best, besti);
    }
    h8_merge<MT>(p, smem, tid, best, besti);
}

// ---- chunked form ----------------------------------------------------------------------------------------------------------------
template <int MT>
struct H8Chunk {
    static constexpr int ROWS = MT * 16;
    static constexpr int KC = MT <= 2 ? 1024 : 512;                          // image chunk: 64 / 48 / 64 KiB, twice (MT = 2 / 3 / 4)
    static constexpr int CPR = KC / 8;
    static constexpr int IMG = ROWS * KC * 2;
    static constexpr int FILL = ROWS * CPR / (H8_WAVES * 64);               // LDS-DMA requests per wave and image
    static constexpr int LDS = 2 * IMG;
    static_assert(ROWS * CPR % (H8_WAVES * 64) == 0 && (CPR & (CPR - 1)) == 0, "whole wave requests, power-of-two rows");
};

template <int MT>
__global__ __launch_bounds__(H8_WAVES * 64) void lm_head_fp8_kchunk_kernel(LmFp8 p) {
    using SH = H8Chunk<MT>;
    constexpr int KC = SH::KC, CPR = SH::CPR, IMG = SH::IMG;
    extern __shared__ __attribute__((aligned(16))) char smem[];             // two images
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int nc = (p.K + KC - 1) / KC, kbt = p.K / 64;
    const int ntiles = p.N / 16, nw = gridDim.x * H8_WAVES, w0 = blockIdx.x * H8_WAVES + wave;

    // image chunk c -> buffer buf: slot (row, s) holds 16-byte chunk s ^ (row & 7) of the row; rows >= T repeat row T-1, chunks behind a ragged last
    // chunk's columns repeat chunk 0 (their 64-column blocks are never read)
    auto issue_img = [&](int c, int buf) {
        const int cols = min(KC, p.K - c * KC);
#pragma unroll
        for (int it = 0; it < SH::FILL; ++it) {
            const int slot0 = (it * H8_WAVES + wave) * 64, pidx = slot0 + lane, row = pidx / CPR;
            int ch = (pidx & (CPR - 1)) ^ (row & 7);
            if (ch * 8 >= cols) ch = 0;
            const half_t *src = p.x + (int64_t)(row < p.T ? row : p.T - 1) * p.ldx + c * KC + ch * 8;
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void *)(smem + buf * IMG + slot0 * 16), 16, 0, 0);
        }
    };

    float4_t acc[H8_TPW][MT];
#pragma unroll
    for (int i = 0; i < H8_TPW; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};
    issue_img(0, 0);
    for (int c = 0; c < nc; ++c) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // this wave's pieces of image c have landed ...
        __syncthreads();                                                    // ... everybody's have, and nobody reads buffer (c + 1) & 1 any more
        if (c + 1 < nc) issue_img(c + 1, (c + 1) & 1);
        const int nkb = min(KC, p.K - c * KC) / 64;
        const char *img = smem + (c & 1) * IMG;
#pragma unroll
        for (int i = 0; i < H8_TPW; ++i) {
            const int tile = w0 + i * nw;
            if (tile >= ntiles) break;                                      // wave-uniform
            h8_blocks<MT>(p.Wq + ((int64_t)tile * kbt + c * (KC / 64)) * 1024, lane * 16u, nkb, img, CPR * 16, r, q, acc[i]);
            // the unrolled tile loop lets the scheduler hoist the NEXT tile's requests above this tile's MFMAs (wanted: more bytes in flight), but at MT = 1
            // it hoisted all eight tiles' (256 registers and scratch): at most two tiles' requests are in flight together
            if (i & 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
    float best[MT]; int besti[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) { best[j] = -INFINITY; besti[j] = 0x7fffffff; }
#pragma unroll
    for (int i = 0; i < H8_TPW; ++i) {
        const int tile = w0 + i * nw;
        if (tile >= ntiles) break;
        h8_finish_tile<MT>(p, tile, r, q, acc[i], best, besti);
    }
    h8_merge<MT>(p, smem, tid, best, besti);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool h8_resident(int64_t T, int64_t K) { return T <= H8_RES_ROWS && K <= H8_RES_K; }
static int64_t h8_wgs(int64_t N) { return std::min<int64_t>(H8_WGS, (N / 16 + H8_WAVES - 1) / H8_WAVES); }

bool lm_head_fp8_ok(int64_t T, int64_t K, int64_t N, int64_t ldx) {
    if (!(T >= 1 && T <= 64 && K >= 64 && K % 64 == 0 && K <= (1ll << 24) && N >= 16 && N % 16 == 0 && N < (1ll << 31) && ldx >= K && ldx % 8 == 0)) return false;
    return h8_resident(T, K) || N / 16 <= h8_wgs(N) * H8_WAVES * H8_TPW;   // chunked form: every wave's tiles fit its accumulator registers
}
int32_t lm_head_fp8_parts(int64_t T, int64_t K, int64_t N, int64_t ldx) { return lm_head_fp8_ok(T, K, N, ldx) ? (int32_t)h8_wgs(N) : 0; }

static int h8_opt_in(const void *f, int lds) {
    hipError_t er = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (er != hipSuccess) return nvr::fail(NVR_ERR_HIP, "lm_head_fp8: hipFuncSetAttribute: %s", hipGetErrorString(er));
    return 0;
}
// opt every instance in to its dynamic LDS (runner init: never inside a stream capture)
int lm_head_fp8_prepare() {
    static bool done = false;
    if (done) return 0;
    if (int rc = h8_opt_in(reinterpret_cast<const void *>(&lm_head_fp8_kernel<1>), 16 * H8_RES_K * 2)) return rc;
    if (int rc = h8_opt_in(reinterpret_cast<const void *>(&lm_head_fp8_kernel<2>), 32 * H8_RES_K * 2)) return rc;
    if (int rc = h8_opt_in(reinterpret_cast<const void *>(&lm_head_fp8_kchunk_kernel<2>), H8Chunk<2>::LDS)) return rc;
    if (int rc = h8_opt_in(reinterpret_cast<const void *>(&lm_head_fp8_kchunk_kernel<3>), H8Chunk<3>::LDS)) return rc;
    if (int rc = h8_opt_in(reinterpret_cast<const void *>(&lm_head_fp8_kchunk_kernel<4>), H8Chunk<4>::LDS)) return rc;
    done = true;
    return 0;
}

// logits (nullable: partials only) and per-workgroup arg-max partials part_val / part_idx [*nparts][T], *nparts = lm_head_fp8_parts(...)
int lm_head_fp8(const half_bits *x, int64_t ldx, const uint8_t *Wq, const float *scales, int64_t T, int64_t K, int64_t N, float *logits, float *part_val,
                int32_t *part_idx, int32_t *nparts, hipStream_t s) {
    if (!x || !Wq || !scales || !part_val || !part_idx || !nparts) return nvr::fail(NVR_ERR_INVALID_ARG, "lm_head_fp8: null pointer");
    if (!lm_head_fp8_ok(T, K, N, ldx))
        return nvr::fail(NVR_ERR_UNSUPPORTED, "lm_head_fp8: T=%ld (1..64) K=%ld (a multiple of 64) N=%ld (a multiple of 16; beyond 32 rows or 2048 columns at most %d) "
                         "ldx=%ld (>= K, a multiple of 8)", (long)T, (long)K, (long)N, 16 * H8_WGS * H8_WAVES * H8_TPW, (long)ldx);
    if (int rc = lm_head_fp8_prepare()) return rc;
    LmFp8 p{(const half_t *)x, ldx, Wq, scales, (int32_t)T, (int32_t)K, (int32_t)N, logits, part_val, part_idx};
    const dim3 grid((unsigned)h8_wgs(N)), block(H8_WAVES * 64);
    *nparts = (int32_t)grid.x;
    const bool resident = h8_resident(T, K);
    const int mt = std::max((int)((T + 15) / 16), resident ? 1 : 2);
    if (resident) {
        const size_t lds = (size_t)mt * 16 * K * 2;
        if (mt == 1) lm_head_fp8_kernel<1><<<grid, block, lds, s>>>(p);
        else lm_head_fp8_kernel<2><<<grid, block, lds, s>>>(p);
    } else if (mt == 2) lm_head_fp8_kchunk_kernel<2><<<grid, block, H8Chunk<2>::LDS, s>>>(p);
    else if (mt == 3) lm_head_fp8_kchunk_kernel<3><<<grid, block, H8Chunk<3>::LDS, s>>>(p);
    else lm_head_fp8_kchunk_kernel<4><<<grid, block, H8Chunk<4>::LDS, s>>>(p);
    hipError_t er = hipGetLastError();
    if (er != hipSuccess) return nvr::fail(NVR_ERR_HIP, "lm_head_fp8 launch failed: %s", hipGetErrorString(er));
    return 0;
}

}}  // namespace nvr::k / nvr::kb (NVR_DT_NS)

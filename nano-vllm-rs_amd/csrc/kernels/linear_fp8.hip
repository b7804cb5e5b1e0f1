// linear_fp8.hip — the FP8 (OCP e4m3fn) weight stream of decode-sized GEMMs: y[T,N] = x[T,K] · (scales[n] · e4m3(Wq[n,k]))^T for T <= 64 with the plain
// 16-bit, the gate_up -> SiluAndMul and the split-k (f32 slabs for add_rmsnorm_slabs) epilogues, and the quantiser that makes Wq (weight_quantize_fp8).
// reference call sites: those of linear_stream.hip (QKVParallelLinear / RowParallelLinear / MergedColumnParallelLinear::forward, src/layers/linear.rs);
// the byte stream itself is an extension (the reference has 16-bit weights only).
//
// Quantiser.  Row n of W[N,K] gets the scale 2^e, e the smallest integer with amax(row) <= 448 · 2^e, clamped to e >= -15; an all-zero row gets e = 0.
// byte = e4m3fn(w / 2^e), round to nearest even, clamped to +-448 in front of the conversion (as kv_store_fp8).  The division by a power of two is exact
// and every byte · 2^e is an fp16 value (e >= -15: the smallest subnormal code, 2^-9, lands on 2^-24) and a bf16 value, so the optional Wd output (the
// dequantised weights, row-major, may alias W) is exact.  PRECONDITION: finite weights, |w| <= 2^15.
//
// Layout of Wq: [N/16][K/64][64 lanes][16 B].  The 16 bytes of lane l = 16 q + r of block (tile, kb) are row tile·16 + r, columns kb·64 + 8 q + 0..7
// (bytes 0..7) and kb·64 + 32 + 8 q + 0..7 (bytes 8..15): the lane's A fragments of the two 16x16x32 MFMAs of that 64-column block, so one 1-KiB
// wave request (global_load_dwordx4, nontemporal) feeds two MFMAs per column tile.  gate_up: W is [2I, K], tiles 0 .. I/16-1 gate, I/16 .. up.
//
// GEMM.  Persistent workgroups (256 of 8 waves; split-k: 256/S per k-slice) own the 16-row weight tiles w, w + 256, ...; TT of them (accumulators in
// registers) per pass over K.  The activation block is a 16-bit image in LDS in K chunks of KC = 1024 (<= 32 rows) or 512 columns, rows padded to the
// 16·MT of the MFMA column tiles by repeating row T-1 (never stored), XOR-swizzled 16-byte chunks as in linear_stream.hip, double buffered and filled
// by LDS-DMA: chunk c+1 is requested right behind the barrier that opens chunk c.  Inside a chunk wave j takes the 64-column blocks j, j + 8: it
// requests ALL its weight pieces of the chunk (TT x parts x KC/512 requests of 1 KiB) before the first conversion, converts them to packed 16-bit
// pairs (v_cvt_scalef32_pk_f16_fp8 / _bf16_fp8, scale operand 1.0: exact) and feeds them to the 16-bit MFMAs as the A operand; activations are not
// quantised.  The waves' partial sums meet in LDS once per tile (fixed order); the row scale multiplies the finished f32 sums once, in the epilogue
// (a power of two: exact), then the rounding points of the 16-bit kernels (linear.hip).  Roofline: HBM, algorithmic bytes N·K.
#include <algorithm>
#include "kernels.h"
#include "device_utils.h"
#include "../common.h"

namespace nvr { namespace NVR_DT_NS {

typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));

// ---- weight_quantize_fp8 ---------------------------------------------------------------------------------------------------------
// One workgroup per weight row: pass 1 the row's amax, pass 2 (behind a barrier: Wd may be W) bytes, scale and dequantised values.
__global__ __launch_bounds__(256) void weight_quantize_fp8_kernel(const half_t *W, int K, uint8_t *__restrict__ Wq, float *__restrict__ scales, half_t *Wd) {
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const half_t *src = W + (int64_t)n * K;
    float am = 0.f;
    for (int c = tid; c < K / 8; c += 256) {
        const half8_t v = *reinterpret_cast<const half8_t *>(src + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf((float)v[e]));
    }
    am = wave_max(am);
    if ((tid & 63) == 0) red[tid >> 6] = am;
    __syncthreads();
    am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // amax = f · 2^p, f in [1, 2): amax <= 448 · 2^e = 1.75 · 2^(8 + e)  <=>  e >= p - 8 (f <= 1.75) or p - 7
    const unsigned bits = __float_as_uint(am);
    int ex = 0;
    if (bits != 0) {
        ex = (int)(bits >> 23) - 127 - ((bits & 0x7FFFFFu) <= 0x600000u ? 8 : 7);
        if (ex < -15) ex = -15;
    }
    const float sc = __uint_as_float((unsigned)(ex + 127) << 23), inv = __uint_as_float((unsigned)(127 - ex) << 23);
    if (tid == 0) scales[n] = sc;
    for (int c = tid; c < K / 8; c += 256) {
        const half8_t v = *reinterpret_cast<const half8_t *>(src + c * 8);
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = fminf(fmaxf((float)v[e] * inv, -448.f), 448.f);
        int r0 = 0, r1 = 0;
        r0 = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], r0, false); r0 = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], r0, true);
        r1 = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], r1, false); r1 = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], r1, true);
        const int kb = c >> 3, hf = (c >> 2) & 1, q = c & 3;               // 64-column block, its k-step, the lane quarter
        uint8_t *dst = Wq + (((int64_t)(n >> 4) * (K / 64) + kb) * 64 + (q * 16 + (n & 15))) * 16 + hf * 8;
        *reinterpret_cast<uint2_t *>(dst) = (uint2_t){(unsigned)r0, (unsigned)r1};
        if (Wd) {
            const float2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(r0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(r0, true);
            const float2_t d = __builtin_amdgcn_cvt_pk_f32_fp8(r1, false), g = __builtin_amdgcn_cvt_pk_f32_fp8(r1, true);
            const half8_t o = {(half_t)(a[0] * sc), (half_t)(a[1] * sc), (half_t)(b[0] * sc), (half_t)(b[1] * sc),
                               (half_t)(d[0] * sc), (half_t)(d[1] * sc), (half_t)(g[0] * sc), (half_t)(g[1] * sc)};
            *reinterpret_cast<half8_t *>(Wd + (int64_t)n * K + c * 8) = o;
        }
    }
}

int weight_quantize_fp8(const half_bits *W, int64_t N, int64_t K, uint8_t *Wq, float *scales, half_bits *Wd, hipStream_t s) {
    if (N < 16 || N % 16 || K < 64 || K % 64 || N > (1ll << 30) || K > (1ll << 24))
        return nvr::fail(NVR_ERR_UNSUPPORTED, "weight_quantize_fp8: N=%ld (a multiple of 16), K=%ld (a multiple of 64)", (long)N, (long)K);
    weight_quantize_fp8_kernel<<<dim3((unsigned)N), dim3(256), 0, s>>>((const half_t *)W, (int)K, Wq, scales, (half_t *)Wd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "weight_quantize_fp8 launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- the GEMM ----------------------------------------------------------------------------------------------------------------------
enum { FEPI_F16 = 0, FEPI_SILU = 1, FEPI_SLAB = 2 };
constexpr int F8_WAVES = 8, F8_WGS = 256;

struct Fp8Gemm {
    const half_t *x; int64_t ldx;
    const uint8_t *Wq; const float *scales;
    int32_t T, K, N;                   // N: columns of the output (SiLU: I)
    int32_t ntiles;                    // 16-row tiles per weight part (N / 16)
    int32_t S, kslice;                 // FEPI_SLAB: k-slices and their columns (a multiple of 64); else 1, K
    void *out;                         // 16-bit [T, N], or f32 slabs [S][T, N]
};

template <int MT, int EPI>
struct Fp8Shape {
    static constexpr int NTT = EPI == FEPI_SILU ? 2 : 1;                    // weight parts per tile (gate, up)
    static constexpr int ROWS = MT * 16;
    static constexpr int KC = MT <= 2 ? 1024 : 512;                         // image chunk: 32 / 64 (48: 48) KiB, twice
    static constexpr int CPR = KC / 8;                                      // 16-byte chunks per image row
    static constexpr int KPW = KC / 64 / F8_WAVES;                          // 64-column blocks per wave and chunk
    // tiles per pass: <= 96 accumulator registers and <= 16 weight requests (64 registers) per wave and chunk
    static constexpr int TT = std::max(1, std::min(4, std::min(24 / (NTT * MT), 16 / (NTT * KPW))));
    static constexpr int IMG = ROWS * KC * 2;
    static constexpr int FILL = ROWS * CPR / (F8_WAVES * 64);               // LDS-DMA requests per wave and image
    static constexpr size_t LDS = std::max<size_t>(2 * IMG, (size_t)F8_WAVES * NTT * MT * 64 * 16);
    static_assert(ROWS * CPR % (F8_WAVES * 64) == 0 && (CPR & (CPR - 1)) == 0, "whole wave requests, power-of-two rows");
};

template <int MT, int EPI>
__global__ __launch_bounds__(F8_WAVES * 64) void linear_fp8_kernel(Fp8Gemm p) {
    using SH = Fp8Shape<MT, EPI>;
    constexpr int NTT = SH::NTT, KC = SH::KC, CPR = SH::CPR, KPW = SH::KPW, TT = SH::TT, IMG = SH::IMG;
    extern __shared__ __attribute__((aligned(16))) char smem[];             // two images; per tile the reduction scratch
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, q = lane >> 4;
    // split-k: workgroup b works on k-slice b % S with the gridDim / S workgroups of that slice
    const int z = EPI == FEPI_SLAB ? (int)blockIdx.x % p.S : 0;
    const int gw = EPI == FEPI_SLAB ? (int)gridDim.x / p.S : (int)gridDim.x;
    const int w0 = EPI == FEPI_SLAB ? (int)blockIdx.x / p.S : (int)blockIdx.x;
    const int k0 = z * p.kslice, kn = p.kslice;                             // this workgroup's columns [k0, k0 + kn)
    const int nc = (kn + KC - 1) / KC, kbt = p.K / 64;
    const int ntl = (p.ntiles - w0 + gw - 1) / gw;                          // tiles w0, w0 + gw, ... of this workgroup (>= 1: host)

    // image chunk c -> buffer buf: slot (row, s) holds 16-byte chunk s ^ (row & 7) of the row; rows >= T repeat row T-1, chunks behind a ragged last
    // chunk's columns repeat chunk 0 (their 64-column blocks are never read)
    auto issue_img = [&](int c, int buf) {
        const int cols = min(KC, kn - c * KC);
#pragma unroll
        for (int it = 0; it < SH::FILL; ++it) {
            const int slot0 = (it * F8_WAVES + wave) * 64, pidx = slot0 + lane, row = pidx / CPR;
            int ch = (pidx & (CPR - 1)) ^ (row & 7);
            if (ch * 8 >= cols) ch = 0;
            const half_t *src = p.x + (int64_t)(row < p.T ? row : p.T - 1) * p.ldx + k0 + c * KC + ch * 8;
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void *)(smem + buf * IMG + slot0 * 16), 16, 0, 0);
        }
    };

    float4_t *part = reinterpret_cast<float4_t *>(smem);                    // [WAVES][NTT * MT][64]
    auto reduce = [&](int slot) {
        float4_t s = part[slot * 64 + lane];
#pragma unroll
        for (int w2 = 1; w2 < F8_WAVES; ++w2) s += part[(w2 * NTT * MT + slot) * 64 + lane];
        return s;
    };

    for (int tb = 0; tb < ntl; tb += TT) {                                  // a pass: TT tiles over all of K
        float4_t acc[TT][NTT][MT];
#pragma unroll
        for (int i = 0; i < TT; ++i)
#pragma unroll
            for (int nt = 0; nt < NTT; ++nt)
#pragma unroll
                for (int j = 0; j < MT; ++j) acc[i][nt][j] = (float4_t){0.f, 0.f, 0.f, 0.f};
        __syncthreads();                                                    // the previous pass's scratch is no longer read
        issue_img(0, 0);
        for (int c = 0; c < nc; ++c) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // this wave's pieces of image c have landed ...
            __syncthreads();                                                // ... everybody's have, and nobody reads buffer (c + 1) & 1 any more
            if (c + 1 < nc) issue_img(c + 1, (c + 1) & 1);
            const int nkb = min(KC, kn - c * KC) / 64;                      // 64-column blocks of this chunk
            // every weight piece of the chunk is requested before the first is used (live tiles only: a uniform branch); a wave's blocks behind a ragged
            // chunk's end re-read block 0 (never used)
            uint4_t wv[TT][NTT][KPW];
#pragma unroll
            for (int i = 0; i < TT; ++i) {
                if (tb + i >= ntl) break;
                const int tile = w0 + (tb + i) * gw;
#pragma unroll
                for (int nt = 0; nt < NTT; ++nt)
#pragma unroll
                    for (int u = 0; u < KPW; ++u) {
                        const int kb = wave + u * F8_WAVES;
                        const uint8_t *src = p.Wq + (((int64_t)(nt * p.ntiles + tile) * kbt + (k0 + c * KC) / 64 + (kb < nkb ? kb : 0)) * 64 + lane) * 16;
                        wv[i][nt][u] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(src));
                    }
            }
            const char *img = smem + (c & 1) * IMG;
#pragma unroll
            for (int i = 0; i < TT; ++i) {
                if (tb + i >= ntl) break;
#pragma unroll
                for (int u = 0; u < KPW; ++u) {
                    const int kb = wave + u * F8_WAVES;
                    if (kb >= nkb) break;
                    half8_t a0[NTT], a1[NTT];
#pragma unroll
                    for (int nt = 0; nt < NTT; ++nt) {
                        a0[nt] = fp8x8_to_half8(wv[i][nt][u][0], wv[i][nt][u][1]);
                        a1[nt] = fp8x8_to_half8(wv[i][nt][u][2], wv[i][nt][u][3]);
                    }
                    const int ch = kb * 8 + q;
#pragma unroll
                    for (int j = 0; j < MT; ++j) {
                        const char *row = img + (j * 16 + r) * (CPR * 16);
                        const half8_t b0 = *reinterpret_cast<const half8_t *>(row + (ch ^ (r & 7)) * 16);
                        const half8_t b1 = *reinterpret_cast<const half8_t *>(row + ((ch + 4) ^ (r & 7)) * 16);
#pragma unroll
                        for (int nt = 0; nt < NTT; ++nt) {
                            acc[i][nt][j] = mfma16(a0[nt], b0, acc[i][nt][j]);
                            acc[i][nt][j] = mfma16(a1[nt], b1, acc[i][nt][j]);
                        }
                    }
                }
            }
        }
        // per tile: the waves' partial sums meet in LDS, then scale and epilogue.  C layout: row (n) = q*4 + e, column (token) = r
#pragma unroll
        for (int i = 0; i < TT; ++i) {
            if (tb + i >= ntl) break;
            const int tile = w0 + (tb + i) * gw;
            __syncthreads();                                                // last image / previous tile's scratch no longer read
#pragma unroll
            for (int nt = 0; nt < NTT; ++nt)
#pragma unroll
                for (int j = 0; j < MT; ++j) part[(wave * NTT * MT + nt * MT + j) * 64 + lane] = acc[i][nt][j];
            __syncthreads();
            for (int j = wave; j < MT; j += F8_WAVES) {
                const int m = j * 16 + r, n = tile * 16 + q * 4;
                if (EPI == FEPI_SILU) {
                    // act = 16bit(silu(16bit gate) * 16bit up), as linear_silu_mul
                    const float4_t g4 = reduce(j) * *reinterpret_cast<const float4_t *>(p.scales + n);
                    const float4_t u4 = reduce(MT + j) * *reinterpret_cast<const float4_t *>(p.scales + p.N + n);
                    if (m < p.T) {
                        half4_t h;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float gf = (float)to_half_rn(g4[e]), uf = (float)to_half_rn(u4[e]);
                            const float sg = sigmoid_fast(gf);
                            h[e] = to_half_rn(__fmul_rn(__fmul_rn(gf, sg), uf));
                        }
                        *reinterpret_cast<half4_t *>((half_t *)p.out + (int64_t)m * p.N + n) = h;
                    }
                } else {
                    const float4_t s = reduce(j) * *reinterpret_cast<const float4_t *>(p.scales + n);
                    if (m < p.T) {
                        if (EPI == FEPI_SLAB) *reinterpret_cast<float4_t *>((float *)p.out + ((int64_t)z * p.T + m) * p.N + n) = s;
                        else *reinterpret_cast<half4_t *>((half_t *)p.out + (int64_t)m * p.N + n) = (half4_t){to_half_rn(s[0]), to_half_rn(s[1]), to_half_rn(s[2]), to_half_rn(s[3])};
                    }
                }
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
template <int MT, int EPI>
static int fp8_opt_in() {
    hipError_t er = hipFuncSetAttribute(reinterpret_cast<const void *>(&linear_fp8_kernel<MT, EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)Fp8Shape<MT, EPI>::LDS);
    if (er != hipSuccess) return nvr::fail(NVR_ERR_HIP, "linear_fp8: hipFuncSetAttribute: %s", hipGetErrorString(er));
    return 0;
}
template <int EPI>
static int fp8_opt_in_rows() {
    if (int rc = fp8_opt_in<1, EPI>()) return rc;
    if (int rc = fp8_opt_in<2, EPI>()) return rc;
    if (int rc = fp8_opt_in<3, EPI>()) return rc;
    return fp8_opt_in<4, EPI>();
}
// opt every instance in to its dynamic LDS (runner init: never inside a stream capture)
int linear_fp8_prepare() {
    static bool done = false;
    if (done) return 0;
    if (int rc = fp8_opt_in_rows<FEPI_F16>()) return rc;
    if (int rc = fp8_opt_in_rows<FEPI_SILU>()) return rc;
    if (int rc = fp8_opt_in_rows<FEPI_SLAB>()) return rc;
    done = true;
    return 0;
}

bool linear_fp8_ok(int64_t T, int64_t K, int64_t N, int64_t ldx) {
    return T >= 1 && T <= 64 && K >= 64 && K % 64 == 0 && N >= 16 && N % 16 == 0 && ldx >= K && ldx % 8 == 0 && K <= (1ll << 24) && N <= (1ll << 24);
}

template <int EPI>
static int fp8_launch(const half_bits *x, int64_t ldx, const uint8_t *Wq, const float *scales, int64_t T, int64_t K, int64_t N, int64_t S, void *out,
                      hipStream_t s, const char *what) {
    if (!x || !Wq || !scales || !out) return nvr::fail(NVR_ERR_INVALID_ARG, "%s: null pointer", what);
    if (!linear_fp8_ok(T, K, N, ldx))
        return nvr::fail(NVR_ERR_UNSUPPORTED, "%s: T=%ld (1..64) K=%ld (a multiple of 64) N=%ld (a multiple of 16) ldx=%ld (>= K, a multiple of 8)", what, (long)T, (long)K, (long)N, (long)ldx);
    if (S < 1 || S > 64 || (K / 64) % S)
        return nvr::fail(NVR_ERR_UNSUPPORTED, "%s: S=%ld does not cut K=%ld into slices of whole 64-column tiles (1..64 slices)", what, (long)S, (long)K);
    if (int rc = linear_fp8_prepare()) return rc;
    Fp8Gemm p{(const half_t *)x, ldx, Wq, scales, (int32_t)T, (int32_t)K, (int32_t)N, (int32_t)(N / 16), (int32_t)S, (int32_t)(K / S), out};
    const int gw = (int)std::min<int64_t>(N / 16, F8_WGS / S);              // workgroups per k-slice: each owns at least one tile
    const dim3 grid((unsigned)(gw * S)), block(F8_WAVES * 64);
    const int mt = (int)((T + 15) / 16);
    if (mt == 1) linear_fp8_kernel<1, EPI><<<grid, block, Fp8Shape<1, EPI>::LDS, s>>>(p);
    else if (mt == 2) linear_fp8_kernel<2, EPI><<<grid, block, Fp8Shape<2, EPI>::LDS, s>>>(p);
    else if (mt == 3) linear_fp8_kernel<3, EPI><<<grid, block, Fp8Shape<3, EPI>::LDS, s>>>(p);
    else linear_fp8_kernel<4, EPI><<<grid, block, Fp8Shape<4, EPI>::LDS, s>>>(p);
    hipError_t er = hipGetLastError();
    if (er != hipSuccess) return nvr::fail(NVR_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(er));
    return 0;
}

int linear_fp8(const half_bits *x, int64_t ldx, const uint8_t *Wq, const float *scales, int64_t T, int64_t K, int64_t N, half_bits *y, hipStream_t s) {
    return fp8_launch<FEPI_F16>(x, ldx, Wq, scales, T, K, N, 1, y, s, "linear_fp8");
}
int linear_silu_mul_fp8(const half_bits *x, int64_t ldx, const uint8_t *Wq, const float *scales, int64_t T, int64_t K, int64_t I, half_bits *out,
                        hipStream_t s) {
    return fp8_launch<FEPI_SILU>(x, ldx, Wq, scales, T, K, I, 1, out, s, "linear_silu_mul_fp8");
}
int linear_splitk_fp8(const half_bits *x, int64_t ldx, const uint8_t *Wq, const float *scales, int64_t T, int64_t K, int64_t N, int64_t S, float *slabs,
                      hipStream_t s) {
    return fp8_launch<FEPI_SLAB>(x, ldx, Wq, scales, T, K, N, S, slabs, s, "linear_splitk_fp8");
}

}}  // namespace nvr::k / nvr::kb (NVR_DT_NS)

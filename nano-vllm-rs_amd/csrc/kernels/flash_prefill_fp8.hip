// flash_prefill_fp8.hip — prefix-cached / chunked prefill attention (K8) over the FP8 (OCP e4m3fn) KV cache on MFMA.
// Semantics: those of flash_prefill.hip's paged form (SURVEY A-9, reference Attention::flash_attention_varlen_with_cache,
// src/layers/attention.rs:211-222,264-318) with K = k_scale * e4m3(byte), V = v_scale * e4m3(byte): caches [NB, bs, KVH, D] BYTES, the queries
// of a tile are consecutive positions of one context and see keys 0 .. own position, f32 online softmax, output in the build's 16-bit type.
//
// Work split: flash_prefill.hip's.  One workgroup = 4 waves = one (FlashTile of 128/G query positions, kv head); a wave owns two 16-row
// query tiles, the QUERY sits on the lane in both products (Sᵀ = K·Qᵀ, Oᵀ += Vᵀ·Pᵀ), so the row max / sum and the rescale are lane-local;
// steps whose 64 keys all precede the tile's first query skip the causal compare.  block_size is a power of two and a multiple of the
// 64-key step (the 16-bit kernel's UB form, the only one built for bytes): a step lies inside one cache block and its block-table entry is
// a v_readlane from a register copy of 64 entries.
//
// Staging: a step's K and V rows go to LDS AS BYTES by LDS-DMA (glds_pieces: 16 B per lane, counted by hand), 64·D bytes per operand — half
// the requests and half the LDS of the 16-bit kernel (2 ring slots: 32 KiB at D = 128).  Bytes become 16-bit values IN REGISTERS, behind the LDS
// read (v_cvt_scalef32_pk_f16_fp8 / _bf16_fp8 with scale 1.0: exact, every e4m3 value is an fp16 and a bf16 value); Q is not quantised and the
// MFMAs are the 16-bit 16x16x32 ones, so the rounding points are those of the 16-bit kernel (P to 16 bits in front of the second product).
// k_scale is folded into the softmax scale, v_scale multiplies the finished row next to 1/sum: neither is in the loop.
//
// Key <-> MFMA row.  The A fragment of Vᵀ comes from ds_read_b64_tr_b8, the transposing byte read: in a 16-lane group, lane i supplies the
// address of 8 bytes = matrix row i/2, columns 8·(i%2) .. +7, and lane r receives column r of the 8 rows (byte e = row e) — measured on
// gfx950 with an identity image, the layout of the 16-bit form with 8 x 16 bytes in place of 4 x 16 halves.  With row = key and column = d,
// the group g4 of a wave gets, per d, the 8 keys of k-slots 8·g4 .. 8·g4+7 of a 32-key half in ONE read when those keys are consecutive:
// k-slot (g4, j) of half k2 <-> key 32·k2 + 8·g4 + j.  The B fragment of that product is the lane's exp'd Sᵀ accumulators of the two
// 16-key tiles 2·k2 and 2·k2+1 (accumulator e of tile mt in lane group g4 = MFMA row 4·g4 + e), so MFMA row ρ of Sᵀ tile mt is given
//     key(mt, ρ) = 32·(mt/2) + 8·(ρ/4) + 4·(mt%2) + ρ%4
// — only the LDS address of the K fragment; the causal compare uses this true key index.
//
// LDS images (rows of D bytes, 16-byte chunks c = 0 .. D/16-1, 64 banks x 4 B = sixteen 16-byte bank segments; a ds_read_b64 is served 32
// lanes at a time, which here is always 16 keys x ONE chunk = 256 B, conflict-free iff the 16 keys sit on 16 different segments).
// Un-swizzled, the segment of (key, c) is (8·key + c) mod 16 at D = 128 and (4·key + c) mod 16 at D = 64: 8- and 4-way conflicts.
//   V (16 consecutive keys per pass):      D = 128: c' = c ^ ((key >> 1) & 7) -> segment 8·(key & 1) + c', all 16;
//                                          D =  64: c' = c ^ ((key >> 2) & 3) -> segment 4·(key & 3) + c', all 16.
//   K (the 16 rows ρ of a tile: key bits 0,1 = ρ bits 0,1, key bits 3,4 = ρ bits 2,3, bits 2 and 5 fixed by mt; a lane's 8 bytes are the
//      half (g4 & 1) of chunk 2·ks + g4/2):
//                                          D = 128: c' = c ^ (((key >> 1) & 1) | (((key >> 3) & 3) << 1)) -> 8·(key & 1) + c', all 16;
//                                          D =  64: c' = c ^ ((key >> 3) & 3)                             -> 4·(key & 3) + c', all 16.
// The XOR is applied to the SOURCE address of a piece (the LDS-DMA writes lane-linear).
//
// Bytes behind a context: the last step of a tile clamps its key rows to the tile's last visible key (as the 16-bit kernel does), so rows at
// or beyond the context — garbage, e4m3 NaN codes included — are never READ, let alone multiplied by a zero probability; block-table entries
// past the context are never dereferenced.
//
// flash_shared_fp8_kernel (below): the same data path for the decode step's shared-prefix pass — decode rows in place of positions, no causal part;
// G in {1, 2, 4} on the prefill tile, and G = 8 on a tile of its own (16 rows x 8 heads, two heads per wave).
#include <type_traits>
#include "kernels.h"
#include "device_utils.h"
#include "flash_common.h"
#include "../common.h"

#if defined(NVR_FLASH_WAVES) && NVR_FLASH_WAVES != 4
#error "flash_prefill_fp8.hip is written for the 4-wave tile of flash_prefill.hip (flash_tile_positions)"
#endif

namespace nvr { namespace NVR_DT_NS {

struct FlashFp8Params {
    const half_t *q; int64_t ldq;
    const uint8_t *k, *v;
    const int32_t *block_tables; int32_t max_blocks, block_size, bs_shift;
    const FlashTile *tiles;
    int32_t H, KVH;
    float scale;                       // softmax scale x k_scale
    float v_scale;
    half_t *out;
};

// chunk XORs of the byte images (header comment; v8_swz and lds_read_tr8: flash_common.h)
template <int D>
__device__ __forceinline__ int k8_swz(int key) { return D == 128 ? (((key >> 1) & 1) | (((key >> 3) & 3) << 1)) : ((key >> 3) & 3); }

// 8 e4m3 bytes (two dwords, byte order = element order) -> 8 values of the build's 16-bit type, exactly
__device__ __forceinline__ half8_t fp8x8_to_half8(int2_t w) {
#ifdef NVR_BF16
#define NVR_CVT8(x, hi) __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((unsigned)(x), 1.0f, hi))
#else
#define NVR_CVT8(x, hi) __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)(x), 1.0f, hi))
#endif
    const half2_t a = NVR_CVT8(w[0], false), b = NVR_CVT8(w[0], true), c = NVR_CVT8(w[1], false), d = NVR_CVT8(w[1], true);
#undef NVR_CVT8
    return __builtin_shufflevector(__builtin_shufflevector(a, b, 0, 1, 2, 3), __builtin_shufflevector(c, d, 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int D, int G>
__global__ __launch_bounds__(256, 2) void flash_prefill_fp8_kernel(FlashFp8Params p) {
    constexpr int NT = 256, KT = 64;             // threads; keys per step
    constexpr int CPR = D / 16;                  // 16-byte chunks per K/V row
    constexpr int PIECES = KT * CPR / NT;        // 16-byte pieces per thread and operand (2 at D = 128, 1 at D = 64)
    constexpr int NKS = D / 32, NDT = D / 16, NQT = 2, NMT = KT / 16, NK2 = KT / 32;
    constexpr int OPB = KT * D;                  // bytes of one operand's image
    constexpr int STAGE = 2 * OPB;               // bytes of one ring slot [K | V]
    static_assert(OPB == PIECES * NT * 16, "glds_pieces walks the pieces of the K image, then of the V image, NT * 16 bytes apart");
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

    const int g = blockIdx.x % p.KVH;
    const FlashTile tile = p.tiles[blockIdx.x / p.KVH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, g4 = lane >> 4;
    const int kv_end = tile.pos0 + tile.nq;

    // the wave's two query tiles: head and position block
    int head[NQT], qpos[NQT], qrow[NQT]; bool qvalid[NQT];
    half8_t qf[NQT][NKS];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        int pblk;
        if (G == 1) { head[t] = g; pblk = wave * 2 + t; }
        else if (G == 2) { head[t] = g * 2 + t; pblk = wave; }
        else { head[t] = g * 4 + (wave & 1) * 2 + t; pblk = wave >> 1; }
        const int qi = pblk * 16 + r;
        qvalid[t] = qi < tile.nq;
        const int qc = qvalid[t] ? qi : tile.nq - 1;
        qpos[t] = tile.pos0 + qc;                                  // absolute position = last visible key
        qrow[t] = tile.q_row0 + qc;
        const half_t *qptr = p.q + (int64_t)qrow[t] * p.ldq + (int64_t)head[t] * D + g4 * 8;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[t][ks] = *reinterpret_cast<const half8_t *>(qptr + ks * 32);
    }
    // last key any lane of this wave may attend to: a step that starts beyond it does no arithmetic in this wave
    const int wave_last = __builtin_amdgcn_readfirstlane(tile.pos0 + min(tile.nq - 1, (G == 1 ? wave * 2 + 1 : (G == 2 ? wave : (wave >> 1))) * 16 + 15));

    // register copy of 64 block-table entries (lane j holds entry 64·c + j), fetched by an asm load that waits for itself: a compiler-visible
    // load inside the step loop would put s_waitcnt vmcnt(0) — which also drains the LDS-DMA in flight — into every step (flash_prefill.hip)
    int bt_reg = 0, bt_chunk = -1;
    auto load_bt_chunk = [&](int c) {
        bt_chunk = c;
        const int idx = min((c << 6) + lane, p.max_blocks - 1);                  // (entries past the table are never selected)
        const int32_t *src = p.block_tables + (int64_t)tile.kv_ref * p.max_blocks + idx;
        asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(bt_reg) : "v"(src) : "memory");
    };
    load_bt_chunk(0);

    // Source addresses of a step: scalar base of the step (block-table entry, offset inside the block) + a per-thread constant
    const unsigned lds_ring = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int64_t kconst[PIECES], vconst[PIECES];      // byte offsets of this thread's pieces inside a step
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int idx = i * NT + threadIdx.x, row = idx / CPR, c = idx % CPR;
        const int ksw = D == 128 ? (((row >> 1) & 1) | (((row >> 3) & 3) << 1)) : ((row >> 3) & 3);   // = k8_swz<D>(row) / v8_swz<D>(row), spelled out
        const int vsw = D == 128 ? ((row >> 1) & 7) : ((row >> 2) & 3);                                 // (flash_prefill.hip: a call here drops the host stub)
        const int64_t rowoff = ((int64_t)row * p.KVH + g) * D;
        kconst[i] = rowoff + (c ^ ksw) * 16;
        vconst[i] = rowoff + (c ^ vsw) * 16;
    }
    // the query fragments must have LANDED before the first LDS-DMA goes out (hipcc would otherwise keep its wait for them inside the loop)
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) asm volatile("" :: "v"(qf[t][ks]));
    auto stage = [&](int buf, int kt) {
        const uint8_t *src[2 * PIECES];
        const int bi = kt >> p.bs_shift;                                      // every key of the step is in this block (kt < kv_end: inside the context)
        if ((bi >> 6) != bt_chunk) load_bt_chunk(bi >> 6);
        const int64_t blk_row0 = (int64_t)__builtin_amdgcn_readlane(bt_reg, bi & 63) * p.block_size;
        if (kt + KT <= kv_end) {                                              // uniform: no key of this step is clamped
            const int64_t sbase = (blk_row0 + (kt & (p.block_size - 1))) * p.KVH * D;
#pragma unroll
            for (int i = 0; i < PIECES; ++i) { src[i] = p.k + sbase + kconst[i]; src[PIECES + i] = p.v + sbase + vconst[i]; }
        } else {                                                              // the tile's last step: rows past its last visible key repeat that key's
#pragma unroll
            for (int i = 0; i < PIECES; ++i) {
                const int idx = i * NT + threadIdx.x, row = idx / CPR, c = idx % CPR;
                const int key = min(kt + row, kv_end - 1);
                const int64_t off = ((blk_row0 + (key & (p.block_size - 1))) * p.KVH + g) * D;
                const int ksw = D == 128 ? (((row >> 1) & 1) | (((row >> 3) & 3) << 1)) : ((row >> 3) & 3);
                const int vsw = D == 128 ? ((row >> 1) & 7) : ((row >> 2) & 3);
                src[i] = p.k + off + (c ^ ksw) * 16;
                src[PIECES + i] = p.v + off + (c ^ vsw) * 16;
            }
        }
        glds_pieces<2 * PIECES, NT * 16>(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_ring + buf * STAGE + wave_u * 1024)));
    };

    // softmax on RAW scores as in flash_prefill.hip: m = running max of q·k, p = 2^((s - m)·c2), row sums from the matrix core (all-ones A)
    float4_t o[NQT][NDT], ol[NQT];
    float m[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        m[t] = -INFINITY; ol[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NDT; ++i) o[t][i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    }
    const float c2 = p.scale * 1.44269504088896340736f;
    half8_t ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (half_t)1.0f;

    // lane-constant parts of the fragment addresses
    const int krow = (r >> 2) * 8 + (r & 3);                         // key(mt, ρ = r) - 32·(mt/2) - 4·(mt%2)
    const int kxor = k8_swz<D>(krow);                                // (bits 2 and 5 of the key are not in the XOR)
    const int koff = krow * D + ((g4 & 1) << 3);
    const int vrow = g4 * 8 + (r >> 1);                              // key of the 8-byte piece this lane addresses - 32·k2
    const int vxor = v8_swz<D>(vrow);
    const int voff = vrow * D + ((r & 1) << 3);

    const int nsteps = (kv_end + KT - 1) / KT;
    // step `it` computes on ring slot it % 2 while tile it+1 is requested into the slot step it-1 released; before its closing barrier
    // every wave waits for its own requests, so tile it+1 has landed for all waves after the barrier
    auto step = [&](auto cur_c, int it) {
        constexpr int cur = decltype(cur_c)::value;
        const int kt = it * KT;
        if (it + 1 < nsteps) stage(cur ^ 1, kt + KT);
        const char *kl = smem + cur * STAGE, *vl = kl + OPB;
        if (kt <= wave_last) {

        // Sᵀ tiles: NMT x (16 keys x 16 queries) per query tile; the K bytes of key tile mt+1 are requested before the MFMAs of tile mt
        float4_t s[NQT][NMT];
        int2_t kb[2][NKS];
        auto read_k = [&](int mt, int2_t (&dst)[NKS]) {
            const char *row = kl + ((mt >> 1) * 32 + (mt & 1) * 4) * D + koff;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) dst[ks] = *reinterpret_cast<const int2_t *>(row + (((ks * 2 + (g4 >> 1)) ^ kxor) << 4));
        };
        read_k(0, kb[0]);
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            if (mt + 1 < NMT) read_k(mt + 1, kb[(mt + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NQT; ++t) s[t][mt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const half8_t kf = fp8x8_to_half8(kb[mt & 1][ks]);
#pragma unroll
                for (int t = 0; t < NQT; ++t) s[t][mt] = mfma16(kf, qf[t][ks], s[t][mt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // causal mask only on steps that reach past the tile's first query; accumulator e of tile mt holds key(mt, 4·g4 + e)
        if (kt + KT - 1 > tile.pos0) {
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (kt + (mt >> 1) * 32 + g4 * 8 + (mt & 1) * 4 + e > qpos[t]) s[t][mt][e] = -INFINITY;
        }
        half8_t pf[NQT][NK2];
        bool moved = false;
        float alpha[NQT];
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            float mx = fmaxf(fmaxf(s[t][0][0], s[t][0][1]), fmaxf(s[t][0][2], s[t][0][3]));
#pragma unroll
            for (int mt = 1; mt < NMT; ++mt) mx = fmaxf(fmaxf(mx, s[t][mt][0]), fmaxf(fmaxf(s[t][mt][1], s[t][mt][2]), s[t][mt][3]));
            mx = max_over_rows(mx);
            const float mn = fmaxf(m[t], mx);                   // finite from the first step on (key 0 <= qpos)
            alpha[t] = __builtin_amdgcn_exp2f((m[t] - mn) * c2);
            moved |= mn != m[t];
            m[t] = mn;
            const float mc = -mn * c2;
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    pf[t][mt >> 1][(mt & 1) * 4 + e] = (half_t)__builtin_amdgcn_exp2f(fmaf(s[t][mt][e], c2, mc));   // k-slot (g4, j): key 32·k2 + 8·g4 + j
        }
        if (__any(moved)) {                                     // wave-uniform: the running max settles after a few steps
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
                ol[t] *= alpha[t];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) o[t][dt] *= alpha[t];
            }
        }
        // Oᵀ += Vᵀ·Pᵀ per 32-key half; one transposing byte read = the 8 keys of this lane group at d = 16·dt + r, for both query tiles
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) {
#pragma unroll
            for (int t = 0; t < NQT; ++t) ol[t] = mfma16(ones, pf[t][k2], ol[t]);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const half8_t vf = fp8x8_to_half8(lds_read_tr8(vl + k2 * 32 * D + voff + ((dt ^ vxor) << 4)));
#pragma unroll
                for (int t = 0; t < NQT; ++t) o[t][dt] = mfma16(vf, pf[t][k2], o[t][dt]);
            }
        }
        }   // kt <= wave_last
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int it = 0; it < nsteps; it += 2) {                    // ring slot as a compile-time constant: LDS addresses fold
        step(std::integral_constant<int, 0>{}, it);
        if (it + 1 < nsteps) step(std::integral_constant<int, 1>{}, it + 1);
    }

#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        if (qvalid[t]) {
            const float ls = ol[t][0];                          // every row of the ones-product holds the query's sum
            const float inv = ls > 0.f ? p.v_scale / ls : 0.f;
            half_t *orow = p.out + ((int64_t)qrow[t] * p.H + head[t]) * D + g4 * 4;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                half4_t hv = {(half_t)(o[t][dt][0] * inv), (half_t)(o[t][dt][1] * inv), (half_t)(o[t][dt][2] * inv), (half_t)(o[t][dt][3] * inv)};
                *reinterpret_cast<half4_t *>(orow + dt * 16) = hv;
            }
        }
    }
}

bool flash_prefill_fp8_ok(int D, int H, int KVH, int block_size) {
    if (KVH <= 0 || H % KVH) return false;
    const int G = H / KVH;
    return (D == 64 || D == 128) && (G == 1 || G == 2 || G == 4) && block_size >= 64 && (block_size & (block_size - 1)) == 0;
}

int flash_prefill_fp8(const FlashFp8Args &a, hipStream_t s) {
    if (a.ntiles == 0) return 0;
    if (!flash_prefill_fp8_ok(a.D, a.H, a.KVH, a.block_size))
        return nvr::fail(NVR_ERR_UNSUPPORTED, "flash_prefill_fp8: D=%d H=%d KVH=%d block_size=%d (D in {64,128}, H/KVH in {1,2,4}, block_size a power of two >= 64)",
                         a.D, a.H, a.KVH, a.block_size);
    if (!(a.k_scale > 0.f) || !(a.v_scale > 0.f)) return nvr::fail(NVR_ERR_INVALID_ARG, "flash_prefill_fp8: scales %g / %g (positive)", a.k_scale, a.v_scale);
    FlashFp8Params p{};
    p.q = (const half_t *)a.q; p.ldq = a.ldq; p.k = a.k; p.v = a.v;
    p.block_tables = a.block_tables; p.max_blocks = a.max_blocks; p.block_size = a.block_size; p.bs_shift = __builtin_ctz(a.block_size);
    p.tiles = a.tiles; p.H = a.H; p.KVH = a.KVH; p.scale = a.scale * a.k_scale; p.v_scale = a.v_scale; p.out = (half_t *)a.out;
    const int G = a.H / a.KVH;
    dim3 grid((unsigned)((int64_t)a.ntiles * a.KVH)), block(256);
#define NVR_FLASH8(DD, GG) if (a.D == DD && G == GG) flash_prefill_fp8_kernel<DD, GG><<<grid, block, 0, s>>>(p);
    NVR_FLASH8(128, 1) NVR_FLASH8(128, 2) NVR_FLASH8(128, 4) NVR_FLASH8(64, 1) NVR_FLASH8(64, 2) NVR_FLASH8(64, 4)
#undef NVR_FLASH8
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "flash_prefill_fp8 launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- shared-prefix decode pass -------------------------------------------------------------------------------------------------------
// The decode step's attention over a prefix that every member of a group of sequences holds in the SAME cache blocks, byte-cache
// counterpart of flash_prefill_kernel<.., SHARED = true> (flash_prefill.hip).  A kernel of its own, so flash_prefill_fp8_kernel keeps its
// instructions; the data path is that kernel's (header comment), the differences are:
//   * grid (ceil(nq / (128/G)) * KVH, sparts): a workgroup = one tile of 128/G DECODE ROWS (row i of the tile = srows[i] when a group is
//     given, else i; rows at or beyond *scount / nq_total are clamped for the loads and never stored) x the G heads of one kv head x
//     partition blockIdx.y = keys [y * part_len, (y + 1) * part_len) through the block-table row of the first member;
//   * part_len is a multiple of the 64-key step and every key of it is visible to every row: no causal compare, no clamped last step, no
//     wave that sits a step out — the loop is stage / K product / softmax / V product and nothing else;
//   * the result leaves as a split-KV partial in the units of attn_fp8_kernel: f32 sums x v_scale, the maximum in SCALED units (raw
//     maximum x softmax scale x k_scale), the sum of the 16-bit-rounded probabilities.
// 2-slot ring and two workgroups per CU as in the prefill kernel: a launch is ~256 workgroups of part_len / 64 (2 at BASELINE configs[4])
// steps, so step 1 is requested while step 0 is computed and nothing deeper could be in flight; other depths: not measured.
// G = 8 (the prefill kernel has no such instantiation): the tile is 16 decode rows x the 8 heads of a kv head, ALL FOUR waves hold the same 16
// rows and wave w owns heads 8g + 2w and 8g + 2w + 1, one 16-row query tile per head, so the member-row lookup is one per lane.  (Tile height 16 against 32
// rows: profiles/fp8_gqa8_shared.txt.)
struct FlashFp8SharedParams {
    const half_t *q; int64_t ldq;
    const uint8_t *k, *v;
    const int32_t *block_tables; int32_t max_blocks, block_size, bs_shift;
    int32_t H, KVH;
    float scale;                       // softmax scale x k_scale
    float v_scale;
    int32_t nq_total, part_len, num_parts;
    float *part_o, *part_ml;           // [nq, H, num_parts, D], [nq, H, num_parts, 2]
    const int32_t *srows, *scount;     // optional group: member rows srows[0 .. *scount)
};

template <int D, int G>
__global__ __launch_bounds__(256, 2) void flash_shared_fp8_kernel(FlashFp8SharedParams p) {
    constexpr int NT = 256, KT = 64, QB = 128 / G;
    constexpr int CPR = D / 16;
    constexpr int PIECES = KT * CPR / NT;
    constexpr int NKS = D / 32, NDT = D / 16, NQT = 2, NMT = KT / 16, NK2 = KT / 32;
    constexpr int OPB = KT * D;
    constexpr int STAGE = 2 * OPB;
    static_assert(OPB == PIECES * NT * 16, "glds_pieces walks the pieces of the K image, then of the V image, NT * 16 bytes apart");
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

    const int g = blockIdx.x % p.KVH;
    const int row0 = (int)(blockIdx.x / p.KVH) * QB;
    const int nq = min(QB, (p.scount ? *p.scount : p.nq_total) - row0);
    if (nq <= 0) return;                                              // (workgroup-uniform: the launch is sized for the whole batch)
    const int kv_ref = p.srows ? p.srows[0] : 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, g4 = lane >> 4;
    const int kv_start = (int)blockIdx.y * p.part_len;
    const int nsteps = p.part_len / KT;

    int head[NQT], qrow[NQT]; bool qvalid[NQT];
    half8_t qf[NQT][NKS];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        int pblk;
        if (G == 1) { head[t] = g; pblk = wave * 2 + t; }
        else if (G == 2) { head[t] = g * 2 + t; pblk = wave; }
        else if (G == 4) { head[t] = g * 4 + (wave & 1) * 2 + t; pblk = wave >> 1; }
        else { head[t] = g * 8 + wave * 2 + t; pblk = 0; }               // G = 8: all four waves hold the same 16 rows, two heads each
        if (G == 8 && t == 1) { qvalid[1] = qvalid[0]; qrow[1] = qrow[0]; }   // the row of the lane's other head: looked up once
        else {
            const int qi = pblk * 16 + r;
            qvalid[t] = qi < nq;
            const int qc = row0 + (qvalid[t] ? qi : nq - 1);
            qrow[t] = p.srows ? p.srows[qc] : qc;
        }
        const half_t *qptr = p.q + (int64_t)qrow[t] * p.ldq + (int64_t)head[t] * D + g4 * 8;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[t][ks] = *reinterpret_cast<const half8_t *>(qptr + ks * 32);
    }

    // register copy of 64 block-table entries, reloaded by the self-waiting asm load when the prefix spans more than 64 blocks
    int bt_reg = 0, bt_chunk = -1;
    auto load_bt_chunk = [&](int c) {
        bt_chunk = c;
        const int idx = min((c << 6) + lane, p.max_blocks - 1);
        const int32_t *src = p.block_tables + (int64_t)kv_ref * p.max_blocks + idx;
        asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(bt_reg) : "v"(src) : "memory");
    };
    load_bt_chunk((kv_start >> p.bs_shift) >> 6);

    const unsigned lds_ring = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int64_t kconst[PIECES], vconst[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int idx = i * NT + threadIdx.x, row = idx / CPR, c = idx % CPR;
        const int ksw = D == 128 ? (((row >> 1) & 1) | (((row >> 3) & 3) << 1)) : ((row >> 3) & 3);
        const int vsw = D == 128 ? ((row >> 1) & 7) : ((row >> 2) & 3);
        const int64_t rowoff = ((int64_t)row * p.KVH + g) * D;
        kconst[i] = rowoff + (c ^ ksw) * 16;
        vconst[i] = rowoff + (c ^ vsw) * 16;
    }
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) asm volatile("" :: "v"(qf[t][ks]));
    // a step = 64 consecutive rows of ONE cache block (block_size a power of two >= 64, kt a multiple of 64)
    auto stage = [&](int buf, int kt) {
        const uint8_t *src[2 * PIECES];
        const int bi = kt >> p.bs_shift;
        if ((bi >> 6) != bt_chunk) load_bt_chunk(bi >> 6);
        const int64_t blk_row0 = (int64_t)__builtin_amdgcn_readlane(bt_reg, bi & 63) * p.block_size;
        const int64_t sbase = (blk_row0 + (kt & (p.block_size - 1))) * p.KVH * D;
#pragma unroll
        for (int i = 0; i < PIECES; ++i) { src[i] = p.k + sbase + kconst[i]; src[PIECES + i] = p.v + sbase + vconst[i]; }
        glds_pieces<2 * PIECES, NT * 16>(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_ring + buf * STAGE + wave_u * 1024)));
    };

    float4_t o[NQT][NDT], ol[NQT];
    float m[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        m[t] = -INFINITY; ol[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NDT; ++i) o[t][i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    }
    const float c2 = p.scale * 1.44269504088896340736f;
    half8_t ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (half_t)1.0f;

    const int krow = (r >> 2) * 8 + (r & 3);
    const int kxor = k8_swz<D>(krow);
    const int koff = krow * D + ((g4 & 1) << 3);
    const int vrow = g4 * 8 + (r >> 1);
    const int vxor = v8_swz<D>(vrow);
    const int voff = vrow * D + ((r & 1) << 3);

    auto step = [&](auto cur_c, int it) {
        constexpr int cur = decltype(cur_c)::value;
        if (it + 1 < nsteps) stage(cur ^ 1, kv_start + (it + 1) * KT);
        const char *kl = smem + cur * STAGE, *vl = kl + OPB;

        float4_t s[NQT][NMT];
        int2_t kb[2][NKS];
        auto read_k = [&](int mt, int2_t (&dst)[NKS]) {
            const char *row = kl + ((mt >> 1) * 32 + (mt & 1) * 4) * D + koff;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) dst[ks] = *reinterpret_cast<const int2_t *>(row + (((ks * 2 + (g4 >> 1)) ^ kxor) << 4));
        };
        read_k(0, kb[0]);
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            if (mt + 1 < NMT) read_k(mt + 1, kb[(mt + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NQT; ++t) s[t][mt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const half8_t kf = fp8x8_to_half8(kb[mt & 1][ks]);
#pragma unroll
                for (int t = 0; t < NQT; ++t) s[t][mt] = mfma16(kf, qf[t][ks], s[t][mt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        half8_t pf[NQT][NK2];
        bool moved = false;
        float alpha[NQT];
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            float mx = fmaxf(fmaxf(s[t][0][0], s[t][0][1]), fmaxf(s[t][0][2], s[t][0][3]));
#pragma unroll
            for (int mt = 1; mt < NMT; ++mt) mx = fmaxf(fmaxf(mx, s[t][mt][0]), fmaxf(fmaxf(s[t][mt][1], s[t][mt][2]), s[t][mt][3]));
            mx = max_over_rows(mx);
            const float mn = fmaxf(m[t], mx);                   // finite from the first step on: all 64 keys are visible
            alpha[t] = __builtin_amdgcn_exp2f((m[t] - mn) * c2);
            moved |= mn != m[t];
            m[t] = mn;
            const float mc = -mn * c2;
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    pf[t][mt >> 1][(mt & 1) * 4 + e] = (half_t)__builtin_amdgcn_exp2f(fmaf(s[t][mt][e], c2, mc));
        }
        if (__any(moved)) {
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
                ol[t] *= alpha[t];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) o[t][dt] *= alpha[t];
            }
        }
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) {
#pragma unroll
            for (int t = 0; t < NQT; ++t) ol[t] = mfma16(ones, pf[t][k2], ol[t]);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const half8_t vf = fp8x8_to_half8(lds_read_tr8(vl + k2 * 32 * D + voff + ((dt ^ vxor) << 4)));
#pragma unroll
                for (int t = 0; t < NQT; ++t) o[t][dt] = mfma16(vf, pf[t][k2], o[t][dt]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    stage(0, kv_start);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int it = 0; it < nsteps; it += 2) {
        step(std::integral_constant<int, 0>{}, it);
        if (it + 1 < nsteps) step(std::integral_constant<int, 1>{}, it + 1);
    }

    // the partial of partition blockIdx.y: accumulator e of d-tile dt in lane group g4 is column 16·dt + 4·g4 + e of query r
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        if (!qvalid[t]) continue;
        const int64_t slot = ((int64_t)qrow[t] * p.H + head[t]) * p.num_parts + blockIdx.y;
        float *po = p.part_o + slot * D + g4 * 4;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) *reinterpret_cast<float4_t *>(po + dt * 16) = o[t][dt] * p.v_scale;
        if (g4 == 0) { p.part_ml[slot * 2] = m[t] * p.scale; p.part_ml[slot * 2 + 1] = ol[t][0]; }
    }
}

// shapes of the shared-prefix pass: the prefill kernel's, or 8 heads per kv head (the tile of 16 decode rows x 8 heads)
bool flash_shared_fp8_ok(int D, int H, int KVH, int block_size) {
    if (flash_prefill_fp8_ok(D, H, KVH, block_size)) return true;
    if (KVH <= 0 || H % KVH) return false;
    return (D == 64 || D == 128) && H / KVH == 8 && block_size >= 64 && (block_size & (block_size - 1)) == 0;
}

// Partitions 0 .. sparts-1 (part_len keys each) of a decode step whose sequences (all nq, or the rows[0 .. *count) of them) share their first
// sparts * part_len cached keys: f32 partials into slots (row, head, partition) of part_o [nq, H, num_parts, D] / part_ml [nq, H, num_parts, 2]
int flash_shared_prefix_fp8(const half_bits *q, int64_t ldq, const uint8_t *k_cache, const uint8_t *v_cache, const int32_t *block_tables,
                            int32_t max_blocks, int32_t block_size, int32_t nq, int32_t H, int32_t KVH, int32_t D, float scale, float k_scale,
                            float v_scale, int32_t part_len, int32_t sparts, int32_t num_parts, float *part_o, float *part_ml, hipStream_t s,
                            const int32_t *rows, const int32_t *count) {
    if (nq == 0) return 0;
    if (!flash_shared_fp8_ok(D, H, KVH, block_size) || part_len <= 0 || part_len % 64 || sparts < 1 || sparts > num_parts)
        return nvr::fail(NVR_ERR_UNSUPPORTED, "flash_shared_prefix_fp8: D=%d H=%d KVH=%d block_size=%d part_len=%d x %d", D, H, KVH, block_size, part_len, sparts);
    FlashFp8SharedParams p{};
    p.q = (const half_t *)q; p.ldq = ldq; p.k = k_cache; p.v = v_cache;
    p.block_tables = block_tables; p.max_blocks = max_blocks; p.block_size = block_size; p.bs_shift = __builtin_ctz(block_size);
    p.H = H; p.KVH = KVH; p.scale = scale * k_scale; p.v_scale = v_scale; p.nq_total = nq; p.part_len = part_len; p.num_parts = num_parts;
    p.part_o = part_o; p.part_ml = part_ml; p.srows = rows; p.scount = count;
    const int G = H / KVH, qb = 128 / G;
    dim3 grid((unsigned)((int64_t)((nq + qb - 1) / qb) * KVH), (unsigned)sparts), block(256);
#define NVR_FLASH8_S(DD, GG) if (D == DD && G == GG) flash_shared_fp8_kernel<DD, GG><<<grid, block, 0, s>>>(p);
    NVR_FLASH8_S(128, 1) NVR_FLASH8_S(128, 2) NVR_FLASH8_S(128, 4) NVR_FLASH8_S(128, 8) NVR_FLASH8_S(64, 1) NVR_FLASH8_S(64, 2) NVR_FLASH8_S(64, 4) NVR_FLASH8_S(64, 8)
#undef NVR_FLASH8_S
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "flash_shared_prefix_fp8 launch failed: %s", hipGetErrorString(e));
    return 0;
}

}}  // namespace nvr::k / nvr::kb (NVR_DT_NS)

// attention_fp8.hip — the FP8 (OCP e4m3fn) KV cache for gfx950: the quantising store (kv_store_fp8) and paged decode attention over
// byte caches (attention_fp8).  Semantics of the decode kernel are those of attention.hip's (query t sees exactly
// ctx_lens[t] keys, softmax in f32, the G = H/KVH query heads of a kv head together); reference call site
// Attention::flash_attention_decode, src/layers/attention.rs:225-235, cache rows :150-174.
//
// Format: caches [NB, bs, KVH, D] BYTES; one k_scale and one v_scale (f32) per call: stored byte = e4m3(x / scale), value read =
// byte * scale.  k_scale is folded into the softmax scale and v_scale multiplies a workgroup's finished f32 sums once (in front of the
// division by the softmax sum, or of the merge of the partitions, which is linear in them), so neither is seen by the inner loop.
//
// Geometry (its own, not attn_rows_kernel's): a K / V row of one kv head is D bytes; a lane holds 16 of them (one 16-byte request),
// so a row is D/16 lanes (8 at D = 128, 4 at D = 64) and one wave-instruction reads 64/(D/16) rows = 1 KiB: 8 tokens at D = 128, 16 at
// D = 64 — twice the tokens per request of the 16-bit kernel.  Requests go straight to VGPRs, non-temporal, U row groups of K and of V
// back to back before any arithmetic.  Dequantisation is in registers: K bytes -> packed 16-bit pairs (v_cvt_scalef32_pk_f16_fp8 /
// _bf16_fp8, scale operand 1.0) -> v_dot2 against the q pairs; V bytes -> f32 pairs (v_cvt_pk_f32_fp8) -> f32 FMA.  The butterfly of a
// row's dot product runs over D/16 lanes and the 64/(D/16) row-group slots of a wave are merged once, at the end.
//
// Two launches: one or more workgroups per (query, kv head) pair (attn_fp8_kernel, + attn_fp8_merge_kernel for split contexts), or — pair counts that fill the
// per-pair rounds badly, ragged batches — workgroups that walk equal shares of all pairs' keys (attn_share_fp8_kernel).  G = 8 does not run here: its
// launches go to the matrix cores (attn_fp8_mfma_kernel per pair, attn_share_fp8_mfma_kernel work-balanced: attention_fp8_mfma.hip) with this file's partials,
// merge kernel and launch rule, the shared-prefix plan included (launch_attn_fp8_mfma).
#include <algorithm>
#include <type_traits>
#include "kernels.h"
#include "device_utils.h"
#include "attn_merge.h"
#include "attn_share.h"
#include "../common.h"

namespace nvr { namespace NVR_DT_NS {

typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));

// ---- kv_store_fp8 ----------------------------------------------------------------------------------------------------------------
// e4m3 of x: round to nearest even, clamped to +-448 in front of the conversion (v_cvt_pk_fp8_f32 saturates or not by a mode bit)
__device__ __forceinline__ float clamp448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }

// One lane = 16 consecutive elements of the K or the V part of one token's qkv row -> one 16-byte store into the byte cache.
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(const half_t *__restrict__ qkv, const int32_t *__restrict__ slots, int64_t T, int H, int KVH, int D,
                                                           float k_scale, float v_scale, uint8_t *__restrict__ kc, uint8_t *__restrict__ vc) {
    const int per_kv = KVH * D / 16, per_tok = 2 * per_kv;              // 16-element pieces of a token's K (or V) columns / of both
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * per_tok) return;
    const int64_t t = idx / per_tok;
    const int c = (int)(idx - t * per_tok);
    const bool is_v = c >= per_kv;
    const int e0 = (is_v ? c - per_kv : c) * 16;                         // first element inside the token's [KVH, D] row
    const int slot = slots[t];
    if (slot < 0) return;
    const half_t *src = qkv + t * (int64_t)(H + 2 * KVH) * D + (int64_t)(H + (is_v ? KVH : 0)) * D + e0;
    const half8_t a = *reinterpret_cast<const half8_t *>(src), b = *reinterpret_cast<const half8_t *>(src + 8);
    const float sc = is_v ? v_scale : k_scale;
    float x[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) { x[j] = clamp448((float)a[j] / sc); x[8 + j] = clamp448((float)b[j] / sc); }
    uint4_t w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j], x[4 * j + 1], r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j + 2], x[4 * j + 3], r, true);
        w[j] = (unsigned int)r;
    }
    *reinterpret_cast<uint4_t *>((is_v ? vc : kc) + (int64_t)slot * KVH * D + e0) = w;
}

int kv_store_fp8(const half_bits *qkv, const int32_t *slots, int64_t T, int64_t H, int64_t KVH, int64_t D, float k_scale, float v_scale,
                 uint8_t *k_cache, uint8_t *v_cache, hipStream_t s) {
    if (T == 0) return 0;
    if (D % 16 || !(k_scale > 0.f) || !(v_scale > 0.f))
        return nvr::fail(NVR_ERR_INVALID_ARG, "kv_store_fp8: head_dim %ld (a multiple of 16), scales %g / %g (positive)", (long)D, k_scale, v_scale);
    const int64_t n = T * 2 * KVH * D / 16;
    kv_store_fp8_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>((const half_t *)qkv, slots, T, (int)H, (int)KVH, (int)D, k_scale, v_scale,
                                                                                 k_cache, v_cache);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "kv_store_fp8 launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- attention_fp8 ---------------------------------------------------------------------------------------------------------------
struct AttnFp8Params {
    const half_t *q; int64_t ldq;
    const uint8_t *k, *v;
    const int32_t *ctx_lens, *block_tables;
    int32_t max_blocks, block_size, bs_shift;
    int32_t H, KVH;
    float scale;                       // softmax scale x k_scale
    float v_scale;
    int32_t part_size, num_parts;
    int32_t part0, kv0;                // shared-prefix decode: partitions 0..part0-1 hold the group's shared keys [0, kv0) (written by
                                       // flash_shared_prefix_fp8); this launch covers partition part0 + i = keys [kv0 + i*part_size, ..)
    const int32_t *kv0_rows;           // per-query kv0 (a group inside the batch: members shared_len, others 0) or null = kv0 for all
    float *part_o; float *part_ml;     // [nq, H, num_parts, D], [nq, H, num_parts, 2]
    half_t *out;                       // [nq, H, D]
};

// 4 e4m3 bytes of w -> two packed 16-bit pairs (bytes 0,1 and 2,3) of the build's type, exactly (every e4m3 value is an fp16 and a bf16 value)
__device__ __forceinline__ void fp8x4_to_half2(unsigned int w, half2_t &lo, half2_t &hi) {
#ifdef NVR_BF16
    lo = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
    hi = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
#else
    lo = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
    hi = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
#endif
}

// sum over the LPR (8 or 4) consecutive lanes that hold one byte row, result in every lane of the group
template <int LPR>
__device__ __forceinline__ float byte_row_sum(float x) {
    if (LPR == 8) x = dpp_add<0x141>(x);                                   // row_half_mirror (8 lanes: i <-> 7-i)
    x = dpp_add<0x4E>(x);                                                  // quad_perm [2,3,0,1]
    x = dpp_add<0xB1>(x);                                                  // quad_perm [1,0,3,2]
    return x;
}
// sum / max over the 64/LPR row-group slots of the wave (lanes with equal lane % LPR), result in every lane
template <int LPR>
__device__ __forceinline__ float slots_sum(float x) {
    if (LPR == 4) x = dpp_add<0x124>(x);                                   // row_ror:4 inside the 16-lane row
    x = dpp_add<0x128>(x);                                                 // row_ror:8
    return xor32_partner_sum(xor16_partner_sum(x));
}
template <int LPR>
__device__ __forceinline__ float slots_max(float x) {
    if (LPR == 4) x = dpp_max<0x124>(x);
    x = dpp_max<0x128>(x);
    return xor32_partner_max(xor16_partner_max(x));
}

// One workgroup of WAVES waves owns (query t, kv head g, partition).  The partition is cut into chunks of U row groups (TPI = U * RPI
// consecutive tokens); in a FULL round every wave takes one whole chunk (chunk r * WAVES + wave) and requests its U groups of K and of V
// with no validity tests; what is left after the last full round is dealt out group by group (group j -> wave j % WAVES) and requested
// AHEAD of the last full round's arithmetic.  UB: block_size (and the partition size) is a multiple of TPI, so a chunk lies inside one
// cache block: its block-table entry is a scalar read (v_readlane) from a register copy of 64 entries, and a row address is scalar base +
// lane offset.  Otherwise every lane looks its row's block up.  num_parts == 1: the workgroup writes the 16-bit rows itself;
// else f32 partials in the layout of attn_workspace_bytes, merged by attn_fp8_merge_kernel.
template <int D, int G, int U, int WAVES, bool UB>
__global__ __launch_bounds__(WAVES * 64) void attn_fp8_kernel(AttnFp8Params p) {
    constexpr int LPR = D / 16;         // lanes per byte row
    constexpr int RPI = 64 / LPR;       // rows per wave-instruction (= tokens per row group)
    constexpr int TPI = RPI * U;        // tokens per chunk
    const int lparts = p.num_parts - p.part0;        // partitions of this launch
    const int part = p.part0 + blockIdx.x % lparts, g = (blockIdx.x / lparts) % p.KVH;
    const int t = blockIdx.x / (lparts * p.KVH);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int dc = lane % LPR, tg = lane / LPR;
    const int p0 = (p.kv0_rows ? p.kv0_rows[t] : p.kv0) + (part - p.part0) * p.part_size;   // (kv0: a multiple of 64, so UB chunks stay inside a block)
    const bool direct = p.num_parts == 1;

    const int32_t *bt = p.block_tables + (int64_t)t * p.max_blocks;
    int bt_chunk = -1, bt_reg = 0;                   // UB: register copy of 64 block-table entries (lane j holds entry 64 * c + j)
    auto load_bt_chunk = [&](int c) {
        bt_chunk = c;
        const int idx = (c << 6) + lane;
        bt_reg = idx < p.max_blocks ? bt[idx] : 0;
    };
    if (UB) load_bt_chunk((p.bs_shift >= 0 ? p0 >> p.bs_shift : p0 / p.block_size) >> 6);   // requested with ctx and q, ahead of their use

    // q slice of this lane (16 elements) for the G heads of kv head g, as 16-bit pairs for v_dot2
    half2_t qv[G][8];
    {
        const half_t *qrow = p.q + (int64_t)t * p.ldq + (int64_t)g * G * D + dc * 16;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const half8_t a = *reinterpret_cast<const half8_t *>(qrow + i * D), b = *reinterpret_cast<const half8_t *>(qrow + i * D + 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) { qv[i][j] = (half2_t){a[2 * j], a[2 * j + 1]}; qv[i][4 + j] = (half2_t){b[2 * j], b[2 * j + 1]}; }
        }
    }
    const int ctx = p.ctx_lens[t];
    if (p0 >= ctx && !direct) return;                // empty partition (or a member with no keys behind the prefix): the merge skips it too
    const int pend = max(p0, min(ctx, p0 + p.part_size));
    const int row_bytes = p.KVH * D;

    // byte offset of (scalar token tb, kv head g, d = 0) through the register copy of the block table
    auto block_base = [&](int tb) -> int64_t {
        int bi, bo;
        if (p.bs_shift >= 0) { bi = tb >> p.bs_shift; bo = tb & (p.block_size - 1); }
        else { bi = tb / p.block_size; bo = tb - bi * p.block_size; }
        if ((bi >> 6) != bt_chunk) load_bt_chunk(bi >> 6);
        const int blk = __builtin_amdgcn_readlane(bt_reg, bi & 63);
        return (((int64_t)blk * p.block_size + bo) * p.KVH + g) * D;
    };
    // per-lane form (block sizes that are no multiple of the chunk)
    auto lane_row = [&](int tok) -> int64_t {
        int bi, bo;
        if (p.bs_shift >= 0) { bi = tok >> p.bs_shift; bo = tok & (p.block_size - 1); }
        else { bi = tok / p.block_size; bo = tok - bi * p.block_size; }
        return (((int64_t)bt[bi] * p.block_size + bo) * p.KVH + g) * D + dc * 16;
    };
    auto load16 = [](const uint8_t *ptr) { return __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(ptr)); };

    // online softmax state per head AND per row-group slot of the wave (merged once at the end)
    float m[G], l[G], acc[G][16];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        m[i] = -INFINITY; l[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    }

    // scores, online softmax and p.v for U row groups; CHECK: slot u holds token tok0 + u * WAVES * RPI + tg, valid < pend
    auto process = [&](auto check, const uint4_t (&kk)[U], const uint4_t (&vv)[U], int tok0) {
        constexpr bool CHECK = decltype(check)::value;
        float s[U][G];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool valid = !CHECK || tok0 + u * (WAVES * RPI) + tg < pend;
            half2_t kh[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) fp8x4_to_half2(kk[u][j], kh[2 * j], kh[2 * j + 1]);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                float d = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) d = dot2(kh[j], qv[i][j], d);
                d = byte_row_sum<LPR>(d);
                s[u][i] = valid ? d * p.scale : -INFINITY;               // (a NaN byte behind the context ends here)
            }
        }
        float alpha[G], ms[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            float mx = s[0][i];
#pragma unroll
            for (int u = 1; u < U; ++u) mx = fmaxf(mx, s[u][i]);
            const float mn = fmaxf(m[i], mx);
            ms[i] = (CHECK && mn == -INFINITY) ? 0.f : mn;               // a slot that has seen no valid token yet
            alpha[i] = __expf(m[i] - ms[i]);                             // m = -inf on first use -> 0
            m[i] = mn;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[i][j] *= alpha[i];
        }
        float ps[G];
#pragma unroll
        for (int i = 0; i < G; ++i) ps[i] = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // the row's V bytes once for all G heads (rows behind the context are never requested: the remainder repeats row pend - 1 with p = 0)
            float vf[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(vv[u][j], false), b = __builtin_amdgcn_cvt_pk_f32_fp8(vv[u][j], true);
                vf[4 * j] = a[0]; vf[4 * j + 1] = a[1]; vf[4 * j + 2] = b[0]; vf[4 * j + 3] = b[1];
            }
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const float pr = __expf(s[u][i] - ms[i]);
                ps[i] += pr;
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[i][j] = fmaf(pr, vf[j], acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < G; ++i) l[i] = __fmaf_rn(l[i], alpha[i], ps[i]);
    };

    const int ng = (pend - p0 + RPI - 1) / RPI;      // row groups of this partition, the last one possibly partial
    const int R = (pend - p0) / (TPI * WAVES);       // full rounds: every wave gets a complete chunk
    const int gt0 = R * (WAVES * U) + wave;          // this wave's remainder groups: gt0, gt0 + WAVES, ..
    auto issue_remainder = [&](uint4_t (&kt)[U], uint4_t (&vt)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int gt = gt0 + u * WAVES;
            if (gt < ng) {                           // uniform
                const int tb = p0 + gt * RPI;        // (rows past the end repeat row pend - 1: inside the cache, masked by CHECK)
                if (UB) {
                    const int64_t base = block_base(tb);
                    const unsigned lo = (unsigned)(min(tg, pend - 1 - tb) * row_bytes + dc * 16);
                    kt[u] = load16(p.k + base + lo); vt[u] = load16(p.v + base + lo);
                } else {
                    const int64_t off = lane_row(min(tb + tg, pend - 1));
                    kt[u] = load16(p.k + off); vt[u] = load16(p.v + off);
                }
            } else {
                kt[u] = (uint4_t){0u, 0u, 0u, 0u}; vt[u] = (uint4_t){0u, 0u, 0u, 0u};
            }
        }
    };

    uint4_t kt[U], vt[U];
    if (R == 0) issue_remainder(kt, vt);
    for (int r = 0; r < R; ++r) {
        const int tb = p0 + (r * WAVES + wave) * TPI;
        uint4_t kk[U], vv[U];
        if (UB) {
            const int64_t base = block_base(tb);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned lo = (unsigned)((u * RPI + tg) * row_bytes + dc * 16);
                kk[u] = load16(p.k + base + lo); vv[u] = load16(p.v + base + lo);
            }
        } else {
            int64_t off[U];
#pragma unroll
            for (int u = 0; u < U; ++u) off[u] = lane_row(tb + u * RPI + tg);
#pragma unroll
            for (int u = 0; u < U; ++u) { kk[u] = load16(p.k + off[u]); vv[u] = load16(p.v + off[u]); }
        }
        if (r == R - 1) issue_remainder(kt, vt);
        process(std::false_type{}, kk, vv, 0);
    }
    if (gt0 < ng) process(std::true_type{}, kt, vt, p0 + gt0 * RPI);

    // bring the row-group slots of the wave to their common max and sum them, then merge the waves through LDS
    __shared__ float sm_acc[WAVES][G][D];
    __shared__ float sm_ml[WAVES][G][2];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const float M = slots_max<LPR>(m[i]);
        const float w = (m[i] == -INFINITY) ? 0.f : __expf(m[i] - M);
        l[i] = slots_sum<LPR>(l[i] * w);
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = slots_sum<LPR>(acc[i][j] * w);
        if (tg == 0) {
#pragma unroll
            for (int j = 0; j < 16; ++j) sm_acc[wave][i][dc * 16 + j] = acc[i][j];
            if (dc == 0) { sm_ml[wave][i][0] = M; sm_ml[wave][i][1] = l[i]; }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < G * D; idx += WAVES * 64) {
        const int i = idx / D, d = idx % D;
        float M = sm_ml[0][i][0];
#pragma unroll
        for (int w2 = 1; w2 < WAVES; ++w2) M = fmaxf(M, sm_ml[w2][i][0]);
        float o = 0.f, L = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < WAVES; ++w2) {
            const float mw = sm_ml[w2][i][0];
            const float wgt = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            o = fmaf(wgt, sm_acc[w2][i][d], o);
            L = fmaf(wgt, sm_ml[w2][i][1], L);
        }
        o *= p.v_scale;                              // once per (query, head, partition): the merge of the partials is linear in o
        const int64_t row = (int64_t)t * p.H + g * G + i;
        if (direct) {
            p.out[row * D + d] = (half_t)(L > 0.f ? o / L : 0.f);
        } else {
            const int64_t slot = row * p.num_parts + part;
            p.part_o[slot * D + d] = o;
            if (d == 0) { p.part_ml[slot * 2] = M; p.part_ml[slot * 2 + 1] = L; }
        }
    }
}

// merge of the split-KV partials (merge_partitions: attn_merge.h; v_scale is already in them): D/4 threads per (query, head)
template <int D>
__global__ __launch_bounds__(256) void attn_fp8_merge_kernel(const float *__restrict__ part_o, const float *__restrict__ part_ml,
                                                             const int32_t *__restrict__ ctx_lens, int H, int part_size, int num_parts, int part0,
                                                             int kv0, const int32_t *__restrict__ kv0_rows, int64_t pairs, half_t *__restrict__ out) {
    constexpr int TPP = D / 4;
    const int64_t pair = (int64_t)blockIdx.x * (256 / TPP) + threadIdx.x / TPP;
    if (pair >= pairs) return;
    const int t = (int)(pair / H), d = (threadIdx.x % TPP) * 4;
    const int my_kv0 = kv0_rows ? kv0_rows[t] : kv0;
    const int first = (part0 > 0 && my_kv0 == 0) ? part0 : 0;   // a query outside the sharing group has no partials in the shared slots
    const int np = min(num_parts, part0 + (max(ctx_lens[t] - my_kv0, 0) + part_size - 1) / part_size) - first;
    const int64_t base = pair * num_parts + first;
    const half4_t hv = merge_partitions(np,
        [&](int i) { return *reinterpret_cast<const float2_t *>(part_ml + (base + i) * 2); },
        [&](int i) { return *reinterpret_cast<const float4_t *>(part_o + (base + i) * D + d); });
    *reinterpret_cast<half4_t *>(out + pair * D + d) = hv;
}

// ---- work-balanced form ------------------------------------------------------------------------------------------------------------
// The byte-cache counterpart of attention.hip's attn_share_kernel, in the geometry of attn_fp8_kernel above.  The launch is nw workgroups of WAVES waves and the
// WORK is cut evenly: the keys of all (query, kv head) pairs, in units of CH = WAVES * TPI keys (one full round of a workgroup: 128 keys at D = 128, 256 at D = 64,
// i.e. 16 KiB of K and of V either way), pair after pair (query-major), form one line of U_tot units; workgroup w walks the units [w * U_tot / nw, (w + 1) * U_tot / nw)
// — a suffix of one pair, whole pairs, a prefix of another: a SEGMENT each.  A pair inside one share is written directly as 16-bit rows; a pair cut by share
// boundaries leaves one f32 partial per share (v_scale applied; slot = share index - first share of the pair) and the LAST of its shares to take the pair's ticket
// merges them in slot order (merge_partitions) and re-arms the counter.  The next segment is OPENED under the tail of the one in front: its query slice, its
// block-table chunk and its first K / V requests are issued before the current segment's cross-wave merge.  Block size: a power of two >= TPI, so a chunk lies in
// one cache block and its block-table entry is a v_readlane from the 64-entry register copy (reloaded when the walk crosses into the next 64 entries).
// Registers: 119 VGPRs at G = 1, 151-153 at G = 2, 219-220 at G = 4, no scratch: from G = 2 on ONE workgroup is resident per CU (the per-pair kernel: two).
// Holding G = 2 to 128 VGPRs (amdgpu_waves_per_eu) spills 104-132 bytes per lane and loses: profiles/fp8_ragged.txt.
template <int D, int G, int U, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attn_share_fp8_kernel(AttnFp8Params p, unsigned int *tickets, int nq, int nw) {
    constexpr int LPR = D / 16, RPI = 64 / LPR, TPI = RPI * U, CH = TPI * WAVES;
    static_assert(G * D <= WAVES * 64 && G * (D / 4) <= WAVES * 64, "one pass over the (head, column) pairs");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int dc = lane % LPR, tg = lane / LPR;
    __shared__ int pre[1025];                               // pre[t] = units of the queries in front of t (a query's KVH pairs have the same count)
    __shared__ int cx[1024];                                // ctx_lens[t]
    __shared__ float sm_acc[WAVES][G][D];
    __shared__ float sm_ml[WAVES][G][2];
    __shared__ unsigned int ticket_s;
    if (wave == 0) {
        int base = 0;
        for (int k = 0; k < nq; k += 64) {
            const int t = k + lane;
            const int c = t < nq ? p.ctx_lens[t] : 0;
            int un = (c + CH - 1) / CH;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(un, o, 64); if (lane >= o) un += v; }
            if (t < nq) { pre[t + 1] = base + un; cx[t] = c; }
            base += __shfl(un, 63, 64);
        }
        if (lane == 0) pre[0] = 0;
    }
    __syncthreads();
    const long long utot = (long long)p.KVH * pre[nq];
    const long long ub = (long long)blockIdx.x * utot / nw, ue = (long long)(blockIdx.x + 1) * utot / nw;
    // a query without keys owns no unit: its output row is zero, as in attn_fp8_kernel (L == 0)
    for (int t0 = blockIdx.x; t0 < nq; t0 += nw)
        if (cx[t0] == 0)
            for (int x = threadIdx.x; x < p.H * D; x += WAVES * 64) p.out[(int64_t)t0 * p.H * D + x] = (half_t)0.f;
    if (ub >= ue) return;                                   // (fewer units than workgroups: an empty share)
    const int row_bytes = p.KVH * D;

    // ---- state of the segment being streamed (set by `open`, which also REQUESTS its first K / V rows) ----
    int t = 0, g = 0, np = 1, slot = 0, p0 = 0, pend = 0, R = 0, ng = 0, gt0 = 0, bt_chunk = -1, bt_reg = 0;
    const int32_t *bt = p.block_tables;
    half2_t qv[G][8];
    uint4_t k0[U], v0[U], kt[U], vt[U];                     // round 0 of the segment; its remainder groups
    auto load16 = [](const uint8_t *ptr) { return __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(ptr)); };
    auto block_base = [&](int tb) -> int64_t {              // byte offset of (scalar token tb, kv head g, d = 0)
        const int bi = tb >> p.bs_shift, bo = tb & (p.block_size - 1);
        if ((bi >> 6) != bt_chunk) { bt_chunk = bi >> 6; const int idx = (bt_chunk << 6) + lane; bt_reg = idx < p.max_blocks ? bt[idx] : 0; }
        const int blk = __builtin_amdgcn_readlane(bt_reg, bi & 63);
        return (((int64_t)blk * p.block_size + bo) * p.KVH + g) * D;
    };
    auto issue_remainder = [&]() {
#pragma unroll
        for (int x = 0; x < U; ++x) {
            const int gt = gt0 + x * WAVES;
            if (gt < ng) {                                  // uniform
                const int tb = p0 + gt * RPI;               // (rows past the segment's end repeat row pend - 1: a key of this context, masked by CHECK)
                const int64_t base = block_base(tb);
                const unsigned off = (unsigned)(min(tg, pend - 1 - tb) * row_bytes + dc * 16);
                kt[x] = load16(p.k + base + off); vt[x] = load16(p.v + base + off);
            } else {
                kt[x] = (uint4_t){0u, 0u, 0u, 0u}; vt[x] = (uint4_t){0u, 0u, 0u, 0u};
            }
        }
    };
    auto load_round = [&](int r, uint4_t (&kk)[U], uint4_t (&vv)[U]) {
        const int64_t base = block_base(p0 + (r * WAVES + wave) * TPI);
#pragma unroll
        for (int x = 0; x < U; ++x) {
            const unsigned off = (unsigned)((x * RPI + tg) * row_bytes + dc * 16);
            kk[x] = load16(p.k + base + off); vv[x] = load16(p.v + base + off);
        }
    };
    // opens the segment that starts at unit u (u < ue); returns its length in units
    auto open = [&](long long u) -> int {
        int lo = 0, hi = nq;                                // the query of unit u: the last t with KVH * pre[t] <= u (queries without keys own no unit)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((long long)p.KVH * pre[mid] <= u) lo = mid; else hi = mid; }
        t = lo;
        const int ut = pre[t + 1] - pre[t], rem = (int)(u - (long long)p.KVH * pre[t]);
        g = rem / ut;
        const int lu = rem - g * ut, seg = (int)min((long long)(ut - lu), ue - u);
        // shares that touch this pair: unit x belongs to share floor(((x + 1) * nw - 1) / utot)
        const long long S = (long long)p.KVH * pre[t] + (long long)g * ut, E = S + ut - 1;
        const int wf = (int)(((S + 1) * nw - 1) / utot), wl = (int)(((E + 1) * nw - 1) / utot);
        np = wl - wf + 1; slot = (int)blockIdx.x - wf;
        p0 = lu * CH; pend = min(cx[t], (lu + seg) * CH);
        ng = (pend - p0 + RPI - 1) / RPI; R = (pend - p0) / CH; gt0 = R * (WAVES * U) + wave;
        bt = p.block_tables + (int64_t)t * p.max_blocks;
        bt_chunk = (p0 >> p.bs_shift) >> 6;
        { const int idx = (bt_chunk << 6) + lane; bt_reg = idx < p.max_blocks ? bt[idx] : 0; }
        const half_t *qrow = p.q + (int64_t)t * p.ldq + (int64_t)g * G * D + dc * 16;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const half8_t a = *reinterpret_cast<const half8_t *>(qrow + i * D), b = *reinterpret_cast<const half8_t *>(qrow + i * D + 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) { qv[i][j] = (half2_t){a[2 * j], a[2 * j + 1]}; qv[i][4 + j] = (half2_t){b[2 * j], b[2 * j + 1]}; }
        }
        if (R >= 1) load_round(0, k0, v0);
        if (R <= 1) issue_remainder();                      // (requested before the arithmetic of the last full round, as in attn_fp8_kernel)
        asm volatile("" ::: "memory");                      // the requests stay HERE: hipcc would sink them to their first use, behind the tail of the segment in front
        return seg;
    };

    long long u = ub;
    u += open(u);
    for (;;) {
        // online softmax state per head AND per row-group slot of the wave (merged once, at the segment's end)
        float m[G], l[G], acc[G][16];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            m[i] = -INFINITY; l[i] = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
        }
        // attn_fp8_kernel's arithmetic; CHECK: slot x holds token tok0 + x * WAVES * RPI + tg, valid < pend
        auto process = [&](auto check, const uint4_t (&kk)[U], const uint4_t (&vv)[U], int tok0) {
            constexpr bool CHECK = decltype(check)::value;
            float s[U][G];
#pragma unroll
            for (int x = 0; x < U; ++x) {
                const bool valid = !CHECK || tok0 + x * (WAVES * RPI) + tg < pend;
                half2_t kh[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) fp8x4_to_half2(kk[x][j], kh[2 * j], kh[2 * j + 1]);
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    float d = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) d = dot2(kh[j], qv[i][j], d);
                    d = byte_row_sum<LPR>(d);
                    s[x][i] = valid ? d * p.scale : -INFINITY;               // (a NaN byte behind the context ends here)
                }
            }
            float alpha[G], ms[G];
#pragma unroll
            for (int i = 0; i < G; ++i) {
                float mx = s[0][i];
#pragma unroll
                for (int x = 1; x < U; ++x) mx = fmaxf(mx, s[x][i]);
                const float mn = fmaxf(m[i], mx);
                ms[i] = (CHECK && mn == -INFINITY) ? 0.f : mn;               // a slot that has seen no valid token yet
                alpha[i] = __expf(m[i] - ms[i]);
                m[i] = mn;
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[i][j] *= alpha[i];
            }
            float ps[G];
#pragma unroll
            for (int i = 0; i < G; ++i) ps[i] = 0.f;
#pragma unroll
            for (int x = 0; x < U; ++x) {
                float vf[16];                                                // the row's V bytes once for all G heads (rows >= pend repeat row pend - 1 with p = 0)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(vv[x][j], false), b = __builtin_amdgcn_cvt_pk_f32_fp8(vv[x][j], true);
                    vf[4 * j] = a[0]; vf[4 * j + 1] = a[1]; vf[4 * j + 2] = b[0]; vf[4 * j + 3] = b[1];
                }
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    const float pr = __expf(s[x][i] - ms[i]);
                    ps[i] += pr;
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[i][j] = fmaf(pr, vf[j], acc[i][j]);
                }
            }
#pragma unroll
            for (int i = 0; i < G; ++i) l[i] = __fmaf_rn(l[i], alpha[i], ps[i]);
        };
        if (R >= 1) process(std::false_type{}, k0, v0, 0);
        for (int r = 1; r < R; ++r) {
            uint4_t kk[U], vv[U];
            load_round(r, kk, vv);
            if (r == R - 1) issue_remainder();
            process(std::false_type{}, kk, vv, 0);
        }
        if (gt0 < ng) process(std::true_type{}, kt, vt, p0 + gt0 * RPI);

        // the segment is in the accumulators: what its tail needs of the state, then the NEXT segment is opened (its query, block table and first K / V rows
        // are on their way while this one is merged and handed over)
        const int st = t, sg = g, snp = np, sslot = slot;
        const bool more = u < ue;
        if (more) u += open(u);

        // row-group slots of the wave -> the wave's sums; waves -> the segment's partial (attn_fp8_kernel's arithmetic)
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const float M = slots_max<LPR>(m[i]);
            const float w = (m[i] == -INFINITY) ? 0.f : __expf(m[i] - M);
            l[i] = slots_sum<LPR>(l[i] * w);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[i][j] = slots_sum<LPR>(acc[i][j] * w);
            if (tg == 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) sm_acc[wave][i][dc * 16 + j] = acc[i][j];
                if (dc == 0) { sm_ml[wave][i][0] = M; sm_ml[wave][i][1] = l[i]; }
            }
        }
        __syncthreads();
        const int64_t pair0 = ((int64_t)st * p.H + (int64_t)sg * G) * p.num_parts;
        const auto rs_o = __builtin_amdgcn_make_buffer_rsrc(p.part_o + pair0 * D, 0, (int)(G * p.num_parts * D * 4), 0x00020000);
        const auto rs_ml = __builtin_amdgcn_make_buffer_rsrc(p.part_ml + pair0 * 2, 0, (int)(G * p.num_parts * 2 * 4), 0x00020000);
        if (threadIdx.x < G * D) {
            const int i = threadIdx.x / D, d = threadIdx.x % D;
            float M = sm_ml[0][i][0];
#pragma unroll
            for (int w2 = 1; w2 < WAVES; ++w2) M = fmaxf(M, sm_ml[w2][i][0]);
            float o = 0.f, L = 0.f;
#pragma unroll
            for (int w2 = 0; w2 < WAVES; ++w2) {
                const float mw = sm_ml[w2][i][0];
                const float wgt = (mw == -INFINITY) ? 0.f : __expf(mw - M);
                o = fmaf(wgt, sm_acc[w2][i][d], o);
                L = fmaf(wgt, sm_ml[w2][i][1], L);
            }
            o *= p.v_scale;                                                   // once per segment: in front of the division, or of the (linear) merge of the partials
            if (snp == 1) {
                p.out[((int64_t)st * p.H + sg * G + i) * D + d] = (half_t)(L > 0.f ? o / L : 0.f);
            } else {
                const int sl = i * p.num_parts + sslot;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), rs_o, (sl * D + d) * 4, 0, 16);
                if (d == 0) { __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(M), rs_ml, sl * 8, 0, 16);
                              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(L), rs_ml, sl * 8 + 4, 0, 16); }
            }
        }
        if (snp > 1) {                                                        // (workgroup-uniform)
            constexpr int TPH = D / 4;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // every storing wave drains its stores (and the next segment's first rows land) ...
            __syncthreads();
            unsigned int *cnt = tickets + (int64_t)st * p.KVH + sg;
            if (threadIdx.x == 0) ticket_s = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... one ticket
            __syncthreads();
            if (ticket_s == (unsigned)(snp - 1)) {                            // the last of the pair's shares to finish merges it
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");        // keeps the sc1 loads below the ticket
                if (threadIdx.x < G * TPH) {
                    const int i = threadIdx.x / TPH, d = (threadIdx.x % TPH) * 4;
                    const half4_t hv = merge_partitions(snp,
                        [&](int pi) { return __builtin_bit_cast(float2_t, __builtin_amdgcn_raw_buffer_load_b64(rs_ml, (i * p.num_parts + pi) * 8, 0, 16)); },
                        [&](int pi) { return __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_o, ((i * p.num_parts + pi) * D + d) * 4, 0, 16)); });
                    *reinterpret_cast<half4_t *>(p.out + ((int64_t)st * p.H + sg * G + i) * D + d) = hv;
                }
                if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for the next launch
            }
        }
        if (!more) break;
        __syncthreads();                                                      // sm_acc / sm_ml / ticket_s are the next segment's too
    }
}

// block sizes the work-balanced form takes: a power of two >= the chunk of its U = 2 (16 keys at D = 128, 32 at D = 64)
constexpr int SHARE_U = 2;
bool attn_share_fp8_ok(int D, int block_size) {
    return (D == 64 || D == 128) && block_size > 0 && (block_size & (block_size - 1)) == 0 && block_size >= 64 / (D / 16) * SHARE_U;
}

template <int D, int G, int WAVES>
static void launch_fp8_cfg(const AttnFp8Params &p, int64_t nwg, hipStream_t s) {
    constexpr int U = 2, TPI = 64 / (D / 16) * U;                        // 2 KiB of K and of V in flight per wave: 16 tokens at D = 128, 32 at D = 64
    const bool ub = p.block_size % TPI == 0 && (p.num_parts == 1 || p.part_size % TPI == 0);
    dim3 grid((unsigned)nwg), block(WAVES * 64);
    if (ub) attn_fp8_kernel<D, G, U, WAVES, true><<<grid, block, 0, s>>>(p);
    else attn_fp8_kernel<D, G, U, WAVES, false><<<grid, block, 0, s>>>(p);
}

template <int D, int G>
static int launch_attn_fp8(const AttnFp8Args &a, hipStream_t s) {
    AttnFp8Params p{};
    p.q = (const half_t *)a.q; p.ldq = a.ldq; p.k = a.k; p.v = a.v; p.ctx_lens = a.ctx_lens; p.block_tables = a.block_tables;
    p.max_blocks = a.max_blocks; p.block_size = a.block_size;
    p.bs_shift = (a.block_size & (a.block_size - 1)) == 0 ? __builtin_ctz(a.block_size) : -1;
    p.H = a.H; p.KVH = a.KVH; p.scale = a.scale * a.k_scale; p.v_scale = a.v_scale; p.out = (half_t *)a.out;
    // Workgroups: the 16-bit kernel's rule (attention.hip, measured there): eight waves per (query, kv head) when ~256 such workgroups can be
    // given >= 64 keys each, the context cut into 64-key-granular partitions only to reach ~256 workgroups; fewer pairs: four waves and ~1024
    // workgroups; >= 2048 pairs of short contexts: two waves (a workgroup's life is mostly start-up and the cross-wave merge otherwise).
    const int64_t mc = a.max_ctx > 0 ? a.max_ctx : 1, pairs = (int64_t)a.nq * a.KVH, units = (mc + 63) / 64;
    int waves = !a.workspace ? 4 : (pairs >= 2048 && mc <= 512) ? 2 : pairs * units >= 256 ? 8 : 4;
    int64_t ps; int np, sparts = 0, shared_part = 0;
    if (a.shared_len > 0) {
        // The plan of the 16-bit launch (attention.hip): the shared keys [0, shared_len) are cut into sparts equal partitions of 64-key granularity
        // until the MFMA launch has ~256 workgroups; the keys behind them are partitioned like a context of their own (one partition per pair
        // when there are enough pairs, else ~256 workgroups); always merged (np >= 2 keeps the partial format when nobody has own keys yet).
        const int qb = 128 / G;                                           // flash_tile_positions
        const int64_t wgs = (int64_t)((a.nq + qb - 1) / qb) * a.KVH, n64 = a.shared_len / 64;
        int64_t c = std::min<int64_t>(std::max<int64_t>(1, (256 + wgs - 1) / wgs), n64);
        while (n64 % c) --c;
        sparts = (int)c;
        const int64_t rest = std::max<int64_t>(a.shared_rows ? mc : mc - a.shared_len, 64);   // a query outside the group reads its whole context
        // the workspace holds cap partials per (query, head): the shared partitions and the remainder's together must fit
        const int64_t cap = a.workspace_bytes ? (int64_t)(a.workspace_bytes / ((size_t)a.nq * a.H * (D + 2) * sizeof(float))) : units;
        if (cap < 2) return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: workspace too small for the shared-prefix pass");
        while (sparts > 1 && sparts > cap / 2) { --sparts; while (n64 % sparts) --sparts; }
        shared_part = a.shared_len / sparts;
        int64_t want = pairs >= 192 ? 1 : (256 + pairs - 1) / pairs;
        want = std::max<int64_t>(1, std::min<int64_t>(want, cap - sparts));
        ps = ((rest + want - 1) / want + 63) / 64 * 64;
        np = sparts + (int)((rest + ps - 1) / ps);
        // own-key workgroups: two waves when there are >= 2048 of them over short partitions (the rule of the plain launch above), else four
        waves = (pairs * (np - sparts) >= 2048 && ps <= 512) ? 2 : 4;
    } else {
        int64_t want = 1;
        if (a.workspace && waves == 8) want = pairs >= 192 ? 1 : (256 + pairs - 1) / pairs;
        else if (a.workspace && waves == 4) want = (1024 + pairs - 1) / pairs;
        want = std::max<int64_t>(1, std::min(want, units));
        ps = ((mc + want - 1) / want + 63) / 64 * 64;
        np = (int)((mc + ps - 1) / ps);
    }
    // Work-balanced form (attn_share_fp8_kernel), under the 16-bit launch's rule (attention.hip): a pair count whose last round of one-workgroup-per-pair launches
    // would be mostly empty (more pairs than CUs with >= 15 % of the rounds' slots unused, contexts long enough for the stream to matter), a caller's balance_hint
    // (a RAGGED batch: per-pair launches size every pair's partitions by the longest context), or NVR_ATTN_SHARE=2.  NVR_ATTN_SHARE=0: off.
    if constexpr (G * D <= 512)
    if (a.shared_len <= 0 && a.workspace && a.tickets && waves == 8 && attn_share_fp8_ok(D, a.block_size) && a.nq <= 1024 && share_enabled()) {
        constexpr int CH = 8 * 64 / (D / 16) * SHARE_U;                   // keys of a unit
        const int64_t cus = share_workgroups(), rounds = (pairs + cus - 1) / cus;
        const int64_t most = (mc + CH - 1) / CH;                          // a pair has at most this many units, so it meets at most this many shares
        const int64_t cap = a.workspace_bytes ? (int64_t)(a.workspace_bytes / ((size_t)a.nq * a.H * (D + 2) * sizeof(float))) : most;
        const bool by_count = pairs > cus && rounds * cus * 100 >= pairs * 115 && mc >= 256;
        // shares: one per CU for the pair-count case; for ragged batches the caller's count; probes: two per CU, three from 2 pairs per CU on
        const int64_t nw = a.balance_hint > 0 ? a.balance_hint : share_mode() == 2 ? cus * (pairs <= 2 * cus ? 2 : 3) : cus;
        if ((by_count || a.balance_hint > 0 || share_mode() == 2) && pairs < 2048 && cap >= most) {
            p.part_size = CH; p.num_parts = (int32_t)most;                // slots per (query, head): [nq, H, most, D] and [nq, H, most, 2]
            p.part_o = (float *)a.workspace; p.part_ml = p.part_o + (int64_t)a.nq * a.H * most * D;
            attn_share_fp8_kernel<D, G, SHARE_U, 8><<<dim3((unsigned)nw), dim3(512), 0, s>>>(p, a.tickets, (int)a.nq, (int)nw);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "attention_fp8 (work-balanced) launch failed: %s", hipGetErrorString(e));
            return 0;
        }
    }
    if (np > 1) {
        const size_t need = (size_t)a.nq * a.H * np * (D + 2) * sizeof(float);
        if (a.workspace_bytes && need > a.workspace_bytes)
            return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: %d partitions of %d queries x %d heads need %zu workspace bytes, %zu given", np, a.nq, a.H, need,
                             a.workspace_bytes);
        p.part_size = (int)ps; p.num_parts = np;
        p.part_o = (float *)a.workspace; p.part_ml = p.part_o + (int64_t)a.nq * a.H * np * D;
    } else { p.part_size = 0x3fffffff; p.num_parts = 1; }
    p.part0 = sparts; p.kv0 = a.shared_len > 0 ? a.shared_len : 0; p.kv0_rows = a.shared_len > 0 ? a.shared_kv0 : nullptr;
    if (sparts > 0)                                                      // partitions [0, sparts): the whole group's rows on the matrix cores
        if (int rc = flash_shared_prefix_fp8(a.q, a.ldq, a.k, a.v, a.block_tables, a.max_blocks, a.block_size, a.nq, a.H, a.KVH, D, a.scale, a.k_scale, a.v_scale,
                                             shared_part, sparts, np, p.part_o, p.part_ml, s, a.shared_rows, a.shared_count)) return rc;
    const int64_t nwg = (int64_t)(p.num_parts - p.part0) * a.KVH * a.nq;
    if (waves == 8) launch_fp8_cfg<D, G, 8>(p, nwg, s);
    else if (waves == 4) launch_fp8_cfg<D, G, 4>(p, nwg, s);
    else launch_fp8_cfg<D, G, 2>(p, nwg, s);
    if (np > 1) {
        const int64_t rows = (int64_t)a.H * a.nq;
        attn_fp8_merge_kernel<D><<<dim3((unsigned)((rows + 256 / (D / 4) - 1) / (256 / (D / 4)))), dim3(256), 0, s>>>(p.part_o, p.part_ml, a.ctx_lens, a.H, p.part_size,
                                                                                                                   np, p.part0, p.kv0, p.kv0_rows, rows, p.out);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "attention_fp8 launch failed: %s", hipGetErrorString(e));
    return 0;
}

// G = 8 (attn_fp8_mfma_ok): attn_fp8_mfma_kernel (attention_fp8_mfma.hip) on the per-pair plan above — one workgroup per (query, kv head) from 192 pairs on,
// else the context cut to reach ~256 workgroups — except that a partition keeps at least one 64-key step for each of the kernel's 4 waves; partitions
// are whole 64-key steps, at most one per 64 keys of max_ctx (the workspace's cap); split contexts take the merge launch.  shared_len > 0: flash_shared_prefix_fp8
// over the shared keys (partitions 0 .. sparts-1), attn_fp8_mfma_kernel<D, 8, true> over the keys behind them, always merged; never work-balanced.
template <int D>
static int launch_attn_fp8_mfma(const AttnFp8Args &a, hipStream_t s) {
    const int64_t mc = a.max_ctx > 0 ? a.max_ctx : 1, pairs = (int64_t)a.nq * a.KVH, units = (mc + 63) / 64;
    // Work-balanced form (attn_share_fp8_mfma_kernel) under launch_attn_fp8's rule: tickets and a workspace with one slot per 64 keys of max_ctx (a pair meets at
    // most that many workers), then the pair-count case, a caller's balance_hint (workgroups; the kernel derives its worker count from the units), or
    // NVR_ATTN_SHARE=2 (two workgroups per CU: both are resident).  NVR_ATTN_SHARE=0 or no tickets: the per-pair launches below, as before.
    if (a.shared_len <= 0 && a.workspace && a.tickets && a.nq <= 1024 && share_enabled()) {
        const int64_t cus = share_workgroups(), rounds = (pairs + cus - 1) / cus;
        const int64_t cap = a.workspace_bytes ? (int64_t)(a.workspace_bytes / ((size_t)a.nq * a.H * (D + 2) * sizeof(float))) : units;
        const bool by_count = pairs > cus && rounds * cus * 100 >= pairs * 115 && mc >= 256;
        const int64_t nw = a.balance_hint > 0 ? a.balance_hint : share_mode() == 2 ? 2 * cus : cus;
        if ((by_count || a.balance_hint > 0 || share_mode() == 2) && pairs < 2048 && cap >= units) return attn_share_fp8_mfma(a, (int32_t)units, (int32_t)nw, s);
    }
    int64_t want = 1, ps;
    int np, sparts = 0;
    if (a.shared_len > 0) {
        // launch_attn_fp8's plan on this function's rule: the shared keys [0, shared_len) in sparts equal partitions of whole 64-key steps until the
        // tile launch (flash_shared_fp8_kernel<D, 8>: 16 decode rows x 8 heads per workgroup) has ~256 workgroups, at most half the workspace's slots;
        // the keys behind them like a context of their own — one partition per pair from 192 pairs, else towards ~256 workgroups, a partition
        // keeps a 64-key step for each of the 4 waves where there are that many; np >= 2: always merged.
        const int qb = 16;                                                // 128 / G
        const int64_t wgs = (int64_t)((a.nq + qb - 1) / qb) * a.KVH, n64 = a.shared_len / 64;
        int64_t c = std::min<int64_t>(std::max<int64_t>(1, (256 + wgs - 1) / wgs), n64);
        while (n64 % c) --c;
        const int64_t rest = std::max<int64_t>(a.shared_rows ? mc : mc - a.shared_len, 64);   // a query outside the group reads its whole context
        const int64_t cap = a.workspace_bytes ? (int64_t)(a.workspace_bytes / ((size_t)a.nq * a.H * (D + 2) * sizeof(float))) : units;
        if (cap < 2) return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: workspace too small for the shared-prefix pass");
        while (c > 1 && c > cap / 2) { --c; while (n64 % c) --c; }
        sparts = (int)c;
        want = pairs >= 192 ? 1 : (256 + pairs - 1) / pairs;
        want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, (rest + 63) / 64 / 4), cap - sparts));
        ps = ((rest + want - 1) / want + 63) / 64 * 64;
        np = sparts + (int)((rest + ps - 1) / ps);
    } else {
        if (a.workspace) want = pairs >= 192 ? 1 : (256 + pairs - 1) / pairs;
        want = std::max<int64_t>(1, std::min<int64_t>(want, units / 4));
        if (a.workspace_bytes) want = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)(a.workspace_bytes / ((size_t)a.nq * a.H * (D + 2) * sizeof(float)))));
        ps = ((mc + want - 1) / want + 63) / 64 * 64;
        np = (int)((mc + ps - 1) / ps);
    }
    float *part_o = (float *)a.workspace, *part_ml = part_o + (int64_t)a.nq * a.H * np * D;
    if (sparts > 0)                                                      // partitions [0, sparts): the whole group's rows against each 64-key step once per tile
        if (int rc = flash_shared_prefix_fp8(a.q, a.ldq, a.k, a.v, a.block_tables, a.max_blocks, a.block_size, a.nq, a.H, a.KVH, D, a.scale, a.k_scale, a.v_scale,
                                             a.shared_len / sparts, sparts, np, part_o, part_ml, s, a.shared_rows, a.shared_count)) return rc;
    if (int rc = attn_fp8_mfma(a, (int32_t)ps, np, part_o, part_ml, s, sparts)) return rc;
    if (np > 1) {
        const int64_t rows = (int64_t)a.H * a.nq;
        attn_fp8_merge_kernel<D><<<dim3((unsigned)((rows + 256 / (D / 4) - 1) / (256 / (D / 4)))), dim3(256), 0, s>>>(part_o, part_ml, a.ctx_lens, a.H, (int)ps, np, sparts,
                                                                                                                   sparts ? a.shared_len : 0,
                                                                                                                   sparts ? a.shared_kv0 : nullptr, rows, (half_t *)a.out);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "attention_fp8 (merge) launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

int attention_fp8(const AttnFp8Args &a, hipStream_t s) {
    if (a.nq == 0) return 0;
    if (a.KVH <= 0 || a.H % a.KVH) return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: H=%d not a multiple of KVH=%d", a.H, a.KVH);
    if (!(a.k_scale > 0.f) || !(a.v_scale > 0.f)) return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: scales %g / %g (positive)", a.k_scale, a.v_scale);
    const int G = a.H / a.KVH;
    const bool shape_ok = (a.D == 64 || a.D == 128) && (G == 1 || G == 2 || G == 4);
    if (a.shared_len > 0) {                                             // the shared-prefix pass (flash_shared_prefix_fp8 in front of the own-key partitions)
        if (a.block_size <= 0 || a.shared_len % a.block_size || a.shared_len % 64 || !a.workspace)
            return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: shared_len needs a workspace and whole blocks of whole 64-key steps (shared_len %d, block_size %d)",
                             a.shared_len, a.block_size);
        if ((a.shared_rows != nullptr) != (a.shared_kv0 != nullptr) || (a.shared_rows != nullptr) != (a.shared_count != nullptr))
            return nvr::fail(NVR_ERR_INVALID_ARG, "attention_fp8: shared_rows / shared_kv0 / shared_count come together");
        if (!flash_shared_fp8_ok(a.D, a.H, a.KVH, a.block_size))
            return nvr::fail(NVR_ERR_UNSUPPORTED, "attention_fp8: the shared-prefix pass takes D in {64,128}, H/KVH in {1,2,4,8}, block_size a power of two >= 64 "
                             "(D=%d H=%d KVH=%d block_size=%d)", a.D, a.H, a.KVH, a.block_size);
    }
    if (G == 8 && attn_fp8_mfma_ok(a.D, a.H, a.KVH, a.block_size))      // wide groups: the MFMA kernels (per-pair launches, or with tickets and under the rule the work-balanced one)
        return a.D == 128 ? launch_attn_fp8_mfma<128>(a, s) : launch_attn_fp8_mfma<64>(a, s);
    if (!shape_ok || a.block_size < 64 / (a.D / 16))                    // a block holds at least one row group (8 rows at D = 128, 16 at D = 64)
        return nvr::fail(NVR_ERR_UNSUPPORTED, "attention_fp8: unsupported head_dim=%d / group=%d / block_size=%d (D in {64,128}, G in {1,2,4}, block_size >= %d; "
                         "G = 8: block_size a power of two >= 64)", a.D, G, a.block_size, shape_ok ? 64 / (a.D / 16) : 8);
#define NVR_ATTN8_CASE(DD, GG) if (a.D == DD && G == GG) return launch_attn_fp8<DD, GG>(a, s);
    NVR_ATTN8_CASE(128, 1) NVR_ATTN8_CASE(128, 2) NVR_ATTN8_CASE(128, 4) NVR_ATTN8_CASE(64, 1) NVR_ATTN8_CASE(64, 2) NVR_ATTN8_CASE(64, 4)
#undef NVR_ATTN8_CASE
    return NVR_ERR_UNSUPPORTED;
}

}}  // namespace nvr::k / nvr::kb (NVR_DT_NS)

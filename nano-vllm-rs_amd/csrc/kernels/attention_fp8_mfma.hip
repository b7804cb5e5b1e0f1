// attention_fp8_mfma.hip — paged decode attention over the FP8 (OCP e4m3fn) KV cache for WIDE query groups (G = H/KVH = 8) on the matrix cores.
// Semantics: attention_fp8.hip's (query t sees exactly ctx_lens[t] keys, K = k_scale * e4m3(byte), V = v_scale * e4m3(byte), f32 online softmax,
// output in the build's 16-bit type).  attn_fp8_kernel does its arithmetic on the VALU and is conversion / FMA bound from G = 2 on; here the G heads
// of ONE query are the N columns of the 16-bit 16x16x32 MFMAs (padded to 16: columns >= G are fed head G - 1 and never stored — the matrix pipe is
// idle in an HBM-bound decode step) and the VALU is left with the byte conversions and the softmax.
//
// Work split.  Workgroup = 4 waves = (query, kv head, partition), grid and split-KV partials exactly as attn_fp8_kernel (part_o [nq·H·np][D] f32 sums
// x v_scale, part_ml = maximum x softmax scale x k_scale and the sum of the 16-bit-rounded probabilities; merged by attn_fp8_merge_kernel).  The KEYS
// are split over the waves: a partition is whole 64-key steps and wave w walks steps w, w + 4, ... on its own — no workgroup barrier inside the
// stream; every wave orders its own requests with its own vmcnt waits.  The query side sits on the lane in both products, as in flash_prefill_fp8.hip:
//   Sᵀ = K·Qᵀ   A = 16 keys x 32 d of K (bytes -> 16-bit in registers, v_cvt_scalef32_pk_f16_fp8 / _bf16_fp8 at scale 1.0: exact), B = Qᵀ (not quantised,
//               loaded once per workgroup into registers);
//   Oᵀ += Vᵀ·Pᵀ A = ds_read_b64_tr_b8 fragments of the V byte image, B = the lane's exp'd Sᵀ accumulators rounded to 16 bits; the row sums come from
//               an all-ones A.  The rounding points are those of the prefill / shared kernels, so the project's MFMA-attention bound applies.
// Key <-> MFMA row and the V swizzle are flash_prefill_fp8.hip's (its header comment): row ρ of Sᵀ tile mt is key 32·(mt/2) + 8·(ρ/4) +
// 4·(mt%2) + ρ%4 of the step; V image chunk c of key k at chunk c ^ v8_swz(k).
//
// K path: STRAIGHT FROM GLOBAL MEMORY, no LDS.  The A fragment of lane (r = lane % 16, g4 = lane / 16) is 8 consecutive d of key row r, so one
// 16-byte request per lane (chunk g4 + 4·j of the row, j < D/64: the four lane groups of a row read 64 contiguous bytes) is TWO fragments: its
// low and high 8 bytes feed two MFMAs whose k-slot (g4, i) stands for d = 16·(g4 + 4·j) + 8·half + i, and the Q fragments are loaded in that same
// permutation (the Wq layout of linear_fp8.hip).  Chosen over staging K as the prefill kernel does because K is read once by one wave
// here (the prefill tile shares a step's K among 4 waves; a decode wave would write and read back its own bytes), and because it halves the ring:
// V only, 2 slots x 64·D bytes per wave = 64 KiB per workgroup at D = 128 (32 KiB at D = 64), so TWO workgroups are resident per CU (LDS-bound at
// D = 128: 160 KiB; 241 VGPRs, two waves per SIMD; D = 64: 161 VGPRs, three workgroups; no scratch) where a K + V ring would leave one at D = 128.
// The ring is not deepened: one step (K in registers, V in LDS: 16 KiB per wave at D = 128) is in flight behind the one being computed.
// Order of requests.  K rows are PLAIN loads, so the compiler owns their registers and waits (as asm loads into tied registers they were copied by
// the register allocator while in flight); the V pieces are glds_pieces' asm, which its wait counting does not see, and loads return in order.  So per
// step: K(i + 1) is requested, Sᵀ(i) is computed (the compiler waits for K(i) there, allowing the NP loads of K(i + 1)), then V(i + 1) is requested,
// then Oᵀ(i).  V(i) sits between K(i) and K(i + 1) in the queue: a hand-written vmcnt(NP) behind Sᵀ(i) (0 at the wave's last step) states that it has
// landed and fences the LDS reads; the compiler's own wait for K(i + 1), one step later, never covers a request younger than K(i + 2).
//
// Bytes behind a context: the last step of a partition clamps its K and V rows to the last visible key (never READ: a NaN code times a zero
// probability is NaN inside an MFMA), scores are masked by key INDEX, block-table entries past the context are not dereferenced.
// Behind a shared prefix (OWN = true, a compile-time variant: the plain instantiation keeps its instructions): attn_fp8_kernel's part0 / kv0 / kv0_rows.  Slots
// 0 .. part0-1 of a (query, head) belong to flash_shared_prefix_fp8 (flash_prefill_fp8.hip: the group's rows against the shared keys once per 16-row tile); this
// launch has num_parts - part0 partitions per pair, partition part0 + i = keys [kv0_t + i·part_size, ..) with kv0_t = kv0_rows[t] or kv0 — a multiple of 64, so
// a step still lies inside one block — and always leaves partials.  A member without own keys and a non-member shorter than a partition return as empty partitions.
// End: the waves' (max, sum, Oᵀ) meet in LDS (each wave's own, drained ring) and are merged in wave order 0..3; a wave without a step contributes
// (-inf, 0, 0) with weight 0; a query without keys writes a zero row; the order is fixed, so two launches agree bit for bit.
#include <type_traits>
#include "kernels.h"
#include "device_utils.h"
#include "flash_common.h"
#include "attn_merge.h"
#include "../common.h"

namespace nvr { namespace NVR_DT_NS {

typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));

struct AttnFp8MfmaParams {
    const half_t *q; int64_t ldq;
    const uint8_t *k, *v;
    const int32_t *ctx_lens, *block_tables;
    int32_t max_blocks, block_size, bs_shift;
    int32_t H, KVH;
    float scale;                       // softmax scale x k_scale
    float v_scale;
    int32_t part_size, num_parts;      // part_size: a multiple of the 64-key step
    float *part_o, *part_ml;           // [nq, H, num_parts, D], [nq, H, num_parts, 2]
    half_t *out;                       // [nq, H, D]
};
// OWN: the keys behind a shared prefix (attn_fp8_kernel's fields of the same names): partitions 0..part0-1 hold the group's shared keys [0, kv0), written
// by flash_shared_prefix_fp8; the launch covers partition part0 + i = keys [kv0_t + i*part_size, ..) of query t and always leaves partials
struct AttnFp8MfmaOwnParams : AttnFp8MfmaParams {
    int32_t part0, kv0;
    const int32_t *kv0_rows;           // per-query kv0 (a group inside the batch: members shared_len, others 0) or null = kv0 for all
};

template <int D, int G, bool OWN>
__global__ __launch_bounds__(256, 2) void attn_fp8_mfma_kernel(std::conditional_t<OWN, AttnFp8MfmaOwnParams, AttnFp8MfmaParams> p) {
    static_assert(G >= 1 && G <= 16 && (D == 64 || D == 128), "the G heads of a kv head are the 16 columns of one MFMA");
    constexpr int KT = 64, WAVES = 4;            // keys per step; waves per workgroup
    constexpr int CPR = D / 16;                  // 16-byte chunks per row
    constexpr int NJ = D / 64;                   // 16-byte K requests per lane and 16-key tile
    constexpr int NMT = KT / 16, NK2 = KT / 32, NDT = D / 16;
    constexpr int OPB = KT * D;                  // bytes of a step's V image
    constexpr int NP = OPB / 1024;               // 1 KiB pieces (wave-instructions) of it = K requests per lane and step
    constexpr int WRING = 2 * OPB;               // a wave's ring
    static_assert((G * D + 2 * G) * 4 <= WRING, "the wave's partial fits its drained ring");
    __shared__ __attribute__((aligned(16))) char smem[WAVES * WRING];

    int lparts = p.num_parts;                        // partitions of this launch
    if constexpr (OWN) lparts -= p.part0;
    int part = blockIdx.x % lparts;
    const int g = (blockIdx.x / lparts) % p.KVH;
    const int t = blockIdx.x / (lparts * p.KVH);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r = lane & 15, g4 = lane >> 4;
    const bool direct = !OWN && p.num_parts == 1;
    int p0 = part * p.part_size;
    if constexpr (OWN) {                             // (kv0: a multiple of 64, so a 64-key step still lies inside one block)
        p0 += p.kv0_rows ? __builtin_amdgcn_readfirstlane(p.kv0_rows[t]) : p.kv0;
        part += p.part0;
    }

    // register copy of 64 block-table entries (lane j holds entry 64·c + j) by a load that waits for itself (flash_prefill_fp8.hip)
    int bt_reg = 0, bt_chunk = -1;
    auto load_bt_chunk = [&](int c) {
        bt_chunk = c;
        const int idx = min((c << 6) + lane, p.max_blocks - 1);                  // (entries past the context are never selected)
        const int32_t *src = p.block_tables + (int64_t)t * p.max_blocks + idx;
        asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(bt_reg) : "v"(src) : "memory");
    };

    // Qᵀ fragments in the permutation of the K requests: qf[j][h] = head min(r, G - 1), d = 64·j + 16·g4 + 8·h .. +7
    half8_t qf[NJ][2];
    {
        const half_t *qptr = p.q + (int64_t)t * p.ldq + (int64_t)(g * G + min(r, G - 1)) * D + g4 * 16;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) qf[j][h] = *reinterpret_cast<const half8_t *>(qptr + j * 64 + h * 8);
    }
    const int ctx = p.ctx_lens[t];
    if (p0 >= ctx && !direct) return;                // empty partition: the merge skips it too (workgroup-uniform)
    const int pend = min(ctx, p0 + p.part_size);
    const int nsteps = (pend - p0 + KT - 1) / KT;    // 64-key steps of this partition, the last one possibly partial; wave w: steps w, w + 4, ..
    const int row_bytes = p.KVH * D;
    if (wave < nsteps) load_bt_chunk(((p0 + wave * KT) >> p.bs_shift) >> 6);
    // everything the compiler knows to be in flight lands HERE, in front of the first hand-counted request
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) asm volatile("" :: "v"(qf[j][h]));

    // lane constants of a step's requests.  K: tile mt is rows krow + 32·(mt/2) + 4·(mt%2), chunk g4 (+ 4·j by the instruction offset).
    // V: piece i is LDS bytes [1024·i, +1024) of the image, lane l at 16·l: row i·(64/CPR) + l/CPR, LDS chunk l%CPR <- source chunk ^ v8_swz(row)
    const int krow = (r >> 2) * 8 + (r & 3);
    const int vrow0 = lane / CPR, vchunk = lane % CPR;
    const unsigned lds_wave = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem + (unsigned)wave * WRING;

    // the 64-key step at kt lies inside ONE cache block (block_size is a power of two >= 64): byte offset of its first row for kv head g, and how
    // many rows behind the first are visible (rows past the last visible key repeat that key's)
    struct StepAt { int64_t sbase; int lim; };
    auto step_at = [&](int kt) -> StepAt {
        const int bi = kt >> p.bs_shift;                                        // kt < pend <= ctx: an entry of the context
        if ((bi >> 6) != bt_chunk) load_bt_chunk(bi >> 6);
        const int64_t row0 = (int64_t)__builtin_amdgcn_readlane(bt_reg, bi & 63) * p.block_size + (kt & (p.block_size - 1));
        return {(row0 * p.KVH + g) * D, pend - 1 - kt};
    };
    auto load_k = [&](uint4_t (&kr)[NMT][NJ], const StepAt &at) {              // plain loads: the compiler waits for them where they are used
        const uint8_t *kbase = p.k + at.sbase;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            const unsigned ko = (unsigned)(min(krow + (mt >> 1) * 32 + (mt & 1) * 4, at.lim) * row_bytes + g4 * 16);
#pragma unroll
            for (int j = 0; j < NJ; ++j) kr[mt][j] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(kbase + ko + j * 64));
        }
    };
    auto stage_v = [&](int slot, const StepAt &at) {                             // LDS-DMA, invisible to the compiler's wait counting
        const uint8_t *vsrc[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int row = i * (64 / CPR) + vrow0;
            vsrc[i] = p.v + at.sbase + (unsigned)(min(row, at.lim) * row_bytes + ((vchunk ^ v8_swz<D>(row)) << 4));
        }
        glds_pieces<NP, 1024>(vsrc, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_wave + slot * OPB)));
    };
    // The V image of the step whose scores were just computed has landed: its pieces are older than the NP K loads of the step behind it (if one was
    // requested: `more`), and loads return in order.  Also the fence that keeps the compiler's LDS reads of that image behind this point.
    auto v_landed = [&](bool more) {
        if (more) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    // softmax on RAW scores as in the prefill kernel: m = running max of q·k, p = 2^((s - m)·c2), sums from the matrix core (all-ones A)
    float4_t o[NDT], ol = {0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NDT; ++i) o[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    const float c2 = p.scale * 1.44269504088896340736f;
    half8_t ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (half_t)1.0f;
    const int vrow = g4 * 8 + (r >> 1);                              // key of the 8-byte piece this lane addresses - 32·k2
    const int vxor = v8_swz<D>(vrow);
    const int voff = vrow * D + ((r & 1) << 3);

    // the step at kt: K in kr, V image in ring slot `slot`; `more`: the K rows of the step at `next` are already requested, its V image follows the scores
    auto compute = [&](int slot, const uint4_t (&kr)[NMT][NJ], int kt, bool more, const StepAt &next) {
        const char *vl = smem + wave * WRING + slot * OPB;
        float4_t s[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            s[mt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) s[mt] = mfma16(fp8x8_to_half8(kr[mt][j][2 * h], kr[mt][j][2 * h + 1]), qf[j][h], s[mt]);
        }
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) asm volatile("" : "+v"(s[mt]));        // the K rows are consumed: the other slot and the next V image can go
        v_landed(more);
        if (more) stage_v(slot ^ 1, next);
        // by key INDEX; accumulator e of tile mt holds key kt + 32·(mt/2) + 8·g4 + 4·(mt%2) + e.  Only the partition's last step has such keys.
        if (kt + KT > pend) {
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kt + (mt >> 1) * 32 + g4 * 8 + (mt & 1) * 4 + e >= pend) s[mt][e] = -INFINITY;
        }
        float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
        for (int mt = 1; mt < NMT; ++mt) mx = fmaxf(fmaxf(mx, s[mt][0]), fmaxf(fmaxf(s[mt][1], s[mt][2]), s[mt][3]));
        mx = max_over_rows(mx);
        const float mn = fmaxf(m, mx);                             // finite: key kt < pend is visible to every column
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
        const bool moved = mn != m;
        m = mn;
        const float mc = -mn * c2;
        half8_t pf[NK2];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) pf[mt >> 1][(mt & 1) * 4 + e] = (half_t)__builtin_amdgcn_exp2f(fmaf(s[mt][e], c2, mc));   // k-slot (g4, j): key 32·k2 + 8·g4 + j
        if (__any(moved)) {                                        // wave-uniform: the running max settles after a few steps
            ol *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
        }
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) {
            ol = mfma16(ones, pf[k2], ol);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const int2_t vb = lds_read_tr8(vl + k2 * 32 * D + voff + ((dt ^ vxor) << 4));
                o[dt] = mfma16(fp8x8_to_half8((unsigned)vb[0], (unsigned)vb[1]), pf[k2], o[dt]);
            }
        }
    };

    uint4_t ka[NMT][NJ], kb[NMT][NJ];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int j = 0; j < NJ; ++j) { ka[mt][j] = (uint4_t){0u, 0u, 0u, 0u}; kb[mt][j] = (uint4_t){0u, 0u, 0u, 0u}; }
    // Ring slot and register set are compile-time constants, and the K loads of the step behind are never issued under a condition of their own: where
    // two paths meet, hipcc's wait for K(i) assumes the path WITHOUT them and drains K(i + 1) too.
    if (wave < nsteps) {
        StepAt at = step_at(p0 + wave * KT);
        stage_v(0, at); load_k(ka, at);
        for (int st = wave;;) {
            if (st + WAVES >= nsteps) { compute(0, ka, p0 + st * KT, false, at); break; }
            at = step_at(p0 + (st + WAVES) * KT); load_k(kb, at);
            compute(0, ka, p0 + st * KT, true, at);
            st += WAVES;
            if (st + WAVES >= nsteps) { compute(1, kb, p0 + st * KT, false, at); break; }
            at = step_at(p0 + (st + WAVES) * KT); load_k(ka, at);
            compute(1, kb, p0 + st * KT, true, at);
            st += WAVES;
        }
    }

    // this wave's requests have all landed and its LDS reads are consumed: its ring is free for its partial [G][D] f32 + [G][2]
    float *wo = reinterpret_cast<float *>(smem + wave * WRING);
    if (r < G) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) *reinterpret_cast<float4_t *>(wo + r * D + dt * 16 + g4 * 4) = o[dt];   // accumulator e: d = 16·dt + 4·g4 + e
        if (g4 == 0) { wo[G * D + 2 * r] = m; wo[G * D + 2 * r + 1] = ol[0]; }                                     // every row of the ones-product holds the sum
    }
    __syncthreads();
    if (threadIdx.x < G * (D / 4)) {
        const int i = threadIdx.x / (D / 4), d = (threadIdx.x % (D / 4)) * 4;
        float mw[WAVES], M = -INFINITY;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { mw[w] = reinterpret_cast<const float *>(smem + w * WRING)[G * D + 2 * i]; M = fmaxf(M, mw[w]); }
        float4_t acc = {0.f, 0.f, 0.f, 0.f};
        float L = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {                          // wave order 0..3, fused multiply-adds spelled out (attn_merge.h)
            const float *pw = reinterpret_cast<const float *>(smem + w * WRING);
            const float wgt = (mw[w] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mw[w] - M) * c2);
            const float4_t ow = *reinterpret_cast<const float4_t *>(pw + i * D + d);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(wgt, ow[e], acc[e]);
            L = __fmaf_rn(wgt, pw[G * D + 2 * i + 1], L);
        }
        acc *= p.v_scale;                                           // once per (query, head, partition): the merge of the partials is linear in it
        const int64_t row = (int64_t)t * p.H + g * G + i;
        if (direct) {
            half4_t hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)(L > 0.f ? acc[e] / L : 0.f);
            *reinterpret_cast<half4_t *>(p.out + row * D + d) = hv;
        } else {
            const int64_t slot = row * p.num_parts + part;
            *reinterpret_cast<float4_t *>(p.part_o + slot * D + d) = acc;
            if (d == 0) { p.part_ml[slot * 2] = M * p.scale; p.part_ml[slot * 2 + 1] = L; }
        }
    }
}

// ---- work-balanced form ------------------------------------------------------------------------------------------------------------
// The data path above on another work split: ONE SHARE PER WAVE.  The four waves of attn_fp8_mfma_kernel never meet inside the key stream (own V ring, own K
// registers, own vmcnt waits), so here they do not meet at all.  Unit = one 64-key step; query t owns ceil(ctx_lens[t] / 64) units per kv head and the units of all
// (query, kv head) pairs, query-major, form one line of U_tot units (attn_share_fp8_kernel's prefix table pre[] / cx[] in LDS, built by wave 0: the barrier behind
// it is the only one of the kernel).  The launch is nw workgroups = W = 4·nw workers; W_eff = clamp(U_tot / 4, 1, W) of them (numbered wave·nw + workgroup) — derived here, from ctx_lens and
// nw alone, so an eager step and a replayed graph cut alike — walk units [w·U_tot / W_eff, (w + 1)·U_tot / W_eff): no share is empty, so the number of workers a
// pair meets (np = last - first + 1) is exact, and no share is shorter than four steps unless the whole line is.  A share is a suffix of one pair, whole pairs, a
// prefix of another: a SEGMENT each, streamed by the per-pair kernel's wave loop with stride 1.  A pair inside one share (np == 1) is normalised and written from
// the accumulators; a cut pair leaves one f32 partial per worker (the per-pair launch's units; slot = worker - first worker of the pair), the worker drains its
// stores and takes the pair's ticket (release / acquire as in attn_share_fp8_kernel; one lane takes it, the wave reads it by v_readfirstlane), and the last arriver
// merges the np partials in slot order (merge_partitions), writes the rows and re-arms the counter: two launches agree bit for bit.
// Segment boundary: stores count in vmcnt on gfx950, so the tail's row / partial stores would stand in the same queue as the next segment's hand-counted requests.
// The boundary DRAINS (vmcnt(0) behind the tail; the next segment's Q and block-table chunk land by load_bt_chunk's own wait) — the next segment is not opened
// under the tail.  Workers >= W_eff only take part in the zero rows (queries without keys, dealt over the workgroups).
template <int D, int G>
__global__ __launch_bounds__(256, 2) void attn_share_fp8_mfma_kernel(AttnFp8MfmaParams p, unsigned int *tickets, int nq) {
    static_assert(G >= 1 && G <= 16 && (D == 64 || D == 128), "the G heads of a kv head are the 16 columns of one MFMA");
    constexpr int KT = 64, WAVES = 4;
    constexpr int CPR = D / 16, NJ = D / 64, NMT = KT / 16, NK2 = KT / 32, NDT = D / 16;
    constexpr int OPB = KT * D, NP = OPB / 1024, WRING = 2 * OPB;
    __shared__ __attribute__((aligned(16))) char smem[WAVES * WRING];
    __shared__ int pre[1025];                               // pre[t] = units of the queries in front of t (a query's KVH pairs have the same count)
    __shared__ int cx[1024];                                // ctx_lens[t]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r = lane & 15, g4 = lane >> 4;
    const int nw = gridDim.x;
    if (wave == 0) {
        int base = 0;
        for (int k = 0; k < nq; k += 64) {
            const int tq = k + lane;
            const int c = tq < nq ? p.ctx_lens[tq] : 0;
            int un = (c + KT - 1) / KT;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(un, o, 64); if (lane >= o) un += v; }
            if (tq < nq) { pre[tq + 1] = base + un; cx[tq] = c; }
            base += __shfl(un, 63, 64);
        }
        if (lane == 0) pre[0] = 0;
    }
    __syncthreads();
    // a query without keys owns no unit: its output row is zero, as in attn_fp8_mfma_kernel
    for (int t0 = blockIdx.x; t0 < nq; t0 += nw)
        if (cx[t0] == 0)
            for (int x = threadIdx.x; x < p.H * D; x += WAVES * 64) p.out[(int64_t)t0 * p.H * D + x] = (half_t)0.f;
    const int utot = p.KVH * __builtin_amdgcn_readfirstlane(pre[nq]);            // (< 2^31: the launch checks pairs x slots)
    const int W_eff = max(1, min(utot / 4, WAVES * nw));
    const int worker = wave * nw + (int)blockIdx.x;         // interleaved over the workgroups: W_eff < W leaves waves idle in EVERY workgroup, not whole CUs
    if (worker >= W_eff) return;
    const int ub = (int)((long long)worker * utot / W_eff), ue = (int)((long long)(worker + 1) * utot / W_eff);
    if (ub >= ue) return;                                   // (no unit at all: every query is a zero row)
    const int row_bytes = p.KVH * D;

    // ---- state of the segment being streamed: wave-uniform (SGPRs) ----
    int t = 0, g = 0, np = 1, slot = 0, p0 = 0, pend = 0, nsteps = 0;
    int bt_reg = 0, bt_chunk = -1;
    auto load_bt_chunk = [&](int c) {                        // 64 block-table entries of query t (lane j: entry 64·c + j) by a load that waits for itself — and for
        bt_chunk = c;                                        // everything older: the segment's Q fragments, the stores of the segment in front
        const int idx = min((c << 6) + lane, p.max_blocks - 1);
        const int32_t *src = p.block_tables + (int64_t)t * p.max_blocks + idx;
        asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(bt_reg) : "v"(src) : "memory");
    };
    half8_t qf[NJ][2];                                       // Qᵀ fragments of the segment's pair in the permutation of the K requests

    // lane constants of a step's requests and of the V reads (attn_fp8_mfma_kernel)
    const int krow = (r >> 2) * 8 + (r & 3);
    const int vrow0 = lane / CPR, vchunk = lane % CPR;
    const unsigned lds_wave = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem + (unsigned)wave * WRING;
    struct StepAt { int64_t sbase; int lim; };
    auto step_at = [&](int kt) -> StepAt {                  // kt < pend <= ctx: an entry of the context
        const int bi = kt >> p.bs_shift;
        if ((bi >> 6) != bt_chunk) load_bt_chunk(bi >> 6);
        const int64_t row0 = (int64_t)__builtin_amdgcn_readlane(bt_reg, bi & 63) * p.block_size + (kt & (p.block_size - 1));
        return {(row0 * p.KVH + g) * D, pend - 1 - kt};
    };
    auto load_k = [&](uint4_t (&kr)[NMT][NJ], const StepAt &at) {              // plain loads: the compiler waits for them where they are used
        const uint8_t *kbase = p.k + at.sbase;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            const unsigned ko = (unsigned)(min(krow + (mt >> 1) * 32 + (mt & 1) * 4, at.lim) * row_bytes + g4 * 16);
#pragma unroll
            for (int j = 0; j < NJ; ++j) kr[mt][j] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(kbase + ko + j * 64));
        }
    };
    auto stage_v = [&](int vslot, const StepAt &at) {                            // LDS-DMA, invisible to the compiler's wait counting
        const uint8_t *vsrc[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int row = i * (64 / CPR) + vrow0;
            vsrc[i] = p.v + at.sbase + (unsigned)(min(row, at.lim) * row_bytes + ((vchunk ^ v8_swz<D>(row)) << 4));
        }
        glds_pieces<NP, 1024>(vsrc, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_wave + vslot * OPB)));
    };
    auto v_landed = [&](bool more) {
        if (more) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    float4_t o[NDT], ol;
    float m;
    const float c2 = p.scale * 1.44269504088896340736f;
    half8_t ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (half_t)1.0f;
    const int vrow = g4 * 8 + (r >> 1);
    const int vxor = v8_swz<D>(vrow);
    const int voff = vrow * D + ((r & 1) << 3);

    // the step at kt (attn_fp8_mfma_kernel's arithmetic): K in kr, V image in ring slot vslot; `more`: the K rows of the step at `next` are requested
    auto compute = [&](int vslot, const uint4_t (&kr)[NMT][NJ], int kt, bool more, const StepAt &next) {
        const char *vl = smem + wave * WRING + vslot * OPB;
        float4_t s[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            s[mt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) s[mt] = mfma16(fp8x8_to_half8(kr[mt][j][2 * h], kr[mt][j][2 * h + 1]), qf[j][h], s[mt]);
        }
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) asm volatile("" : "+v"(s[mt]));
        v_landed(more);
        if (more) stage_v(vslot ^ 1, next);
        if (kt + KT > pend) {                                      // only a segment's last step, where it ends the context
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kt + (mt >> 1) * 32 + g4 * 8 + (mt & 1) * 4 + e >= pend) s[mt][e] = -INFINITY;
        }
        float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
        for (int mt = 1; mt < NMT; ++mt) mx = fmaxf(fmaxf(mx, s[mt][0]), fmaxf(fmaxf(s[mt][1], s[mt][2]), s[mt][3]));
        mx = max_over_rows(mx);
        const float mn = fmaxf(m, mx);                             // finite: key kt < pend is visible to every column
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
        const bool moved = mn != m;
        m = mn;
        const float mc = -mn * c2;
        half8_t pf[NK2];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) pf[mt >> 1][(mt & 1) * 4 + e] = (half_t)__builtin_amdgcn_exp2f(fmaf(s[mt][e], c2, mc));
        if (__any(moved)) {
            ol *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
        }
#pragma unroll
        for (int k2 = 0; k2 < NK2; ++k2) {
            ol = mfma16(ones, pf[k2], ol);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const int2_t vb = lds_read_tr8(vl + k2 * 32 * D + voff + ((dt ^ vxor) << 4));
                o[dt] = mfma16(fp8x8_to_half8((unsigned)vb[0], (unsigned)vb[1]), pf[k2], o[dt]);
            }
        }
    };

    uint4_t ka[NMT][NJ], kb[NMT][NJ];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int j = 0; j < NJ; ++j) { ka[mt][j] = (uint4_t){0u, 0u, 0u, 0u}; kb[mt][j] = (uint4_t){0u, 0u, 0u, 0u}; }

    for (int u = ub; u < ue;) {
        // ---- open the segment that starts at unit u ----
        {
            int lo = 0, hi = nq;                            // the query of unit u: the last t with KVH * pre[t] <= u (queries without keys own no unit)
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.KVH * __builtin_amdgcn_readfirstlane(pre[mid]) <= u) lo = mid; else hi = mid; }
            t = lo;
            const int pt = __builtin_amdgcn_readfirstlane(pre[t]), ut = __builtin_amdgcn_readfirstlane(pre[t + 1]) - pt;
            const int rem = u - p.KVH * pt;
            g = rem / ut;
            const int lu = rem - g * ut, seg = min(ut - lu, ue - u);
            // workers that touch this pair: unit x belongs to worker floor(((x + 1) * W_eff - 1) / utot)
            const int S = p.KVH * pt + g * ut;          // the pair's first unit; its last: S + ut - 1
            const int wf = (int)(((long long)(S + 1) * W_eff - 1) / utot), wl = (int)(((long long)(S + ut) * W_eff - 1) / utot);
            np = wl - wf + 1; slot = worker - wf;
            p0 = lu * KT; pend = min(__builtin_amdgcn_readfirstlane(cx[t]), (lu + seg) * KT); nsteps = seg;
            u += seg;
        }
        {
            const half_t *qptr = p.q + (int64_t)t * p.ldq + (int64_t)(g * G + min(r, G - 1)) * D + g4 * 16;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) qf[j][h] = *reinterpret_cast<const half8_t *>(qptr + j * 64 + h * 8);
        }
        load_bt_chunk((p0 >> p.bs_shift) >> 6);
        // everything the compiler knows to be in flight lands HERE, in front of the first hand-counted request
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) asm volatile("" :: "v"(qf[j][h]));
        m = -INFINITY; ol = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NDT; ++i) o[i] = (float4_t){0.f, 0.f, 0.f, 0.f};

        // ---- stream its steps: ring slot and register set are compile-time constants, no K load under a condition of its own ----
        {
            StepAt at = step_at(p0);
            stage_v(0, at); load_k(ka, at);
            for (int st = 0;;) {
                if (st + 1 >= nsteps) { compute(0, ka, p0 + st * KT, false, at); break; }
                at = step_at(p0 + (st + 1) * KT); load_k(kb, at);
                compute(0, ka, p0 + st * KT, true, at);
                st += 1;
                if (st + 1 >= nsteps) { compute(1, kb, p0 + st * KT, false, at); break; }
                at = step_at(p0 + (st + 1) * KT); load_k(ka, at);
                compute(1, kb, p0 + st * KT, true, at);
                st += 1;
            }
        }

        // ---- its end: lane r < G holds head r (accumulator e of o[dt]: d = 16·dt + 4·g4 + e; every row of the ones-product holds the sum) ----
        const int64_t row0 = (int64_t)t * p.H + (int64_t)g * G;
        const float L = ol[0];
        if (np == 1) {
            if (r < G) {
                half_t *orow = p.out + (row0 + r) * D + g4 * 4;
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const float4_t acc = o[dt] * p.v_scale;
                    half4_t hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (half_t)(L > 0.f ? acc[e] / L : 0.f);
                    *reinterpret_cast<half4_t *>(orow + dt * 16) = hv;
                }
            }
        } else {
            const auto rs_o = __builtin_amdgcn_make_buffer_rsrc(p.part_o + row0 * p.num_parts * D, 0, (int)(G * p.num_parts * D * 4), 0x00020000);
            const auto rs_ml = __builtin_amdgcn_make_buffer_rsrc(p.part_ml + row0 * p.num_parts * 2, 0, (int)(G * p.num_parts * 2 * 4), 0x00020000);
            if (r < G) {
                const int sl = r * p.num_parts + slot;
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, o[dt] * p.v_scale), rs_o, (sl * D + dt * 16 + g4 * 4) * 4, 0, 16);
                if (g4 == 0) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(uint2_t, (float2_t){m * p.scale, L}), rs_ml, sl * 8, 0, 16);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the wave's partial is out ...
            unsigned int *cnt = tickets + (int64_t)t * p.KVH + g;
            unsigned int tk = 0;
            if (lane == 0) tk = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                  // ... one ticket
            tk = (unsigned)__builtin_amdgcn_readfirstlane((int)tk);
            if (tk == (unsigned)(np - 1)) {                                   // the last of the pair's workers to finish merges it
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");        // keeps the sc1 loads below the ticket
                constexpr int TPH = D / 4;
                for (int x = lane; x < G * TPH; x += 64) {
                    const int i = x / TPH, d = (x % TPH) * 4;
                    const half4_t hv = merge_partitions(np,
                        [&](int pi) { return __builtin_bit_cast(float2_t, __builtin_amdgcn_raw_buffer_load_b64(rs_ml, (i * p.num_parts + pi) * 8, 0, 16)); },
                        [&](int pi) { return __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_o, ((i * p.num_parts + pi) * D + d) * 4, 0, 16)); });
                    *reinterpret_cast<half4_t *>(p.out + (row0 + i) * D + d) = hv;
                }
                if (lane == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for the next launch
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the boundary drains: no store of this tail stands among the next segment's hand-counted requests
    }
}

bool attn_fp8_mfma_ok(int D, int H, int KVH, int block_size) {
    if (KVH <= 0 || H % KVH) return false;
    return (D == 64 || D == 128) && H / KVH == 8 && block_size >= 64 && (block_size & (block_size - 1)) == 0;
}

// One launch of nq * KVH * num_parts workgroups; num_parts == 1: 16-bit rows into a.out, else partials into part_o / part_ml for attn_fp8_merge_kernel
// (the partition plan and the merge launch: launch_attn_fp8_mfma, attention_fp8.hip)
// part0 > 0: the own keys behind a shared prefix — partitions part0 .. num_parts-1 from key a.shared_kv0[t] (or a.shared_len) on, partials always
int attn_fp8_mfma(const AttnFp8Args &a, int32_t part_size, int32_t num_parts, float *part_o, float *part_ml, hipStream_t s, int32_t part0) {
    if (!attn_fp8_mfma_ok(a.D, a.H, a.KVH, a.block_size) || num_parts < 1 || (num_parts > 1 && (part_size <= 0 || part_size % 64 || !part_o || !part_ml)) ||
        part0 < 0 || (part0 > 0 && (part0 >= num_parts || a.shared_len <= 0 || a.shared_len % 64)))
        return nvr::fail(NVR_ERR_UNSUPPORTED, "attn_fp8_mfma: D=%d H=%d KVH=%d block_size=%d, %d partitions of %d keys, %d of them behind %d shared keys (D in {64,128}, "
                         "H/KVH = 8, block_size a power of two >= 64, partitions and shared keys of whole 64-key steps)", a.D, a.H, a.KVH, a.block_size, num_parts,
                         part_size, num_parts - part0, a.shared_len);
    AttnFp8MfmaOwnParams p{};
    p.q = (const half_t *)a.q; p.ldq = a.ldq; p.k = a.k; p.v = a.v; p.ctx_lens = a.ctx_lens; p.block_tables = a.block_tables;
    p.max_blocks = a.max_blocks; p.block_size = a.block_size; p.bs_shift = __builtin_ctz(a.block_size);
    p.H = a.H; p.KVH = a.KVH; p.scale = a.scale * a.k_scale; p.v_scale = a.v_scale;
    p.part_size = num_parts > 1 ? part_size : 0x3fffffc0; p.num_parts = num_parts; p.part_o = part_o; p.part_ml = part_ml; p.out = (half_t *)a.out;
    p.part0 = part0; p.kv0 = a.shared_len; p.kv0_rows = a.shared_kv0;
    dim3 grid((unsigned)((int64_t)a.nq * a.KVH * (num_parts - part0))), block(256);
    if (part0 > 0) {
        if (a.D == 128) attn_fp8_mfma_kernel<128, 8, true><<<grid, block, 0, s>>>(p);
        else attn_fp8_mfma_kernel<64, 8, true><<<grid, block, 0, s>>>(p);
    } else {
        if (a.D == 128) attn_fp8_mfma_kernel<128, 8, false><<<grid, block, 0, s>>>(p);
        else attn_fp8_mfma_kernel<64, 8, false><<<grid, block, 0, s>>>(p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "attn_fp8_mfma launch failed: %s", hipGetErrorString(e));
    return 0;
}

// The work-balanced launch: nw workgroups (4·nw workers) over `slots` partial slots per (query, head) in the workspace — one per 64 keys of max_ctx, the most
// workers a pair can meet.  The rule that selects it: launch_attn_fp8_mfma, attention_fp8.hip.
int attn_share_fp8_mfma(const AttnFp8Args &a, int32_t slots, int32_t nw, hipStream_t s) {
    if (!attn_fp8_mfma_ok(a.D, a.H, a.KVH, a.block_size) || !a.tickets || !a.workspace || a.nq > 1024 || slots < 1 || nw < 1 ||
        (int64_t)slots * 64 < a.max_ctx || (int64_t)8 * slots * a.D * 4 > 0x7fffffff || (int64_t)a.nq * a.KVH * slots > 0x7fffffff)
        return nvr::fail(NVR_ERR_UNSUPPORTED, "attn_share_fp8_mfma: D=%d H=%d KVH=%d block_size=%d nq=%d, %d slots for max_ctx %d, %d workgroups (attn_fp8_mfma_ok, "
                         "tickets and a workspace, nq <= 1024, one slot per 64 keys of max_ctx)", a.D, a.H, a.KVH, a.block_size, a.nq, slots, a.max_ctx, nw);
    if (a.workspace_bytes && (size_t)a.nq * a.H * slots * (a.D + 2) * sizeof(float) > a.workspace_bytes)
        return nvr::fail(NVR_ERR_INVALID_ARG, "attn_share_fp8_mfma: %d slots of %d queries x %d heads do not fit %zu workspace bytes", slots, a.nq, a.H, a.workspace_bytes);
    AttnFp8MfmaParams p{};
    p.q = (const half_t *)a.q; p.ldq = a.ldq; p.k = a.k; p.v = a.v; p.ctx_lens = a.ctx_lens; p.block_tables = a.block_tables;
    p.max_blocks = a.max_blocks; p.block_size = a.block_size; p.bs_shift = __builtin_ctz(a.block_size);
    p.H = a.H; p.KVH = a.KVH; p.scale = a.scale * a.k_scale; p.v_scale = a.v_scale;
    p.part_size = 64; p.num_parts = slots; p.part_o = (float *)a.workspace; p.part_ml = p.part_o + (int64_t)a.nq * a.H * slots * a.D; p.out = (half_t *)a.out;
    dim3 grid((unsigned)nw), block(256);
    if (a.D == 128) attn_share_fp8_mfma_kernel<128, 8><<<grid, block, 0, s>>>(p, a.tickets, a.nq);
    else attn_share_fp8_mfma_kernel<64, 8><<<grid, block, 0, s>>>(p, a.tickets, a.nq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return nvr::fail(NVR_ERR_HIP, "attn_share_fp8_mfma launch failed: %s", hipGetErrorString(e));
    return 0;
}

}}  // namespace nvr::k / nvr::kb (NVR_DT_NS)

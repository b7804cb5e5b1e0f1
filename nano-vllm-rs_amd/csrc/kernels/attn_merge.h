// attn_merge.h — the merge of split-KV partials shared by the decode attention kernels (attention.hip, attention_fp8.hip).
#pragma once
#include "device_utils.h"

namespace nvr { namespace NVR_DT_NS {

// out = sum_p e^(m_p-M) o_p / sum_p e^(m_p-M) l_p over partitions [0, np) of ONE (query, head), 4 columns per thread: the partials of up
// to 8 partitions are requested together (a runtime-count loop of dependent loads would pay one round trip per partition); sums run over
// the partitions in ascending order for every column.  load_ml(i) / load_o(i): (max, sum) and the 4 columns of partition i — plain loads
// in the merge kernel, sc1 loads in the last arriver of the fused form (the same arithmetic: the two forms agree bit for bit).
template <class LoadML, class LoadO>
__device__ __forceinline__ half4_t merge_partitions(int np, LoadML load_ml, LoadO load_o) {
    float M = -INFINITY;
    float4_t o = {0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
    for (int i0 = 0; i0 < np; i0 += 8) {
        float2_t ml[8]; float4_t po[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + u, np - 1);
            ml[u] = load_ml(i);
            po[u] = load_o(i);
        }
        float Mn = M;
#pragma unroll
        for (int u = 0; u < 8; ++u) if (i0 + u < np) Mn = fmaxf(Mn, ml[u][0]);
        if (i0 > 0 && Mn != M) { const float r = __expf(M - Mn); o *= r; L *= r; }     // (more than 8 partitions: rescale what is summed)
        M = Mn;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + u < np) {
                const float w = __expf(ml[u][0] - M);
                // (spelled out as fused multiply-adds: under -ffp-contract=fast hipcc decides per INSTANTIATION whether "a += w * b" becomes an fma,
                //  and this function is inlined into three kernels whose results are promised to agree bit for bit; fma is what the merge kernel got)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = __fmaf_rn(w, po[u][e], o[e]);
                L = __fmaf_rn(w, ml[u][1], L);
            }
        }
    }
    half4_t hv;
#pragma unroll
    for (int e = 0; e < 4; ++e) hv[e] = (half_t)(L > 0.f ? o[e] / L : 0.f);
    return hv;
}

}}  // namespace nvr::k / nvr::kb (NVR_DT_NS)

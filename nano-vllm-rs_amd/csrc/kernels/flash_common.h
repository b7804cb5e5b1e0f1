// flash_common.h — device helpers shared by the MFMA flash prefill kernels (flash_prefill.hip: 16-bit K/V, flash_prefill_fp8.hip: byte caches).
#pragma once
#include "device_utils.h"

namespace nvr {

// One K/V tile into LDS by LDS-DMA (global_load_lds_dwordx4: 16 B per lane, 1 KiB per wave-instruction, lane-linear at M0), written as
// inline asm ON PURPOSE: hipcc treats the builtin as a pending write to LDS and drains it (s_waitcnt vmcnt(0)) in front of the first
// transposing read (ds_read_b64_tr_b16) of the tile IN USE, i.e. in the middle of every step, 1-2 k cycles after the requests went
// out (r02 .s: the stall behind the 27 % MFMA-busy figure).  As asm the requests are invisible to its wait insertion; they are
// counted by hand at the end of the step (s_waitcnt vmcnt + barrier in step()), one whole step after they were issued.  N pieces of
// STRIDE-apart LDS destinations (STRIDE = 16 B x the workgroup's threads) starting at `lds` (wave-uniform byte address); M0 is saved and
// restored inside the statement.
template <int N, int STRIDE, typename T>
__device__ __forceinline__ void glds_pieces(const T *const (&src)[N], unsigned lds) {
    static_assert(N == 2 || N == 4 || N == 8, "1, 2 or 4 pieces per operand");
    unsigned keep;
    if constexpr (N == 8) {
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %9\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %6, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %7, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %8, off\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src[0]), "v"(src[1]), "v"(src[2]), "v"(src[3]), "v"(src[4]), "v"(src[5]), "v"(src[6]), "v"(src[7]), "s"(lds), [st] "n"(STRIDE)
                     : "memory", "scc");
    } else if constexpr (N == 2) {
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src[0]), "v"(src[1]), "s"(lds), [st] "n"(STRIDE)
                     : "memory", "scc");
    } else {
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off\n\t"
                     "s_add_u32 m0, m0, %[st]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, off\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src[0]), "v"(src[1]), "v"(src[2]), "v"(src[3]), "s"(lds), [st] "n"(STRIDE)
                     : "memory", "scc");
    }
}

// Byte images of K / V rows (flash_prefill_fp8.hip's header comment derives them; attention_fp8_mfma.hip stages V the same way): chunk XOR of
// the V image, and ds_read_b64_tr_b8, the hardware-transposed LDS read of 8 rows x 16 columns of bytes
typedef int int2_t __attribute__((ext_vector_type(2)));
template <int D>
__device__ __forceinline__ int v8_swz(int key) { return D == 128 ? ((key >> 1) & 7) : ((key >> 2) & 3); }
__device__ __forceinline__ int2_t lds_read_tr8(const char *lds_addr) {
    return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) int2_t *)lds_addr);
}

// max over the four 16-lane rows of a wave (the 4 key quads of a query), in the vector ALU: v_permlane16_swap / v_permlane32_swap of a
// value with itself leave {own, partner} in the two results (an LDS round trip per ds_bpermute before: two dependent ones per step)
__device__ __forceinline__ float max_over_rows(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

}  // namespace nvr

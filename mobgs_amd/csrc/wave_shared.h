// The cross-lane primitives of every kernel file, in one place: the wave-local LDS fence, the xor butterflies, the DPP
// row reductions and the permlane-swap wave reductions.  Several kernels promise bit-identical results to one another
// (forward and backward compositor, the layered pass and three single passes, the fixed-order sums of
// reduce_shared.h); they keep that promise by calling the SAME reduction, not a copy of it.
//
// Every function here is wave-wide: all 64 lanes of the wave must make the call.
#pragma once
#include "common.h"

namespace mobgs {

// Orders the LDS accesses of ONE wave: what any lane wrote before the call is what any lane of the same wave reads
// after it.  LDS operations of one wave execute in issue order; only the compiler has to be told, so a fence suffices
// and no s_barrier is paid.  Says nothing about other waves of the workgroup.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- xor butterflies, 32 down to 1: every lane gets the result, with the same bits in each (a + b == b + a) ------------
// The loop itself, folding the variable v in place with OP (max, min, MOBGS_WAVE_ADD).  Call wave_sum / wave_min /
// wave_max.  The statement form is for the few sites (tile scans, raster_bwd's last-index search, the weight-gradient
// and hex-count sums) whose instruction schedule is pinned: a function is optimised on its own before it is inlined,
// and there that schedules the lane-index arithmetic differently from the loop unrolled in the kernel body.
#define MOBGS_WAVE_ADD(a, b) ((a) + (b))
#define MOBGS_WAVE_FOLD(v, OP) \
    _Pragma("unroll") for (int off_ = MOBGS_WAVE / 2; off_ > 0; off_ >>= 1) v = OP(v, __shfl_xor(v, off_, MOBGS_WAVE))

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    MOBGS_WAVE_FOLD(v, MOBGS_WAVE_ADD);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
    MOBGS_WAVE_FOLD(v, min);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
    MOBGS_WAVE_FOLD(v, max);
    return v;
}

// ---- DPP: one VALU instruction reads another lane of the same 16-lane row ------------------------------------------------
// CTRL: 0xB1 = quad_perm:[1,0,3,2] (lane ^ 1), 0x4E = quad_perm:[2,3,0,1] (lane ^ 2), 0x1B = quad_perm:[3,2,1,0],
// 0x141 = row_half_mirror (l -> 7 - l inside each 8 lanes), 0x128 = row_ror:8 (lane ^ 8), 0x124 = row_ror:4 (lane l reads
// lane l - 4 of its row, cyclically)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// v + (v of lane ^ 4).  row_half_mirror would pair l with 7 - l (the other quarter of the 8 lanes), so two masked
// shifts do it instead: banks {0, 2} take lane + 4, banks {1, 3} lane - 4, and a lane gets 0 from the shift that is not its own
__device__ __forceinline__ float dpp_add_xor4(float v) {
    const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x104, 0xF, 0x5, true));  // row_shl:4
    const float dn = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xA, true));  // row_shr:4
    return v + (up + dn);
}
// sum over each 16-lane row, in every lane of the row
__device__ __forceinline__ float row_allreduce(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm:[1,0,3,2]
    v = dpp_add<0x4E>(v);   // quad_perm:[2,3,0,1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    v = dpp_add<0x128>(v);  // row_ror:8
    return v;
}
// sum over the 32 lanes of each half-wave, in every lane of the half
__device__ __forceinline__ float half_wave_sum(float v) {
    v = row_allreduce(v);
    v += __shfl_xor(v, 16, MOBGS_WAVE);
    return v;
}
// sum over the wave, in every lane: the two swap stages of wave_reduce_components on one register, then the rows
__device__ __forceinline__ float wave_allreduce(float v) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    return row_allreduce(v);
}

// ---- permlane swaps: wave-wide sums of many per-lane values ----------------------------------------------------------------
// Wave-wide sum of NVP per-lane values with the cross-lane hardware of gfx950, no LDS traffic, no selects:
//   1. v_permlane32_swap pairs component i with i+NVP/2: one swap + one add leaves the sum over lane bit 5 of
//      the low-half components in lanes 0-31 and of the high-half components in lanes 32-63;
//   2. v_permlane16_swap does the same for lane bit 4 (odd/even rows of 16 lanes);
//   3. the NVP/4 survivors are all-reduced inside each 16-lane row with four DPP adds
//      (quad_perm xor 1, quad_perm xor 2, row_half_mirror, row_ror:8).
// Afterwards every lane of row r (= lane >> 4) holds, in v[0 .. NVP/4), the wave totals of components
//   (r >> 1) * NVP/2 + (r & 1) * NVP/4 + k.
template <int NVP>
__device__ __forceinline__ void wave_reduce_components(float (&v)[NVP]) {
    static_assert(NVP >= 8 && (NVP & (NVP - 1)) == 0, "NVP must be a power of two >= 8");
#pragma unroll
    for (int i = 0; i < NVP / 2; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + NVP / 2]), false,
                                                        false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < NVP / 4; ++i) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + NVP / 4]), false,
                                                        false);
        v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < NVP / 4; ++i) v[i] = row_allreduce(v[i]);
}

// One or two further components (NV = 17, 18: e.g. 9 features + 2 flow channels + depth) next to sixteen others:
// one permlane32 swap + add puts the bit-5 sums of e0 into lanes 0-31 and of e1 into lanes 32-63, four DPP adds
// all-reduce every 16-lane row, one permlane16 swap of the register with itself + add folds the two rows of each
// half: 8 instructions, against 80 for the generic 32-component reduction such a kernel used before.  Afterwards
// lanes 0-31 hold the wave total of e0, lanes 32-63 that of e1.
__device__ __forceinline__ float wave_reduce_pair(float e0, float e1) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(e0), __float_as_uint(e1), false, false);
    float x = row_allreduce(__uint_as_float(r[0]) + __uint_as_float(r[1]));
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}

}  // namespace mobgs

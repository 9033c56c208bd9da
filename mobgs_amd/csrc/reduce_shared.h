// The fixed-order sums and the small input helpers of the scoring kernels (csrc/loss.hip, flowloss.hip, regterms.hip,
// metrics.hip, pose.hip, lpips.hip, tof.hip, scene_seed.hip), in one place so that their summation orders cannot drift
// apart.
//
// The contract of every sum in this file:
//   - its order is fixed by the template arguments and the element count alone -- not by an address, a launch size or
//     the timing of a run: no atomic, no hand-off between workgroups.  The same values give the same bits, every time;
//   - block_sum and rows_sum return the total to thread 0 (other threads: unspecified); wave_sum, wave_rows_sum and
//     block_sum4 return it to every thread that took part, with the same bits in each (a + b == b + a);
//   - every thread of the workgroup (wave_sum, wave_rows_sum: of the wave) must make the call: they shuffle, and the
//     block sums meet at barriers.  A block sum may be called again at once with the same LDS array: it ends with a barrier.
#pragma once
#include "common.h"
#include "wave_shared.h"

namespace mobgs {

// ---- float64: down the wave by shuffles, then the waves' values in wave order -----------------------------------------
// s_wave: LDS [WAVES]; the workgroup has WAVES full waves
// Lane 0's chain is the xor butterfly's tree: u[l] = v[l] + v[l + 32], then u[l] + u[l + 16], .. + u[l + 1]; then ((w0 + w1) + w2) + ..
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* s_wave) {
#pragma unroll
    for (int off = MOBGS_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, MOBGS_WAVE);
    if ((threadIdx.x & (MOBGS_WAVE - 1)) == 0) s_wave[threadIdx.x / MOBGS_WAVE] = v;
    __syncthreads();
    double total = s_wave[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) total += s_wave[w];
    __syncthreads();    // (s_wave is reused by the next call)
    return total;
}

// rows values at p[0], p[stride], ...: thread t of the BLOCK adds its run [t per, min(t per + per, rows)) in ascending
// order, per = ceil(rows / BLOCK); block_sum adds the runs
template <int BLOCK>
__device__ __forceinline__ double rows_sum(const double* __restrict__ p, int rows, int stride, double* s_wave) {
    const int per = (rows + BLOCK - 1) / BLOCK;
    const int r0 = threadIdx.x * per;
    const int r1 = r0 + per < rows ? r0 + per : rows;
    double s = 0.0;
    for (int r = r0; r < r1; ++r) s += p[(size_t)r * stride];
    return block_sum<BLOCK / MOBGS_WAVE>(s, s_wave);
}

// ---- one wave: wave_sum is the xor butterfly of wave_shared.h (float or double) -----------------------------------------
// n values at p[0], p[stride], ...: lane l adds its run [l per, min(l per + per, n)), per = ceil(n / 64); wave_sum adds
// the 64 lane sums
__device__ __forceinline__ double wave_rows_sum(const double* __restrict__ p, int n, int stride, int lane) {
    const int per = (n + MOBGS_WAVE - 1) / MOBGS_WAVE;
    const int r0 = min(lane * per, n), r1 = min(r0 + per, n);
    double s = 0.0;
    for (int r = r0; r < r1; ++r) s += p[(size_t)r * stride];
    return wave_sum(s);
}

// ---- fp32, a workgroup of four waves: a butterfly inside each wave, then ((w0 + w1) + w2) + w3; sm: LDS [4] --------------
__device__ __forceinline__ float block_sum4(float v, float* sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return r;
}

// ---- inputs -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }
// the 8-bit version of a value, as the reference forms it in fp32 (eval.py:162: clip, * 255, truncate, / 255).  No a * b + c:
// the value does not depend on the translation unit's -ffp-contract setting.
__device__ __forceinline__ float quantize8(float x) { return floorf(clamp01(x) * 255.f) / 255.f; }

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// host: p is a multiple of bytes (a power of two); NULL counts as aligned
inline bool aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace mobgs

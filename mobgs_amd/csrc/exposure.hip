// K20: exposure-time estimate from two rendered flow maps (the reference's train.py:474-492 after its two
// get_flow_static calls): quantile threshold on the camera-flow magnitude, lower median of latent / camera over the
// pixels above it, one float stored on the device.  gfx950 only.  No sort, no read-back, no float atomics.
//
// Exact selection by radix select on the fp32 bit pattern: every key is a magnitude or a quotient of magnitudes, so it is
// non-negative and the unsigned order of its bits is its numeric order.  Four passes of 8 bits, most significant first.
// A pass is a histogram launch (per-workgroup LDS histogram of the digit of every key that carries the current prefix,
// merged into a global table with integer atomics) and a single-workgroup pick launch (prefix sum over the 256 bins: the
// bin that holds the wanted rank extends the prefix, the rank becomes the rank inside that bin).  After the fourth pick
// the prefix IS the order statistic.
//
//   expo_prep_kernel            cam_mag = sqrt(x x + y y), lat_mag likewise, ratio = lat_mag / cam_mag, stored ONCE as
//                               their bit patterns (two uint32 arrays in scratch); counts non-finite magnitudes; fills
//                               the first histogram of the quantile (top digit of cam_mag, no prefix yet)
//   expo_pick_kernel<false> x4  the two ranks floor / ceil(q (n - 1)) of torch.quantile's linear interpolation, side by
//   expo_hist_kernel<false> x3  side: while their prefixes agree they share one table, afterwards each has its own.  The
//                               last pick interpolates the threshold exactly as ATen's lerp does.
//   expo_hist_kernel<true>  x4  ratio keys of the pixels with cam_mag > threshold.  n_valid exists only on the device:
//   expo_pick_kernel<true>  x4  the first pick reads it as the total of its table and derives the median's rank
//                               (n_valid - 1) / 2; the last one stores median * scale to *slot and the four stats.
//
// 16 launches and one hipMemsetAsync (control words + all tables) on the caller's stream.  No workgroup waits on another;
// every loop is bounded by n (grid-stride, capped grid) or by the 256 bins.  Two calls on one scratch buffer are
// independent: everything a call reads from scratch it has zeroed or written itself.
//
// Built with -ffp-contract=off: x x + y y and the interpolation a + w (b - a) | b - (b - a)(1 - w) are evaluated as
// written, so that magnitudes, threshold and median are bit-equal to torch on the CPU for the same inputs
// (tests/exposure_restatement.py).
#include "common.h"

namespace mobgs {

constexpr int EXPO_BLOCK = 256;         // lanes per workgroup = bins per digit
constexpr int EXPO_MAX_GRID = 1024;     // workgroups of the streaming kernels at most (4 per CU); beyond: grid-stride
constexpr int EXPO_BINS = 256;
constexpr int EXPO_PASSES = 4;
constexpr int64_t EXPO_MAX_N = (int64_t)1 << 30;   // counts and ranks are int32

// control words at the start of scratch (int32 each)
enum {
    EXPO_NONFINITE = 0,   // magnitudes (either map) that are inf or NaN
    EXPO_PREF_A, EXPO_PREF_B,   // quantile: key prefixes of rank floor / ceil
    EXPO_RANK_A, EXPO_RANK_B,   // ... and the ranks inside those prefixes
    EXPO_THRESHOLD,       // bits of the interpolated quantile
    EXPO_NVALID,
    EXPO_PREF_M, EXPO_RANK_M,   // median
    EXPO_CTRL_WORDS = 16
};
// scratch: [control 16][quantile tables 4 x 2 x 256][median tables 4 x 256][cam_mag bits n][ratio bits n]
constexpr size_t EXPO_QTAB = EXPO_CTRL_WORDS;
constexpr size_t EXPO_MTAB = EXPO_QTAB + (size_t)EXPO_PASSES * 2 * EXPO_BINS;
constexpr size_t EXPO_HEADER_WORDS = EXPO_MTAB + (size_t)EXPO_PASSES * EXPO_BINS;   // zeroed by every call

__host__ __device__ inline int expo_grid(int64_t n) {
    const int64_t g = (n + EXPO_BLOCK - 1) / EXPO_BLOCK;
    return (int)(g < EXPO_MAX_GRID ? g : EXPO_MAX_GRID);
}
// keys that agree with the prefix in the digits above `shift + 8` (the top digit has no prefix)
__device__ __forceinline__ uint32_t expo_prefix_mask(int shift) { return shift >= 24 ? 0u : ~0u << (shift + 8); }

__device__ __forceinline__ void expo_flush(const uint32_t* s_hist, uint32_t* __restrict__ table) {
    const uint32_t c = s_hist[threadIdx.x];
    if (c) atomicAdd(&table[threadIdx.x], c);
}

__global__ void __launch_bounds__(EXPO_BLOCK) expo_prep_kernel(
    int64_t n, const float2* __restrict__ cam, const float2* __restrict__ lat, uint32_t* __restrict__ cam_keys,
    uint32_t* __restrict__ ratio_keys, int32_t* __restrict__ ctrl, uint32_t* __restrict__ table) {
    __shared__ uint32_t s_hist[EXPO_BINS];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * EXPO_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * EXPO_BLOCK + threadIdx.x; i < n; i += stride) {
        const float2 c = cam[i], l = lat[i];
        // sqrtf and / are the correctly rounded forms here (hipcc's default; __fsqrt_rn is the 1-ulp hardware root)
        const float cm = sqrtf(c.x * c.x + c.y * c.y);
        const float lm = sqrtf(l.x * l.x + l.y * l.y);
        const uint32_t cb = __float_as_uint(cm), lb = __float_as_uint(lm);
        bad += ((cb & 0x7f800000u) == 0x7f800000u) + ((lb & 0x7f800000u) == 0x7f800000u);
        cam_keys[i] = cb;
        ratio_keys[i] = __float_as_uint(lm / cm);
        atomicAdd(&s_hist[cb >> 24], 1u);
    }
    __syncthreads();
    expo_flush(s_hist, table);
    if (bad) atomicAdd(&ctrl[EXPO_NONFINITE], bad);
}

// MEDIAN false: keys = cam_mag bits, two prefixes (tables 0 and 1; table 0 alone while they agree).
// MEDIAN true:  keys = ratio bits of the pixels whose cam_mag is above the threshold, one prefix.
template <bool MEDIAN>
__global__ void __launch_bounds__(EXPO_BLOCK) expo_hist_kernel(
    int64_t n, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ cam_keys,
    const int32_t* __restrict__ ctrl, uint32_t* __restrict__ table, int shift) {
    __shared__ uint32_t s_hist[2][EXPO_BINS];
    s_hist[0][threadIdx.x] = 0;
    s_hist[1][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t mask = expo_prefix_mask(shift);
    const uint32_t pref_a = (uint32_t)ctrl[MEDIAN ? EXPO_PREF_M : EXPO_PREF_A] & mask;
    const uint32_t pref_b = MEDIAN ? pref_a : ((uint32_t)ctrl[EXPO_PREF_B] & mask);
    const bool two = pref_a != pref_b;
    const float threshold = __uint_as_float((uint32_t)ctrl[EXPO_THRESHOLD]);
    const int64_t stride = (int64_t)gridDim.x * EXPO_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * EXPO_BLOCK + threadIdx.x; i < n; i += stride) {
        if (MEDIAN && !(__uint_as_float(cam_keys[i]) > threshold)) continue;
        const uint32_t key = keys[i];
        const uint32_t digit = (key >> shift) & (EXPO_BINS - 1);
        if ((key & mask) == pref_a) atomicAdd(&s_hist[0][digit], 1u);
        if (two && (key & mask) == pref_b) atomicAdd(&s_hist[1][digit], 1u);
    }
    __syncthreads();
    expo_flush(s_hist[0], table);
    if (two) expo_flush(s_hist[1], table + EXPO_BINS);
}

// One workgroup.  Inclusive prefix sums of the pass's table(s) in LDS; the lane whose bin holds the rank extends the
// prefix.  first: the ranks come from (q, n) / from the table's total instead of from the control words.  last: the
// prefixes are the order statistics themselves -- the threshold / the result is formed and stored.
template <bool MEDIAN>
__global__ void __launch_bounds__(EXPO_BLOCK) expo_pick_kernel(
    int64_t n, float q, float scale, int32_t* __restrict__ ctrl, const uint32_t* __restrict__ table, int shift,
    float* __restrict__ slot, int32_t* __restrict__ stats) {
    __shared__ uint32_t s_incl[2][EXPO_BINS];
    __shared__ uint32_t s_found[2];
    const int t = threadIdx.x;
    const bool first = shift == 24, last = shift == 0;
    uint32_t pref[2];
    int32_t rank[2];
    pref[0] = first ? 0u : (uint32_t)ctrl[MEDIAN ? EXPO_PREF_M : EXPO_PREF_A];
    pref[1] = MEDIAN ? pref[0] : (first ? 0u : (uint32_t)ctrl[EXPO_PREF_B]);
    const bool two = pref[0] != pref[1];
    float w = 0.f;
    if (!MEDIAN) {
        // torch.quantile, linear: the position q (n - 1) is formed in fp32
        const float pos = q * (float)(n - 1);
        const float lo = floorf(pos);
        w = pos - lo;
        const float top = (float)(n - 1);    // (q <= 1, so only the rounding of a count past 2^24 could exceed it)
        rank[0] = first ? (int32_t)fminf(lo, top) : ctrl[EXPO_RANK_A];
        rank[1] = first ? (int32_t)fminf(ceilf(pos), top) : ctrl[EXPO_RANK_B];
    } else {
        rank[0] = rank[1] = first ? 0 : ctrl[EXPO_RANK_M];
    }
    s_incl[0][t] = table[t];
    s_incl[1][t] = two ? table[EXPO_BINS + t] : 0u;
    if (t < 2) s_found[t] = pref[t];    // (kept when no bin holds the rank: an empty selection)
    __syncthreads();
    for (int off = 1; off < EXPO_BINS; off <<= 1) {
        const uint32_t a = t >= off ? s_incl[0][t - off] : 0u;
        const uint32_t b = t >= off ? s_incl[1][t - off] : 0u;
        __syncthreads();
        s_incl[0][t] += a;
        s_incl[1][t] += b;
        __syncthreads();
    }
    int32_t n_valid = 0;
    if (MEDIAN) {
        if (first) {
            n_valid = (int32_t)s_incl[0][EXPO_BINS - 1];
            rank[0] = rank[1] = n_valid > 0 ? (n_valid - 1) / 2 : 0;
            if (t == 0) ctrl[EXPO_NVALID] = n_valid;
        } else {
            n_valid = ctrl[EXPO_NVALID];
        }
    }
    for (int k = 0; k < (MEDIAN ? 1 : 2); ++k) {
        const int tab = (k == 1 && two) ? 1 : 0;
        const uint32_t incl = s_incl[tab][t], excl = t ? s_incl[tab][t - 1] : 0u;
        if ((uint32_t)rank[k] >= excl && (uint32_t)rank[k] < incl) {    // exactly one lane, or none if the table is empty
            const uint32_t p = pref[k] | ((uint32_t)t << shift);
            ctrl[MEDIAN ? EXPO_PREF_M : (k ? EXPO_PREF_B : EXPO_PREF_A)] = (int32_t)p;
            ctrl[MEDIAN ? EXPO_RANK_M : (k ? EXPO_RANK_B : EXPO_RANK_A)] = rank[k] - (int32_t)excl;
            s_found[k] = p;
        }
    }
    if (!last) return;
    __syncthreads();
    if (t != 0) return;
    if (!MEDIAN) {
        // ATen lerp: a + w (b - a) below one half, b - (b - a)(1 - w) from there on
        const float a = __uint_as_float(s_found[0]), b = __uint_as_float(s_found[1]);
        const float thr = w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w);
        ctrl[EXPO_THRESHOLD] = (int32_t)__float_as_uint(thr);
    } else {
        const int32_t nonfinite = ctrl[EXPO_NONFINITE];
        const int32_t updated = (n_valid > 0 && nonfinite == 0) ? 1 : 0;
        if (updated) *slot = __uint_as_float(s_found[0]) * scale;
        stats[0] = n_valid;
        stats[1] = nonfinite;
        stats[2] = updated;
        stats[3] = 0;
    }
}

static bool expo_n_in_range(int64_t n) { return n >= 1 && n <= EXPO_MAX_N; }

}  // namespace mobgs

using namespace mobgs;

extern "C" {

size_t mobgs_exposure_scratch_bytes(int64_t n) {
    if (!expo_n_in_range(n)) return 0;
    return (EXPO_HEADER_WORDS + 2 * (size_t)n) * sizeof(uint32_t);
}

int mobgs_exposure_estimate(int64_t n, const float* cam_flow, const float* latent_flow, float q, float scale,
                            float* slot, int32_t* stats, void* scratch, void* stream) {
    if (!expo_n_in_range(n)) {
        set_error("mobgs_exposure_estimate: n = %lld pixels; need 1 <= n <= 2^30", (long long)n);
        return MOBGS_E_INVALID;
    }
    if (!cam_flow || !latent_flow || !slot || !stats || !scratch) {
        set_error("mobgs_exposure_estimate: NULL buffer");
        return MOBGS_E_INVALID;
    }
    if (!(q >= 0.f && q <= 1.f)) {    // (false for NaN)
        set_error("mobgs_exposure_estimate: quantile q = %g outside [0, 1]", (double)q);
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)cam_flow & 7) || ((uintptr_t)latent_flow & 7) || ((uintptr_t)slot & 3) || ((uintptr_t)stats & 3) ||
        ((uintptr_t)scratch & 3)) {
        set_error("mobgs_exposure_estimate: flow maps must be 8-byte aligned, slot, stats and scratch 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* ctrl = (int32_t*)scratch;
    uint32_t* words = (uint32_t*)scratch;
    uint32_t* qtab = words + EXPO_QTAB;
    uint32_t* mtab = words + EXPO_MTAB;
    uint32_t* cam_keys = words + EXPO_HEADER_WORDS;
    uint32_t* ratio_keys = cam_keys + n;
    if (hipMemsetAsync(scratch, 0, EXPO_HEADER_WORDS * sizeof(uint32_t), s) != hipSuccess) {
        (void)hipGetLastError();
        set_error("mobgs_exposure_estimate: hipMemsetAsync failed");
        return MOBGS_E_LAUNCH;
    }
    const dim3 grid((unsigned)expo_grid(n)), block(EXPO_BLOCK), one(1);
    hipLaunchKernelGGL(expo_prep_kernel, grid, block, 0, s, n, (const float2*)cam_flow, (const float2*)latent_flow,
                       cam_keys, ratio_keys, ctrl, qtab);
    for (int p = 0; p < EXPO_PASSES; ++p) {
        const int shift = 24 - 8 * p;
        uint32_t* table = qtab + (size_t)p * 2 * EXPO_BINS;
        if (p > 0)
            hipLaunchKernelGGL(expo_hist_kernel<false>, grid, block, 0, s, n, (const uint32_t*)cam_keys,
                               (const uint32_t*)cam_keys, (const int32_t*)ctrl, table, shift);
        hipLaunchKernelGGL(expo_pick_kernel<false>, one, block, 0, s, n, q, scale, ctrl, (const uint32_t*)table, shift,
                           slot, stats);
    }
    for (int p = 0; p < EXPO_PASSES; ++p) {
        const int shift = 24 - 8 * p;
        uint32_t* table = mtab + (size_t)p * EXPO_BINS;
        hipLaunchKernelGGL(expo_hist_kernel<true>, grid, block, 0, s, n, (const uint32_t*)ratio_keys,
                           (const uint32_t*)cam_keys, (const int32_t*)ctrl, table, shift);
        hipLaunchKernelGGL(expo_pick_kernel<true>, one, block, 0, s, n, q, scale, ctrl, (const uint32_t*)table, shift,
                           slot, stats);
    }
    return check_launch("mobgs_exposure_estimate");
}

}  // extern "C"

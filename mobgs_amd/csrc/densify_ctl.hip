// Densification controller kernels (include/mobgs_hip.h K34): the statistics of one training iteration over all views
// of its batch in one launch, and the row list of a resize -- clone + split, or one of three prunes -- as ONE plan of two
// launches whose four counts the host reads back once.  Replaces the per-set gradient split of
// /root/reference/train.py:634-648 with the statistics update of :813-817, and the host-driven list building of
// TrainableGaussians.densify_pruneclone / prune_points (one selection launch, three single-workgroup mask_indices
// launches with a read-back each, arange / cat) under /root/reference/helper_train.py:222-258 and :167-180.
// The kernels of densify.hip are left as they are; the gather and the children kernel there consume the plan's list.
#include "common.h"
#include "wave_shared.h"

namespace mobgs {

// ---- statistics of a batch ----------------------------------------------------------------------------------------
constexpr int MAX_VIEWS = MOBGS_STATS_MAX_VIEWS;   // include/mobgs_hip.h: the bindings read the same number
struct BatchViews {
    const float* grad[MAX_VIEWS];
    const int32_t* radii[MAX_VIEWS];
};

// row i of the set = row row0 + i of every view's arrays.  The gradient is summed over the views FIRST, in view order,
// and its norm taken afterwards (the norm of the sum is not the sum of the norms); built without FMA contraction.
__global__ void __launch_bounds__(256)
densify_stats_batch_kernel(BatchViews V, int n_views, int vstride, int row0, int n, float sx, float sy,
                           float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ max_radii,
                           float* __restrict__ grad_sum, int32_t* __restrict__ radii_max,
                           uint8_t* __restrict__ visible) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)row0 + i;
    float gx = 0.f, gy = 0.f;
    int r = V.radii[0][row];
    for (int v = 0; v < n_views; ++v) {
        const float* g = V.grad[v] + row * vstride;
        gx = gx + g[0];
        gy = gy + g[1];
        r = max(r, V.radii[v][row]);
    }
    gx = gx * sx;
    gy = gy * sy;
    const bool vis = r > 0;  // any view's radius > 0
    if (grad_sum) *reinterpret_cast<float2*>(grad_sum + 2 * (size_t)i) = make_float2(gx, gy);
    if (radii_max) radii_max[i] = r;
    if (visible) visible[i] = vis ? 1 : 0;
    if (!vis) return;
    max_radii[i] = fmaxf(max_radii[i], (float)r);
    accum[i] += __fsqrt_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)));  // as densify_stats_kernel rounds it
    denom[i] += 1.f;
}

// ---- statistics of a batch, both sets in one launch -----------------------------------------------------------------
// The arithmetic of densify_stats_batch_kernel, row for row, over up to two sets whose rows are dealt to the threads one
// after the other (a workgroup may hold the last rows of the first set and the first rows of the second).  The radii of a
// view are either contiguous int32 or fp32-coded integers (the last third of a gradient message's slot: exact below 2^24,
// converted with a round-to-nearest that has nothing to round).
struct SetsViews {
    const float* grad[MAX_VIEWS];
    const void* radii[MAX_VIEWS];
};
struct StatsSet {
    int row0, n;
    float *accum, *denom, *max_radii;
};

template <bool CODED>
__device__ __forceinline__ int radius_at(const void* radii, size_t row) {
    if (CODED) return __float2int_rn(static_cast<const float*>(radii)[row]);
    return static_cast<const int32_t*>(radii)[row];
}

template <bool CODED>
__global__ void __launch_bounds__(256)
densify_stats_sets_kernel(SetsViews V, int n_views, int vstride, StatsSet A, StatsSet B, float sx, float sy) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n + B.n) return;
    const bool second = t >= A.n;
    const int i = second ? t - A.n : t;
    const size_t row = (size_t)(second ? B.row0 : A.row0) + i;
    float* __restrict__ accum = second ? B.accum : A.accum;
    float* __restrict__ denom = second ? B.denom : A.denom;
    float* __restrict__ max_radii = second ? B.max_radii : A.max_radii;
    float gx = 0.f, gy = 0.f;
    int r = radius_at<CODED>(V.radii[0], row);
    for (int v = 0; v < n_views; ++v) {
        const float* g = V.grad[v] + row * vstride;
        gx = gx + g[0];
        gy = gy + g[1];
        r = max(r, radius_at<CODED>(V.radii[v], row));
    }
    gx = gx * sx;
    gy = gy * sy;
    if (!(r > 0)) return;  // visible in no view: not written
    max_radii[i] = fmaxf(max_radii[i], (float)r);
    accum[i] += __fsqrt_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)));
    denom[i] += 1.f;
}

// ---- the plan -----------------------------------------------------------------------------------------------------
struct PlanArgs {
    int op, n, n_split;
    const float *accum, *denom, *scaling, *opacity, *xyz, *bounds;
    const uint8_t* mask;
    float thr, size_thr, min_opacity;
};

// What becomes of row i: keep = it stays (first section), clone / split = it gets a new copy in the second / third
// section.  Every comparison is false on NaN, so a NaN row is kept and neither cloned nor split.
__device__ __forceinline__ void plan_flags(const PlanArgs& A, int i, bool& keep, bool& clone, bool& split) {
    clone = split = false;
    if (A.op == MOBGS_PLAN_PRUNECLONE) {  // the expression of densify_select_kernel (densify.hip) with n_grads = n
        float g = A.accum[i] / A.denom[i];
        if (g != g) g = 0.f;
        const float s = fmaxf(fmaxf(expf(A.scaling[3 * (size_t)i]), expf(A.scaling[3 * (size_t)i + 1])),
                              expf(A.scaling[3 * (size_t)i + 2]));
        const bool hot = fabsf(g) >= A.thr, hot_split = g >= A.thr, big = s > A.size_thr;
        clone = hot && !big;
        split = hot_split && big;
        keep = !split;
    } else if (A.op == MOBGS_PLAN_PRUNE_OPACITY) {
        keep = !(1.f / (1.f + expf(-A.opacity[i])) < A.min_opacity);
    } else if (A.op == MOBGS_PLAN_PRUNE_BOUNDS) {  // bounds = {max.x, max.y, max.z, min.x, min.y, min.z}, strict
        const float x = A.xyz[3 * (size_t)i], y = A.xyz[3 * (size_t)i + 1], z = A.xyz[3 * (size_t)i + 2];
        keep = !(x > A.bounds[0] || y > A.bounds[1] || z > A.bounds[2] || x < A.bounds[3] || y < A.bounds[4] ||
                 z < A.bounds[5]);
    } else {
        keep = A.mask[i] == 0;
    }
}

constexpr int PLAN_ROWS = 1024;  // rows per workgroup = threads per workgroup, 16 waves

// count pass: scratch[3 b + k] = rows of block b with flag k (keep, clone, split)
__global__ void __launch_bounds__(PLAN_ROWS) plan_count_kernel(PlanArgs A, int32_t* __restrict__ scratch) {
    __shared__ int wsum[3][16];
    const int i = blockIdx.x * PLAN_ROWS + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool f[3] = {false, false, false};
    if (i < A.n) plan_flags(A, i, f[0], f[1], f[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t ballot = __builtin_amdgcn_ballot_w64(f[k]);
        if (lane == 0) wsum[k][wv] = __builtin_popcountll(ballot);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += wsum[threadIdx.x][w];
        scratch[3 * (size_t)blockIdx.x + threadIdx.x] = tot;
    }
}

// write pass: every block sums the counts of the blocks before it and of all blocks (each thread a strided share, the 16
// wave sums meet in LDS), takes its rows' flags again and writes each row to its final place in every section:
//   [ keep, ascending | -(clone + 1), ascending | -(split + 1), ascending, the run n_split times over ]
// Every block reads the whole scratch, 12 bytes per block: 293 blocks read 3.5 KB each at 300 k rows, out of L2.  The reads
// grow with the square of the block count -- 1 GB in all at 10 M rows, where a scan of the counts between the passes would pay.
__global__ void __launch_bounds__(PLAN_ROWS)
plan_write_kernel(PlanArgs A, const int32_t* __restrict__ scratch, int n_blocks, int32_t* __restrict__ index,
                  int32_t* __restrict__ counts) {
    __shared__ int wsum[3][16];
    __shared__ int part[6][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int acc[6] = {0, 0, 0, 0, 0, 0};  // [k]: blocks before this one; [3 + k]: all blocks
    for (int j = threadIdx.x; j < n_blocks; j += PLAN_ROWS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = scratch[3 * (size_t)j + k];
            acc[3 + k] += c;
            if (j < (int)blockIdx.x) acc[k] += c;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int s = wave_sum(acc[k]);
        if (lane == 0) part[k][wv] = s;
    }
    const int i = blockIdx.x * PLAN_ROWS + threadIdx.x;
    bool f[3] = {false, false, false};
    if (i < A.n) plan_flags(A, i, f[0], f[1], f[2]);
    int before[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t ballot = __builtin_amdgcn_ballot_w64(f[k]);
        before[k] = __builtin_popcountll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[k][wv] = __builtin_popcountll(ballot);
    }
    __syncthreads();
    int base[3], total[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int b = 0, t = 0, off = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            b += part[k][w];
            t += part[3 + k][w];
            if (w < wv) off += wsum[k][w];
        }
        base[k] = b + off + before[k];
        total[k] = t;
    }
    if (f[0]) index[base[0]] = i;
    if (f[1]) index[total[0] + base[1]] = -(i + 1);
    if (f[2]) {
        int32_t* run = index + total[0] + total[1] + base[2];
        for (int r = 0; r < A.n_split; ++r) run[(size_t)r * total[2]] = -(i + 1);
    }
    if ((int)blockIdx.x == n_blocks - 1 && threadIdx.x < 4)
        counts[threadIdx.x] = threadIdx.x == 0 ? total[0] : threadIdx.x == 1 ? total[1] : threadIdx.x == 2 ? total[2]
                              : total[0] + total[1] + A.n_split * total[2];
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_densify_stats_batch(int n_views, const float* const* grads_host, int grad_stride,
                              const int32_t* const* radii_host, int row0, int n, float sx, float sy,
                              float* xyz_gradient_accum, float* denom, float* max_radii2D, float* grad_sum,
                              int32_t* radii_max, uint8_t* visible, void* stream) {
    if (n_views < 1 || n_views > MAX_VIEWS) {
        set_error("mobgs_densify_stats_batch: n_views = %d (1..%d)", n_views, MAX_VIEWS);
        return MOBGS_E_INVALID;
    }
    if (n < 0 || row0 < 0 || grad_stride < 2 || !grads_host || !radii_host ||
        (n > 0 && (!xyz_gradient_accum || !denom || !max_radii2D))) {
        set_error("mobgs_densify_stats_batch: bad arguments n=%d row0=%d stride=%d or a NULL table", n, row0, grad_stride);
        return MOBGS_E_INVALID;
    }
    BatchViews V;
    for (int v = 0; v < MAX_VIEWS; ++v) {
        V.grad[v] = v < n_views ? grads_host[v] : nullptr;
        V.radii[v] = v < n_views ? radii_host[v] : nullptr;
        if (v < n_views && n > 0 && (!V.grad[v] || !V.radii[v])) {
            set_error("mobgs_densify_stats_batch: view %d has a NULL pointer", v);
            return MOBGS_E_INVALID;
        }
    }
    if (n == 0) return MOBGS_OK;
    hipLaunchKernelGGL(densify_stats_batch_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, V, n_views,
                       grad_stride, row0, n, sx, sy, xyz_gradient_accum, denom, max_radii2D, grad_sum, radii_max, visible);
    return check_launch("densify_stats_batch_kernel");
}

int mobgs_densify_stats_sets(int n_views, const float* const* grads_host, int grad_stride, const void* const* radii_host,
                             int radii_encoding, float sx, float sy, int row0_a, int n_a, float* xyz_gradient_accum_a,
                             float* denom_a, float* max_radii2D_a, int row0_b, int n_b, float* xyz_gradient_accum_b,
                             float* denom_b, float* max_radii2D_b, void* stream) {
    if (n_views < 1 || n_views > MAX_VIEWS) {
        set_error("mobgs_densify_stats_sets: n_views = %d (1..%d)", n_views, MAX_VIEWS);
        return MOBGS_E_INVALID;
    }
    if (radii_encoding != MOBGS_RADII_INT32 && radii_encoding != MOBGS_RADII_FP32) {
        set_error("mobgs_densify_stats_sets: radii_encoding = %d (MOBGS_RADII_INT32 or MOBGS_RADII_FP32)", radii_encoding);
        return MOBGS_E_INVALID;
    }
    if (n_a < 0 || n_b < 0 || row0_a < 0 || row0_b < 0 || grad_stride < 2 || !grads_host || !radii_host ||
        (long long)n_a + n_b > 2147483647ll ||
        (n_a > 0 && (!xyz_gradient_accum_a || !denom_a || !max_radii2D_a)) ||
        (n_b > 0 && (!xyz_gradient_accum_b || !denom_b || !max_radii2D_b))) {
        set_error("mobgs_densify_stats_sets: bad arguments n=%d+%d row0=%d,%d stride=%d or a NULL table", n_a, n_b, row0_a,
                  row0_b, grad_stride);
        return MOBGS_E_INVALID;
    }
    SetsViews V;
    for (int v = 0; v < MAX_VIEWS; ++v) {
        V.grad[v] = v < n_views ? grads_host[v] : nullptr;
        V.radii[v] = v < n_views ? radii_host[v] : nullptr;
        if (v < n_views && n_a + n_b > 0 && (!V.grad[v] || !V.radii[v])) {
            set_error("mobgs_densify_stats_sets: view %d has a NULL pointer", v);
            return MOBGS_E_INVALID;
        }
    }
    if (n_a + n_b == 0) return MOBGS_OK;
    const StatsSet A = {row0_a, n_a, xyz_gradient_accum_a, denom_a, max_radii2D_a};
    const StatsSet B = {row0_b, n_b, xyz_gradient_accum_b, denom_b, max_radii2D_b};
    const dim3 grid((n_a + n_b + 255) / 256), block(256);
    if (radii_encoding == MOBGS_RADII_FP32)
        hipLaunchKernelGGL(densify_stats_sets_kernel<true>, grid, block, 0, (hipStream_t)stream, V, n_views, grad_stride, A,
                           B, sx, sy);
    else
        hipLaunchKernelGGL(densify_stats_sets_kernel<false>, grid, block, 0, (hipStream_t)stream, V, n_views, grad_stride, A,
                           B, sx, sy);
    return check_launch("densify_stats_sets_kernel");
}

int mobgs_densify_plan(int op, int n, int n_split, const float* xyz_gradient_accum, const float* denom,
                       const float* scaling, float grad_threshold, float size_threshold, const float* opacity,
                       float min_opacity, const float* xyz, const float* bounds, const uint8_t* mask, int32_t* index,
                       int32_t* counts, int32_t* scratch, void* stream) {
    if (n_split < 1 || n_split > 8) {
        set_error("mobgs_densify_plan: n_split = %d (1..8)", n_split);
        return MOBGS_E_INVALID;
    }
    if (op < MOBGS_PLAN_PRUNECLONE || op > MOBGS_PLAN_PRUNE_MASK || n < 0 || !counts ||
        (long long)n * (n_split > 2 ? n_split : 2) > 2147483647ll) {
        set_error("mobgs_densify_plan: bad arguments op=%d n=%d n_split=%d or no counts", op, n, n_split);
        return MOBGS_E_INVALID;
    }
    if (n == 0) {
        const hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), (hipStream_t)stream);
        if (e != hipSuccess) {
            set_error("mobgs_densify_plan: clearing the counts: %s", hipGetErrorString(e));
            return MOBGS_E_LAUNCH;
        }
        return MOBGS_OK;
    }
    const bool has_inputs = op == MOBGS_PLAN_PRUNECLONE ? (xyz_gradient_accum && denom && scaling)
                          : op == MOBGS_PLAN_PRUNE_OPACITY ? opacity != nullptr
                          : op == MOBGS_PLAN_PRUNE_BOUNDS ? (xyz && bounds) : mask != nullptr;
    if (!has_inputs || !index || !scratch) {
        set_error("mobgs_densify_plan: op %d is missing an input array, the list or the scratch", op);
        return MOBGS_E_INVALID;
    }
    PlanArgs A;
    A.op = op, A.n = n, A.n_split = n_split;
    A.accum = xyz_gradient_accum, A.denom = denom, A.scaling = scaling, A.opacity = opacity, A.xyz = xyz, A.bounds = bounds;
    A.mask = mask;
    A.thr = grad_threshold, A.size_thr = size_threshold, A.min_opacity = min_opacity;
    const int n_blocks = (n + PLAN_ROWS - 1) / PLAN_ROWS;
    hipLaunchKernelGGL(plan_count_kernel, dim3(n_blocks), dim3(PLAN_ROWS), 0, (hipStream_t)stream, A, scratch);
    int rc = check_launch("plan_count_kernel");
    if (rc != MOBGS_OK) return rc;
    hipLaunchKernelGGL(plan_write_kernel, dim3(n_blocks), dim3(PLAN_ROWS), 0, (hipStream_t)stream, A, scratch, n_blocks,
                       index, counts);
    return check_launch("plan_write_kernel");
}

}  // extern "C"

// K18: drop one spline control point per dynamic Gaussian (the reference's GaussianModel.onedown_control_pts,
// scene/gaussian_model.py:274-371: inverse_cubic_hermite_for_prune + compute_prune_error + the commit).  gfx950 only.
//
// A row with n control points (old knot times k / (n - 1)) is refitted with m = n - 1 points in the least-squares
// sense.  The design matrix of that fit depends on n only, so the whole fit is
//     new[j] = sum_k P_n[j][k] old[k],   P_n = pinv(hermite_design(k / (n - 1), m))   (float64 on the host, fp32 here)
// with one zero-padded [11, 12] block of `pinv_table` per n = 5..12.  Both splines are then evaluated at the time of
// every interior view, projected with that view's world-to-camera matrix and K = [focal, focal, cx, cy], and the
// pixel distance is averaged.  Rows with n == 4 are not candidates (the reference floors m at 4 and its dummy
// equation then fights the real ones over the fourth point: DESIGN.md); they report error 0 and are never written.
//
// One wave per workgroup, one row per lane.  The 144-byte control rows of the 64 rows are staged through LDS with
// coalesced loads; the lane's own row is read back into registers for the fit (static indices), the fitted points go
// to a second LDS array.  The spline evaluation indexes control points by a segment that depends on the lane's count
// and on the view time: both arrays are read from LDS there (odd row strides: lanes hit different banks), so nothing
// is indexed dynamically in registers and the kernel needs no scratch.  Camera records are addressed by the loop
// counter only and arrive through scalar loads.  Every row is read completely (into LDS) before the barrier and
// written only after it, by its own workgroup: the in-place commit is safe.
//
// Expression order follows the reference where a choice exists: the Hermite basis as in interpolate_cubic_hermite
// (:373-400), `* 1e-2`, the homogeneous divide by (w + 1e-7) (geom_transform_points) and the pinhole divide by
// (z + 1e-7) with u = f x + cx z (cam2pixel multiplies by K before it divides).
#include "common.h"

namespace mobgs {

constexpr int CP_MAX = 12;                 // control points per row (GaussianModel.control_num)
constexpr int CP_ROWS = 64;                // rows per workgroup = lanes
constexpr int CP_OLD_STRIDE = 37;          // floats per staged row (36 + 1: odd, so lanes fall on different banks)
constexpr int CP_NEW_STRIDE = 33;          // 11 fitted points
constexpr int CP_TABLE = 8 * 11 * 12;      // floats in pinv_table

// The cubic Hermite spline through `N` of the points at p (LDS, xyz interleaved) at time `time`, times 1e-2.
__device__ __forceinline__ void cp_spline(const float* p, int N, float time, float& x, float& y, float& z) {
    const float ts = time * (float)(N - 1);
    int i = (int)floorf(ts);
    i = min(max(i, 0), N - 2);
    const int il = max(i - 1, 0), ir = min(i + 1, N - 1), irr = min(i + 2, N - 1);
    const float t = ts - (float)i;
    const float omt = 1.f - t;
    const float h00 = (1.f + 2.f * t) * (omt * omt);
    const float h10 = t * (omt * omt);
    const float h01 = (t * t) * (3.f - 2.f * t);
    const float h11 = (t * t) * (t - 1.f);
    const bool first = il == i, last = irr == ir;
    float out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p0 = p[3 * il + c], p1 = p[3 * i + c], p2 = p[3 * ir + c], p3 = p[3 * irr + c];
        const float m0 = first ? (p2 - p1) : (p2 - p0) / 2.f;
        const float m1 = last ? (p2 - p1) : (p3 - p1) / 2.f;
        out[c] = (((h00 * p1 + h10 * m0) + h01 * p2) + h11 * m1) * 1e-2f;
    }
    x = out[0], y = out[1], z = out[2];
}

// pts2pixel: row-major world-to-camera matrix M (column-vector convention), K = [f, 0, cx; 0, f, cy; 0, 0, 1]
__device__ __forceinline__ void cp_project(const float* __restrict__ M, float f, float cx, float cy, float x, float y,
                                           float z, float& u, float& v) {
    const float w = ((M[12] * x + M[13] * y) + M[14] * z) + M[15];
    const float dw = w + 0.0000001f;
    const float xc = (((M[0] * x + M[1] * y) + M[2] * z) + M[3]) / dw;
    const float yc = (((M[4] * x + M[5] * y) + M[6] * z) + M[7]) / dw;
    const float zc = (((M[8] * x + M[9] * y) + M[10] * z) + M[11]) / dw;
    const float dz = zc + 0.0000001f;
    u = (f * xc + cx * zc) / dz;
    v = (f * yc + cy * zc) / dz;
}

__global__ void __launch_bounds__(CP_ROWS) control_onedown_kernel(
    int n_rows, int n_views, const float* __restrict__ viewmats, const float* __restrict__ times, float focal, float cx,
    float cy, const float* __restrict__ pinv_table, float threshold, float* control_xyz, int64_t* control_num,
    float* __restrict__ err_out, float* __restrict__ new_out, int* __restrict__ counters, int commit) {
    __shared__ __attribute__((aligned(16))) float s_table[CP_TABLE];
    __shared__ float s_old[CP_ROWS * CP_OLD_STRIDE];
    __shared__ float s_new[CP_ROWS * CP_NEW_STRIDE];
    __shared__ int s_write[CP_ROWS];

    const int lane = threadIdx.x;
    const int base = blockIdx.x * CP_ROWS;
    const int rows_here = min(CP_ROWS, n_rows - base);
    const int row = base + lane;
    const bool valid = lane < rows_here;

    // ---- stage the table and the workgroup's rows (consecutive lanes read consecutive floats) ----------------------
    for (int i = lane; i < CP_TABLE; i += CP_ROWS) s_table[i] = pinv_table[i];
    const float* src = control_xyz + (size_t)base * (CP_MAX * 3);
    for (int i = lane; i < rows_here * (CP_MAX * 3); i += CP_ROWS) {
        const int r = i / (CP_MAX * 3);
        s_old[r * CP_OLD_STRIDE + (i - r * (CP_MAX * 3))] = src[i];
    }
    const int64_t n64 = valid ? control_num[row] : (int64_t)4;
    const bool bad = n64 < 4 || n64 > CP_MAX;
    const int n = bad ? 4 : (int)n64;        // a count outside 4..12 is reported, never used as an index
    const bool candidate = valid && !bad && n >= 5;
    const int m = candidate ? n - 1 : n;
    __syncthreads();

    // ---- the fit: new[j] = sum_k P_n[j][k] old[k]; slots k >= n hold anything (NaN included) and are masked --------
    float* my_old = s_old + lane * CP_OLD_STRIDE;
    float* my_new = s_new + lane * CP_NEW_STRIDE;
    {
        float o[CP_MAX * 3];
#pragma unroll
        for (int k = 0; k < CP_MAX; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = valid ? my_old[3 * k + c] : 0.f;
                o[3 * k + c] = (k < n) ? v : 0.f;
            }
        }
        const float4* tab = reinterpret_cast<const float4*>(s_table + (candidate ? n - 5 : 0) * (11 * CP_MAX));
#pragma unroll
        for (int j = 0; j < CP_MAX - 1; ++j) {
            const float4 a = tab[3 * j], b = tab[3 * j + 1], d = tab[3 * j + 2];
            const float w[CP_MAX] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
            float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
            for (int k = 0; k < CP_MAX; ++k) {
                sx += w[k] * o[3 * k];
                sy += w[k] * o[3 * k + 1];
                sz += w[k] * o[3 * k + 2];
            }
            // a row that is no candidate keeps its points: what it reports as "new" is what it has
            my_new[3 * j] = candidate ? sx : o[3 * j];
            my_new[3 * j + 1] = candidate ? sy : o[3 * j + 1];
            my_new[3 * j + 2] = candidate ? sz : o[3 * j + 2];
        }
    }
    // (each lane reads back only what it wrote itself: no barrier needed before the view loop)

    // ---- mean pixel distance over the interior views -------------------------------------------------------------
    float sum = 0.f;
    if (__ballot(candidate) != 0ull) {
#pragma unroll 1
        for (int v = 1; v < n_views - 1; ++v) {
            const float* __restrict__ M = viewmats + (size_t)v * 16;   // wave-uniform: scalar loads
            const float time = times[v];
            float x0, y0, z0, x1, y1, z1, u0, v0, u1, v1;
            cp_spline(my_old, n, time, x0, y0, z0);
            cp_spline(my_new, m, time, x1, y1, z1);
            cp_project(M, focal, cx, cy, x0, y0, z0, u0, v0);
            cp_project(M, focal, cx, cy, x1, y1, z1, u1, v1);
            const float du = u0 - u1, dv = v0 - v1;
            sum += sqrtf(du * du + dv * dv);
        }
    }
    const float err = candidate ? sum / (float)(n_views - 2) : 0.f;
    const bool prune = candidate && commit != 0 && err <= threshold;   // (NaN compares false: the row stays)
    if (valid) err_out[row] = err;

    // ---- counters: one atomic per wave and counter ------------------------------------------------------------------
    const unsigned long long pm = __ballot(prune), bm = __ballot(valid && bad);
    if (pm != 0ull && lane == __ffsll((long long)pm) - 1) atomicAdd(&counters[0], __popcll(pm));
    if (bm != 0ull && lane == __ffsll((long long)bm) - 1) atomicAdd(&counters[1], __popcll(bm));

    // ---- outputs, again with consecutive lanes on consecutive floats -------------------------------------------------
    s_write[lane] = prune ? 1 : 0;
    if (prune) control_num[row] = (int64_t)m;
    __syncthreads();
    if (new_out) {
        float* dst = new_out + (size_t)base * ((CP_MAX - 1) * 3);
        for (int i = lane; i < rows_here * CP_NEW_STRIDE; i += CP_ROWS) dst[i] = s_new[i];
    }
    if (pm != 0ull) {
        float* dst = control_xyz + (size_t)base * (CP_MAX * 3);
        for (int i = lane; i < rows_here * CP_NEW_STRIDE; i += CP_ROWS) {
            const int r = i / CP_NEW_STRIDE;
            if (s_write[r]) dst[r * (CP_MAX * 3) + (i - r * CP_NEW_STRIDE)] = s_new[i];   // slot 11 stays
        }
    }
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_control_onedown(int n_rows, int n_views, const float* viewmats, const float* times, float focal, float cx,
                          float cy, const float* pinv_table, float threshold, float* control_xyz, int64_t* control_num,
                          float* err_out, float* new_control_out, int* counters, int commit, void* stream) {
    if (n_views < 3) {
        set_error("mobgs_control_onedown: n_views = %d; the first and the last view are skipped, so at least 3 are "
                  "needed", n_views);
        return MOBGS_E_INVALID;
    }
    if (n_rows < 0) {
        set_error("mobgs_control_onedown: n_rows = %d", n_rows);
        return MOBGS_E_INVALID;
    }
    if (!pinv_table) {
        set_error("mobgs_control_onedown: NULL pinv_table (float32 [8,11,12], mobgs_amd.scene_init.one_down_tables)");
        return MOBGS_E_INVALID;
    }
    if (n_rows == 0) return MOBGS_OK;
    if (!viewmats || !times || !control_xyz || !control_num || !err_out || !counters) {
        set_error("mobgs_control_onedown: NULL buffer");
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)pinv_table & 3) || ((uintptr_t)control_xyz & 3) || ((uintptr_t)control_num & 7)) {
        set_error("mobgs_control_onedown: misaligned buffer");
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(control_onedown_kernel, dim3((unsigned)((n_rows + CP_ROWS - 1) / CP_ROWS)), dim3(CP_ROWS), 0,
                       (hipStream_t)stream, n_rows, n_views, viewmats, times, focal, cx, cy, pinv_table, threshold,
                       control_xyz, control_num, err_out, new_control_out, counters, commit);
    return check_launch("mobgs_control_onedown");
}

}  // extern "C"

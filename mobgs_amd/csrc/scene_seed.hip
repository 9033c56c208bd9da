// K19: seeding the two Gaussian sets from depth maps, poses and 2-D tracks (the numerical part of the reference's
// scene_initialization, train.py:58-199).  gfx950 only.  Three launches, no float atomics, no host synchronisation:
//
//   seed_consistency_kernel   every view i is compared with every view j through i's depth map: pixel (u, v) of i with
//                             depth d lands in j at the homogeneous pixel P_ij (d u, d v, d, 1)^T, where
//                             P_ij = K_j [R_j R_i^T | t_j - R_j R_i^T t_i] K_i^-1 is one 3x4 row of `pair_table`
//                             (float64 on the host, rounded once).  One lane per target pixel, the lane loops over j; the
//                             row is addressed by blockIdx.y and the loop counter only and arrives through scalar loads.
//                             What inverse_warp_rt1_rt2 + grid_sample + the masked mean are per (i, j) -- about 25 torch
//                             launches -- is one loop iteration here.  Writes accum_error and one partial sum per workgroup.
//   seed_classify_kernel      sums the partials of its view in a fixed order (every workgroup of the view does, so the
//                             mean is the same number everywhere and needs no atomics), thresholds, classifies and
//                             unprojects: world = U_i (d u, d v, d, 1)^T with U_i = [R_i^T K_i^-1 | -R_i^T t_i].
//   seed_trajectories_kernel  nearest 2-D track per chosen pixel (argmin of the squared distance over all M tracks,
//                             start positions staged through LDS in chunks of 1024) and that track's 3-D trajectory, read
//                             out of the per-view point maps by nearest-pixel lookup.
//
// Ordered to match torch: the squared distance (dx dx + dy dy) -- this file is built with -ffp-contract=off, so the
// compare is bit-equal with torch's square().sum(-1) and ties resolve to the lowest index as argmin does -- and the
// sampling rules (the |z| < 1e-6 clamp, normalisation by W - 1 / H - 1, "outside [-1, 1] samples zero", the tap order
// nw, ne, sw, se of grid_sample, mask = (channel sum > 0), mean over 3 channels).  Not ordered to match: the chain of
// four 3x3 products per pixel is one 3x4 product here, so reprojections differ from the reference's in the last bits.
//
// The sampling rules are stated in two more places, which change with this file: the float64 composition for host
// tensors (mobgs_amd/scene_init.py: _seed_maps_host and the host branch of track_trajectories) and the restatement the
// tests compare against (tests/seed_restatement.py).
#include "reduce_shared.h"

namespace mobgs {

constexpr int SEED_BLOCK = 256;            // lanes per workgroup, one pixel / one point each
constexpr int SEED_WAVES = SEED_BLOCK / MOBGS_WAVE;
constexpr int SEED_CHUNK = 1024;           // track start positions per LDS chunk

__host__ __device__ inline int seed_tiles(int H, int W) { return (H * W + SEED_BLOCK - 1) / SEED_BLOCK; }

static_assert(SEED_WAVES == 4, "block_sum4 adds four wave sums");

__global__ void __launch_bounds__(SEED_BLOCK) seed_consistency_kernel(
    int V, int H, int W, const float* __restrict__ images, const float* __restrict__ depths,
    const float* __restrict__ pair_table, float* __restrict__ accum_error, float* __restrict__ partials) {
    __shared__ float s_wave[SEED_WAVES];
    const int HW = H * W;
    const int i = blockIdx.y;
    const int p = blockIdx.x * SEED_BLOCK + threadIdx.x;
    const bool valid = p < HW;
    const int pc = valid ? p : 0;            // lanes past the image work on pixel 0 and write nothing
    const int v = pc / W, u = pc - v * W;
    const float* __restrict__ img_i = images + (size_t)i * 3 * HW;
    const float d = depths[(size_t)i * HW + pc];
    const float c0 = img_i[pc], c1 = img_i[HW + pc], c2 = img_i[2 * (size_t)HW + pc];
    const float du = d * (float)u, dv = d * (float)v;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);

    float acc = 0.f;
#pragma unroll 1
    for (int j = 0; j < V; ++j) {
        const float* __restrict__ P = pair_table + ((size_t)i * V + j) * 12;   // workgroup-uniform: scalar loads
        const float px = ((P[0] * du + P[1] * dv) + P[2] * d) + P[3];
        const float py = ((P[4] * du + P[5] * dv) + P[6] * d) + P[7];
        float z = ((P[8] * du + P[9] * dv) + P[10] * d) + P[11];
        if (fabsf(z) < 1e-6f) z = 1e-6f;
        const float xn = 2.f * (px / z) / wm1 - 1.f;
        const float yn = 2.f * (py / z) / hm1 - 1.f;
        // (written so that a NaN coordinate counts as outside)
        const bool inside = xn >= -1.f && xn <= 1.f && yn >= -1.f && yn <= 1.f;
        float contrib = 0.f;
        if (inside) {
            const float* __restrict__ img_j = images + (size_t)j * 3 * HW;
            const float ix = ((xn + 1.f) / 2.f) * wm1, iy = ((yn + 1.f) / 2.f) * hm1;
            const float fx = floorf(ix), fy = floorf(iy);
            const int x0 = (int)fx, y0 = (int)fy;               // in [0, W-1] / [0, H-1] up to rounding: checked below
            const float w_nw = ((fx + 1.f) - ix) * ((fy + 1.f) - iy);
            const float w_ne = (ix - fx) * ((fy + 1.f) - iy);
            const float w_sw = ((fx + 1.f) - ix) * (iy - fy);
            const float w_se = (ix - fx) * (iy - fy);
            const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
            const bool ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
            const int xs0 = xa ? x0 : 0, xs1 = xb ? x0 + 1 : 0, ys0 = ya ? y0 : 0, ys1 = yb ? y0 + 1 : 0;
            const int o_nw = ys0 * W + xs0, o_ne = ys0 * W + xs1, o_sw = ys1 * W + xs0, o_se = ys1 * W + xs1;
            const float m_nw = (xa && ya) ? w_nw : 0.f, m_ne = (xb && ya) ? w_ne : 0.f;
            const float m_sw = (xa && yb) ? w_sw : 0.f, m_se = (xb && yb) ? w_se : 0.f;
            float s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* __restrict__ ch = img_j + (size_t)c * HW;
                // a tap outside the image contributes nothing (zero padding); its address was clamped to pixel 0
                s[c] = ((ch[o_nw] * m_nw + ch[o_ne] * m_ne) + ch[o_sw] * m_sw) + ch[o_se] * m_se;
            }
            if ((s[0] + s[1]) + s[2] > 0.f)
                contrib = ((fabsf(s[0] - c0) + fabsf(s[1] - c1)) + fabsf(s[2] - c2)) / 3.f;
        }
        acc += contrib;
    }
    if (valid) accum_error[(size_t)i * HW + p] = acc;
    const float total = block_sum4(valid ? acc : 0.f, s_wave);
    if (threadIdx.x == 0) partials[(size_t)i * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(SEED_BLOCK) seed_classify_kernel(
    int V, int H, int W, const float* __restrict__ accum_error, const float* __restrict__ partials,
    const float* __restrict__ depths, const uint8_t* __restrict__ motion, const float* __restrict__ unproject_table,
    uint8_t* __restrict__ inconsistent, uint8_t* __restrict__ cls, float* __restrict__ points,
    float* __restrict__ mean_out) {
    __shared__ float s_wave[SEED_WAVES];
    const int HW = H * W;
    const int tiles = gridDim.x;
    const int i = blockIdx.y;
    // ---- the view's mean: lane t takes partials t, t + 256, ... in order, then the fixed-order workgroup sum ----------
    float part = 0.f;
    for (int k = threadIdx.x; k < tiles; k += SEED_BLOCK) part += partials[(size_t)i * tiles + k];
    const float mean = block_sum4(part, s_wave) / (float)HW;
    if (blockIdx.x == 0 && threadIdx.x == 0) mean_out[i] = mean;

    const int p = blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (p >= HW) return;
    const int v = p / W, u = p - v * W;
    const size_t at = (size_t)i * HW + p;
    const bool inc = accum_error[at] > mean;
    const uint8_t mo = motion[at];            // 0 = still, 1 = moving, anything else = neither
    inconsistent[at] = inc ? 1 : 0;
    cls[at] = (!inc && mo == 0) ? 0 : ((inc && mo == 1) ? 1 : 2);
    const float* __restrict__ U = unproject_table + (size_t)i * 12;   // workgroup-uniform: scalar loads
    const float d = depths[at];
    const float du = d * (float)u, dv = d * (float)v;
    float* __restrict__ out = points + at * 3;
    out[0] = ((U[0] * du + U[1] * dv) + U[2] * d) + U[3];
    out[1] = ((U[4] * du + U[5] * dv) + U[6] * d) + U[7];
    out[2] = ((U[8] * du + U[9] * dv) + U[10] * d) + U[11];
}

__global__ void __launch_bounds__(SEED_BLOCK) seed_trajectories_kernel(
    int N, int T, int M, int H, int W, const float* __restrict__ coords, const float* __restrict__ tracklet,
    const float* __restrict__ points, int32_t* __restrict__ track_index, float* __restrict__ trajectory) {
    __shared__ float2 s_start[SEED_CHUNK];
    const int n = blockIdx.x * SEED_BLOCK + threadIdx.x;
    const bool valid = n < N;
    const float cx = valid ? coords[2 * (size_t)n] : 0.f, cy = valid ? coords[2 * (size_t)n + 1] : 0.f;
    const float2* __restrict__ start = reinterpret_cast<const float2*>(tracklet);   // tracklet[0]: [M, 2]
    float best = __builtin_inff();
    int idx = 0;
    for (int m0 = 0; m0 < M; m0 += SEED_CHUNK) {
        const int len = min(SEED_CHUNK, M - m0);
        __syncthreads();                       // (the previous chunk has been read by every lane)
        for (int k = threadIdx.x; k < len; k += SEED_BLOCK) s_start[k] = start[m0 + k];
        __syncthreads();
        for (int k = 0; k < len; ++k) {        // every lane reads the same address: an LDS broadcast
            const float2 s = s_start[k];
            const float dx = cx - s.x, dy = cy - s.y;
            const float dist = dx * dx + dy * dy;
            if (dist < best) {                 // strict: ties stay with the lowest index, as torch.argmin
                best = dist;
                idx = m0 + k;
            }
        }
    }
    if (!valid) return;
    track_index[n] = idx;
    const size_t HW = (size_t)H * W;
    for (int t = 0; t < T; ++t) {
        const float2 uv = reinterpret_cast<const float2*>(tracklet)[(size_t)t * M + idx];
        // grid_sample(mode="nearest", align_corners=False) of (u / W) * 2 - 1: the pixel nearbyint(u - 0.5), ties to even
        const float fx = nearbyintf(uv.x - 0.5f), fy = nearbyintf(uv.y - 0.5f);
        float x = 0.f, y = 0.f, z = 0.f;
        if (fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H) {     // (false for NaN)
            const float* __restrict__ src = points + ((size_t)t * HW + (size_t)((int)fy * W + (int)fx)) * 3;
            x = src[0], y = src[1], z = src[2];
        }
        float* __restrict__ dst = trajectory + ((size_t)n * T + t) * 3;
        dst[0] = x, dst[1] = y, dst[2] = z;
    }
}

// sizes every entry point accepts: H * W up to 2^28 pixels, V up to 4096 views
static bool seed_shape_in_range(int V, int H, int W) {
    return V >= 2 && V <= 4096 && H >= 2 && W >= 2 && (int64_t)H * W <= ((int64_t)1 << 28);
}
static bool seed_shape_ok(const char* what, int V, int H, int W) {
    if (!seed_shape_in_range(V, H, W)) {
        set_error("%s: V = %d, H = %d, W = %d; need 2 <= V <= 4096, H >= 2, W >= 2 and H * W <= 2^28", what, V, H, W);
        return false;
    }
    return true;
}
// the partial sums handed from mobgs_seed_consistency to mobgs_seed_classify, and the 3x4 table rows
static bool seed_buffers_ok(const char* what, int V, int H, int W, const void* scratch, size_t scratch_bytes,
                            const float* table, const char* table_name) {
    const size_t need = (size_t)V * (size_t)seed_tiles(H, W) * sizeof(float);
    if (scratch_bytes < need) {
        set_error("%s: scratch holds %zu bytes, mobgs_seed_scratch_bytes asks for %zu", what, scratch_bytes, need);
        return false;
    }
    if (((uintptr_t)scratch & 3) || ((uintptr_t)table & 3)) {
        set_error("%s: scratch and %s must be 4-byte aligned", what, table_name);
        return false;
    }
    return true;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

size_t mobgs_seed_scratch_bytes(int V, int H, int W) {
    if (!seed_shape_in_range(V, H, W)) return 0;
    return (size_t)V * (size_t)seed_tiles(H, W) * sizeof(float);
}

int mobgs_seed_consistency(int V, int H, int W, const float* images, const float* depths, const float* pair_table,
                           float* accum_error, void* scratch, size_t scratch_bytes, void* stream) {
    if (!seed_shape_ok("mobgs_seed_consistency", V, H, W)) return MOBGS_E_INVALID;
    if (!images || !depths || !pair_table || !accum_error || !scratch) {
        set_error("mobgs_seed_consistency: NULL buffer");
        return MOBGS_E_INVALID;
    }
    if (!seed_buffers_ok("mobgs_seed_consistency", V, H, W, scratch, scratch_bytes, pair_table, "pair_table"))
        return MOBGS_E_INVALID;
    hipLaunchKernelGGL(seed_consistency_kernel, dim3((unsigned)seed_tiles(H, W), (unsigned)V), dim3(SEED_BLOCK), 0,
                       (hipStream_t)stream, V, H, W, images, depths, pair_table, accum_error, (float*)scratch);
    return check_launch("mobgs_seed_consistency");
}

int mobgs_seed_classify(int V, int H, int W, const float* accum_error, const void* scratch, size_t scratch_bytes,
                        const float* depths, const uint8_t* motion, const float* unproject_table,
                        uint8_t* inconsistent, uint8_t* cls, float* points, float* mean, void* stream) {
    if (!seed_shape_ok("mobgs_seed_classify", V, H, W)) return MOBGS_E_INVALID;
    if (!accum_error || !scratch || !depths || !motion || !unproject_table || !inconsistent || !cls || !points ||
        !mean) {
        set_error("mobgs_seed_classify: NULL buffer");
        return MOBGS_E_INVALID;
    }
    if (!seed_buffers_ok("mobgs_seed_classify", V, H, W, scratch, scratch_bytes, unproject_table, "unproject_table"))
        return MOBGS_E_INVALID;
    hipLaunchKernelGGL(seed_classify_kernel, dim3((unsigned)seed_tiles(H, W), (unsigned)V), dim3(SEED_BLOCK), 0,
                       (hipStream_t)stream, V, H, W, accum_error, (const float*)scratch, depths, motion,
                       unproject_table, inconsistent, cls, points, mean);
    return check_launch("mobgs_seed_classify");
}

int mobgs_seed_trajectories(int N, int T, int M, int V, int H, int W, const float* coords, const float* tracklet,
                            const float* points, int32_t* track_index, float* trajectory, void* stream) {
    if (!seed_shape_ok("mobgs_seed_trajectories", V, H, W)) return MOBGS_E_INVALID;
    if (T != V) {
        set_error("mobgs_seed_trajectories: the tracklet has %d frames, the point maps %d views; one frame per view "
                  "is needed", T, V);
        return MOBGS_E_INVALID;
    }
    if (N < 0 || M < 1 || N > (1 << 28) || M > (1 << 28)) {
        set_error("mobgs_seed_trajectories: N = %d points, M = %d tracks; need 0 <= N <= 2^28, 1 <= M <= 2^28", N, M);
        return MOBGS_E_INVALID;
    }
    if (N == 0) return MOBGS_OK;
    if (!coords || !tracklet || !points || !track_index || !trajectory) {
        set_error("mobgs_seed_trajectories: NULL buffer");
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)tracklet & 7) || ((uintptr_t)coords & 3)) {
        set_error("mobgs_seed_trajectories: tracklet must be 8-byte aligned, coords 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(seed_trajectories_kernel, dim3((unsigned)((N + SEED_BLOCK - 1) / SEED_BLOCK)), dim3(SEED_BLOCK),
                       0, (hipStream_t)stream, N, T, M, H, W, coords, tracklet, points, track_index, trajectory);
    return check_launch("mobgs_seed_trajectories");
}

}  // extern "C"

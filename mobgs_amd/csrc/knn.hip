// K17: exact 3-nearest-neighbour mean squared distance (the reference's simple_knn distCUDA2, which sets every initial
// scale in create_from_pcd*).  gfx950 only.
//
//   dist2[i] = (d0 + d1 + d2) / 3,  d0 <= d1 <= d2 the three smallest pair_dist2(p_i, p_j) over j != i
//
// Exactness.  pair_dist2 is ONE fp32 expression, ((dx dx + dy dy) + dz dz), compiled without FMA contraction
// (build.EXTRA_FLAGS): it is symmetric in its arguments and the same for every pair on every path.  The result is a
// function of the MULTISET of those values only (sorted insert, fixed summation order), so it does not depend on the
// order of the rows, on the launch geometry or on which boxes were skipped.
//
// Pruning.  Rows are taken as they come, in boxes of KNN_BOX consecutive rows and super-boxes of KNN_SUPER boxes,
// each with a min/max AABB.  box_dist2 evaluates the SAME expression on the per-axis gaps to the AABB; fp32
// subtraction, multiplication and addition are monotonic under round-to-nearest, so box_dist2(p, B) <= pair_dist2(p, q)
// for every q in B *in fp32*, not just in exact arithmetic.  A box is skipped by a wave only when no lane has
// box_dist2 < best[2]: then no row of it can change any lane's three smallest values.  Skipping is therefore exact for
// ANY row order; the order decides only how much is skipped (callers pass rows sorted along a Morton curve).
//
// One wave per workgroup, one row per lane: a box that some lane still needs is staged through LDS with coalesced
// loads and read back as broadcasts, every lane updating its sorted best-3 in registers (the update is a no-op for
// lanes that did not need the box).
#include "common.h"
#include "wave_shared.h"

namespace mobgs {

constexpr int KNN_BOX = 256;             // rows per box
constexpr int KNN_SUPER = 16;            // boxes per super-box
constexpr int KNN_SUPER_ROWS = KNN_BOX * KNN_SUPER;
constexpr int KNN_MAX_N = 1 << 30;       // n + KNN_SUPER_ROWS must not wrap a 32-bit index

__host__ __device__ inline size_t knn_boxes(size_t n) { return (n + KNN_BOX - 1) / KNN_BOX; }
__host__ __device__ inline size_t knn_supers(size_t n) { return (n + KNN_SUPER_ROWS - 1) / KNN_SUPER_ROWS; }

__device__ __forceinline__ float pair_dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}
// lower bound (in fp32, see above) of pair_dist2(p, q) over the rows q of a box
__device__ __forceinline__ float box_dist2(float px, float py, float pz, const float4& lo, const float4& hi) {
    const float ex = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f);
    const float ey = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f);
    const float ez = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}

// One workgroup (4 waves) per super-box; wave w reduces boxes 4w .. 4w+3 of it, lane l rows l, l+64, l+128, l+192 of a box.
// aabb[2b] = min corner, aabb[2b+1] = max corner of box b; the super-boxes follow the n_box boxes.  A box without rows
// gets (+inf, -inf): its distance to anything is +inf.
__global__ void __launch_bounds__(256) knn_aabb_kernel(int n, const float* __restrict__ pts, float4* __restrict__ aabb) {
    __shared__ float red[KNN_SUPER][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_box = (int)knn_boxes((size_t)n);
    const float inf = __builtin_inff();
#pragma unroll 1
    for (int k = 0; k < KNN_SUPER / 4; ++k) {
        const int local = wave * (KNN_SUPER / 4) + k;
        const int b = blockIdx.x * KNN_SUPER + local;
        float lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
#pragma unroll
        for (int r = 0; r < KNN_BOX / 64; ++r) {
            const int j = b * KNN_BOX + r * 64 + lane;
            if (j < n) {
                const float x = pts[3 * (size_t)j], y = pts[3 * (size_t)j + 1], z = pts[3 * (size_t)j + 2];
                lx = fminf(lx, x), ly = fminf(ly, y), lz = fminf(lz, z);
                hx = fmaxf(hx, x), hy = fmaxf(hy, y), hz = fmaxf(hz, z);
            }
        }
        lx = wave_min(lx), ly = wave_min(ly), lz = wave_min(lz);
        hx = wave_max(hx), hy = wave_max(hy), hz = wave_max(hz);
        if (lane == 0) {
            if (b < n_box) {
                aabb[2 * (size_t)b] = make_float4(lx, ly, lz, 0.f);
                aabb[2 * (size_t)b + 1] = make_float4(hx, hy, hz, 0.f);
            }
            red[local][0] = lx, red[local][1] = ly, red[local][2] = lz;
            red[local][3] = hx, red[local][4] = hy, red[local][5] = hz;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
#pragma unroll
        for (int k = 0; k < KNN_SUPER; ++k) {
            lx = fminf(lx, red[k][0]), ly = fminf(ly, red[k][1]), lz = fminf(lz, red[k][2]);
            hx = fmaxf(hx, red[k][3]), hy = fmaxf(hy, red[k][4]), hz = fmaxf(hz, red[k][5]);
        }
        const size_t s = (size_t)n_box + blockIdx.x;
        aabb[2 * s] = make_float4(lx, ly, lz, 0.f);
        aabb[2 * s + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

struct Best3 {
    float b0, b1, b2;  // sorted
    __device__ __forceinline__ void insert(float d) {
        const float t0 = fmaxf(b0, d);
        b0 = fminf(b0, d);
        const float t1 = fmaxf(b1, t0);
        b1 = fminf(b1, t0);
        b2 = fminf(b2, t1);
    }
};

// Stage box `b` in LDS and insert every row of it into each lane's best-3.  SELF: this is the box holding the wave's
// own rows; row `self` (the lane's own) is left out BY INDEX, so a duplicate of it still counts with distance 0.
template <bool SELF>
__device__ __forceinline__ void knn_scan_box(int b, int n, const float* __restrict__ pts, float4* stage, int lane,
                                             int self, float px, float py, float pz, Best3& best) {
    const float inf = __builtin_inff();
    __syncthreads();  // (one wave per workgroup) the previous box has been read by every lane
#pragma unroll
    for (int r = 0; r < KNN_BOX / 64; ++r) {
        const int j = b * KNN_BOX + r * 64 + lane;
        float4 q = make_float4(inf, inf, inf, 0.f);  // rows past the end: distance +inf to everything
        if (j < n) q = make_float4(pts[3 * (size_t)j], pts[3 * (size_t)j + 1], pts[3 * (size_t)j + 2], 0.f);
        stage[r * 64 + lane] = q;
    }
    __syncthreads();
    const int first = b * KNN_BOX;
#pragma unroll 8
    for (int k = 0; k < KNN_BOX; ++k) {
        const float4 q = stage[k];  // same address in every lane: a broadcast
        float d = pair_dist2(px, py, pz, q.x, q.y, q.z);
        if (SELF) d = (first + k == self) ? inf : d;
        best.insert(d);
    }
}

__global__ void __launch_bounds__(64) knn3_kernel(int n, const float* __restrict__ pts, const float4* __restrict__ aabb,
                                                  float* __restrict__ dist2) {
    __shared__ float4 stage[KNN_BOX];
    const int lane = threadIdx.x;
    const int base = blockIdx.x * 64;
    const int i = base + lane;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const float px = pts[3 * (size_t)ii], py = pts[3 * (size_t)ii + 1], pz = pts[3 * (size_t)ii + 2];
    const float inf = __builtin_inff();
    // lanes past the end never ask for a box (nothing is < 0) and never write
    Best3 best{valid ? inf : 0.f, valid ? inf : 0.f, valid ? inf : 0.f};
    const int n_box = (int)knn_boxes((size_t)n), n_super = (int)knn_supers((size_t)n);
    const int own = base / KNN_BOX;  // 64 divides KNN_BOX: the wave's rows lie in one box
    knn_scan_box<true>(own, n, pts, stage, lane, i, px, py, pz, best);
#pragma unroll 1
    for (int s = 0; s < n_super; ++s) {
        const float4 slo = aabb[2 * ((size_t)n_box + s)], shi = aabb[2 * ((size_t)n_box + s) + 1];
        if (__ballot(box_dist2(px, py, pz, slo, shi) < best.b2) == 0ull) continue;
        const int b_end = min((s + 1) * KNN_SUPER, n_box);
#pragma unroll 1
        for (int b = s * KNN_SUPER; b < b_end; ++b) {
            if (b == own) continue;
            const float4 lo = aabb[2 * (size_t)b], hi = aabb[2 * (size_t)b + 1];
            if (__ballot(box_dist2(px, py, pz, lo, hi) < best.b2) == 0ull) continue;
            knn_scan_box<false>(b, n, pts, stage, lane, i, px, py, pz, best);
        }
    }
    if (valid) dist2[i] = ((best.b0 + best.b1) + best.b2) / 3.0f;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

size_t mobgs_knn3_scratch_bytes(int n) {
    if (n < 4 || n > KNN_MAX_N) return 0;
    return (knn_boxes((size_t)n) + knn_supers((size_t)n)) * 2 * sizeof(float4);
}

int mobgs_knn3_mean_dist2(int n, const float* points, float* dist2, void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 4) {
        set_error("mobgs_knn3_mean_dist2: n = %d; a point needs three neighbours (n >= 4)", n);
        return MOBGS_E_INVALID;
    }
    if (n > KNN_MAX_N) {
        set_error("mobgs_knn3_mean_dist2: n = %d exceeds %d (32-bit row indices, scratch size)", n, KNN_MAX_N);
        return MOBGS_E_INVALID;
    }
    if (!points || !dist2 || !scratch) {
        set_error("mobgs_knn3_mean_dist2: NULL buffer");
        return MOBGS_E_INVALID;
    }
    const size_t need = mobgs_knn3_scratch_bytes(n);
    if (scratch_bytes < need) {
        set_error("mobgs_knn3_mean_dist2: scratch holds %zu bytes, %zu needed (mobgs_knn3_scratch_bytes)", scratch_bytes,
                  need);
        return MOBGS_E_CAPACITY;
    }
    if (((uintptr_t)scratch & 15) != 0) {
        set_error("mobgs_knn3_mean_dist2: scratch must be 16-byte aligned");
        return MOBGS_E_INVALID;
    }
    float4* aabb = (float4*)scratch;
    hipLaunchKernelGGL(knn_aabb_kernel, dim3((unsigned)knn_supers((size_t)n)), dim3(256), 0, (hipStream_t)stream, n, points,
                       aabb);
    int rc = check_launch("mobgs_knn3_mean_dist2 (boxes)");
    if (rc != MOBGS_OK) return rc;
    hipLaunchKernelGGL(knn3_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, points,
                       (const float4*)aabb, dist2);
    return check_launch("mobgs_knn3_mean_dist2");
}

}  // extern "C"

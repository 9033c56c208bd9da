// K25: the temporal optical-flow metric tOF (include/mobgs_hip.h): dense Farneback flow between consecutive frames as
// cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0) computes it (the reference's metrics.py:14-29,
// :108-120), and the mean distance of two flow fields over the crop_8x8 window.  Forward only.  gfx950 only.
//
//   tof_grey_kernel         [F,3,H,W] fp32 -> [F,H,W] 8-bit grey values held as fp32 (pointwise)
//   tof_pyramid_kernel      one level image: the Gaussian blur of the full-size grey image and the bilinear resize, fused:
//                           only the four blurred values under an output pixel are formed (separably, (taps + 1)^2 reads)
//   tof_polyexp_kernel      16x16 tile, 26x26 replicate-border patch in LDS, vertical then horizontal 11-tap pass: the five
//                           polynomial coefficients per pixel; once per FRAME and level
//   tof_update_kernel       the first update matrices of a level, with the x2 bilinear upsampling of the coarser level's
//                           flow fused in (pointwise, one bilinear gather of the next frame's coefficients)
//   tof_blur_solve_kernel   16x16 tile, the 30x30 replicate-border patches of the five values in LDS, separable 15x15 box mean
//                           in float64 (the horizontal sums slide along a patch row),
//                           the 2x2 solve; <true>: the next round's update matrices of the thread's own pixel from the flow
//                           it has just solved, written to the OTHER matrix buffer (pointwise in the new flow)
//   tof_score_kernel        |flow_a - flow_b|_2 (x mask) over the crop window: per-workgroup float64 partial sums
//   tof_score_finish_kernel one workgroup: per pair, adds the partial sums in index order and divides
//
// A frame pair is a grid index: nothing is shared between pairs, there is no float atomic and no hand-off between
// workgroups, so a pair's flow is bit-identical from run to run and does not depend on the batch around it.
//
// Arithmetic: fp32 as OpenCV's, with three exceptions that only make it more exact.  (1) Resize coordinates are exact
// rationals ((2 dx + 1) src - dst) / (2 dst): an integer floor and ONE rounded division for the weight.  (2) The sample
// position x + u is split as (x + floor(u), u - floor(u)), both exact, so the in-bounds test is an integer test.  (3) The
// polynomial expansion subtracts a value near the tile's centre value before fitting (a constant changes only the constant
// coefficient, which is not kept): r_xx = b_1 ig03 + b_xx ig33 then cancels on values of the size of the local contrast, not
// of the grey level; the value is limited so that no patch entry grows in magnitude (tof_polyexp_kernel).  The 15x15 box
// sums and the 2x2 solve are float64 (OpenCV's are too).  Built with -ffp-contract=off.
#include <math.h>

#include "reduce_shared.h"

namespace mobgs {

constexpr int TOF_T = 16;
constexpr int TOF_BLOCK = TOF_T * TOF_T;
constexpr int TOF_WAVES = TOF_BLOCK / MOBGS_WAVE;
constexpr int TOF_MAX_EDGE = 1 << 14, TOF_MAX_F = 1 << 12, TOF_MIN_EDGE = 48;
constexpr int TOF_MAX_TAPS = 19;         // levels + 1 = 4 scales: sigma <= 3.5
constexpr int TOF_PN = 5;                // poly_n
constexpr int TOF_PP = TOF_T + 2 * TOF_PN;
constexpr int TOF_WR = 7;                // winsize 15
constexpr int TOF_WP = TOF_T + 2 * TOF_WR;
constexpr int TOF_SCORE_PER_BLOCK = TOF_BLOCK * 8;

__host__ __device__ inline int tof_tiles(int n) { return (n + TOF_T - 1) / TOF_T; }
__device__ __forceinline__ int tof_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
// OpenCV's BORDER_REFLECT_101 (d c b | a b c d | c b a); radius < n
__device__ __forceinline__ int tof_reflect101(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return tof_clampi(i, n);
}

// INTER_LINEAR source position of destination index d: s = (d + 0.5) src / dst - 0.5, clamped to [0, src - 1]
__device__ __forceinline__ void tof_resize_tap(int d, int src, int dst, int& i0, float& frac) {
    const int num = (2 * d + 1) * src - dst, den = 2 * dst;        // < 2^30 for edges <= 2^14
    if (num < 0) {
        i0 = 0;
        frac = 0.f;
        return;
    }
    i0 = num / den;
    frac = (float)(num - i0 * den) / (float)den;
    if (i0 >= src - 1) {
        i0 = src - 1;
        frac = 0.f;
    }
}

// ---- grey ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tof_to_u8(float x, int clamp, int quantize) {
    if (clamp) x = clamp01(x);
    if (quantize) x = quantize8(x);
    const float t = truncf(x * 255.f);                              // (gt_img * 255.0).astype(np.uint8), saturated
    return t < 0.f ? 0 : (t > 255.f ? 255 : (int)t);
}

__global__ void __launch_bounds__(TOF_BLOCK) tof_grey_kernel(size_t plane, const float* __restrict__ rgb, int clamp,
                                                             int quantize, float* __restrict__ grey) {
    const size_t i = (size_t)blockIdx.x * TOF_BLOCK + threadIdx.x;
    if (i >= plane) return;
    const float* p = rgb + (size_t)blockIdx.y * 3 * plane + i;
    const int r = tof_to_u8(p[0], clamp, quantize), g = tof_to_u8(p[plane], clamp, quantize);
    const int b = tof_to_u8(p[2 * plane], clamp, quantize);
    grey[(size_t)blockIdx.y * plane + i] = (float)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14);
}

// ---- pyramid level -----------------------------------------------------------------------------------------------------
struct TofPyrArgs {
    int H, W, h, w, taps;
    const float* grey;                   // [F,H,W]
    float* out;                          // [F,h,w]
    float g[TOF_MAX_TAPS];
};

__global__ void __launch_bounds__(TOF_BLOCK) tof_pyramid_kernel(TofPyrArgs a) {
    const int x = blockIdx.x * TOF_T + (threadIdx.x & (TOF_T - 1)), y = blockIdx.y * TOF_T + threadIdx.x / TOF_T;
    if (x >= a.w || y >= a.h) return;
    const float* src = a.grey + (size_t)blockIdx.z * a.H * a.W;
    int x0, y0;
    float fx, fy;
    tof_resize_tap(x, a.W, a.w, x0, fx);
    tof_resize_tap(y, a.H, a.h, y0, fy);
    const int r = a.taps >> 1;
    float acc0 = 0.f, acc1 = 0.f;        // the blurred column values at rows y0 and y0 + 1
    for (int j = -r; j <= r + 1; ++j) {
        const float* row = src + (size_t)tof_reflect101(y0 + j, a.H) * a.W;
        float h0 = 0.f, h1 = 0.f;        // the row blurred at x0 and at x0 + 1
        for (int i = -r; i <= r + 1; ++i) {
            const float v = row[tof_reflect101(x0 + i, a.W)];
            if (i <= r) h0 += a.g[i + r] * v;
            if (i > -r) h1 += a.g[i + r - 1] * v;
        }
        const float hv = (1.f - fx) * h0 + fx * h1;
        if (j <= r) acc0 += a.g[j + r] * hv;
        if (j > -r) acc1 += a.g[j + r - 1] * hv;
    }
    a.out[((size_t)blockIdx.z * a.h + y) * a.w + x] = (1.f - fy) * acc0 + fy * acc1;
}

// ---- polynomial expansion ----------------------------------------------------------------------------------------------
struct TofPolyArgs {
    int h, w;
    const float* img;                    // [F,h,w]
    float* R;                            // [F,5,h,w]: r_x, r_y, r_xx, r_yy, r_xy
    float g[2 * TOF_PN + 1];
    float ig11, ig03, ig33, ig55;
};

__global__ void __launch_bounds__(TOF_BLOCK) tof_polyexp_kernel(TofPolyArgs a) {
    __shared__ float s_p[TOF_PP][TOF_PP + 1];
    __shared__ float s_v[3][TOF_T][TOF_PP + 1];
    __shared__ float s_lo[TOF_WAVES], s_hi[TOF_WAVES];
    const int h = a.h, w = a.w;
    const size_t plane = (size_t)h * w;
    const float* src = a.img + (size_t)blockIdx.z * plane;
    const int x0 = blockIdx.x * TOF_T, y0 = blockIdx.y * TOF_T;
    float centre = src[(size_t)tof_clampi(y0 + TOF_T / 2, h) * w + tof_clampi(x0 + TOF_T / 2, w)];
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < TOF_PP * TOF_PP; i += TOF_BLOCK) {
        const int py = i / TOF_PP, px = i - py * TOF_PP;
        const float v = src[(size_t)tof_clampi(y0 + py - TOF_PN, h) * w + tof_clampi(x0 + px - TOF_PN, w)];
        s_p[py][px] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & (MOBGS_WAVE - 1)) == 0) {
        s_lo[threadIdx.x / MOBGS_WAVE] = lo;
        s_hi[threadIdx.x / MOBGS_WAVE] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TOF_WAVES; ++k) {
        lo = fminf(lo, s_lo[k]);
        hi = fmaxf(hi, s_hi[k]);
    }
    // the value every patch entry is taken relative to: the tile's centre value, limited to twice the patch's value nearest
    // to 0 (0 if the patch changes sign).  For lo >= 0 that is c = min(centre, 2 lo), and |v - c| <= |v| for every entry:
    // v >= c gives v - c <= v, v < c gives c - v <= 2 lo - v <= v.  No term of a sum grows, so a dark region next to a bright
    // one is as exact as without the shift.  2 lo is exact; on a flat patch c is its value and every entry exactly 0.
    centre = lo >= 0.f ? fminf(centre, 2.f * lo) : (hi <= 0.f ? fmaxf(centre, 2.f * hi) : 0.f);
    for (int i = threadIdx.x; i < TOF_PP * TOF_PP; i += TOF_BLOCK) {
        const int py = i / TOF_PP, px = i - py * TOF_PP;
        s_p[py][px] -= centre;
    }
    __syncthreads();
    // vertical pass: 16 rows x 26 columns: sum g s, sum k g s, sum k^2 g s
    for (int i = threadIdx.x; i < TOF_T * TOF_PP; i += TOF_BLOCK) {
        const int r = i / TOF_PP, c = i - r * TOF_PP;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
        for (int k = -TOF_PN; k <= TOF_PN; ++k) {
            const float t = a.g[k + TOF_PN] * s_p[r + TOF_PN + k][c];
            v0 += t;
            v1 += (float)k * t;
            v2 += (float)(k * k) * t;
        }
        s_v[0][r][c] = v0;
        s_v[1][r][c] = v1;
        s_v[2][r][c] = v2;
    }
    __syncthreads();
    const int lx = threadIdx.x & (TOF_T - 1), ly = threadIdx.x / TOF_T;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    float b1 = 0.f, bx = 0.f, bxx = 0.f, by = 0.f, bxy = 0.f, byy = 0.f;
#pragma unroll
    for (int k = -TOF_PN; k <= TOF_PN; ++k) {
        const float gk = a.g[k + TOF_PN];
        const float t0 = gk * s_v[0][ly][lx + TOF_PN + k], t1 = gk * s_v[1][ly][lx + TOF_PN + k];
        b1 += t0;
        bx += (float)k * t0;
        bxx += (float)(k * k) * t0;
        by += t1;
        bxy += (float)k * t1;
        byy += gk * s_v[2][ly][lx + TOF_PN + k];
    }
    float* o = a.R + (size_t)blockIdx.z * 5 * plane + (size_t)y * w + x;
    o[0] = bx * a.ig11;
    o[plane] = by * a.ig11;
    o[2 * plane] = b1 * a.ig03 + bxx * a.ig33;
    o[3 * plane] = b1 * a.ig03 + byy * a.ig33;
    o[4 * plane] = bxy * a.ig55;
}

// ---- update matrices ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tof_border_factor(int x, int y, int w, int h) {
    const float t[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    float s = 1.f;
    if (x < 5) s *= t[x];
    if (y < 5) s *= t[y];
    if (x >= w - 5) s *= t[w - 1 - x];
    if (y >= h - 5) s *= t[h - 1 - y];
    return s;
}

// (G11, G12, G22, h1, h2) of pixel (x, y) with flow (u, v): R0, R1 the coefficient planes of the pair's two frames
__device__ __forceinline__ void tof_update_at(const float* __restrict__ R0, const float* __restrict__ R1, size_t plane,
                                              int w, int h, int x, int y, float u, float v, float* __restrict__ M) {
    const size_t o = (size_t)y * w + x;
    const float r0x = R0[o], r0y = R0[plane + o], r0xx = R0[2 * plane + o], r0yy = R0[3 * plane + o];
    const float r0xy = R0[4 * plane + o];
    float bx, by, axx = r0xx, ayy = r0yy, axy = r0xy * 0.5f, sx = 0.f, sy = 0.f;
    bool in = fabsf(u) < 1e6f && fabsf(v) < 1e6f;                   // (also false for a NaN)
    if (in) {
        const float fu = floorf(u), fv = floorf(v);
        const int x1 = x + (int)fu, y1 = y + (int)fv;
        in = x1 >= 0 && x1 < w - 1 && y1 >= 0 && y1 < h - 1;
        if (in) {
            const float fx = u - fu, fy = v - fv;                   // exact
            const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
            const float* q = R1 + (size_t)y1 * w + x1;
            float s[5];
#pragma unroll
            for (int c = 0; c < 5; ++c)
                s[c] = a00 * q[c * plane] + a01 * q[c * plane + 1] + a10 * q[c * plane + w] + a11 * q[c * plane + w + 1];
            sx = s[0];
            sy = s[1];
            axx = (r0xx + s[2]) * 0.5f;
            ayy = (r0yy + s[3]) * 0.5f;
            axy = (r0xy + s[4]) * 0.25f;
        }
    }
    bx = (r0x - sx) * 0.5f;
    by = (r0y - sy) * 0.5f;
    bx += axx * u + axy * v;
    by += axy * u + ayy * v;
    const float sc = tof_border_factor(x, y, w, h);
    axx *= sc;
    ayy *= sc;
    axy *= sc;
    bx *= sc;
    by *= sc;
    M[o] = axx * axx + axy * axy;
    M[plane + o] = (axx + ayy) * axy;
    M[2 * plane + o] = ayy * ayy + axy * axy;
    M[3 * plane + o] = axx * bx + axy * by;
    M[4 * plane + o] = axy * bx + ayy * by;
}

// flow_in [P,sh,sw,2] or NULL (= 0); (sh, sw) != (h, w): resized bilinearly and doubled.  flow_out [P,h,w,2] or NULL.
__global__ void __launch_bounds__(TOF_BLOCK) tof_update_kernel(int h, int w, const float* __restrict__ R,
                                                               const float* __restrict__ flow_in, int sh, int sw,
                                                               float* __restrict__ flow_out, float* __restrict__ M) {
    const int x = blockIdx.x * TOF_T + (threadIdx.x & (TOF_T - 1)), y = blockIdx.y * TOF_T + threadIdx.x / TOF_T;
    if (x >= w || y >= h) return;
    const int p = blockIdx.z;
    const size_t plane = (size_t)h * w;
    float u = 0.f, v = 0.f;
    if (flow_in) {
        const float* f = flow_in + (size_t)p * sh * sw * 2;
        if (sh == h && sw == w) {
            u = f[((size_t)y * w + x) * 2];
            v = f[((size_t)y * w + x) * 2 + 1];
        } else {
            int x0, y0;
            float fx, fy;
            tof_resize_tap(x, sw, w, x0, fx);
            tof_resize_tap(y, sh, h, y0, fy);
            const int x1 = x0 + 1 < sw ? x0 + 1 : x0, y1 = y0 + 1 < sh ? y0 + 1 : y0;
            const float* a = f + ((size_t)y0 * sw) * 2;
            const float* b = f + ((size_t)y1 * sw) * 2;
            const float u0 = (1.f - fx) * a[2 * x0] + fx * a[2 * x1], u1 = (1.f - fx) * b[2 * x0] + fx * b[2 * x1];
            const float v0 = (1.f - fx) * a[2 * x0 + 1] + fx * a[2 * x1 + 1];
            const float v1 = (1.f - fx) * b[2 * x0 + 1] + fx * b[2 * x1 + 1];
            u = 2.f * ((1.f - fy) * u0 + fy * u1);
            v = 2.f * ((1.f - fy) * v0 + fy * v1);
        }
    }
    if (flow_out) {
        float* o = flow_out + ((size_t)p * plane + (size_t)y * w + x) * 2;
        o[0] = u;
        o[1] = v;
    }
    tof_update_at(R + (size_t)p * 5 * plane, R + (size_t)(p + 1) * 5 * plane, plane, w, h, x, y, u, v,
                  M + (size_t)p * 5 * plane);
}

// ---- box mean + solve (+ the next update) --------------------------------------------------------------------------------
template <bool FUSE>
__global__ void __launch_bounds__(TOF_BLOCK) tof_blur_solve_kernel(int h, int w, const float* __restrict__ M_in,
                                                                   float* __restrict__ flow, const float* __restrict__ R,
                                                                   float* __restrict__ M_out) {
    __shared__ float s_p[5][TOF_WP][TOF_WP + 1];
    __shared__ double s_h[5][TOF_WP][TOF_T + 1];
    const int p = blockIdx.z;
    const size_t plane = (size_t)h * w;
    const int x0 = blockIdx.x * TOF_T, y0 = blockIdx.y * TOF_T;
    const int lx = threadIdx.x & (TOF_T - 1), ly = threadIdx.x / TOF_T;
    // the five values go through each phase together: three barriers per tile, and five loads in flight per thread
    for (int i = threadIdx.x; i < TOF_WP * TOF_WP; i += TOF_BLOCK) {
        const int py = i / TOF_WP, px = i - py * TOF_WP;
        const float* src = M_in + (size_t)p * 5 * plane + (size_t)tof_clampi(y0 + py - TOF_WR, h) * w +
                           tof_clampi(x0 + px - TOF_WR, w);
#pragma unroll
        for (int c = 0; c < 5; ++c) s_p[c][py][px] = src[c * plane];
    }
    __syncthreads();
    // horizontal: one thread per (value, patch row); the window slides along the row (30 LDS reads for 16 sums, in float64:
    // a value that has left the window leaves 2^-53 of itself behind, and sums over zeros stay exactly 0)
    for (int i = threadIdx.x; i < 5 * TOF_WP; i += TOF_BLOCK) {
        const int c = i / TOF_WP, r = i - c * TOF_WP;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * TOF_WR + 1; ++k) s += (double)s_p[c][r][k];
        s_h[c][r][0] = s;
#pragma unroll
        for (int cx = 1; cx < TOF_T; ++cx) {
            s = (s + (double)s_p[c][r][cx + 2 * TOF_WR]) - (double)s_p[c][r][cx - 1];
            s_h[c][r][cx] = s;
        }
    }
    __syncthreads();
    double q[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * TOF_WR + 1; ++k) s += s_h[c][ly + k][lx];
        q[c] = s * (1.0 / 225.0);
    }
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const double det = q[0] * q[2] - q[1] * q[1] + 1e-3;
    const float u = (float)((q[2] * q[3] - q[1] * q[4]) / det), v = (float)((q[0] * q[4] - q[1] * q[3]) / det);
    float* o = flow + ((size_t)p * plane + (size_t)y * w + x) * 2;
    o[0] = u;
    o[1] = v;
    if (FUSE)
        tof_update_at(R + (size_t)p * 5 * plane, R + (size_t)(p + 1) * 5 * plane, plane, w, h, x, y, u, v,
                      M_out + (size_t)p * 5 * plane);
}

// ---- score ----------------------------------------------------------------------------------------------------------------
struct TofCrop {
    int y, x, h, w;
};
// metrics.py:32-47
static inline TofCrop tof_crop(int H, int W) {
    TofCrop c;
    c.h = (H / 32) * 32;
    c.w = (W / 32) * 32;
    while (c.h > H - 16) c.h -= 32;
    while (c.w > W - 16) c.w -= 32;
    c.y = (H - c.h) / 2;
    c.x = (W - c.w) / 2;
    return c;
}
static inline int tof_score_blocks(const TofCrop& c) {
    return (int)(((size_t)c.h * c.w + TOF_SCORE_PER_BLOCK - 1) / TOF_SCORE_PER_BLOCK);
}

// partial [P, blocks, 2] = {sum |a - b|_2 mask, sum mask}
__global__ void __launch_bounds__(TOF_BLOCK) tof_score_kernel(int H, int W, TofCrop c, const float* __restrict__ fa,
                                                              const float* __restrict__ fb, const float* __restrict__ mask,
                                                              double* __restrict__ partial) {
    __shared__ double s_wave[TOF_WAVES];
    const int p = blockIdx.y;
    const size_t plane = (size_t)H * W, n = (size_t)c.h * c.w;
    double sd = 0.0, sm = 0.0;
    for (int k = 0; k < 8; ++k) {
        const size_t i = (size_t)blockIdx.x * TOF_SCORE_PER_BLOCK + (size_t)k * TOF_BLOCK + threadIdx.x;
        if (i >= n) break;
        const int r = (int)(i / c.w), col = (int)(i - (size_t)r * c.w);
        const size_t o = (size_t)p * plane + (size_t)(c.y + r) * W + (c.x + col);
        const double du = (double)fa[2 * o] - (double)fb[2 * o], dv = (double)fa[2 * o + 1] - (double)fb[2 * o + 1];
        const double m = mask ? (double)mask[o] : 1.0;
        sd += sqrt(du * du + dv * dv) * m;
        sm += m;
    }
    sd = block_sum<TOF_WAVES>(sd, s_wave);
    sm = block_sum<TOF_WAVES>(sm, s_wave);
    if (threadIdx.x == 0) {
        double* o = partial + ((size_t)p * gridDim.x + blockIdx.x) * 2;
        o[0] = sd;
        o[1] = sm;
    }
}

__global__ void __launch_bounds__(TOF_BLOCK) tof_score_finish_kernel(int P, int blocks, int masked, double n,
                                                                     const double* __restrict__ partial,
                                                                     double* __restrict__ out) {
    __shared__ double s_wave[TOF_WAVES];
    for (int p = 0; p < P; ++p) {
        const double* q = partial + (size_t)p * blocks * 2;
        const double sd = rows_sum<TOF_BLOCK>(q, blocks, 2, s_wave), sm = rows_sum<TOF_BLOCK>(q + 1, blocks, 2, s_wave);
        if (threadIdx.x == 0) out[p] = masked ? sd / sm : sd / n;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static bool tof_image_ok(int H, int W) {
    return H >= TOF_MIN_EDGE && W >= TOF_MIN_EDGE && H <= TOF_MAX_EDGE && W <= TOF_MAX_EDGE;
}
static bool tof_level_ok(int h, int w) { return h >= 2 && w >= 2 && h <= TOF_MAX_EDGE && w <= TOF_MAX_EDGE; }
static bool tof_count_ok(int n) { return n >= 1 && n <= TOF_MAX_F; }

static int tof_levels_host(int H, int W, MobgsTofLevel* out) {
    double scale = 1.0;
    int k = 0;
    for (; k < 3; ++k) {
        scale *= 0.5;
        if (W * scale < 32 || H * scale < 32) break;
    }
    const int n = k + 1;
    for (int i = 0; i < n; ++i) {
        const double s = ldexp(1.0, -(k - i));                      // coarsest first
        const double sigma = (1.0 / s - 1.0) * 0.5;
        const int taps = (int)rint(sigma * 5.0) | 1;
        out[i].width = (int)rint(W * s);
        out[i].height = (int)rint(H * s);
        out[i].taps = taps < 3 ? 3 : taps;
        out[i].sigma = sigma;
    }
    return n;
}

// cv::getGaussianKernel: the fixed table for sigma <= 0 (3 taps), else exp(-t^2 / (2 sigma^2)) normalised to sum 1
static void tof_gauss_taps(int taps, double sigma, float* g) {
    if (!(sigma > 0.0)) {
        g[0] = 0.25f;
        g[1] = 0.5f;
        g[2] = 0.25f;
        return;
    }
    double w[TOF_MAX_TAPS], sum = 0.0;
    for (int i = 0; i < taps; ++i) {
        const double t = (double)(i - taps / 2);
        w[i] = exp(-(t * t) / (2.0 * sigma * sigma));
        sum += w[i];
    }
    for (int i = 0; i < taps; ++i) g[i] = (float)(w[i] / sum);
}

static void tof_launch_pyramid(int F, int H, int W, const float* grey, const MobgsTofLevel& lv, float* out, hipStream_t s) {
    TofPyrArgs a;
    a.H = H;
    a.W = W;
    a.h = lv.height;
    a.w = lv.width;
    a.taps = lv.taps;
    a.grey = grey;
    a.out = out;
    for (int i = 0; i < TOF_MAX_TAPS; ++i) a.g[i] = 0.f;
    tof_gauss_taps(lv.taps, lv.sigma, a.g);
    hipLaunchKernelGGL(tof_pyramid_kernel, dim3(tof_tiles(a.w), tof_tiles(a.h), F), dim3(TOF_BLOCK), 0, s, a);
}

static void tof_launch_polyexp(int F, int h, int w, const float* img, float* R, hipStream_t s) {
    TofPolyArgs a;
    a.h = h;
    a.w = w;
    a.img = img;
    a.R = R;
    double g[2 * TOF_PN + 1], sum = 0.0, m2 = 0.0, m4 = 0.0;
    for (int k = -TOF_PN; k <= TOF_PN; ++k) {
        g[k + TOF_PN] = exp(-(double)(k * k) / (2.0 * 1.2 * 1.2));
        sum += g[k + TOF_PN];
    }
    for (int k = -TOF_PN; k <= TOF_PN; ++k) {
        g[k + TOF_PN] /= sum;
        a.g[k + TOF_PN] = (float)g[k + TOF_PN];
        m2 += g[k + TOF_PN] * k * k;
        m4 += g[k + TOF_PN] * k * k * k * k;
    }
    // the normal equations of (1, x, y, x^2, y^2, xy) under the weight g(x) g(y) decouple: <x,x> = m2, <xy,xy> = m2^2, and
    // the (1, x^2, y^2) block has the Schur complement diag(m4 - m2^2)
    a.ig11 = (float)(1.0 / m2);
    a.ig33 = (float)(1.0 / (m4 - m2 * m2));
    a.ig03 = (float)(-m2 / (m4 - m2 * m2));
    a.ig55 = (float)(1.0 / (m2 * m2));
    hipLaunchKernelGGL(tof_polyexp_kernel, dim3(tof_tiles(w), tof_tiles(h), F), dim3(TOF_BLOCK), 0, s, a);
}

static void tof_launch_update(int P, int h, int w, const float* R, const float* flow_in, int sh, int sw, float* flow_out,
                              float* M, hipStream_t s) {
    hipLaunchKernelGGL(tof_update_kernel, dim3(tof_tiles(w), tof_tiles(h), P), dim3(TOF_BLOCK), 0, s, h, w, R, flow_in, sh,
                       sw, flow_out, M);
}

static void tof_launch_blur_solve(int P, int h, int w, const float* M_in, float* flow, const float* R, float* M_out,
                                  hipStream_t s) {
    const dim3 grid(tof_tiles(w), tof_tiles(h), P);
    if (M_out)
        hipLaunchKernelGGL(tof_blur_solve_kernel<true>, grid, dim3(TOF_BLOCK), 0, s, h, w, M_in, flow, R, M_out);
    else
        hipLaunchKernelGGL(tof_blur_solve_kernel<false>, grid, dim3(TOF_BLOCK), 0, s, h, w, M_in, flow, R, M_out);
}

static size_t tof_round256(size_t n) { return (n + 255) & ~(size_t)255; }

// scratch of mobgs_tof_flow: level image [F,H,W], coefficients [F,5,H,W], two matrix buffers [P,5,H,W], two flow buffers of
// the second-finest level's size
struct TofScratch {
    size_t img, R, M0, M1, flow0, flow1, total;
};
static TofScratch tof_scratch_layout(int F, int H, int W) {
    MobgsTofLevel lv[4];
    const int n = tof_levels_host(H, W, lv);
    const size_t plane = (size_t)H * W, P = (size_t)F - 1;
    const size_t coarse = n >= 2 ? (size_t)lv[n - 2].width * lv[n - 2].height : 0;
    TofScratch t;
    size_t at = 0;
    t.img = at;
    at += tof_round256((size_t)F * plane * 4);
    t.R = at;
    at += tof_round256((size_t)F * 5 * plane * 4);
    t.M0 = at;
    at += tof_round256(P * 5 * plane * 4);
    t.M1 = at;
    at += tof_round256(P * 5 * plane * 4);
    t.flow0 = at;
    at += tof_round256(P * coarse * 8);
    t.flow1 = at;
    at += tof_round256(P * coarse * 8);
    t.total = at > 0 ? at : 256;
    return t;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_tof_levels(int H, int W, MobgsTofLevel* out) {
    if (!tof_image_ok(H, W) || !out) {
        set_error("mobgs_tof_levels: H = %d, W = %d outside %d <= H, W <= %d, or a NULL out", H, W, TOF_MIN_EDGE,
                  TOF_MAX_EDGE);
        return 0;
    }
    return tof_levels_host(H, W, out);
}

int mobgs_tof_crop(int H, int W, int32_t* yxhw) {
    if (!tof_image_ok(H, W) || !yxhw) {
        set_error("mobgs_tof_crop: H = %d, W = %d outside %d <= H, W <= %d, or a NULL yxhw", H, W, TOF_MIN_EDGE, TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    const TofCrop c = tof_crop(H, W);
    yxhw[0] = c.y;
    yxhw[1] = c.x;
    yxhw[2] = c.h;
    yxhw[3] = c.w;
    return MOBGS_OK;
}

size_t mobgs_tof_scratch_bytes(int F, int H, int W) {
    if (!tof_image_ok(H, W) || F < 2 || !tof_count_ok(F)) return 0;
    return tof_scratch_layout(F, H, W).total;
}

size_t mobgs_tof_score_scratch_doubles(int P, int H, int W) {
    if (!tof_image_ok(H, W) || !tof_count_ok(P)) return 0;
    return (size_t)P * tof_score_blocks(tof_crop(H, W)) * 2;
}

int mobgs_tof_grey(int F, int H, int W, const float* rgb, int flags, float* grey, void* stream) {
    if (!tof_count_ok(F) || !tof_level_ok(H, W) || (flags & ~(MOBGS_METRICS_CLAMP | MOBGS_METRICS_QUANTIZE))) {
        set_error("mobgs_tof_grey: F = %d, H = %d, W = %d outside 1 <= F <= %d, 2 <= H, W <= %d, or an unknown flag in %d", F,
                  H, W, TOF_MAX_F, TOF_MAX_EDGE, flags);
        return MOBGS_E_INVALID;
    }
    if (!rgb || !grey || !aligned(rgb, 4) || !aligned(grey, 4)) {
        set_error("mobgs_tof_grey: NULL or misaligned rgb / grey");
        return MOBGS_E_INVALID;
    }
    const size_t plane = (size_t)H * W;
    hipLaunchKernelGGL(tof_grey_kernel, dim3((unsigned)((plane + TOF_BLOCK - 1) / TOF_BLOCK), F), dim3(TOF_BLOCK), 0,
                       (hipStream_t)stream, plane, rgb, (flags & MOBGS_METRICS_CLAMP) ? 1 : 0,
                       (flags & MOBGS_METRICS_QUANTIZE) ? 1 : 0, grey);
    return check_launch("mobgs_tof_grey");
}

int mobgs_tof_pyramid_level(int F, int H, int W, const float* grey, const MobgsTofLevel* level, float* out, void* stream) {
    if (!tof_count_ok(F) || !tof_image_ok(H, W) || !level) {
        set_error("mobgs_tof_pyramid_level: F = %d, H = %d, W = %d outside 1 <= F <= %d, %d <= H, W <= %d, or a NULL level", F,
                  H, W, TOF_MAX_F, TOF_MIN_EDGE, TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (!tof_level_ok(level->height, level->width) || level->width > W || level->height > H || level->taps < 3 ||
        level->taps > TOF_MAX_TAPS || !(level->taps & 1) || !(level->sigma >= 0.0) || level->sigma > 64.0 ||
        (level->sigma == 0.0 && level->taps != 3)) {
        set_error("mobgs_tof_pyramid_level: a level of %d x %d, %d taps, sigma %g is not one of a %d x %d image",
                  level->width, level->height, level->taps, level->sigma, W, H);
        return MOBGS_E_INVALID;
    }
    if (!grey || !out || !aligned(grey, 4) || !aligned(out, 4)) {
        set_error("mobgs_tof_pyramid_level: NULL or misaligned grey / out");
        return MOBGS_E_INVALID;
    }
    tof_launch_pyramid(F, H, W, grey, *level, out, (hipStream_t)stream);
    return check_launch("mobgs_tof_pyramid_level");
}

int mobgs_tof_polyexp(int F, int h, int w, const float* img, float* R, void* stream) {
    if (!tof_count_ok(F) || !tof_level_ok(h, w)) {
        set_error("mobgs_tof_polyexp: F = %d, h = %d, w = %d outside 1 <= F <= %d, 2 <= h, w <= %d", F, h, w, TOF_MAX_F,
                  TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (!img || !R || !aligned(img, 4) || !aligned(R, 4)) {
        set_error("mobgs_tof_polyexp: NULL or misaligned img / R");
        return MOBGS_E_INVALID;
    }
    tof_launch_polyexp(F, h, w, img, R, (hipStream_t)stream);
    return check_launch("mobgs_tof_polyexp");
}

int mobgs_tof_update_matrices(int P, int h, int w, const float* R, const float* flow, int src_h, int src_w,
                              float* flow_out, float* M, void* stream) {
    if (!tof_count_ok(P) || !tof_level_ok(h, w)) {
        set_error("mobgs_tof_update_matrices: P = %d, h = %d, w = %d outside 1 <= P <= %d, 2 <= h, w <= %d", P, h, w,
                  TOF_MAX_F, TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (flow && (src_h < 1 || src_w < 1 || src_h > h || src_w > w)) {
        set_error("mobgs_tof_update_matrices: a flow of %d x %d cannot seed a level of %d x %d", src_w, src_h, w, h);
        return MOBGS_E_INVALID;
    }
    if (!R || !M || !aligned(R, 4) || !aligned(M, 4) || !aligned(flow, 4) || !aligned(flow_out, 4)) {
        set_error("mobgs_tof_update_matrices: NULL R / M or a misaligned pointer");
        return MOBGS_E_INVALID;
    }
    tof_launch_update(P, h, w, R, flow, src_h, src_w, flow_out, M, (hipStream_t)stream);
    return check_launch("mobgs_tof_update_matrices");
}

int mobgs_tof_blur_solve(int P, int h, int w, const float* M_in, float* flow, const float* R, float* M_out, void* stream) {
    if (!tof_count_ok(P) || !tof_level_ok(h, w)) {
        set_error("mobgs_tof_blur_solve: P = %d, h = %d, w = %d outside 1 <= P <= %d, 2 <= h, w <= %d", P, h, w, TOF_MAX_F,
                  TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (!M_in || !flow || (M_out && !R) || M_out == M_in || !aligned(M_in, 4) || !aligned(flow, 4) ||
        !aligned(R, 4) || !aligned(M_out, 4)) {
        set_error("mobgs_tof_blur_solve: NULL M_in / flow, M_out without R or equal to M_in, or a misaligned pointer");
        return MOBGS_E_INVALID;
    }
    tof_launch_blur_solve(P, h, w, M_in, flow, R, M_out, (hipStream_t)stream);
    return check_launch("mobgs_tof_blur_solve");
}

int mobgs_tof_flow(int F, int H, int W, const float* grey, void* scratch, float* flow_out, void* stream) {
    if (F < 2 || !tof_count_ok(F) || !tof_image_ok(H, W)) {
        set_error("mobgs_tof_flow: F = %d, H = %d, W = %d outside 2 <= F <= %d, %d <= H, W <= %d", F, H, W, TOF_MAX_F,
                  TOF_MIN_EDGE, TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (!grey || !scratch || !flow_out || !aligned(grey, 4) || !aligned(scratch, 256) || !aligned(flow_out, 4)) {
        set_error("mobgs_tof_flow: NULL grey / scratch / flow_out, or a misaligned pointer (scratch: 256 bytes)");
        return MOBGS_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P = F - 1;
    MobgsTofLevel lv[4];
    const int n = tof_levels_host(H, W, lv);
    const TofScratch t = tof_scratch_layout(F, H, W);
    char* base = (char*)scratch;
    float* img = (float*)(base + t.img);
    float* R = (float*)(base + t.R);
    float* M[2] = {(float*)(base + t.M0), (float*)(base + t.M1)};
    float* fl[2] = {(float*)(base + t.flow0), (float*)(base + t.flow1)};
    const float* prev = nullptr;
    int ph = 0, pw = 0;
    for (int i = 0; i < n; ++i) {
        const int h = lv[i].height, w = lv[i].width;
        float* flow = i == n - 1 ? flow_out : fl[i & 1];
        tof_launch_pyramid(F, H, W, grey, lv[i], img, s);
        tof_launch_polyexp(F, h, w, img, R, s);
        tof_launch_update(P, h, w, R, prev, ph, pw, flow, M[0], s);
        tof_launch_blur_solve(P, h, w, M[0], flow, R, M[1], s);
        tof_launch_blur_solve(P, h, w, M[1], flow, R, M[0], s);
        tof_launch_blur_solve(P, h, w, M[0], flow, nullptr, nullptr, s);
        prev = flow;
        ph = h;
        pw = w;
    }
    return check_launch("mobgs_tof_flow");
}

int mobgs_tof_score(int P, int H, int W, const float* flow_a, const float* flow_b, const float* mask, double* partial,
                    double* out, void* stream) {
    if (!tof_count_ok(P) || !tof_image_ok(H, W)) {
        set_error("mobgs_tof_score: P = %d, H = %d, W = %d outside 1 <= P <= %d, %d <= H, W <= %d", P, H, W, TOF_MAX_F,
                  TOF_MIN_EDGE, TOF_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (!flow_a || !flow_b || !partial || !out || !aligned(flow_a, 4) || !aligned(flow_b, 4) ||
        !aligned(mask, 4) || !aligned(partial, 8) || !aligned(out, 8)) {
        set_error("mobgs_tof_score: NULL flow_a / flow_b / partial / out, or a misaligned pointer (partial, out: 8 bytes)");
        return MOBGS_E_INVALID;
    }
    const TofCrop c = tof_crop(H, W);
    const int blocks = tof_score_blocks(c);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tof_score_kernel, dim3(blocks, P), dim3(TOF_BLOCK), 0, s, H, W, c, flow_a, flow_b, mask, partial);
    hipLaunchKernelGGL(tof_score_finish_kernel, dim3(1), dim3(TOF_BLOCK), 0, s, P, blocks, mask ? 1 : 0,
                       (double)c.h * (double)c.w, (const double*)partial, out);
    return check_launch("mobgs_tof_score");
}

}  // extern "C"

// K22: evaluation metrics of a batch of image pairs (include/mobgs_hip.h): the error sums behind L1 / MSE / PSNR, the
// box-window SSIM of skimage's structural_similarity(multichannel=True) (the reference's metrics.py:124, :54-64) and the
// Gaussian partial-convolution SSIM of the reference's dycheck_metrics.py:95-200.  Forward only.  gfx950 only.
//
//   metrics_kernel<KIND>    one workgroup owns MET_STRIP horizontally adjacent 16x16 tiles of ONE image (grid: strips x
//                           tile rows x images) and walks its three channels: the halo patch of both images (and of the
//                           mask) goes to LDS, the separable window runs horizontally, then vertically out of LDS, the SSIM
//                           map value of the thread's pixel is added to the thread's own float64 sums; at the end ONE row
//                           of float64 partial sums per workgroup.  KIND is the window: MET_BOX = 7 equal taps, `reflect`
//                           borders, the map has the image's size; MET_GAUSS = 11 taps, sigma 1.5, `valid`, renormalised
//                           per 1-D pass by 11 / (mask count), the map is (H - 10) x (W - 10).  Straight-line over the taps.
//   metrics_finish_kernel   one workgroup: per image, adds the rows in index order (float64) and forms the metrics.
//
// No float atomics and no hand-off between workgroups inside a launch: the summation order is a function of H and W alone,
// so a result is bit-identical from run to run, and an image's row does not depend on the batch it is scored in.
//
// Arithmetic: the inputs are fp32; the optional clamp and the 8-bit quantisation of the prediction are fp32 operations, as
// the reference writes them (eval.py:162: clip, * 255, truncate, / 255).  Everything after that is float64 -- differences,
// squares, window sums, the SSIM formula: skimage itself widens to float64, and E[x^2] - mu^2 in fp32 is 1e-5 off on
// smooth images (docs/MEASUREMENT_LOG.md).  This file is built with -ffp-contract=off: with both images equal, or flat,
// numerator and denominator of the SSIM map are then the same operations on the same values and the map is exactly 1.
#include "reduce_shared.h"

namespace mobgs {

constexpr int MET_T = 16;                // output tile edge
constexpr int MET_STRIP = 4;             // tiles per workgroup, along x
constexpr int MET_BLOCK = MET_T * MET_T;
constexpr int MET_WAVES = MET_BLOCK / MOBGS_WAVE;
constexpr int MET_BOX = 0, MET_GAUSS = 1;
constexpr int MET_MAX_EDGE = 1 << 15, MET_MAX_B = 1 << 14;
// columns of a partial row: {sum |a - b|, sum (a - b)^2, sum (a - b)^2 m, sum m (pixels)} (written by the first arm that is
// launched), {box map over the cropped region, per channel; box map x mask, uncropped} (box arm), {Gaussian map} (Gaussian)
constexpr int MET_COL_ERR = 0, MET_COL_BOX = 4, MET_COL_BOX_MASKED = 7, MET_COL_GAUSS = 8, MET_NCOL = 9;
static_assert(MOBGS_METRICS_COLUMNS == 9, "out columns of include/mobgs_hip.h");

struct MetArgs {
    int H, W;
    const float *pred, *gt, *mask;       // [B,3,H,W], [B,3,H,W], [B,H,W] or NULL (= all ones)
    int clamp, quantize, do_err;
    double c1, c2;
    double w[11];                        // the Gaussian taps (unused by the box arm)
};

__host__ __device__ inline int met_strips(int W) { return ((W + MET_T - 1) / MET_T + MET_STRIP - 1) / MET_STRIP; }
__host__ __device__ inline int met_tile_rows(int H) { return (H + MET_T - 1) / MET_T; }

__device__ __forceinline__ bool met_owns(int kind, int do_err, int c) {
    return c < MET_COL_BOX ? do_err != 0 : (c < MET_COL_GAUSS ? kind == MET_BOX : kind == MET_GAUSS);
}

// scipy.ndimage's `reflect` (d c b a | a b c d | d c b a), then clamped: the clamp only acts for lanes past the image's
// edge in a ragged tile, whose values are not used
__device__ __forceinline__ int met_reflect(int i, int n) {
    i = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

template <int KIND>
__global__ void __launch_bounds__(MET_BLOCK) metrics_kernel(MetArgs a, double* __restrict__ partial) {
    constexpr int TAPS = KIND == MET_BOX ? 7 : 11;
    constexpr int OFF = KIND == MET_BOX ? 3 : 0;        // the thread's own pixel inside the patch
    constexpr int P = MET_T + TAPS - 1;
    __shared__ float s_a[P][P + 1], s_b[P][P + 1], s_m[P][P + 1];
    __shared__ double s_h[5][P][MET_T + 1];
    __shared__ float s_hm[P][MET_T + 1];
    __shared__ double s_wave[MET_WAVES];
    const int H = a.H, W = a.W;
    const int img = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float* pm = a.mask ? a.mask + (size_t)img * plane : nullptr;
    const int lx = threadIdx.x & (MET_T - 1), ly = threadIdx.x / MET_T;
    const int y0 = blockIdx.y * MET_T;
    double acc[MET_NCOL];
#pragma unroll
    for (int c = 0; c < MET_NCOL; ++c) acc[c] = 0.0;

    for (int t = 0; t < MET_STRIP; ++t) {
        const int x0 = (blockIdx.x * MET_STRIP + t) * MET_T;
        if (x0 >= W) break;                              // (uniform over the workgroup)
        const int gx = x0 + lx, gy = y0 + ly;
        const bool inside = gx < W && gy < H;
        for (int c = 0; c < 3; ++c) {
            const float* pa = a.pred + ((size_t)img * 3 + c) * plane;
            const float* pb = a.gt + ((size_t)img * 3 + c) * plane;
            __syncthreads();                             // the previous pass has read s_a, s_b, s_m, s_h, s_hm
            for (int i = threadIdx.x; i < P * P; i += MET_BLOCK) {
                const int py = i / P, px = i - py * P;
                int sx = x0 + px - OFF, sy = y0 + py - OFF;
                bool in = true;
                if (KIND == MET_BOX) {
                    sx = met_reflect(sx, W);
                    sy = met_reflect(sy, H);
                } else {
                    in = sx < W && sy < H;
                }
                float u = 0.f, v = 0.f, m = 0.f;
                if (in) {
                    const size_t o = (size_t)sy * W + sx;
                    u = pa[o];
                    v = pb[o];
                    if (a.clamp) {
                        u = clamp01(u);
                        v = clamp01(v);
                    }
                    if (a.quantize) u = quantize8(u);
                    if (c == 0) m = pm ? pm[o] : 1.f;
                }
                s_a[py][px] = u;
                s_b[py][px] = v;
                if (c == 0) s_m[py][px] = m;
            }
            __syncthreads();
            // horizontal pass: P rows x 16 columns x 5 quantities
            for (int i = threadIdx.x; i < P * MET_T; i += MET_BLOCK) {
                const int r = i / MET_T, cx = i - r * MET_T;
                double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, cnt = 0.0;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) {
                    const double u = (double)s_a[r][cx + k], v = (double)s_b[r][cx + k];
                    if (KIND == MET_BOX) {
                        q[0] += u;
                        q[1] += v;
                        q[2] += u * u;
                        q[3] += v * v;
                        q[4] += u * v;
                    } else {
                        const double m = (double)s_m[r][cx + k], wk = a.w[k];
                        cnt += m;
                        q[0] += wk * (u * m);
                        q[1] += wk * (v * m);
                        q[2] += wk * ((u * u) * m);
                        q[3] += wk * ((v * v) * m);
                        q[4] += wk * ((u * v) * m);
                    }
                }
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    if (KIND == MET_BOX)
                        s_h[j][r][cx] = q[j] / 7.0;
                    else
                        s_h[j][r][cx] = cnt != 0.0 ? q[j] * 11.0 / cnt : 0.0;
                }
                if (KIND == MET_GAUSS) s_hm[r][cx] = cnt != 0.0 ? 1.f : 0.f;
            }
            __syncthreads();
            // vertical pass and the map value of the thread's pixel
            double q[5], cnt = 0.0;
#pragma unroll
            for (int j = 0; j < 5; ++j) q[j] = 0.0;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                if (KIND == MET_GAUSS) cnt += (double)s_hm[ly + k][lx];
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const double h = s_h[j][ly + k][lx];
                    // (a row whose window held no mask pixel is 0 already: h x its mask is h)
                    q[j] += KIND == MET_BOX ? h : a.w[k] * h;
                }
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (KIND == MET_BOX)
                    q[j] = q[j] / 7.0;
                else
                    q[j] = cnt != 0.0 ? q[j] * 11.0 / cnt : 0.0;
            }
            const double m_own = (double)s_m[ly + OFF][lx + OFF];
            if (KIND == MET_BOX) {
                // skimage: sample covariance (x 49 / 48), S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
                const double cov_norm = 49.0 / 48.0;
                const double ux = q[0], uy = q[1];
                const double vx = cov_norm * (q[2] - ux * ux), vy = cov_norm * (q[3] - uy * uy);
                const double vxy = cov_norm * (q[4] - ux * uy);
                const double A1 = 2.0 * ux * uy + a.c1, A2 = 2.0 * vxy + a.c2;
                const double B1 = ux * ux + uy * uy + a.c1, B2 = vx + vy + a.c2;
                const double S = (A1 * A2) / (B1 * B2);
                if (inside) {
                    acc[MET_COL_BOX_MASKED] += S * m_own;
                    if (gx >= 3 && gx < W - 3 && gy >= 3 && gy < H - 3) acc[MET_COL_BOX + c] += S;
                }
            } else {
                // dycheck_metrics.py:176-197
                const double mu0 = q[0], mu1 = q[1];
                const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
                double s00 = q[2] - mu00, s11 = q[3] - mu11, s01 = q[4] - mu01;
                s00 = s00 > 0.0 ? s00 : 0.0;
                s11 = s11 > 0.0 ? s11 : 0.0;
                const double lim = sqrt(s00 * s11), mag = fabs(s01);
                const double sgn = (double)((s01 > 0.0) - (s01 < 0.0));
                s01 = sgn * (lim < mag ? lim : mag);
                const double numer = (2.0 * mu01 + a.c1) * (2.0 * s01 + a.c2);
                const double denom = (mu00 + mu11 + a.c1) * (s00 + s11 + a.c2);
                if (gx < W - 10 && gy < H - 10) acc[MET_COL_GAUSS] += numer / denom;
            }
            if (a.do_err && inside) {
                const double d = (double)s_a[ly + OFF][lx + OFF] - (double)s_b[ly + OFF][lx + OFF];
                acc[MET_COL_ERR] += fabs(d);
                acc[MET_COL_ERR + 1] += d * d;
                acc[MET_COL_ERR + 2] += (d * d) * m_own;
                if (c == 0) acc[MET_COL_ERR + 3] += m_own;
            }
        }
    }
    const size_t row = ((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int c = 0; c < MET_NCOL; ++c) {
        if (!met_owns(KIND, a.do_err, c)) continue;      // (uniform)
        const double total = block_sum<MET_WAVES>(acc[c], s_wave);
        if (threadIdx.x == 0) partial[row * MET_NCOL + c] = total;
    }
}

// out [B, MOBGS_METRICS_COLUMNS]; rows = partial rows of one image.  A column of an arm that did not run is NaN.
__global__ void __launch_bounds__(MET_BLOCK) metrics_finish_kernel(int B, int H, int W, int rows, int arms,
                                                                   const double* __restrict__ partial,
                                                                   double* __restrict__ out) {
    __shared__ double s_wave[MET_WAVES];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int b = 0; b < B; ++b) {
        const double* p = partial + (size_t)b * rows * MET_NCOL;
        double S[MET_NCOL];
#pragma unroll
        for (int c = 0; c < MET_NCOL; ++c) {
            const bool have = c < MET_COL_BOX || (c < MET_COL_GAUSS ? (arms & MOBGS_METRICS_BOX) != 0
                                                                    : (arms & MOBGS_METRICS_GAUSS) != 0);
            S[c] = have ? rows_sum<MET_BLOCK>(p + c, rows, MET_NCOL, s_wave) : nan;
        }
        if (threadIdx.x == 0) {
            double* o = out + (size_t)b * MOBGS_METRICS_COLUMNS;
            const double n = 3.0 * (double)H * (double)W;
            const double mask_sum = 3.0 * S[3];                       // over the mask broadcast to [3,H,W]
            const double mse = S[1] / n;
            o[0] = S[0] / n;
            o[1] = mse;
            o[2] = 20.0 * log10(1.0 / sqrt(mse));                     // utils/image_utils.py:30-31
            // dycheck_metrics.py:57-64, :91-92
            o[3] = -10.0 / log(10.0) * log(S[2] / (mask_sum > 1e-6 ? mask_sum : 1e-6));
            const double nc = (double)(H - 6) * (double)(W - 6);
            o[4] = ((S[4] / nc + S[5] / nc) + S[6] / nc) / 3.0;       // metrics.py:124
            o[5] = S[7] / (mask_sum + 1e-8);                          // metrics.py:62-64
            o[6] = S[8] / (3.0 * (double)(H - 10) * (double)(W - 10));
            o[7] = S[2];
            o[8] = mask_sum;
        }
    }
}

static bool met_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= MET_MAX_B && H >= 1 && W >= 1 && H <= MET_MAX_EDGE && W <= MET_MAX_EDGE;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

size_t mobgs_image_metrics_scratch_doubles(int B, int H, int W) {
    if (!met_shape_ok(B, H, W)) return 0;
    return (size_t)B * met_tile_rows(H) * met_strips(W) * MET_NCOL;
}

int mobgs_image_metrics(int B, int H, int W, const float* pred, const float* gt, const float* mask, int arms, int flags,
                        double data_range, double* partial, double* out, void* stream) {
    if (!met_shape_ok(B, H, W)) {
        set_error("mobgs_image_metrics: B = %d, H = %d, W = %d outside 1 <= B <= %d, 1 <= H, W <= %d", B, H, W, MET_MAX_B,
                  MET_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    if (arms == 0 || (arms & ~(MOBGS_METRICS_BOX | MOBGS_METRICS_GAUSS)) ||
        (flags & ~(MOBGS_METRICS_CLAMP | MOBGS_METRICS_QUANTIZE))) {
        set_error("mobgs_image_metrics: arms = %d must name a window, flags = %d only known bits", arms, flags);
        return MOBGS_E_INVALID;
    }
    if ((arms & MOBGS_METRICS_BOX) && (H < 7 || W < 7)) {
        set_error("mobgs_image_metrics: the 7x7 box window needs H, W >= 7, got %d x %d", H, W);
        return MOBGS_E_INVALID;
    }
    if ((arms & MOBGS_METRICS_GAUSS) && (H < 11 || W < 11)) {
        set_error("mobgs_image_metrics: the 11-tap Gaussian window (valid mode) needs H, W >= 11, got %d x %d", H, W);
        return MOBGS_E_INVALID;
    }
    if (!(data_range > 0.0) || data_range > 1e30) {
        set_error("mobgs_image_metrics: data_range must be a positive finite number");
        return MOBGS_E_INVALID;
    }
    if (!pred || !gt || !partial || !out) {
        set_error("mobgs_image_metrics: NULL pred, gt, partial or out");
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)pred & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)mask & 3) || ((uintptr_t)partial & 7) ||
        ((uintptr_t)out & 7)) {
        set_error("mobgs_image_metrics: images and mask must be 4-byte aligned, partial and out 8-byte aligned");
        return MOBGS_E_INVALID;
    }
    MetArgs a;
    a.H = H;
    a.W = W;
    a.pred = pred;
    a.gt = gt;
    a.mask = mask;
    a.clamp = (flags & MOBGS_METRICS_CLAMP) ? 1 : 0;
    a.quantize = (flags & MOBGS_METRICS_QUANTIZE) ? 1 : 0;
    a.c1 = (0.01 * data_range) * (0.01 * data_range);
    a.c2 = (0.03 * data_range) * (0.03 * data_range);
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        const double f = (double)(i - 5) / 1.5;
        a.w[i] = exp(-0.5 * (f * f));
        sum += a.w[i];
    }
    for (int i = 0; i < 11; ++i) a.w[i] /= sum;
    const dim3 grid((unsigned)met_strips(W), (unsigned)met_tile_rows(H), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    a.do_err = 1;
    if (arms & MOBGS_METRICS_BOX) {
        hipLaunchKernelGGL(metrics_kernel<MET_BOX>, grid, dim3(MET_BLOCK), 0, s, a, partial);
        a.do_err = 0;
    }
    if (arms & MOBGS_METRICS_GAUSS) hipLaunchKernelGGL(metrics_kernel<MET_GAUSS>, grid, dim3(MET_BLOCK), 0, s, a, partial);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MET_BLOCK), 0, s, B, H, W, (int)(grid.x * grid.y), arms,
                       (const double*)partial, out);
    return check_launch("mobgs_image_metrics");
}

}  // extern "C"

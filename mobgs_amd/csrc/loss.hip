// Fused photometric loss kernels for gfx950: L1 + SSIM forward and backward.
//
// Restates for the GPU (the per-pixel cost right after the rasterizer in a train step):
//   /root/reference/utils/loss_utils.py:233-239   l1_loss (mask=None): mean |a - b|
//   /root/reference/utils/loss_utils.py:251-260   11-tap Gaussian window, sigma 1.5, outer product, per channel
//   /root/reference/utils/loss_utils.py:351-381   ssim: five zero-padded 11x11 depthwise convolutions (mu1, mu2,
//                                                 E[x^2], E[y^2], E[xy]) and the SSIM map, mean over all elements
//   /root/reference/train.py:621-628              photo_loss = L1 + lambda_dssim * (1 - ssim)
//
// The reference spends 5 conv2d + ~15 element-wise launches forward and as many backward on 3 x H x W images.  Here
// one workgroup owns a 16x16 output tile of one channel: the 26x26 input patch (halo 5) of both images goes to LDS,
// the separable window runs horizontally then vertically out of LDS, and the kernel emits the per-tile SSIM / L1
// partial sums plus the three derivative maps d(ssim)/d(mu1, E[x^2], E[xy]).  Backward convolves those maps with
// the same window and combines them with the pixel values.  HBM traffic: 8 B read + 12 B written per element
// forward, 20 B read + 4 B written backward.
#include "reduce_shared.h"

namespace mobgs {

constexpr int SS_T = 16;             // output tile edge
constexpr int SS_R = 5;              // window radius (window_size 11)
constexpr int SS_IN = SS_T + 2 * SS_R;  // 26
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

struct Window {
    float w[11];
};

// img1, img2: [C,H,W].  partial: [n_blocks, 2] = {sum of ssim_map, sum of |img1-img2|} per workgroup.
// dmaps: [3][C,H,W] = d ssim / d{mu1, E[x^2], E[xy]} (only when non-null).
__global__ void __launch_bounds__(256)
ssim_l1_fwd_kernel(int C, int H, int W, Window win, const float* __restrict__ img1, const float* __restrict__ img2,
                   float* __restrict__ partial, float* __restrict__ dmaps) {
    __shared__ float s1[SS_IN][SS_IN + 1], s2[SS_IN][SS_IN + 1];
    __shared__ float hz[5][SS_IN][SS_T + 1];
    __shared__ float red[4];
    const int c = blockIdx.z;
    const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
    const size_t plane = (size_t)H * W;
    const float* a = img1 + c * plane;
    const float* b = img2 + c * plane;
    for (int i = threadIdx.x; i < SS_IN * SS_IN; i += 256) {
        const int ly = i / SS_IN, lx = i - ly * SS_IN;
        const int gx = x0 + lx - SS_R, gy = y0 + ly - SS_R;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        s1[ly][lx] = in ? a[(size_t)gy * W + gx] : 0.f;
        s2[ly][lx] = in ? b[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    // horizontal pass: 26 rows x 16 columns x 5 quantities
    for (int i = threadIdx.x; i < SS_IN * SS_T; i += 256) {
        const int ly = i / SS_T, lx = i - ly * SS_T;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float u = s1[ly][lx + k], v = s2[ly][lx + k], wk = win.w[k];
            m1 = __fmaf_rn(wk, u, m1);
            m2 = __fmaf_rn(wk, v, m2);
            e11 = __fmaf_rn(wk, u * u, e11);
            e22 = __fmaf_rn(wk, v * v, e22);
            e12 = __fmaf_rn(wk, u * v, e12);
        }
        hz[0][ly][lx] = m1;
        hz[1][ly][lx] = m2;
        hz[2][ly][lx] = e11;
        hz[3][ly][lx] = e22;
        hz[4][ly][lx] = e12;
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int gx = x0 + lx, gy = y0 + ly;
    float ssim_v = 0.f, l1_v = 0.f;
    if (gx < W && gy < H) {
        float q[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) acc = __fmaf_rn(win.w[k], hz[t][ly + k][lx], acc);
            q[t] = acc;
        }
        const float mu1 = q[0], mu2 = q[1];
        const float sg1 = q[2] - mu1 * mu1, sg2 = q[3] - mu2 * mu2, sg12 = q[4] - mu1 * mu2;
        const float A1 = 2.f * mu1 * mu2 + SS_C1, A2 = 2.f * sg12 + SS_C2;
        const float B1 = mu1 * mu1 + mu2 * mu2 + SS_C1, B2 = sg1 + sg2 + SS_C2;
        const float inv = 1.f / (B1 * B2);
        ssim_v = A1 * A2 * inv;
        l1_v = fabsf(s1[ly + SS_R][lx + SS_R] - s2[ly + SS_R][lx + SS_R]);
        if (dmaps) {
            // d ssim / d mu1 (also through sg1 = E[x^2] - mu1^2 and sg12 = E[xy] - mu1 mu2), / d E[x^2], / d E[xy]
            const float d_mu1 = (2.f * mu2 * A2 - 2.f * mu2 * A1) * inv - ssim_v * (2.f * mu1 * B2 - 2.f * mu1 * B1) * inv;
            const float d_e11 = -ssim_v / B2;
            const float d_e12 = 2.f * A1 * inv;
            const size_t o = c * plane + (size_t)gy * W + gx;
            const size_t CP = (size_t)C * plane;
            dmaps[o] = d_mu1;
            dmaps[CP + o] = d_e11;
            dmaps[2 * CP + o] = d_e12;
        }
    }
    const float ts = block_sum4(ssim_v, red);
    const float tl = block_sum4(l1_v, red);
    if (threadIdx.x == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * blk] = ts;
        partial[2 * blk + 1] = tl;
    }
}

// v_img1 = g_ssim * [ conv(d_mu1) + 2 img1 conv(d_e11) + img2 conv(d_e12) ] + g_l1 * sign(img1 - img2)
// scales: device float[C][2] = per channel {g_ssim, g_l1} (already divided by the element count)
__global__ void __launch_bounds__(256)
ssim_l1_bwd_kernel(int C, int H, int W, Window win, const float* __restrict__ img1, const float* __restrict__ img2,
                   const float* __restrict__ dmaps, const float* __restrict__ scales, float* __restrict__ v_img1) {
    __shared__ float sm[3][SS_IN][SS_IN + 1];
    __shared__ float hz[3][SS_IN][SS_T + 1];
    const int c = blockIdx.z;
    const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
    const size_t plane = (size_t)H * W;
    const size_t CP = (size_t)C * plane;
    const float g_ssim = scales[2 * c], g_l1 = scales[2 * c + 1];  // wave-uniform (one channel per workgroup)
    if (g_ssim != 0.f) {
        for (int i = threadIdx.x; i < SS_IN * SS_IN; i += 256) {
            const int ly = i / SS_IN, lx = i - ly * SS_IN;
            const int gx = x0 + lx - SS_R, gy = y0 + ly - SS_R;
            const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
            const size_t o = c * plane + (size_t)gy * W + gx;
#pragma unroll
            for (int t = 0; t < 3; ++t) sm[t][ly][lx] = in ? dmaps[t * CP + o] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < SS_IN * SS_T; i += 256) {
            const int ly = i / SS_T, lx = i - ly * SS_T;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc = __fmaf_rn(win.w[k], sm[t][ly][lx + k], acc);
                hz[t][ly][lx] = acc;
            }
        }
        __syncthreads();
    }
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int gx = x0 + lx, gy = y0 + ly;
    if (gx < W && gy < H) {
        const size_t o = c * plane + (size_t)gy * W + gx;
        const float u = img1[o], v = img2[o];
        float out = 0.f;
        if (g_ssim != 0.f) {
            float q[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc = __fmaf_rn(win.w[k], hz[t][ly + k][lx], acc);
                q[t] = acc;
            }
            out = g_ssim * (q[0] + 2.f * u * q[1] + v * q[2]);
        }
        const float d = u - v;
        out += g_l1 * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        v_img1[o] = out;
    }
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

static Window make_window() {
    // gaussian(11, 1.5) as the reference builds it: float32 exp values, their float32 sum, float32 division.  torch's
    // sum of the 11 values is the correctly rounded one (3.7592328); adding them one by one in float32 ends one ulp
    // below it (3.7592325), which moves taps by an ulp and every window mean by 6e-8 of its value in the same direction
    Window w;
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        w.w[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += (double)w.w[i];
    }
    const float fsum = (float)sum;
    for (int i = 0; i < 11; ++i) w.w[i] /= fsum;
    return w;
}

int mobgs_ssim_l1_blocks(int C, int H, int W) { return C * ((H + SS_T - 1) / SS_T) * ((W + SS_T - 1) / SS_T); }

int mobgs_ssim_l1_fwd(int C, int H, int W, const float* img1, const float* img2, float* partial, float* dmaps,
                      void* stream) {
    if (C <= 0 || H <= 0 || W <= 0) {
        set_error("mobgs_ssim_l1_fwd: bad sizes C=%d H=%d W=%d", C, H, W);
        return MOBGS_E_INVALID;
    }
    dim3 grid((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, C);
    hipLaunchKernelGGL(ssim_l1_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, C, H, W, make_window(), img1, img2,
                       partial, dmaps);
    return check_launch("ssim_l1_fwd_kernel");
}

int mobgs_ssim_l1_bwd(int C, int H, int W, const float* img1, const float* img2, const float* dmaps,
                      const float* scales, float* v_img1, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0) {
        set_error("mobgs_ssim_l1_bwd: bad sizes C=%d H=%d W=%d", C, H, W);
        return MOBGS_E_INVALID;
    }
    dim3 grid((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, C);
    hipLaunchKernelGGL(ssim_l1_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, C, H, W, make_window(), img1, img2,
                       dmaps, scales, v_img1);
    return check_launch("ssim_l1_bwd_kernel");
}

}  // extern "C"

// K21: the regularisation block of the training loss (the reference's train.py:651-655 with utils/loss_utils.py:233-239,
// :264-276, :285-295, and the PSNR of train.py:622 / utils/image_utils.py:17-38): depth L1, entropy and sparsity of the
// dynamic alpha map, their weighted sum, and optionally the per-image PSNR.  gfx950 only.
//
//   reg_fwd_kernel      one streaming pass over the flattened maps: per workgroup one row {sum |depth - gt|, sum of the
//                       entropy terms, sum alpha^2, sum (image - gt)^2 per image} of float64 partial sums
//   reg_finish_kernel   one workgroup: adds the rows in index order (float64), rounds each sum to fp32 ONCE and forms the
//                       losses in fp32, in the reference's order of operations; the PSNRs in float64, rounded at the end
//   reg_bwd_kernel      one element-wise pass: v_depth and / or v_alpha recomputed from the inputs, fully written
//
// Two ordinary launches forward, one backward, on the caller's stream.  No float atomics and no hand-off between
// workgroups inside a launch: the summation order is a function of the sizes alone, so a result is bit-identical from
// run to run.  Every term is evaluated in fp32 as the reference's statements are written (this file is built with
// -ffp-contract=off); only the ADDING is done in float64 -- a term is rounded as torch rounds it, the sum of the terms is
// then exact to fp32's last place, whatever the map size.
//
// Nothing is clamped: for alpha outside [-eps, 1 + eps] a logarithm has a negative argument, and the NaN it gives reaches
// every output that depends on it, as it does in the reference (where train.py:681 ends the run on it).
//
// Vector access: a map's address only has to be 4-byte aligned (a channel slice, the second image of a batch whose size
// is odd).  Each map is cut into a scalar head (up to 3 elements, until the FIRST array of the map is 16-byte aligned),
// a body of float4 and a scalar tail; the head and the tail are two more "vectors" of the same grid-stride loop.  A
// second array or an output whose own address is not 16-byte aligned at the body's start is accessed element by element
// (a branch that is uniform over the launch).
#include "reduce_shared.h"

namespace mobgs {

constexpr int REG_BLOCK = 256;
constexpr int REG_VEC = 4;
// workgroups at most: 4 per CU, all resident at once (4 waves each; the kernels use few registers); beyond: grid-stride
constexpr int REG_MAX_GRID = 1024;
constexpr int REG_WAVES = REG_BLOCK / MOBGS_WAVE;
constexpr float REG_EPS = 1e-6f;            // utils/loss_utils.py:275
constexpr int REG_SUMS = 3;                 // columns of a partial row ahead of the per-image ones
constexpr int REG_OUT_PSNR = 5;             // out = {reg_loss, depth_loss, mask_loss, entropy, sparsity, psnr[B]}
constexpr int64_t REG_MAX_N = (int64_t)1 << 40;

__host__ __device__ inline int reg_grid(int64_t n) {
    const int64_t per = (int64_t)REG_BLOCK * REG_VEC;
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g < REG_MAX_GRID ? g : REG_MAX_GRID));
}

// fn(x, y) for every element of a[0..n) (y = b[i], or 0 without b); with STORE its value goes to out[i].
template <bool STORE, class Fn>
__device__ __forceinline__ void reg_walk(int64_t n, const float* __restrict__ a, const float* __restrict__ b,
                                         float* __restrict__ out, Fn fn) {
    const int64_t to_boundary = (int64_t)((4 - (((uintptr_t)a >> 2) & 3)) & 3);
    const int64_t head = to_boundary < n ? to_boundary : n;
    const int64_t nvec = (n - head) / REG_VEC;
    const int64_t tail0 = head + nvec * REG_VEC;
    const bool b_vec = b && aligned16(b + head);
    const bool o_vec = STORE && aligned16(out + head);
    const int64_t stride = (int64_t)gridDim.x * REG_BLOCK;
    for (int64_t v = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; v < nvec + 2; v += stride) {
        if (v < nvec) {
            const int64_t i = head + v * REG_VEC;
            const float4 x = *reinterpret_cast<const float4*>(a + i);
            float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b_vec)
                y = *reinterpret_cast<const float4*>(b + i);
            else if (b)
                y = make_float4(b[i], b[i + 1], b[i + 2], b[i + 3]);
            const float4 r = make_float4(fn(x.x, y.x), fn(x.y, y.y), fn(x.z, y.z), fn(x.w, y.w));
            if (STORE) {
                if (o_vec) {
                    *reinterpret_cast<float4*>(out + i) = r;
                } else {
                    out[i] = r.x;
                    out[i + 1] = r.y;
                    out[i + 2] = r.z;
                    out[i + 3] = r.w;
                }
            }
        } else {
            const int64_t lo = v == nvec ? 0 : tail0;
            const int64_t hi = v == nvec ? head : n;
            for (int64_t i = lo; i < hi; ++i) {
                const float r = fn(a[i], b ? b[i] : 0.f);
                if (STORE) out[i] = r;
            }
        }
    }
}

struct RegMaps {
    int64_t n_d, n_a, n_img;          // elements of depth, of alpha, of ONE image (3 H W)
    const float *depth, *gt_depth;    // both NULL: no depth term
    const float* alpha;               // NULL: no alpha term
    const float *image, *gt_image;    // [B, n_img]; both NULL: no PSNR
    int B, entropy, sparsity;
};

// one entropy term, each operation rounded to fp32 as torch rounds it: a log(a + eps) + (1 - a) log(1 - a + eps)
__device__ __forceinline__ float reg_entropy_term(float a) {
    const float na = 1.f - a;
    return a * logf(a + REG_EPS) + na * logf(na + REG_EPS);
}

__global__ void __launch_bounds__(REG_BLOCK) reg_fwd_kernel(RegMaps m, double* __restrict__ partial) {
    __shared__ double s_wave[REG_WAVES];
    double* row = partial + (size_t)blockIdx.x * (REG_SUMS + m.B);
    double sd = 0.0, se = 0.0, ss = 0.0;
    if (m.depth)
        reg_walk<false>(m.n_d, m.depth, m.gt_depth, nullptr, [&](float x, float y) {
            sd += (double)fabsf(x - y);
            return 0.f;
        });
    if (m.alpha) {
        const bool entropy = m.entropy != 0, sparsity = m.sparsity != 0;
        reg_walk<false>(m.n_a, m.alpha, nullptr, nullptr, [&](float a, float) {
            if (entropy) se += (double)reg_entropy_term(a);
            if (sparsity) ss += (double)(a * a);
            return 0.f;
        });
    }
    sd = block_sum<REG_WAVES>(sd, s_wave);
    se = block_sum<REG_WAVES>(se, s_wave);
    ss = block_sum<REG_WAVES>(ss, s_wave);
    if (threadIdx.x == 0) {
        row[0] = sd;
        row[1] = se;
        row[2] = ss;
    }
    for (int b = 0; b < m.B; ++b) {
        double sq = 0.0;
        reg_walk<false>(m.n_img, m.image + (size_t)b * m.n_img, m.gt_image + (size_t)b * m.n_img, nullptr,
                        [&](float x, float y) {
                            const float d = x - y;
                            sq += (double)(d * d);
                            return 0.f;
                        });
        sq = block_sum<REG_WAVES>(sq, s_wave);
        if (threadIdx.x == 0) row[REG_SUMS + b] = sq;
    }
}

__global__ void __launch_bounds__(REG_BLOCK) reg_finish_kernel(RegMaps m, int nb, float w_d, float w_e, float w_s,
                                                               const double* __restrict__ partial,
                                                               float* __restrict__ out) {
    __shared__ double s_wave[REG_WAVES];
    const int ncol = REG_SUMS + m.B;
    // (the three sums are meaningful in thread 0 only, which is the one that uses them)
    const float S_d = (float)rows_sum<REG_BLOCK>(partial, nb, ncol, s_wave);
    const float S_e = (float)rows_sum<REG_BLOCK>(partial + 1, nb, ncol, s_wave);
    const float S_s = (float)rows_sum<REG_BLOCK>(partial + 2, nb, ncol, s_wave);
    if (threadIdx.x == 0) {
        // train.py:651-655: depth_loss = mean |.|; reg_loss = 0 + 0.2 depth_loss; mask_loss = 1e-7 E + 1e-7 S;
        // reg_loss += mask_loss
        const float depth_loss = m.depth ? S_d / (float)m.n_d : 0.f;
        const float entropy = -S_e;
        const float mask_loss = w_e * entropy + w_s * S_s;
        out[0] = (0.f + w_d * depth_loss) + mask_loss;
        out[1] = depth_loss;
        out[2] = mask_loss;
        out[3] = entropy;
        out[4] = S_s;
    }
    for (int b = 0; b < m.B; ++b) {
        const double S_b = rows_sum<REG_BLOCK>(partial + REG_SUMS + b, nb, ncol, s_wave);
        if (threadIdx.x == 0) {
            // utils/image_utils.py:30-31: 20 log10(1 / sqrt(mean((img1 - img2)^2))).  The one value formed in float64 and
            // rounded at the end: at 16 .. 32 dB the last place of an fp32 is 1.9e-6 dB and one ulp of an fp32 log10
            // becomes 2.4e-6 dB, more than a relative error of 8 x 2^-24 of the mean squared error is worth (2.1e-6 dB).
            out[REG_OUT_PSNR + b] = (float)(20.0 * log10(1.0 / sqrt(S_b / (double)m.n_img)));
        }
    }
}

__global__ void __launch_bounds__(REG_BLOCK) reg_bwd_kernel(RegMaps m, float w_d, float w_e, float w_s,
                                                            const float* __restrict__ v_loss,
                                                            float* __restrict__ v_depth, float* __restrict__ v_alpha) {
    const float g = *v_loss;
    if (v_depth) {
        // autograd's own chain: (g w_d) / n_d through the mean, times sgn(depth - gt) through abs (sgn(0) = 0; the
        // product, not a select, so that a zero carries the sign torch gives it)
        const float c = (g * w_d) / (float)m.n_d;
        reg_walk<true>(m.n_d, m.depth, m.gt_depth, v_depth, [&](float x, float y) {
            const float d = x - y;
            return c * (float)((d > 0.f) - (d < 0.f));
        });
    }
    if (v_alpha) {
        const bool entropy = m.entropy != 0, sparsity = m.sparsity != 0;
        const float ge = -(g * w_e), gs = g * w_s;
        reg_walk<true>(m.n_a, m.alpha, nullptr, v_alpha, [&](float a, float) {
            float v = 0.f;
            if (entropy) {
                // d/da [a log(a + eps) + (1 - a) log(1 - a + eps)]
                const float p = a + REG_EPS, na = 1.f - a, q = na + REG_EPS;
                v = ge * ((logf(p) + a / p) - (logf(q) + na / q));
            }
            if (sparsity) v += gs * (2.f * a);
            return v;
        });
    }
}

static bool reg_n_ok(int64_t n) { return n >= 1 && n <= REG_MAX_N; }

// The checks that forward and backward share.  -> NULL, or what is wrong.
static const char* reg_check_maps(int64_t n_d, const float* depth, const float* gt_depth, int64_t n_a, const float* alpha,
                                  int terms) {
    if ((depth == nullptr) != (gt_depth == nullptr)) return "depth and gt_depth must both be given or both be NULL";
    if (depth ? !reg_n_ok(n_d) : n_d != 0) return "n_d must be in [1, 2^40] with a depth map and 0 without";
    if (alpha ? !reg_n_ok(n_a) : n_a != 0) return "n_a must be in [1, 2^40] with an alpha map and 0 without";
    if (terms & ~(MOBGS_REG_ENTROPY | MOBGS_REG_SPARSITY)) return "unknown bit in terms";
    if ((alpha != nullptr) != (terms != 0)) return "terms must name an alpha term exactly when alpha is given";
    if (!depth && !alpha) return "neither a depth map nor an alpha map";
    if (((uintptr_t)depth & 3) || ((uintptr_t)gt_depth & 3) || ((uintptr_t)alpha & 3)) return "maps must be 4-byte aligned";
    return nullptr;
}

static int64_t reg_largest(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_reg_terms_blocks(int64_t n) { return reg_n_ok(n) ? reg_grid(n) : 0; }

int mobgs_reg_terms_fwd(int64_t n_d, const float* depth, const float* gt_depth, int64_t n_a, const float* alpha,
                        int terms, float w_d, float w_e, float w_s, int B, int H, int W, const float* image,
                        const float* gt_image, double* partial, float* out, void* stream) {
    if (const char* why = reg_check_maps(n_d, depth, gt_depth, n_a, alpha, terms)) {
        set_error("mobgs_reg_terms_fwd: %s", why);
        return MOBGS_E_INVALID;
    }
    if ((image == nullptr) != (gt_image == nullptr)) {
        set_error("mobgs_reg_terms_fwd: image and gt_image must both be given or both be NULL");
        return MOBGS_E_INVALID;
    }
    const int64_t n_img = image ? (int64_t)3 * H * W : 0;
    if (image ? (B < 1 || B > MOBGS_REG_MAX_IMAGES || H < 1 || W < 1 || !reg_n_ok(n_img)) : (B != 0)) {
        set_error("mobgs_reg_terms_fwd: B = %d, H = %d, W = %d; images need 1 <= B <= %d and H, W >= 1, and B = 0 "
                  "goes without images", B, H, W, MOBGS_REG_MAX_IMAGES);
        return MOBGS_E_INVALID;
    }
    if (!partial || !out) {
        set_error("mobgs_reg_terms_fwd: NULL partial or out");
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)image & 3) || ((uintptr_t)gt_image & 3) || ((uintptr_t)partial & 7) || ((uintptr_t)out & 3)) {
        set_error("mobgs_reg_terms_fwd: images and out must be 4-byte aligned, partial 8-byte aligned");
        return MOBGS_E_INVALID;
    }
    RegMaps m{n_d, n_a, n_img, depth, gt_depth, alpha, image, gt_image, B, terms & MOBGS_REG_ENTROPY,
              terms & MOBGS_REG_SPARSITY};
    const int nb = reg_grid(reg_largest(n_d, n_a, n_img));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(reg_fwd_kernel, dim3((unsigned)nb), dim3(REG_BLOCK), 0, s, m, partial);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(REG_BLOCK), 0, s, m, nb, w_d, w_e, w_s,
                       (const double*)partial, out);
    return check_launch("mobgs_reg_terms_fwd");
}

int mobgs_reg_terms_bwd(int64_t n_d, const float* depth, const float* gt_depth, int64_t n_a, const float* alpha,
                        int terms, float w_d, float w_e, float w_s, const float* v_loss, float* v_depth,
                        float* v_alpha, void* stream) {
    if (const char* why = reg_check_maps(n_d, depth, gt_depth, n_a, alpha, terms)) {
        set_error("mobgs_reg_terms_bwd: %s", why);
        return MOBGS_E_INVALID;
    }
    if (!v_loss || (!v_depth && !v_alpha)) {
        set_error("mobgs_reg_terms_bwd: NULL v_loss, or neither v_depth nor v_alpha");
        return MOBGS_E_INVALID;
    }
    if ((v_depth && !depth) || (v_alpha && !alpha)) {
        set_error("mobgs_reg_terms_bwd: a gradient is wanted for a map that is not given");
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)v_loss & 3) || ((uintptr_t)v_depth & 3) || ((uintptr_t)v_alpha & 3)) {
        set_error("mobgs_reg_terms_bwd: v_loss, v_depth and v_alpha must be 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    RegMaps m{n_d, n_a, 0, depth, gt_depth, alpha, nullptr, nullptr, 0, terms & MOBGS_REG_ENTROPY,
              terms & MOBGS_REG_SPARSITY};
    const int nb = reg_grid(reg_largest(v_depth ? n_d : 0, v_alpha ? n_a : 0, 1));
    hipLaunchKernelGGL(reg_bwd_kernel, dim3((unsigned)nb), dim3(REG_BLOCK), 0, (hipStream_t)stream, m, w_d, w_e, w_s,
                       v_loss, v_depth, v_alpha);
    return check_launch("mobgs_reg_terms_bwd");
}

}  // extern "C"

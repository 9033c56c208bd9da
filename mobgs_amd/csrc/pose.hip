// K23: test-time pose refinement (the reference's eval.py:43-166, render_test_tto): the pose head -- quaternion and
// translation to a world-to-camera matrix, pytorch3d's quaternion_to_matrix as eval.py:122-123 uses it --, the -PSNR loss
// of eval.py:137-139 with its gradient, and the optimiser step on the seven pose values.  gfx950 only.
//
//   pose_head_fwd_kernel   one wave: w2c [4,4] from q [4] (real part first, NOT normalised) and t [3]
//   pose_head_bwd_kernel   one wave: the exact Jacobian of that expression, two_s = 2 / (q . q) included
//   neg_psnr_fwd_kernel    one streaming pass: per workgroup the float64 sum of the fp32 squares of its range
//   neg_psnr_finish_kernel one workgroup: adds the partial sums in a fixed order, mse (float64) and the loss (fp32)
//   neg_psnr_bwd_kernel    one element-wise pass: v_pred = c (pred - gt), c read from the device
//   pose_step_kernel       one wave: head backward, Adam on the seven values (csrc/adam_shared.h: the arithmetic of
//                          adam_step_kernel), head forward for the next step; the cotangent is cleared
//
// Built with -ffp-contract=off: every fp32 expression is evaluated as written, so the head inside pose_step_kernel gives
// the bits the stand-alone head kernels give, and a sum of squares does not depend on what the compiler fuses.
//
// The loss.  Differences and squares in fp32, as the reference forms them; the ADDING in float64.  The image is cut into
// quads of four consecutive elements counted from element 0; workgroup b owns a fixed contiguous run of quads, thread t
// of it the quads t, t + 256, ... of the run, and the sums are combined in a fixed order (down the wave by shuffles, the
// waves in wave order; the workgroups' sums likewise, each thread of the finishing launch first adding a run of
// consecutive workgroups).  Which element is added where is a function of n alone -- not of the address: the same data
// at another address gives the same bits, and there is no atomic.  A base pointer only has to be 4-byte aligned (a slice
// images[k] of a stack): an array whose address is 16-byte aligned is read with one 16-byte load per quad, another one
// element by element (a branch that is uniform over the launch); the last, partial quad is read element by element in
// either case.
#include "adam_shared.h"
#include "reduce_shared.h"

namespace mobgs {

constexpr int POSE_BLOCK = 256;
constexpr int POSE_WAVES = POSE_BLOCK / MOBGS_WAVE;
// workgroups at most: 4 per CU, all resident at once; beyond that a workgroup's run of quads grows
constexpr int POSE_MAX_GRID = 1024;
constexpr int64_t POSE_MAX_N = (int64_t)1 << 40;

__host__ __device__ inline bool pose_n_ok(int64_t n) { return n >= 1 && n <= POSE_MAX_N; }
__host__ __device__ inline int64_t pose_quads(int64_t n) { return (n + 3) / 4; }
__host__ __device__ inline int pose_grid(int64_t n) {
    const int64_t g = (pose_quads(n) + POSE_BLOCK - 1) / POSE_BLOCK;
    return (int)(g < POSE_MAX_GRID ? g : POSE_MAX_GRID);
}
// quads per workgroup: the same for every workgroup (the last ones may own fewer, or none)
__host__ __device__ inline int64_t pose_run(int64_t n) {
    const int g = pose_grid(n);
    return (pose_quads(n) + g - 1) / g;
}

// ---- the head -------------------------------------------------------------------------------------------------------
// pytorch3d.transforms.quaternion_to_matrix as written: q = (r, i, j, k), two_s = 2 / (q . q), and
//   R = [[1 - two_s (jj + kk), two_s (ij - kr), two_s (ik + jr)],
//        [two_s (ij + kr), 1 - two_s (ii + kk), two_s (jk - ir)],
//        [two_s (ik - jr), two_s (jk + ir), 1 - two_s (ii + jj)]];   w2c = [[R, t], [0 0 0 1]], row-major.
__device__ __forceinline__ float pose_two_s(const float q[4]) {
    return 2.f / (((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
}

__device__ __forceinline__ void pose_head(const float q[4], const float t[3], float w[16]) {
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float s = pose_two_s(q);
    w[0] = 1.f - s * (j * j + k * k);
    w[1] = s * (i * j - k * r);
    w[2] = s * (i * k + j * r);
    w[3] = t[0];
    w[4] = s * (i * j + k * r);
    w[5] = 1.f - s * (i * i + k * k);
    w[6] = s * (j * k - i * r);
    w[7] = t[1];
    w[8] = s * (i * k - j * r);
    w[9] = s * (j * k + i * r);
    w[10] = 1.f - s * (i * i + j * j);
    w[11] = t[2];
    w[12] = 0.f;
    w[13] = 0.f;
    w[14] = 0.f;
    w[15] = 1.f;
}

// With R = I + s M(q): v_q = s (dM/dq)^T g + (ds/dq) <g, M>, ds/dq = -s^2 q.  g = the cotangent of w2c, of which the
// bottom row does not depend on the pose.  The two parts cancel along q (R does not depend on |q|).
__device__ __forceinline__ void pose_head_vjp(const float q[4], const float g[16], float vq[4], float vt[3]) {
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float s = pose_two_s(q);
    const float g00 = g[0], g01 = g[1], g02 = g[2], g10 = g[4], g11 = g[5], g12 = g[6], g20 = g[8], g21 = g[9], g22 = g[10];
    // <g, M>: the cotangent of s
    const float vs = ((((-(j * j + k * k)) * g00 + (i * j - k * r) * g01) + (i * k + j * r) * g02) +
                      (((i * j + k * r) * g10 + (-(i * i + k * k)) * g11) + (j * k - i * r) * g12)) +
                     (((i * k - j * r) * g20 + (j * k + i * r) * g21) + (-(i * i + j * j)) * g22);
    const float c = (s * s) * vs;
    const float a01 = g01 + g10, a02 = g02 + g20, a12 = g12 + g21;      // the symmetric part of g
    const float d10 = g10 - g01, d02 = g02 - g20, d21 = g21 - g12;      // the antisymmetric part
    vq[0] = s * ((k * d10 + j * d02) + i * d21) - c * r;
    vq[1] = s * (((j * a01 + k * a02) - 2.f * i * (g11 + g22)) + r * d21) - c * i;
    vq[2] = s * (((i * a01 + k * a12) - 2.f * j * (g00 + g22)) + r * d02) - c * j;
    vq[3] = s * (((i * a02 + j * a12) - 2.f * k * (g00 + g11)) + r * d10) - c * k;
    vt[0] = g[3];
    vt[1] = g[7];
    vt[2] = g[11];
}

// The three kernels below do their work in lane 0 of one wave: about a hundred dependent fp32 operations on seven values.
__global__ void __launch_bounds__(MOBGS_WAVE)
pose_head_fwd_kernel(const float* __restrict__ q, const float* __restrict__ t, float* __restrict__ w2c) {
    if (threadIdx.x != 0) return;
    const float qq[4] = {q[0], q[1], q[2], q[3]}, tt[3] = {t[0], t[1], t[2]};
    float w[16];
    pose_head(qq, tt, w);
#pragma unroll
    for (int e = 0; e < 16; ++e) w2c[e] = w[e];
}

__global__ void __launch_bounds__(MOBGS_WAVE)
pose_head_bwd_kernel(const float* __restrict__ q, const float* __restrict__ v_w2c, float* __restrict__ v_q,
                     float* __restrict__ v_t) {
    if (threadIdx.x != 0) return;
    const float qq[4] = {q[0], q[1], q[2], q[3]};
    float g[16], vq[4], vt[3];
#pragma unroll
    for (int e = 0; e < 16; ++e) g[e] = v_w2c[e];
    pose_head_vjp(qq, g, vq, vt);
#pragma unroll
    for (int e = 0; e < 4; ++e) v_q[e] = vq[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) v_t[e] = vt[e];
}

struct PoseStep {
    float *q, *t, *v_w2c, *exp_avg, *exp_avg_sq, *w2c;   // exp_avg, exp_avg_sq [7]: q's four values, then t's three
    float step_size_q, step_size_t, bias2_sqrt, w1, beta2, w2, eps;
};

// (no __restrict__: q, t and the moments are read and written)
__global__ void __launch_bounds__(MOBGS_WAVE) pose_step_kernel(PoseStep a) {
    if (threadIdx.x != 0) return;
    float p[7] = {a.q[0], a.q[1], a.q[2], a.q[3], a.t[0], a.t[1], a.t[2]};
    float g[16], v[7];
#pragma unroll
    for (int e = 0; e < 16; ++e) g[e] = a.v_w2c[e];
    pose_head_vjp(p, g, v, v + 4);
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        float m = a.exp_avg[e], s = a.exp_avg_sq[e];
        adam_update(p[e], v[e], m, s, a.w1, a.beta2, a.w2, a.eps, e < 4 ? a.step_size_q : a.step_size_t, a.bias2_sqrt);
        a.exp_avg[e] = m;
        a.exp_avg_sq[e] = s;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a.q[e] = p[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) a.t[e] = p[4 + e];
    float w[16];
    pose_head(p, p + 4, w);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        a.w2c[e] = w[e];
        a.v_w2c[e] = 0.f;      // optimizer.zero_grad() of the next step
    }
}

// ---- the loss -------------------------------------------------------------------------------------------------------
// the four elements of quad qd (all inside the array)
__device__ __forceinline__ float4 pose_load_quad(const float* __restrict__ a, int64_t qd, bool vec) {
    const float* p = a + qd * 4;
    return vec ? *reinterpret_cast<const float4*>(p) : make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ float pose_sq(float x, float y) {
    const float d = x - y;
    return d * d;
}

__global__ void __launch_bounds__(POSE_BLOCK)
neg_psnr_fwd_kernel(int64_t n, const float* __restrict__ pred, const float* __restrict__ gt, double* __restrict__ partial) {
    __shared__ double s_wave[POSE_WAVES];
    const int64_t full = n / 4, run = pose_run(n);       // full: the quads that lie inside the array entirely
    const int64_t q0 = (int64_t)blockIdx.x * run;
    const int64_t q1 = q0 + run < pose_quads(n) ? q0 + run : pose_quads(n);
    const bool pv = aligned16(pred), gv = aligned16(gt);
    double sum = 0.0;
    for (int64_t qd = q0 + threadIdx.x; qd < q1; qd += POSE_BLOCK) {
        if (qd < full) {
            const float4 x = pose_load_quad(pred, qd, pv), y = pose_load_quad(gt, qd, gv);
            sum += (double)pose_sq(x.x, y.x);
            sum += (double)pose_sq(x.y, y.y);
            sum += (double)pose_sq(x.z, y.z);
            sum += (double)pose_sq(x.w, y.w);
        } else {
            for (int64_t e = qd * 4; e < n; ++e) sum += (double)pose_sq(pred[e], gt[e]);
        }
    }
    sum = block_sum<POSE_WAVES>(sum, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(POSE_BLOCK)
neg_psnr_finish_kernel(int64_t n, int nb, const double* __restrict__ partial, double* __restrict__ mse,
                       float* __restrict__ loss) {
    __shared__ double s_wave[POSE_WAVES];
    const double s = rows_sum<POSE_BLOCK>(partial, nb, 1, s_wave);
    if (threadIdx.x == 0) {
        // eval.py:137-139: -(20 log10(1 / sqrt(mse))), in float64 and rounded once (csrc/regterms.hip says why); mse == 0
        // gives -inf
        const double m = s / (double)n;
        *mse = m;
        *loss = (float)(-(20.0 * log10(1.0 / sqrt(m))));
    }
}

__global__ void __launch_bounds__(POSE_BLOCK)
neg_psnr_bwd_kernel(int64_t n, const float* __restrict__ pred, const float* __restrict__ gt,
                    const double* __restrict__ mse, const float* __restrict__ v_loss, float* __restrict__ v_pred) {
    // d loss / d mse = 10 / (ln 10 mse), d mse / d pred = 2 (pred - gt) / n.  The factor in float64, rounded once; with
    // mse == 0 it is +inf and every element inf * 0 = NaN, which is what autograd gives.
    const double up = v_loss ? (double)*v_loss : 1.0;
    const float c = (float)(up * 20.0 / (2.302585092994045684 * (double)n * *mse));
    const int64_t full = n / 4, quads = pose_quads(n);
    const bool pv = aligned16(pred), gv = aligned16(gt), ov = aligned16(v_pred);
    const int64_t stride = (int64_t)gridDim.x * POSE_BLOCK;
    for (int64_t qd = (int64_t)blockIdx.x * POSE_BLOCK + threadIdx.x; qd < quads; qd += stride) {
        if (qd < full) {
            const float4 x = pose_load_quad(pred, qd, pv), y = pose_load_quad(gt, qd, gv);
            const float4 r = make_float4(c * (x.x - y.x), c * (x.y - y.y), c * (x.z - y.z), c * (x.w - y.w));
            float* o = v_pred + qd * 4;
            if (ov) {
                *reinterpret_cast<float4*>(o) = r;
            } else {
                o[0] = r.x;
                o[1] = r.y;
                o[2] = r.z;
                o[3] = r.w;
            }
        } else {
            for (int64_t e = qd * 4; e < n; ++e) v_pred[e] = c * (pred[e] - gt[e]);
        }
    }
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_pose_head_fwd(const float* q, const float* t, float* w2c, void* stream) {
    if (!q || !t || !w2c || !aligned(q, 4) || !aligned(t, 4) || !aligned(w2c, 4)) {
        set_error("mobgs_pose_head_fwd: q, t and w2c must be given and 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(pose_head_fwd_kernel, dim3(1), dim3(MOBGS_WAVE), 0, (hipStream_t)stream, q, t, w2c);
    return check_launch("mobgs_pose_head_fwd");
}

int mobgs_pose_head_bwd(const float* q, const float* v_w2c, float* v_q, float* v_t, void* stream) {
    if (!q || !v_w2c || !v_q || !v_t || !aligned(q, 4) || !aligned(v_w2c, 4) || !aligned(v_q, 4) || !aligned(v_t, 4)) {
        set_error("mobgs_pose_head_bwd: q, v_w2c, v_q and v_t must be given and 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(pose_head_bwd_kernel, dim3(1), dim3(MOBGS_WAVE), 0, (hipStream_t)stream, q, v_w2c, v_q, v_t);
    return check_launch("mobgs_pose_head_bwd");
}

int mobgs_pose_step(float* q, float* t, float* v_w2c, float* exp_avg, float* exp_avg_sq, float step_size_q,
                    float step_size_t, float bias2_sqrt, double beta1, double beta2, double eps, float* w2c,
                    void* stream) {
    float* const all[6] = {q, t, v_w2c, exp_avg, exp_avg_sq, w2c};
    for (float* p : all) {
        if (!p || !aligned(p, 4)) {
            set_error("mobgs_pose_step: q, t, v_w2c, exp_avg, exp_avg_sq and w2c must be given and 4-byte aligned");
            return MOBGS_E_INVALID;
        }
    }
    // (1 - beta is formed in double before it is rounded, as mobgs_adam_step and torch do)
    PoseStep a{q, t, v_w2c, exp_avg, exp_avg_sq, w2c, step_size_q, step_size_t, bias2_sqrt,
               (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    hipLaunchKernelGGL(pose_step_kernel, dim3(1), dim3(MOBGS_WAVE), 0, (hipStream_t)stream, a);
    return check_launch("mobgs_pose_step");
}

size_t mobgs_neg_psnr_scratch_doubles(int64_t n) { return pose_n_ok(n) ? (size_t)pose_grid(n) : 0; }

int mobgs_neg_psnr_fwd(int64_t n, const float* pred, const float* gt, double* partial, double* mse, float* loss,
                       void* stream) {
    if (!pose_n_ok(n)) {
        set_error("mobgs_neg_psnr_fwd: n = %lld outside [1, 2^40]", (long long)n);
        return MOBGS_E_INVALID;
    }
    if (!pred || !gt || !partial || !mse || !loss) {
        set_error("mobgs_neg_psnr_fwd: NULL pred, gt, partial, mse or loss");
        return MOBGS_E_INVALID;
    }
    if (!aligned(pred, 4) || !aligned(gt, 4) || !aligned(loss, 4) || !aligned(partial, 8) || !aligned(mse, 8)) {
        set_error("mobgs_neg_psnr_fwd: pred, gt and loss must be 4-byte aligned, partial and mse 8-byte aligned");
        return MOBGS_E_INVALID;
    }
    const int nb = pose_grid(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(neg_psnr_fwd_kernel, dim3((unsigned)nb), dim3(POSE_BLOCK), 0, s, n, pred, gt, partial);
    hipLaunchKernelGGL(neg_psnr_finish_kernel, dim3(1), dim3(POSE_BLOCK), 0, s, n, nb, (const double*)partial, mse, loss);
    return check_launch("mobgs_neg_psnr_fwd");
}

int mobgs_neg_psnr_bwd(int64_t n, const float* pred, const float* gt, const double* mse, const float* v_loss,
                       float* v_pred, void* stream) {
    if (!pose_n_ok(n)) {
        set_error("mobgs_neg_psnr_bwd: n = %lld outside [1, 2^40]", (long long)n);
        return MOBGS_E_INVALID;
    }
    if (!pred || !gt || !mse || !v_pred) {
        set_error("mobgs_neg_psnr_bwd: NULL pred, gt, mse or v_pred");
        return MOBGS_E_INVALID;
    }
    if (!aligned(pred, 4) || !aligned(gt, 4) || !aligned(v_loss, 4) || !aligned(v_pred, 4) || !aligned(mse, 8)) {
        set_error("mobgs_neg_psnr_bwd: pred, gt, v_loss and v_pred must be 4-byte aligned, mse 8-byte aligned");
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(neg_psnr_bwd_kernel, dim3((unsigned)pose_grid(n)), dim3(POSE_BLOCK), 0, (hipStream_t)stream, n,
                       pred, gt, mse, v_loss, v_pred);
    return check_launch("mobgs_neg_psnr_bwd");
}

}  // extern "C"

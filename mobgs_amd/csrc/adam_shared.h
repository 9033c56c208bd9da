// The Adam update of one fp32 value (include/mobgs_hip.h K16), shared by adam_step_kernel (csrc/densify.hip) and
// pose_step_kernel (csrc/pose.hip, K23) so that the two cannot drift apart.
//
// The three multiply-adds are written as explicit fused operations and nothing else may be contracted: the value an
// element gets is then a function of its inputs alone -- not of the translation unit's -ffp-contract setting, and not of
// whether the element sits in the float4 body or in the scalar tail of a tensor.  (Left to the compiler, the float4 body
// of adam_step_kernel was built with all three fused while its scalar tail formed beta2 v and w2 g^2 as two products and
// an add: one rounding more in exp_avg_sq for the up to three tail elements of a tensor.  The forms below are the float4
// body's.)
#pragma once
#include <hip/hip_runtime.h>

namespace mobgs {

// w1 = 1 - beta1 and w2 = 1 - beta2 (formed in double by the caller, then rounded); step_size = lr / (1 - beta1^t),
// bias2_sqrt = sqrt(1 - beta2^t).
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float w1, float beta2, float w2,
                                            float eps, float step_size, float bias2_sqrt) {
#pragma clang fp contract(off)
    m = __builtin_fmaf(w1, g - m, m);                 // exp_avg.lerp_(grad, 1 - beta1)
    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2); torch.optim.Adam's multi-tensor addcmul forms
    // grad * grad first, so |grad| >= 1.9e19 overflows to inf there -- (w2 * g) * g stayed finite up to 5.8e20
    v = __builtin_fmaf(w2, g * g, v * beta2);
    const float denom = sqrtf(v) / bias2_sqrt + eps;
    p = __builtin_fmaf(-step_size, m / denom, p);     // param.addcdiv_(exp_avg, denom, value = -step_size)
}

}  // namespace mobgs

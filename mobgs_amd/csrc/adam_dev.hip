// The Adam step with its factors formed on the device (include/mobgs_hip.h K27): what makes the optimiser step of an
// iteration recordable into a graph.  mobgs_adam_step (csrc/densify.hip, K16) takes lr / (1 - beta1^t) and sqrt(1 - beta2^t)
// from the host in its argument block; here a prologue kernel looks them up in float64 tables the host filled once and
// advances the counters, and the update kernel reads descriptors and factors from device memory.
//
// Built with the flags of densify.hip and with nothing that loosens floating point (no -ffast-math, no reciprocal
// substitution): the double quotient below is then the correctly rounded one and its conversion rounds to nearest even,
// i.e. the bits of the host's lr / (1.0 - b1 ** t) passed through a c_float, and adam_update is the code K16 runs.
#include "adam_shared.h"
#include "common.h"

namespace mobgs {

// one workgroup; a thread per tensor (strided when there are more tensors than threads).  Every thread reads the iteration
// before the barrier, one thread advances it after.
__global__ void __launch_bounds__(256)
adam_dev_factors_kernel(int n, const MobgsAdamDevSchedule* __restrict__ sched, int32_t* __restrict__ counters,
                        float* __restrict__ factors) {
    const int32_t it = counters[0];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const MobgsAdamDevSchedule S = sched[i];
        const int32_t step = counters[1 + i];
        int32_t row = it < 0 ? 0 : it;
        row = row > S.lr_rows - 1 ? S.lr_rows - 1 : row;
        row = row < 0 ? 0 : row;
        int32_t t = step < 0 ? 0 : (step < 0x7fffffff ? step + 1 : step);
        t = t > S.bc_rows - 1 ? S.bc_rows - 1 : t;
        t = t < 0 ? 0 : t;
        const double lr = S.lr[(int64_t)row * S.lr_stride];
        factors[2 * i] = (float)(lr / S.bc1[t]);
        factors[2 * i + 1] = (float)S.bc2s[t];
        counters[1 + i] = step < 0x7fffffff ? step + 1 : step;
    }
    __syncthreads();
    if (threadIdx.x == 0) counters[0] = it < 0x7fffffff ? it + 1 : it;
}

// adam_step_kernel's body (csrc/densify.hip), the tensor's record and factors read from device memory.
// grid (blocks over the longest tensor, tensor): tensors shorter than the grid exit at once
__global__ void __launch_bounds__(256)
adam_dev_step_kernel(const MobgsAdamDevTensor* __restrict__ tensors, const float* __restrict__ factors) {
    const MobgsAdamDevTensor T = tensors[blockIdx.y];
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= T.n) return;
    const float step_size = factors[2 * blockIdx.y], bias2_sqrt = factors[2 * blockIdx.y + 1];
    auto one = [&](float& p, float g, float& m, float& v) {
        adam_update(p, g, m, v, T.w1, T.beta2, T.w2, T.eps, step_size, bias2_sqrt);   // csrc/adam_shared.h
    };
    if (i0 + 4 <= T.n && ((((uintptr_t)T.param | (uintptr_t)T.grad | (uintptr_t)T.exp_avg | (uintptr_t)T.exp_avg_sq) & 15) == 0)) {
        float4 p = *reinterpret_cast<float4*>(T.param + i0);
        const float4 g = *reinterpret_cast<const float4*>(T.grad + i0);
        float4 m = *reinterpret_cast<float4*>(T.exp_avg + i0);
        float4 v = *reinterpret_cast<float4*>(T.exp_avg_sq + i0);
        one(p.x, g.x, m.x, v.x);
        one(p.y, g.y, m.y, v.y);
        one(p.z, g.z, m.z, v.z);
        one(p.w, g.w, m.w, v.w);
        *reinterpret_cast<float4*>(T.param + i0) = p;
        *reinterpret_cast<float4*>(T.exp_avg + i0) = m;
        *reinterpret_cast<float4*>(T.exp_avg_sq + i0) = v;
    } else {
        for (int64_t i = i0; i < T.n && i < i0 + 4; ++i) one(T.param[i], T.grad[i], T.exp_avg[i], T.exp_avg_sq[i]);
    }
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_adam_dev_factors(int n_tensors, const MobgsAdamDevSchedule* schedules_dev, int32_t* counters_dev,
                           float* factors_dev, void* stream) {
    if (n_tensors < 0 || n_tensors > 65535 || !counters_dev || (n_tensors > 0 && (!schedules_dev || !factors_dev))) {
        set_error("mobgs_adam_dev_factors: n_tensors = %d (0..65535) or a NULL pointer", n_tensors);
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(adam_dev_factors_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_tensors, schedules_dev,
                       counters_dev, factors_dev);
    return check_launch("adam_dev_factors_kernel");
}

int mobgs_adam_dev_step(int n_tensors, const MobgsAdamDevTensor* tensors_dev, const float* factors_dev, int64_t longest,
                        void* stream) {
    if (n_tensors < 0 || n_tensors > 65535 || (n_tensors > 0 && (!tensors_dev || !factors_dev))) {
        set_error("mobgs_adam_dev_step: n_tensors = %d (0..65535) or a NULL pointer", n_tensors);
        return MOBGS_E_INVALID;
    }
    const int64_t blocks = longest < 0 ? -1 : (longest + 1023) / 1024;
    if (blocks < 0 || blocks > 0x7fffffffLL) {
        set_error("mobgs_adam_dev_step: longest = %lld", (long long)longest);
        return MOBGS_E_INVALID;
    }
    if (n_tensors == 0 || blocks == 0) return MOBGS_OK;
    hipLaunchKernelGGL(adam_dev_step_kernel, dim3((unsigned)blocks, (unsigned)n_tensors), dim3(256), 0, (hipStream_t)stream,
                       tensors_dev, factors_dev);
    return check_launch("adam_dev_step_kernel");
}

}  // extern "C"

// K33: probes of the cross-lane primitives (wave_shared.h) and the fixed-order sums (reduce_shared.h), one per function and
// instantiation the kernel files use (tests/test_gpu_lane_primitives.py against the model in tests/lane_model.py).
// gfx950 only.  Test support, not part of the drop-in surface.
//
// Every kernel here is thin: a thread loads its KI values, calls ONE header function and stores the KO values it holds
// afterwards.  No arithmetic of its own and no cross-lane step of its own: what the output shows is the header's doing.
//
// Layout.  A group is one full wave (64 threads), for the block sums one workgroup of PROBE_BLOCK threads; one launch runs
// n_groups independent groups, one per workgroup.  Thread t of group g reads in[(g T + t) KI + i] and writes
// out[(g T + t) KO + j], T the group's thread count.  The two row sums read arrays instead: group g of ROWS_SUM reads
// n stride doubles at in + (2 g) n stride for its first call and at in + (2 g + 1) n stride for the second, group g of
// WAVE_ROWS_SUM n stride doubles at in + g n stride.  Every wave launched is full and every thread makes every call.
#include "reduce_shared.h"

namespace mobgs {

constexpr int PROBE_BLOCK = 256;   // REG_BLOCK, POSE_BLOCK, GR_BLOCK, MET_BLOCK, TOF_BLOCK: the one size in use
constexpr int PROBE_WAVES = PROBE_BLOCK / MOBGS_WAVE;

// ---- one wave per group: x[KI] -> y[KO] ----------------------------------------------------------------------------------
struct ProbeWaveSum {
    template <class T> static __device__ __forceinline__ void run(const T (&x)[1], T (&y)[1]) { y[0] = wave_sum(x[0]); }
};
struct ProbeWaveMin {
    template <class T> static __device__ __forceinline__ void run(const T (&x)[1], T (&y)[1]) { y[0] = wave_min(x[0]); }
};
struct ProbeWaveMax {
    template <class T> static __device__ __forceinline__ void run(const T (&x)[1], T (&y)[1]) { y[0] = wave_max(x[0]); }
};
struct ProbeFoldMax {
    template <class T> static __device__ __forceinline__ void run(const T (&x)[1], T (&y)[1]) {
        T v = x[0];
        MOBGS_WAVE_FOLD(v, max);
        y[0] = v;
    }
};
struct ProbeFoldAdd {
    template <class T> static __device__ __forceinline__ void run(const T (&x)[1], T (&y)[1]) {
        T v = x[0];
        MOBGS_WAVE_FOLD(v, MOBGS_WAVE_ADD);
        y[0] = v;
    }
};
template <int CTRL>
struct ProbeDppMov {
    static __device__ __forceinline__ void run(const uint32_t (&x)[1], uint32_t (&y)[1]) { y[0] = dpp_mov<CTRL>(x[0]); }
};
struct ProbeDppMovXor4 {   // isect.hip's lane ^ 4
    static __device__ __forceinline__ void run(const uint32_t (&x)[1], uint32_t (&y)[1]) {
        y[0] = dpp_mov<0x1B>(dpp_mov<0x141>(x[0]));
    }
};
template <int CTRL>
struct ProbeDppAdd {
    static __device__ __forceinline__ void run(const float (&x)[1], float (&y)[1]) { y[0] = dpp_add<CTRL>(x[0]); }
};
struct ProbeDppAddXor4 {
    static __device__ __forceinline__ void run(const float (&x)[1], float (&y)[1]) { y[0] = dpp_add_xor4(x[0]); }
};
struct ProbeRowAllreduce {
    static __device__ __forceinline__ void run(const float (&x)[1], float (&y)[1]) { y[0] = row_allreduce(x[0]); }
};
struct ProbeHalfWaveSum {
    static __device__ __forceinline__ void run(const float (&x)[1], float (&y)[1]) { y[0] = half_wave_sum(x[0]); }
};
struct ProbeWaveAllreduce {
    static __device__ __forceinline__ void run(const float (&x)[1], float (&y)[1]) { y[0] = wave_allreduce(x[0]); }
};
template <int NVP>
struct ProbeComponents {   // the NVP / 4 registers the header documents
    static __device__ __forceinline__ void run(const float (&x)[NVP], float (&y)[NVP / 4]) {
        float v[NVP];
#pragma unroll
        for (int i = 0; i < NVP; ++i) v[i] = x[i];
        wave_reduce_components<NVP>(v);
#pragma unroll
        for (int i = 0; i < NVP / 4; ++i) y[i] = v[i];
    }
};
struct ProbePair {
    static __device__ __forceinline__ void run(const float (&x)[2], float (&y)[1]) { y[0] = wave_reduce_pair(x[0], x[1]); }
};
// the fence through its purpose: a value another lane wrote before the fence is the value read after it, twice in a row
struct ProbeFence {
    static __device__ __forceinline__ void run(const uint32_t (&x)[1], uint32_t (&y)[2]) {
        __shared__ uint32_t slot[MOBGS_WAVE];
        const int l = threadIdx.x;
        slot[l] = x[0];
        wave_lds_fence();
        const uint32_t first = slot[MOBGS_WAVE - 1 - l];
        slot[(l + 17) & (MOBGS_WAVE - 1)] = first;
        wave_lds_fence();
        y[0] = first;
        y[1] = slot[l];
    }
};

template <class T, int KI, int KO, class F>
__global__ void __launch_bounds__(MOBGS_WAVE) wave_probe_kernel(const T* __restrict__ in, T* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * MOBGS_WAVE + threadIdx.x;
    T x[KI], y[KO];
#pragma unroll
    for (int i = 0; i < KI; ++i) x[i] = in[t * KI + i];
    F::run(x, y);
#pragma unroll
    for (int j = 0; j < KO; ++j) out[t * KO + j] = y[j];
}

// ---- one workgroup per group: every block sum twice in a row on the same LDS array --------------------------------------
__global__ void __launch_bounds__(PROBE_BLOCK) block_sum_probe_kernel(const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double s_wave[PROBE_WAVES];
    const size_t t = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    const double a = block_sum<PROBE_WAVES>(in[2 * t], s_wave);
    const double b = block_sum<PROBE_WAVES>(in[2 * t + 1], s_wave);
    out[2 * t] = a;
    out[2 * t + 1] = b;
}

__global__ void __launch_bounds__(PROBE_BLOCK) block_sum4_probe_kernel(const float* __restrict__ in, float* __restrict__ out) {
    __shared__ float sm[4];
    const size_t t = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    const float a = block_sum4(in[2 * t], sm);
    const float b = block_sum4(in[2 * t + 1], sm);
    out[2 * t] = a;
    out[2 * t + 1] = b;
}

__global__ void __launch_bounds__(PROBE_BLOCK)
rows_sum_probe_kernel(int n, int stride, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double s_wave[PROBE_WAVES];
    const size_t t = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x, span = (size_t)n * stride;
    const double* p = in + 2 * (size_t)blockIdx.x * span;
    const double a = rows_sum<PROBE_BLOCK>(p, n, stride, s_wave);
    const double b = rows_sum<PROBE_BLOCK>(p + span, n, stride, s_wave);
    out[2 * t] = a;
    out[2 * t + 1] = b;
}

__global__ void __launch_bounds__(MOBGS_WAVE)
wave_rows_sum_probe_kernel(int n, int stride, const double* __restrict__ in, double* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * MOBGS_WAVE + threadIdx.x;
    out[t] = wave_rows_sum(in + (size_t)blockIdx.x * n * stride, n, stride, (int)threadIdx.x);
}

template <class T, int KI, int KO, class F>
static void launch_wave_probe(int n_groups, const void* in, void* out, hipStream_t stream) {
    hipLaunchKernelGGL((wave_probe_kernel<T, KI, KO, F>), dim3((unsigned)n_groups), dim3(MOBGS_WAVE), 0, stream,
                       static_cast<const T*>(in), static_cast<T*>(out));
}

// bytes of one element of the op's arrays, 0 for an unknown op
static int probe_element_bytes(int op) {
    if (op < 0 || op >= MOBGS_LANE_OPS) return 0;
    return op == MOBGS_LANE_WAVE_SUM_F64 || op == MOBGS_LANE_BLOCK_SUM || op == MOBGS_LANE_ROWS_SUM ||
                   op == MOBGS_LANE_WAVE_ROWS_SUM
               ? 8
               : 4;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_lane_probe(int op, int n_groups, int n, int stride, const void* in, void* out, void* stream) {
    const int bytes = probe_element_bytes(op);
    if (bytes == 0) {
        set_error("mobgs_lane_probe: unknown op=%d (0 .. %d)", op, MOBGS_LANE_OPS - 1);
        return MOBGS_E_INVALID;
    }
    if (!in || !out || n_groups < 1 || n < 0 || stride < 1) {
        set_error("mobgs_lane_probe: bad arguments n_groups=%d (>= 1) n=%d (>= 0) stride=%d (>= 1), or a NULL pointer",
                  n_groups, n, stride);
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(bytes - 1)) {
        set_error("mobgs_lane_probe: in and out must be %d-byte aligned for op=%d", bytes, op);
        return MOBGS_E_INVALID;
    }
    if ((op == MOBGS_LANE_ROWS_SUM || op == MOBGS_LANE_WAVE_ROWS_SUM) &&
        (int64_t)n * stride > ((int64_t)1 << 40) / n_groups) {
        set_error("mobgs_lane_probe: n_groups=%d arrays of n=%d stride=%d overflow", n_groups, n, stride);
        return MOBGS_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)n_groups);
    switch (op) {
        case MOBGS_LANE_WAVE_SUM_F32: launch_wave_probe<float, 1, 1, ProbeWaveSum>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_SUM_I32: launch_wave_probe<int, 1, 1, ProbeWaveSum>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_SUM_F64: launch_wave_probe<double, 1, 1, ProbeWaveSum>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_MIN_F32: launch_wave_probe<float, 1, 1, ProbeWaveMin>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_MIN_I32: launch_wave_probe<int, 1, 1, ProbeWaveMin>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_MAX_F32: launch_wave_probe<float, 1, 1, ProbeWaveMax>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_MAX_I32: launch_wave_probe<int, 1, 1, ProbeWaveMax>(n_groups, in, out, s); break;
        case MOBGS_LANE_FOLD_MAX_I32: launch_wave_probe<int, 1, 1, ProbeFoldMax>(n_groups, in, out, s); break;
        case MOBGS_LANE_FOLD_ADD_I32: launch_wave_probe<int, 1, 1, ProbeFoldAdd>(n_groups, in, out, s); break;
        case MOBGS_LANE_FOLD_ADD_F32: launch_wave_probe<float, 1, 1, ProbeFoldAdd>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_MOV_XOR1: launch_wave_probe<uint32_t, 1, 1, ProbeDppMov<0xB1>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_MOV_XOR2: launch_wave_probe<uint32_t, 1, 1, ProbeDppMov<0x4E>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_MOV_QUAD_REVERSE: launch_wave_probe<uint32_t, 1, 1, ProbeDppMov<0x1B>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_MOV_HALF_MIRROR: launch_wave_probe<uint32_t, 1, 1, ProbeDppMov<0x141>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_MOV_ROR8: launch_wave_probe<uint32_t, 1, 1, ProbeDppMov<0x128>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_MOV_XOR4: launch_wave_probe<uint32_t, 1, 1, ProbeDppMovXor4>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_ADD_XOR1: launch_wave_probe<float, 1, 1, ProbeDppAdd<0xB1>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_ADD_XOR2: launch_wave_probe<float, 1, 1, ProbeDppAdd<0x4E>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_ADD_HALF_MIRROR: launch_wave_probe<float, 1, 1, ProbeDppAdd<0x141>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_ADD_ROR8: launch_wave_probe<float, 1, 1, ProbeDppAdd<0x128>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_ADD_ROR4: launch_wave_probe<float, 1, 1, ProbeDppAdd<0x124>>(n_groups, in, out, s); break;
        case MOBGS_LANE_DPP_ADD_XOR4: launch_wave_probe<float, 1, 1, ProbeDppAddXor4>(n_groups, in, out, s); break;
        case MOBGS_LANE_ROW_ALLREDUCE: launch_wave_probe<float, 1, 1, ProbeRowAllreduce>(n_groups, in, out, s); break;
        case MOBGS_LANE_HALF_WAVE_SUM: launch_wave_probe<float, 1, 1, ProbeHalfWaveSum>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_ALLREDUCE: launch_wave_probe<float, 1, 1, ProbeWaveAllreduce>(n_groups, in, out, s); break;
        case MOBGS_LANE_REDUCE_COMPONENTS_8: launch_wave_probe<float, 8, 2, ProbeComponents<8>>(n_groups, in, out, s); break;
        case MOBGS_LANE_REDUCE_COMPONENTS_16: launch_wave_probe<float, 16, 4, ProbeComponents<16>>(n_groups, in, out, s); break;
        case MOBGS_LANE_REDUCE_COMPONENTS_32: launch_wave_probe<float, 32, 8, ProbeComponents<32>>(n_groups, in, out, s); break;
        case MOBGS_LANE_REDUCE_COMPONENTS_64: launch_wave_probe<float, 64, 16, ProbeComponents<64>>(n_groups, in, out, s); break;
        case MOBGS_LANE_REDUCE_PAIR: launch_wave_probe<float, 2, 1, ProbePair>(n_groups, in, out, s); break;
        case MOBGS_LANE_WAVE_FENCE: launch_wave_probe<uint32_t, 1, 2, ProbeFence>(n_groups, in, out, s); break;
        case MOBGS_LANE_BLOCK_SUM:
            hipLaunchKernelGGL(block_sum_probe_kernel, grid, dim3(PROBE_BLOCK), 0, s, static_cast<const double*>(in),
                               static_cast<double*>(out));
            break;
        case MOBGS_LANE_ROWS_SUM:
            hipLaunchKernelGGL(rows_sum_probe_kernel, grid, dim3(PROBE_BLOCK), 0, s, n, stride,
                               static_cast<const double*>(in), static_cast<double*>(out));
            break;
        case MOBGS_LANE_WAVE_ROWS_SUM:
            hipLaunchKernelGGL(wave_rows_sum_probe_kernel, grid, dim3(MOBGS_WAVE), 0, s, n, stride,
                               static_cast<const double*>(in), static_cast<double*>(out));
            break;
        default:   // MOBGS_LANE_BLOCK_SUM4
            hipLaunchKernelGGL(block_sum4_probe_kernel, grid, dim3(PROBE_BLOCK), 0, s, static_cast<const float*>(in),
                               static_cast<float*>(out));
            break;
    }
    return check_launch("mobgs_lane_probe");
}

}  // extern "C"

// K24: LPIPS (net-lin, AlexNet trunk, version 0.1, spatial average) of a batch of image pairs (include/mobgs_hip.h): the
// reference's models/networks_basic.py:68-105 over models/pretrained_networks.py:57-95.  Forward, and the gradient with respect to the images.  gfx950 only.
//
//   lpips_conv_kernel<FIRST>   a convolution + bias + ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32: M = the output
//                              pixels of all 2B images, N = Cout, K = Cin k k.  One workgroup (4 waves) owns a 128 x 64 tile
//                              of the output and walks K in steps of 32: the 128 x 32 patch slab and the 32 x 64 weight
//                              slab go to LDS, each wave holds two 32 x 32 accumulators (64 rows x 32 columns).  Activations
//                              are channel-last and Cin is a multiple of 32 from layer 2 on, so a K step lies inside one
//                              (ky, kx) tap and a pixel's part of the slab is 128 contiguous bytes, or zeros in the padding.
//                              FIRST: the slab is gathered from the caller's [B,3,H,W] images, with the clamp, the 8-bit
//                              truncation, 2 x - 1 and the scaling layer applied on load; K = 363 is padded to 384 with
//                              zero weight rows, there is no tail path.
//   lpips_pool_kernel          maxpool(3, stride 2, floor), a kernel of its own, channel-last, four channels per thread.
//   lpips_dist_kernel          one wave per pixel of a pair: both feature vectors are read once (<= 6 values per lane and
//                              image), the two norms, the normalised squared difference and the head dot product are fp32,
//                              reduced over the wave by a butterfly (every lane ends with the same bits); the wave adds
//                              its 16 pixels in float64, the workgroup its 4 waves, into ONE float64 partial sum.
//   lpips_finish_kernel        one workgroup, one wave per pair: per layer the lanes add contiguous runs of the partial sums
//                              and a butterfly adds the lane sums (float64, an order that depends on the tap's size
//                              alone), divides by the tap's pixels, adds the five layer values.
//
// The spatial and masked forms (mobgs_lpips_alex_spatial: networks_basic.py:16-28, :79-82, dycheck_metrics.py:203-244):
//   lpips_dist_kernel<true>    the same kernel; a pixel's d is also stored into a small map [B, sum h_l w_l].
//   lpips_mask_sum_kernel      one launch for the five taps: d m_l (fp32 product) and m_l, m_l = the mask's nearest
//                              neighbour, added in float64 per 64 pixels in the distance kernel's order.
//   lpips_upsample_kernel      per output pixel the bilinear value (align_corners = False) of each of the five d maps, their
//                              fp32 sum in layer order, an optional store, float64 sums of map m, m and map: thread,
//                              wave butterfly, workgroup, one partial row per 1024 pixels of a pair.
//   lpips_spatial_finish_kernel  one workgroup, one wave per pair: the sums in lpips_finish_kernel's order, the row.
//
// The backward pass (mobgs_lpips_alex_bwd: the gradient of the total with respect to the images, LPIPS as a loss):
//   lpips_dist_bwd_kernel      the distance head's gradient per tap, one wave per pixel of a wanted image.
//   lpips_conv_kernel<LP_BWD_TAP / LP_BWD_POOL>  the backward-data pass of layers 5 .. 2: the same GEMM body over the
//                              flipped, channel-exchanged weight; the epilogue adds the tap's distance gradient and masks.
//   lpips_pool_bwd_kernel      max-pool backward as a gather (first maximum in row-major order on ties).
//   lpips_first_bwd_kernel     layer 1 into [B,3,H,W], with the scaling layer, 2 x - 1 and the clamp.
//
// Every output of a convolution is one k-ordered fmaf chain (the fp32 MFMA adds nothing wider), the same chain whatever tile
// or row of a tile the pixel falls into; the workgroups of the distance kernel are cut per pair.  No float atomic, no
// hand-off between workgroups inside a launch.  So a pair's result is bit-identical from run to run, whatever the batch
// around it; and with equal images both feature vectors, norms and normalised values are equal and every difference is 0.
#include "reduce_shared.h"

namespace mobgs {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LP_LAYERS = 5;
constexpr int LP_BM = 128, LP_BN = 64, LP_BK = 32, LP_THREADS = 256;
constexpr int LP_APITCH = LP_BK + 1;         // sA[m][k]: the 32 lanes of a fragment read 32 rows -> 32 banks
constexpr int LP_FINISH_THREADS = 1024;
constexpr int LP_DPIX = 64;                  // pixels per workgroup of the distance kernel (16 per wave)
constexpr int LP_MAX_B = 4096, LP_MAX_EDGE = 16384, LP_MIN_EDGE = 31;
constexpr long long LP_MAX_M = 1ll << 30;
constexpr int LP_K1 = 363;
static_assert(MOBGS_LPIPS_COLUMNS == LP_LAYERS + 1, "out columns of include/mobgs_hip.h");
constexpr int LP_UPIX = 4;                   // output pixels per thread of the upsample kernel
constexpr int LP_UP_BLOCK = LP_THREADS * LP_UPIX;
static_assert(MOBGS_LPIPS_SPATIAL_COLUMNS == 6 + 3 * LP_LAYERS, "out columns of the spatial call");
static_assert(LP_THREADS / MOBGS_WAVE == 4, "the workgroups add four wave sums");

static const int LP_CIN[LP_LAYERS] = {3, 64, 192, 384, 256};
static const int LP_COUT[LP_LAYERS] = {64, 192, 384, 256, 256};
static const int LP_KS[LP_LAYERS] = {11, 5, 3, 3, 3};
static const int LP_STRIDE[LP_LAYERS] = {4, 1, 1, 1, 1};
static const int LP_PAD[LP_LAYERS] = {2, 2, 1, 1, 1};

struct LpConvArgs {
    const float* in;                 // [N, Hi, Wi, Cin] channel-last (layers 2 .. 5)
    const float *img0, *img1;        // [B,3,Hi,Wi] (layer 1)
    const float *w, *bias;           // [Kpad, Cout], [Cout]
    float* out;                      // [N, Ho, Wo, Cout]
    int N, Hi, Wi, Cin, Ho, Wo, Cout, ks, stride, pad, Kpad, M, flags;
    // the backward-data arms: `in` and `out` hold the wanted images alone, image q of them is image q n_stride + n_off of tap
    const float* tap;                // [2B, Ho, Wo, Cout]: the forward's ReLU map at the output (LP_BWD_TAP)
    int n_stride, n_off;
};

// the arms of lpips_conv_kernel: what is staged and what the epilogue does.  The K loop is one text for all of them.
constexpr int LP_FIRST = 0;          // layer 1: the slab is gathered from the images; bias + ReLU
constexpr int LP_FWD = 1;            // layers 2 .. 5: bias + ReLU
constexpr int LP_BWD_TAP = 2;        // backward-data onto a tap: out already holds the tap's distance gradient; add, mask
constexpr int LP_BWD_POOL = 3;       // backward-data onto a pooled map: a plain store

// the value the first convolution sees at (image n = 2 b + s, channel c, y, x): inside the image only
__device__ __forceinline__ float lp_input(const LpConvArgs& a, int n, int c, int y, int x) {
    const int s = n & 1;
    const float* img = s ? a.img1 : a.img0;
    float v = img[(((size_t)(n >> 1) * 3 + c) * a.Hi + y) * a.Wi + x];
    if (a.flags & MOBGS_LPIPS_CLAMP) v = clamp01(v);
    if ((a.flags & MOBGS_LPIPS_QUANTIZE) && s) v = quantize8(v);
    if (a.flags & MOBGS_LPIPS_UNIT_RANGE) v = 2.f * v - 1.f;
    const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    return (v - shift) / scale;
}

template <int MODE>
__global__ void __launch_bounds__(LP_THREADS) lpips_conv_kernel(LpConvArgs a) {
    constexpr bool FIRST = MODE == LP_FIRST;
    __shared__ float sA[LP_BM * LP_APITCH];
    __shared__ __attribute__((aligned(16))) float sB[LP_BK * LP_BN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_tiles = a.Cout / LP_BN;
    const int m0 = (int)(blockIdx.x / n_tiles) * LP_BM, n0 = (int)(blockIdx.x % n_tiles) * LP_BN;
    // the slab rows this thread stages: r = (t >> 3) + 32 j, four consecutive k at 4 (t & 7)
    const int kq = (t & 7) * 4;
    int img_n[4], iy0[4], ix0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + (t >> 3) + 32 * j;
        const bool row = m < a.M;                        // a row past M: zeros, never stored
        const int mm = row ? m : 0, q = mm / a.Wo;
        img_n[j] = row ? q / a.Ho : -1;
        iy0[j] = (q % a.Ho) * a.stride - a.pad;
        ix0[j] = (mm % a.Wo) * a.stride - a.pad;
    }
    lp_f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][i] = acc[1][i] = 0.f;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 32;

    for (int k0 = 0; k0 < a.Kpad; k0 += LP_BK) {
        // ---- stage the slabs (registers first, so the loads are in flight together) ----
        float4 va[4];
        if (FIRST) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float e[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + kq + i;
                    const int c = k / 121, r = k - c * 121, ky = r / 11, kx = r - ky * 11;
                    const int y = iy0[j] + ky, x = ix0[j] + kx;
                    const bool in = img_n[j] >= 0 && k < LP_K1 && y >= 0 && y < a.Hi && x >= 0 && x < a.Wi;
                    e[i] = in ? lp_input(a, img_n[j], c, y, x) : 0.f;
                }
                va[j] = make_float4(e[0], e[1], e[2], e[3]);
            }
        } else {
            const int tap = k0 / a.Cin, c0 = k0 - tap * a.Cin, ky = tap / a.ks, kx = tap - ky * a.ks;   // (uniform)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = iy0[j] + ky, x = ix0[j] + kx;
                const bool in = img_n[j] >= 0 && y >= 0 && y < a.Hi && x >= 0 && x < a.Wi;
                va[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in)
                    va[j] = *reinterpret_cast<const float4*>(a.in + (((size_t)img_n[j] * a.Hi + y) * a.Wi + x) * a.Cin +
                                                             c0 + kq);
            }
        }
        const float* pw = a.w + (size_t)(k0 + (t >> 4)) * a.Cout + n0 + (t & 15) * 4;
        const float4 vb0 = *reinterpret_cast<const float4*>(pw);
        const float4 vb1 = *reinterpret_cast<const float4*>(pw + (size_t)16 * a.Cout);
        __syncthreads();                                 // the previous step has read sA, sB
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float* p = sA + ((t >> 3) + 32 * j) * LP_APITCH + kq;
            p[0] = va[j].x;
            p[1] = va[j].y;
            p[2] = va[j].z;
            p[3] = va[j].w;
        }
        *reinterpret_cast<float4*>(sB + (t >> 4) * LP_BN + (t & 15) * 4) = vb0;
        *reinterpret_cast<float4*>(sB + ((t >> 4) + 16) * LP_BN + (t & 15) * 4) = vb1;
        __syncthreads();
        // ---- 16 k-steps of 2: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31] ----
        const float* pa = sA + (wm + (lane & 31)) * LP_APITCH + (lane >> 5);
        const float* pb = sB + (lane >> 5) * LP_BN + wn + (lane & 31);
#pragma unroll
        for (int s = 0; s < LP_BK / 2; ++s) {
            const float b = pb[2 * s * LP_BN];
            const float a0 = pa[2 * s], a1 = pa[32 * LP_APITCH + 2 * s];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
        }
    }
    // ---- bias + ReLU; accumulator register i of lane l is row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31 ----
    // the backward arms: out = the tap's distance gradient + the sum, where the tap is positive (LP_BWD_TAP); the sum (LP_BWD_POOL)
    const int col = n0 + wn + (lane & 31);
    const float bias = MODE <= LP_FWD ? a.bias[col] : 0.f;
    const int P = a.Ho * a.Wo;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + wm + 32 * h + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            if (m < a.M) {
                if (MODE <= LP_FWD) {
                    const float v = acc[h][i] + bias;
                    a.out[(size_t)m * a.Cout + col] = v > 0.f ? v : 0.f;
                } else if (MODE == LP_BWD_TAP) {
                    const int q = m / P;
                    const float f = a.tap[((size_t)(q * a.n_stride + a.n_off) * P + (m - q * P)) * a.Cout + col];
                    float* o = a.out + (size_t)m * a.Cout + col;
                    const float v = *o + acc[h][i];
                    *o = f > 0.f ? v : 0.f;
                } else {
                    a.out[(size_t)m * a.Cout + col] = acc[h][i];
                }
            }
        }
    }
}

// in [N, Hi, Wi, C] -> out [N, Ho, Wo, C], Ho = (Hi - 3) / 2 + 1: every window lies inside the input
__global__ void __launch_bounds__(LP_THREADS) lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                int Hi, int Wi, int Ho, int Wo, int C4, size_t total) {
    const size_t idx = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C4);
    size_t q = idx / C4;
    const int ox = (int)(q % Wo);
    q /= Wo;
    const int oy = (int)(q % Ho);
    const size_t n = q / Ho;
    const float4* p = reinterpret_cast<const float4*>(in) + ((n * Hi + 2 * oy) * Wi + 2 * ox) * C4 + c;
    float4 m = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = p[((size_t)dy * Wi + dx) * C4];
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    }
    reinterpret_cast<float4*>(out)[idx] = m;
}

// the MAP arm of the distance kernel (mobgs_lpips_alex_spatial): where a pixel's d goes
struct LpMapArgs {
    float* dmap;                     // [B, p_total]: this tap's d at p_off + p
    int p_total, p_off;
};

// feat [2B, P, C] (P pixels per image), lin [C]; grid (rows, B); partial[b * rows_total + row_off + blockIdx.x].
// MAP: the same statements, and the wave also stores the pixel's d -- every lane, without a branch.  Nothing else differs,
// on purpose: which products the compiler fuses or pairs in the loop depends on what surrounds them (a store under
// `lane == 0` splits the block, and the packed multiplications of the plain arm become fused ones: d moves by an ulp), and
// both arms must form the same fp32 d.  The two arms' floating-point instruction sequences were compared after the build;
// tests/test_gpu_lpips_spatial.py holds the values together (numerators of an all-ones mask against the plain call).
template <bool MAP>
__global__ void __launch_bounds__(LP_THREADS) lpips_dist_kernel(const float* __restrict__ feat,
                                                                const float* __restrict__ lin, int P, int C,
                                                                int rows_total, int row_off,
                                                                double* __restrict__ partial, LpMapArgs ma) {
    __shared__ double s_wave[LP_THREADS / MOBGS_WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t pair = blockIdx.y;
    const float* f0 = feat + (2 * pair) * (size_t)P * C;
    const float* f1 = f0 + (size_t)P * C;
    const int nj = C / MOBGS_WAVE;                       // 1, 3, 6, 4, 4
    float w[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) w[j] = j < nj ? lin[lane + MOBGS_WAVE * j] : 0.f;
    double sum = 0.0;
    for (int i = 0; i < LP_DPIX / 4; ++i) {
        const int p = blockIdx.x * LP_DPIX + 4 * i + wave;
        if (p >= P) break;                               // (uniform over the wave)
        float u[6], v[6], su = 0.f, sv = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            u[j] = j < nj ? f0[(size_t)p * C + lane + MOBGS_WAVE * j] : 0.f;
            v[j] = j < nj ? f1[(size_t)p * C + lane + MOBGS_WAVE * j] : 0.f;
            su += u[j] * u[j];
            sv += v[j] * v[j];
        }
        const float du = sqrtf(wave_sum(su)) + 1e-10f, dv = sqrtf(wave_sum(sv)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float e = u[j] / du - v[j] / dv;
            d += w[j] * (e * e);
        }
        const float dp = wave_sum(d);
        if (MAP) ma.dmap[pair * ma.p_total + ma.p_off + p] = dp;       // (every lane holds the same bits: one address, one value)
        sum += (double)dp;
    }
    if (lane == 0) s_wave[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[pair * rows_total + row_off + blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// the masked sums of the five d maps (the reference's spatial_average with a mask), one launch for all taps
struct LpMaskSumArgs {
    const float* dmap;               // [B, p_total]
    const float* mask;               // [B, H, W], or nullptr = all ones
    double* partial;                 // [B, rows_total, 2]: sum d m_l, sum m_l over 64 pixels of a tap
    int H, W, p_total, rows_total;
    int P[LP_LAYERS], w[LP_LAYERS], p_off[LP_LAYERS], row_off[LP_LAYERS];
    float sH[LP_LAYERS], sW[LP_LAYERS];      // (float)H / (float)h, (float)W / (float)w
};

// grid (rows_total, B), one wave: the workgroup owns the 64 pixels the distance kernel's workgroup of that row owns, a lane
// one pixel.  m_l = the mask's nearest neighbour of the pixel; d m_l is an fp32 product.  The sums are float64 in the
// distance kernel's order -- pixels q, q + 4, q + 8, ... for q = 0 .. 3, then ((s0 + s1) + s2) + s3 --, so that with a mask
// of ones the numerator has the bits of the plain call's sum.
__global__ void __launch_bounds__(MOBGS_WAVE) lpips_mask_sum_kernel(LpMaskSumArgs a) {
    __shared__ float s_dm[LP_DPIX], s_m[LP_DPIX];
    __shared__ double s_q[8];
    const int t = threadIdx.x, row = blockIdx.x;
    const size_t pair = blockIdx.y;
    int l = 0;
#pragma unroll
    for (int k = 1; k < LP_LAYERS; ++k) l += row >= a.row_off[k] ? 1 : 0;
    const int p = (row - a.row_off[l]) * LP_DPIX + t;
    float dm = 0.f, m = 0.f;
    if (p < a.P[l]) {
        m = 1.f;
        if (a.mask) {
            const int ty = p / a.w[l], tx = p - ty * a.w[l];
            const int iy = min((int)floorf((float)ty * a.sH[l]), a.H - 1), ix = min((int)floorf((float)tx * a.sW[l]), a.W - 1);
            m = a.mask[(pair * a.H + iy) * a.W + ix];
        }
        dm = a.dmap[pair * a.p_total + a.p_off[l] + p] * m;
    }
    s_dm[t] = dm;
    s_m[t] = m;
    __syncthreads();
    if (t < 8) {                                         // lanes 0 .. 3: d m_l of pixels t, t + 4, ...; lanes 4 .. 7: m_l
        const float* src = t < 4 ? s_dm : s_m;
        const int n = min(LP_DPIX, a.P[l] - (row - a.row_off[l]) * LP_DPIX);
        double s = 0.0;
        for (int q = t & 3; q < n; q += 4) s += (double)src[q];
        s_q[t] = s;
    }
    __syncthreads();
    if (t < 2) {
        const double* q = s_q + 4 * t;
        a.partial[(pair * a.rows_total + row) * 2 + t] = ((q[0] + q[1]) + q[2]) + q[3];
    }
}

struct LpFinishArgs {
    int B, rows_total;
    int rows[LP_LAYERS], row_off[LP_LAYERS];
    double pixels[LP_LAYERS];
};

// one workgroup of LP_FINISH_THREADS; wave v owns the pairs v, v + 16, ...: per layer its lanes add contiguous runs of the
// partial sums, a butterfly adds the 64 lane sums (a + b == b + a: every lane holds the same bits)
__global__ void __launch_bounds__(LP_FINISH_THREADS) lpips_finish_kernel(LpFinishArgs a, const double* __restrict__ partial,
                                                                         double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < a.B; b += LP_FINISH_THREADS / MOBGS_WAVE) {
        double total = 0.0;
        for (int l = 0; l < LP_LAYERS; ++l) {
            const double* p = partial + (size_t)b * a.rows_total + a.row_off[l];
            const double v = wave_rows_sum(p, a.rows[l], 1, lane) / a.pixels[l];
            if (lane == 0) out[(size_t)b * MOBGS_LPIPS_COLUMNS + 1 + l] = v;
            total += v;
        }
        if (lane == 0) out[(size_t)b * MOBGS_LPIPS_COLUMNS] = total;
    }
}

// ---- the spatial map: bilinear upsample of the five d maps, their fp32 sum, the float64 sums over the image -------------
struct LpUpArgs {
    const float* dmap;               // [B, p_total]: the five d maps of a pair, tap l at p_off[l]
    const float* mask;               // [B, H, W], or nullptr = all ones
    float* map;                      // [B, H, W], or nullptr
    double* partial;                 // [B, gridDim.x, 3]: sum map m, sum m, sum map of a workgroup's pixels
    int H, W, p_total;
    int h[LP_LAYERS], w[LP_LAYERS], p_off[LP_LAYERS];
    float sy[LP_LAYERS], sx[LP_LAYERS];      // (float)h / (float)H, (float)w / (float)W
};

// align_corners = False: the source coordinate of output index dst, its two neighbours and the weight of the second
__device__ __forceinline__ void lp_source(float s, int dst, int n, int& i0, int& i1, float& t) {
    const float src = fmaxf(fmaf(s, (float)dst + 0.5f, -0.5f), 0.f);
    i0 = min((int)src, n - 1);                           // (src < n - 1/2: the min never acts; it keeps the reads inside)
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    t = src - (float)i0;
}

// grid (blocks, B); a workgroup owns LP_UP_BLOCK consecutive pixels of a pair's H x W image, a thread the pixels t, t + 256,
// ... of them (coalesced mask reads and map stores).  The d maps are small (L2 / L1 hits).  A thread adds its pixels in
// float64 in that order, a butterfly adds the lanes (every lane ends with the same bits), thread 0 the four waves.
__global__ void __launch_bounds__(LP_THREADS) lpips_upsample_kernel(LpUpArgs a) {
    __shared__ double s_wave[3 * (LP_THREADS / MOBGS_WAVE)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t pair = blockIdx.y;
    const int HW = a.H * a.W;                            // <= 2^28
    const float* dm = a.dmap + pair * a.p_total;
    double s_mm = 0.0, s_m = 0.0, s_map = 0.0;
    for (int k = 0; k < LP_UPIX; ++k) {
        const long long idx = (long long)blockIdx.x * LP_UP_BLOCK + k * LP_THREADS + threadIdx.x;
        if (idx < HW) {
            const int y = (int)(idx / a.W), x = (int)(idx - (long long)y * a.W);
            int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
            float ty = 0.f, tx = 0.f, val = 0.f;
#pragma unroll
            for (int l = 0; l < LP_LAYERS; ++l) {
                if (l < 3) {                             // taps 3, 4 and 5 have one size
                    lp_source(a.sy[l], y, a.h[l], y0, y1, ty);
                    lp_source(a.sx[l], x, a.w[l], x0, x1, tx);
                }
                const float* q = dm + a.p_off[l];
                const float v00 = q[y0 * a.w[l] + x0], v01 = q[y0 * a.w[l] + x1];
                const float v10 = q[y1 * a.w[l] + x0], v11 = q[y1 * a.w[l] + x1];
                const float up = (1.f - ty) * ((1.f - tx) * v00 + tx * v01) + ty * ((1.f - tx) * v10 + tx * v11);
                val = l == 0 ? up : val + up;
            }
            const float m = a.mask ? a.mask[pair * HW + idx] : 1.f;
            if (a.map) a.map[pair * HW + idx] = val;
            s_mm += (double)val * (double)m;             // (exact product)
            s_m += (double)m;
            s_map += (double)val;
        }
    }
    s_mm = wave_sum(s_mm);
    s_m = wave_sum(s_m);
    s_map = wave_sum(s_map);
    if (lane == 0) {
        s_wave[3 * wave] = s_mm;
        s_wave[3 * wave + 1] = s_m;
        s_wave[3 * wave + 2] = s_map;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        a.partial[(pair * gridDim.x + blockIdx.x) * 3 + c] = ((s_wave[c] + s_wave[3 + c]) + s_wave[6 + c]) + s_wave[9 + c];
    }
}

struct LpSpatialFinishArgs {
    int B, rows_total, up_blocks;
    int rows[LP_LAYERS], row_off[LP_LAYERS];
    double pixels;                   // H W
};

// one workgroup of LP_FINISH_THREADS; wave v owns the pairs v, v + 16, ...; writes the row of include/mobgs_hip.h
__global__ void __launch_bounds__(LP_FINISH_THREADS) lpips_spatial_finish_kernel(LpSpatialFinishArgs a,
                                                                                 const double* __restrict__ dpart,
                                                                                 const double* __restrict__ upart,
                                                                                 double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < a.B; b += LP_FINISH_THREADS / MOBGS_WAVE) {
        double* o = out + (size_t)b * MOBGS_LPIPS_SPATIAL_COLUMNS;
        const double* u = upart + (size_t)b * a.up_blocks * 3;
        const double mm = wave_rows_sum(u, a.up_blocks, 3, lane), m = wave_rows_sum(u + 1, a.up_blocks, 3, lane);
        const double sm = wave_rows_sum(u + 2, a.up_blocks, 3, lane);
        double total = 0.0;
        for (int l = 0; l < LP_LAYERS; ++l) {
            const double* p = dpart + ((size_t)b * a.rows_total + a.row_off[l]) * 2;
            const double num = wave_rows_sum(p, a.rows[l], 2, lane), den = wave_rows_sum(p + 1, a.rows[l], 2, lane);
            const double v = num / (den + 1e-8);
            if (lane == 0) {
                o[6 + l] = v;
                o[11 + l] = num;
                o[16 + l] = den;
            }
            total += v;
        }
        if (lane == 0) {
            o[0] = sm / a.pixels;
            o[1] = mm / fmax(m, 1e-6);
            o[2] = mm;
            o[3] = m;
            o[4] = sm;
            o[5] = total;
        }
    }
}

// ---- the backward pass (mobgs_lpips_alex_bwd): the gradient of the total with respect to the images ---------------------
// Only the wanted images are walked: the gradient maps hold n = 1 or 2 images per pair, image q = n b + k of them being
// image q n_stride + n_off of the taps ((1, 0) with both sides wanted, (2, side) with one).

// One wave per pixel of a wanted image, in lpips_dist_kernel's layout.  x: the image's own vector, y: the other side's.
//   a = |x| + 1e-10, b = |y| + 1e-10, e = x / a - y / b, s = 2 w e, g = (s / a - x (sum s x) / (a^2 |x|)) v_total / P
// and g = 0 where x = 0 (the ReLU mask; it also removes s / a where |x| = 0, and the second term is defined as 0 there).
// With equal images e is x / a - x / a = +0 for either side, and every later value is +0.
// feat [2B, P, C]; grad [n B, P, C]; grid (ceil(P / 64), n B).
__global__ void __launch_bounds__(LP_THREADS) lpips_dist_bwd_kernel(const float* __restrict__ feat,
                                                                    const float* __restrict__ lin,
                                                                    const float* __restrict__ v_total, int P, int C,
                                                                    int n_stride, int n_off, float* __restrict__ grad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t q = blockIdx.y, n = q * n_stride + n_off;
    const float* fx = feat + n * (size_t)P * C;
    const float* fy = feat + (n ^ 1) * (size_t)P * C;
    float* g = grad + q * (size_t)P * C;
    const int nj = C / MOBGS_WAVE;                       // 1, 3, 6, 4, 4
    const float scale = v_total[n >> 1] / (float)P;
    float w[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) w[j] = j < nj ? lin[lane + MOBGS_WAVE * j] : 0.f;
    for (int i = 0; i < LP_DPIX / 4; ++i) {
        const int p = blockIdx.x * LP_DPIX + 4 * i + wave;
        if (p >= P) break;                               // (uniform over the wave)
        float x[6], y[6], sx = 0.f, sy = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            x[j] = j < nj ? fx[(size_t)p * C + lane + MOBGS_WAVE * j] : 0.f;
            y[j] = j < nj ? fy[(size_t)p * C + lane + MOBGS_WAVE * j] : 0.f;
            sx += x[j] * x[j];
            sy += y[j] * y[j];
        }
        const float nx = sqrtf(wave_sum(sx)), a = nx + 1e-10f, b = sqrtf(wave_sum(sy)) + 1e-10f;
        float s[6], dot = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            s[j] = 2.f * w[j] * (x[j] / a - y[j] / b);
            dot += s[j] * x[j];
        }
        dot = wave_sum(dot);
        const float k = nx > 0.f ? dot / (a * a * nx) : 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (j < nj) g[(size_t)p * C + lane + MOBGS_WAVE * j] = x[j] > 0.f ? (s[j] / a - x[j] * k) * scale : 0.f;
    }
}

// maxpool(3, 2) backward as a gather onto a tap.  tap [2B, Hi, Wi, C]; gp [nB, Ho, Wo, C]: the gradient of the pooled map;
// grad [nB, Hi, Wi, C]: holds the tap's distance gradient on entry, the tap's gradient on exit.  A position lies in at most
// 2 x 2 windows; it takes a window's gradient if it is the window's maximum, the FIRST one in row-major order on ties
// (v > best moves the choice, as torch's kernels do), recomputed from the tap.  The windows are added in (oy, ox) order; a
// row or column that no window covers keeps the distance gradient; then the ReLU mask.  Four channels per thread.
__global__ void __launch_bounds__(LP_THREADS) lpips_pool_bwd_kernel(const float* __restrict__ tap,
                                                                    const float* __restrict__ gp, float* __restrict__ grad,
                                                                    int Hi, int Wi, int Ho, int Wo, int C4, int n_stride,
                                                                    int n_off, size_t total) {
    const size_t idx = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C4);
    size_t r = idx / C4;
    const int x = (int)(r % Wi);
    r /= Wi;
    const int y = (int)(r % Hi);
    const size_t q = r / Hi, n = q * n_stride + n_off;
    const float4* t = reinterpret_cast<const float4*>(tap) + n * Hi * Wi * C4 + c;
    const float4* g = reinterpret_cast<const float4*>(gp) + q * Ho * Wo * C4 + c;
    const int here = y * Wi + x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int oy0 = max((y - 1) >> 1, 0), oy1 = min(y >> 1, Ho - 1);      // 2 oy <= y <= 2 oy + 2
    const int ox0 = max((x - 1) >> 1, 0), ox1 = min(x >> 1, Wo - 1);
    for (int oy = oy0; oy <= oy1; ++oy) {
        for (int ox = ox0; ox <= ox1; ++ox) {
            const int first = 2 * oy * Wi + 2 * ox;
            const float4 v0 = t[(size_t)first * C4];
            float best[4] = {v0.x, v0.y, v0.z, v0.w};
            int at[4] = {first, first, first, first};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int pos = first + dy * Wi + dx;
                    const float4 v4 = t[(size_t)pos * C4];
                    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (v[k] > best[k]) {
                            best[k] = v[k];
                            at[k] = pos;
                        }
                    }
                }
            }
            const float4 g4 = g[((size_t)oy * Wo + ox) * C4];
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (at[k] == here) acc[k] += gv[k];
        }
    }
    const float4 f = t[(size_t)here * C4];
    float4* o = reinterpret_cast<float4*>(grad) + idx;
    const float4 d = *o;
    float4 out;
    out.x = f.x > 0.f ? d.x + acc[0] : 0.f;
    out.y = f.y > 0.f ? d.y + acc[1] : 0.f;
    out.z = f.z > 0.f ? d.z + acc[2] : 0.f;
    out.w = f.w > 0.f ? d.w + acc[3] : 0.f;
    *o = out;
}

// The first layer's backward-data pass, a direct gather: one thread per pixel (y, x) of a wanted image, its three colour
// channels.  The outputs whose 11 x 11 window holds the pixel are oy with 4 oy - 2 <= y <= 4 oy + 8 (at most 3, ky = y + 2 -
// 4 oy), columns alike; per output 64 channels, read as float4 against the forward's packed weight (row (c 11 + ky) 11 + kx,
// 64 contiguous columns).  One fmaf chain per channel in (oy, ox, co) order.  Then the chain through the scaling layer
// (1 / scale_c), 2 x - 1 (MOBGS_LPIPS_UNIT_RANGE) and the clamp: the gradient passes where 0 <= v <= 1, bounds included, as
// torch.clamp does.  A pixel in no window gets +0.
// The threads of a workgroup share the pixel's place (py, px) in its 4 x 4 cell: ky = (py + 2) mod 4 + 4 i and kx are then
// uniform over the workgroup, so the weight reads are uniform (one row for all lanes) and a lane's own reads are its outputs'
// 64 channels.  (One thread per pixel in image order spent half the backward pass in this kernel at 1352 x 1014: four
// vector loads per four channels.)
// g1 [nB, h1, w1, 64]; img, gimg [B, 3, H, W]; grid (ceil(cells / 256), 16, B), cells = ceil(H / 4) ceil(W / 4).
__global__ void __launch_bounds__(LP_THREADS) lpips_first_bwd_kernel(const float* __restrict__ g1,
                                                                     const float* __restrict__ w1,
                                                                     const float* __restrict__ img, float* __restrict__ gimg,
                                                                     int H, int W, int h1, int w1n, int n_stride_q,
                                                                     int n_off_q, int flags) {
    const int cells_x = (W + 3) >> 2, cells_y = (H + 3) >> 2;
    const int cell = blockIdx.x * LP_THREADS + threadIdx.x;
    if (cell >= cells_x * cells_y) return;
    const int py = blockIdx.y >> 2, px = blockIdx.y & 3;                        // (uniform)
    const int cy = cell / cells_x, cx = cell - cy * cells_x;
    const int y = 4 * cy + py, x = 4 * cx + px;
    if (y >= H || x >= W) return;
    const size_t b = blockIdx.z, q = b * n_stride_q + n_off_q;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int iy = 2; iy >= 0; --iy) {                                            // ky falls, oy rises
        const int ky = ((py + 2) & 3) + 4 * iy;
        if (ky > 10) continue;
        const int oy = (y + 2 - ky) >> 2;                                        // (y + 2 - ky is a multiple of 4)
        for (int ix = 2; ix >= 0; --ix) {
            const int kx = ((px + 2) & 3) + 4 * ix;
            if (kx > 10) continue;
            const int ox = (x + 2 - kx) >> 2;
            if (oy < 0 || oy >= h1 || ox < 0 || ox >= w1n) continue;             // (per lane: the image's border)
            const float4* g = reinterpret_cast<const float4*>(g1 + ((q * h1 + oy) * w1n + ox) * 64);
            const float4* wr = reinterpret_cast<const float4*>(w1 + (size_t)(ky * 11 + kx) * 64);
#pragma unroll 4
            for (int c4 = 0; c4 < 16; ++c4) {
                const float4 gv = g[c4];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 wv = wr[c * (121 * 16) + c4];
                    acc[c] = fmaf(gv.x, wv.x, acc[c]);
                    acc[c] = fmaf(gv.y, wv.y, acc[c]);
                    acc[c] = fmaf(gv.z, wv.z, acc[c]);
                    acc[c] = fmaf(gv.w, wv.w, acc[c]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t at = ((b * 3 + c) * H + y) * W + x;
        const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
        float v = acc[c] / scale;
        if (flags & MOBGS_LPIPS_UNIT_RANGE) v = 2.f * v;
        if (flags & MOBGS_LPIPS_CLAMP) {
            const float p = img[at];
            v = (p >= 0.f && p <= 1.f) ? v : 0.f;
        }
        gimg[at] = v;
    }
}

// ---- host: sizes and the scratch layout ------------------------------------------------------------------------------
struct LpPlan {
    int h[LP_LAYERS], w[LP_LAYERS];      // the taps
    int ph[2], pw[2];                    // the two pooled maps
    int rows[LP_LAYERS], row_off[LP_LAYERS], rows_total;
    size_t region[2], off_region[2], off_partial, bytes;
};

static size_t lp_align(size_t x) { return (x + 255) & ~(size_t)255; }

static bool lp_plan(int B, int H, int W, LpPlan& p) {
    if (B < 1 || B > LP_MAX_B || H < LP_MIN_EDGE || W < LP_MIN_EDGE || H > LP_MAX_EDGE || W > LP_MAX_EDGE) return false;
    p.h[0] = (H - 7) / 4 + 1;
    p.w[0] = (W - 7) / 4 + 1;
    p.ph[0] = (p.h[0] - 3) / 2 + 1;
    p.pw[0] = (p.w[0] - 3) / 2 + 1;
    p.h[1] = p.ph[0];
    p.w[1] = p.pw[0];
    p.ph[1] = (p.h[1] - 3) / 2 + 1;
    p.pw[1] = (p.w[1] - 3) / 2 + 1;
    for (int l = 2; l < LP_LAYERS; ++l) {
        p.h[l] = p.ph[1];
        p.w[l] = p.pw[1];
    }
    if ((long long)2 * B * p.h[0] * p.w[0] > LP_MAX_M) return false;
    const size_t N = 2 * (size_t)B;
    size_t tap[LP_LAYERS], pool[2];
    p.rows_total = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        tap[l] = N * p.h[l] * p.w[l] * LP_COUT[l];
        p.rows[l] = (p.h[l] * p.w[l] + LP_DPIX - 1) / LP_DPIX;
        p.row_off[l] = p.rows_total;
        p.rows_total += p.rows[l];
    }
    for (int i = 0; i < 2; ++i) pool[i] = N * p.ph[i] * p.pw[i] * LP_COUT[i];
    // the layers alternate between two regions: tap 1 -> X, pool -> Y, tap 2 -> X, pool -> Y, tap 3 -> X, tap 4 -> Y, tap 5 -> X
    size_t x = tap[0], y = pool[0];
    x = tap[1] > x ? tap[1] : x;
    x = tap[2] > x ? tap[2] : x;
    x = tap[4] > x ? tap[4] : x;
    y = pool[1] > y ? pool[1] : y;
    y = tap[3] > y ? tap[3] : y;
    p.region[0] = x;
    p.region[1] = y;
    p.off_region[0] = 0;
    p.off_region[1] = lp_align(x * sizeof(float));
    p.off_partial = p.off_region[1] + lp_align(y * sizeof(float));
    p.bytes = p.off_partial + lp_align((size_t)B * p.rows_total * sizeof(double));
    return true;
}

// what mobgs_lpips_alex_spatial needs behind the plain call's scratch
struct LpSpatialPlan {
    int p_off[LP_LAYERS], p_total;       // the five d maps of a pair, floats
    int up_blocks;                       // workgroups of the upsample kernel per pair
    size_t off_dmap, off_dpart, off_upart, bytes;
};

static bool lp_spatial_plan(int B, int H, int W, LpPlan& p, LpSpatialPlan& q) {
    if (!lp_plan(B, H, W, p)) return false;
    q.p_total = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        q.p_off[l] = q.p_total;
        q.p_total += p.h[l] * p.w[l];
    }
    q.up_blocks = (int)(((long long)H * W + LP_UP_BLOCK - 1) / LP_UP_BLOCK);
    q.off_dmap = p.bytes;
    q.off_dpart = q.off_dmap + lp_align((size_t)B * q.p_total * sizeof(float));
    q.off_upart = q.off_dpart + lp_align((size_t)B * p.rows_total * 2 * sizeof(double));
    q.bytes = q.off_upart + lp_align((size_t)B * q.up_blocks * 3 * sizeof(double));
    return true;
}

// both entry points: the checks, the trunk with its distance kernels, the finish.  sp: the spatial call's plan or nullptr
static int lp_run(const char* name, const LpPlan& p, const LpSpatialPlan* sp, int B, int H, int W, const float* img0,
                  const float* img1, const MobgsLpipsWeights* weights, const float* mask, int flags, void* scratch,
                  size_t scratch_bytes, float* map, double* out, float* const* taps, void* stream) {
    const size_t need = sp ? sp->bytes : p.bytes;
    if (flags & ~(MOBGS_LPIPS_UNIT_RANGE | MOBGS_LPIPS_CLAMP | MOBGS_LPIPS_QUANTIZE)) {
        set_error("%s: flags = %d has unknown bits", name, flags);
        return MOBGS_E_INVALID;
    }
    if (!img0 || !img1 || !weights || !scratch || !out) {
        set_error("%s: NULL img0, img1, weights, scratch or out", name);
        return MOBGS_E_INVALID;
    }
    const float* w[LP_LAYERS] = {weights->w1, weights->w2, weights->w3, weights->w4, weights->w5};
    const float* bias[LP_LAYERS] = {weights->b1, weights->b2, weights->b3, weights->b4, weights->b5};
    const float* lin[LP_LAYERS] = {weights->lin1, weights->lin2, weights->lin3, weights->lin4, weights->lin5};
    for (int l = 0; l < LP_LAYERS; ++l) {
        if (!w[l] || !bias[l] || !lin[l] || (taps && !taps[l])) {
            set_error("%s: NULL weight, bias, head or tap pointer of layer %d", name, l + 1);
            return MOBGS_E_INVALID;
        }
        if (((uintptr_t)w[l] & 15) || ((uintptr_t)bias[l] & 3) || ((uintptr_t)lin[l] & 3) ||
            (taps && ((uintptr_t)taps[l] & 15))) {
            set_error("%s: layer %d: packed weights and taps must be 16-byte aligned, biases and heads 4-byte", name, l + 1);
            return MOBGS_E_INVALID;
        }
    }
    if (((uintptr_t)img0 & 3) || ((uintptr_t)img1 & 3) || ((uintptr_t)scratch & 255) || ((uintptr_t)out & 7)) {
        set_error("%s: images must be 4-byte aligned, scratch 256-byte aligned, out 8-byte aligned", name);
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)mask & 3) || ((uintptr_t)map & 3)) {
        set_error("%s: mask and map must be 4-byte aligned", name);
        return MOBGS_E_INVALID;
    }
    if (scratch_bytes < need) {
        set_error("%s: scratch_bytes = %zu, %s(%d, %d, %d) = %zu", name, scratch_bytes,
                  sp ? "mobgs_lpips_spatial_scratch_bytes" : "mobgs_lpips_scratch_bytes", B, H, W, need);
        return MOBGS_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    float* region[2] = {(float*)(base + p.off_region[0]), (float*)(base + p.off_region[1])};
    double* partial = (double*)(base + p.off_partial);
    float* dmap = sp ? (float*)(base + sp->off_dmap) : nullptr;
    double* dpart = sp ? (double*)(base + sp->off_dpart) : nullptr;
    double* upart = sp ? (double*)(base + sp->off_upart) : nullptr;
    const int N = 2 * B;
    static const int tap_region[LP_LAYERS] = {0, 0, 0, 1, 0};
    const float* cur = nullptr;                          // the input of the next convolution
    int cur_h = H, cur_w = W;
    for (int l = 0; l < LP_LAYERS; ++l) {
        float* tap = taps ? taps[l] : region[tap_region[l]];
        LpConvArgs a;
        a.in = cur;
        a.img0 = img0;
        a.img1 = img1;
        a.w = w[l];
        a.bias = bias[l];
        a.out = tap;
        a.N = N;
        a.Hi = cur_h;
        a.Wi = cur_w;
        a.Cin = LP_CIN[l];
        a.Ho = p.h[l];
        a.Wo = p.w[l];
        a.Cout = LP_COUT[l];
        a.ks = LP_KS[l];
        a.stride = LP_STRIDE[l];
        a.pad = LP_PAD[l];
        a.Kpad = mobgs_lpips_pack_k(l + 1);
        a.M = N * p.h[l] * p.w[l];
        a.flags = flags;
        const unsigned blocks = (unsigned)((a.M + LP_BM - 1) / LP_BM) * (unsigned)(a.Cout / LP_BN);
        if (l == 0)
            hipLaunchKernelGGL(lpips_conv_kernel<LP_FIRST>, dim3(blocks), dim3(LP_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL(lpips_conv_kernel<LP_FWD>, dim3(blocks), dim3(LP_THREADS), 0, s, a);
        const int P = p.h[l] * p.w[l];
        LpMapArgs ma = {};
        if (sp) {
            ma.dmap = dmap;
            ma.p_total = sp->p_total;
            ma.p_off = sp->p_off[l];
            hipLaunchKernelGGL(lpips_dist_kernel<true>, dim3((unsigned)p.rows[l], (unsigned)B), dim3(LP_THREADS), 0, s,
                               (const float*)tap, lin[l], P, a.Cout, p.rows_total, p.row_off[l], partial, ma);
        } else {
            hipLaunchKernelGGL(lpips_dist_kernel<false>, dim3((unsigned)p.rows[l], (unsigned)B), dim3(LP_THREADS), 0, s,
                               (const float*)tap, lin[l], P, a.Cout, p.rows_total, p.row_off[l], partial, ma);
        }
        cur = tap;
        cur_h = p.h[l];
        cur_w = p.w[l];
        if (l < 2) {
            float* pooled = region[1];
            const int C4 = a.Cout / 4;
            const size_t total = (size_t)N * p.ph[l] * p.pw[l] * C4;
            hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS),
                               0, s, (const float*)tap, pooled, cur_h, cur_w, p.ph[l], p.pw[l], C4, total);
            cur = pooled;
            cur_h = p.ph[l];
            cur_w = p.pw[l];
        }
    }
    if (sp) {
        LpMaskSumArgs ms;
        ms.dmap = dmap;
        ms.mask = mask;
        ms.partial = dpart;
        ms.H = H;
        ms.W = W;
        ms.p_total = sp->p_total;
        ms.rows_total = p.rows_total;
        for (int l = 0; l < LP_LAYERS; ++l) {
            ms.P[l] = p.h[l] * p.w[l];
            ms.w[l] = p.w[l];
            ms.p_off[l] = sp->p_off[l];
            ms.row_off[l] = p.row_off[l];
            ms.sH[l] = (float)H / (float)p.h[l];
            ms.sW[l] = (float)W / (float)p.w[l];
        }
        hipLaunchKernelGGL(lpips_mask_sum_kernel, dim3((unsigned)p.rows_total, (unsigned)B), dim3(MOBGS_WAVE), 0, s, ms);
        LpUpArgs u;
        u.dmap = dmap;
        u.mask = mask;
        u.map = map;
        u.partial = upart;
        u.H = H;
        u.W = W;
        u.p_total = sp->p_total;
        LpSpatialFinishArgs f;
        f.B = B;
        f.rows_total = p.rows_total;
        f.up_blocks = sp->up_blocks;
        f.pixels = (double)H * (double)W;
        for (int l = 0; l < LP_LAYERS; ++l) {
            u.h[l] = p.h[l];
            u.w[l] = p.w[l];
            u.p_off[l] = sp->p_off[l];
            u.sy[l] = (float)p.h[l] / (float)H;
            u.sx[l] = (float)p.w[l] / (float)W;
            f.rows[l] = p.rows[l];
            f.row_off[l] = p.row_off[l];
        }
        hipLaunchKernelGGL(lpips_upsample_kernel, dim3((unsigned)sp->up_blocks, (unsigned)B), dim3(LP_THREADS), 0, s, u);
        hipLaunchKernelGGL(lpips_spatial_finish_kernel, dim3(1), dim3(LP_FINISH_THREADS), 0, s, f, (const double*)dpart,
                           (const double*)upart, out);
        return check_launch(name);
    }
    LpFinishArgs f;
    f.B = B;
    f.rows_total = p.rows_total;
    for (int l = 0; l < LP_LAYERS; ++l) {
        f.rows[l] = p.rows[l];
        f.row_off[l] = p.row_off[l];
        f.pixels[l] = (double)p.h[l] * (double)p.w[l];
    }
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(LP_FINISH_THREADS), 0, s, f, (const double*)partial, out);
    return check_launch(name);
}

// the backward call's scratch: the five tap gradients and the gradients of the two pooled maps, sized for both sides
struct LpBwdPlan {
    size_t off_grad[LP_LAYERS], off_pool[2], bytes;
};

static bool lp_bwd_plan(int B, int H, int W, LpPlan& p, LpBwdPlan& q) {
    if (!lp_plan(B, H, W, p)) return false;
    const size_t N = 2 * (size_t)B;
    size_t at = 0;
    for (int l = 0; l < LP_LAYERS; ++l) {
        q.off_grad[l] = at;
        at += lp_align(N * p.h[l] * p.w[l] * LP_COUT[l] * sizeof(float));
    }
    for (int i = 0; i < 2; ++i) {
        q.off_pool[i] = at;
        at += lp_align(N * p.ph[i] * p.pw[i] * LP_COUT[i] * sizeof(float));
    }
    q.bytes = at;
    return true;
}

static int lp_bwd_pack_k(int layer) {
    if (layer < 2 || layer > LP_LAYERS) return 0;
    return LP_COUT[layer - 1] * LP_KS[layer - 1] * LP_KS[layer - 1];
}

static int lp_bwd_run(const char* name, const LpPlan& p, const LpBwdPlan& bp, int B, int H, int W, const float* img0,
                      const float* img1, const MobgsLpipsWeights* weights, const MobgsLpipsBwdWeights* bwd_weights, int flags,
                      const float* const* taps, const float* v_total, void* scratch, size_t scratch_bytes, float* g_img0,
                      float* g_img1, float* const* tap_grads, void* stream) {
    if (flags & ~(MOBGS_LPIPS_UNIT_RANGE | MOBGS_LPIPS_CLAMP | MOBGS_LPIPS_QUANTIZE)) {
        set_error("%s: flags = %d has unknown bits", name, flags);
        return MOBGS_E_INVALID;
    }
    if (!img0 || !img1 || !weights || !bwd_weights || !taps || !v_total || !scratch) {
        set_error("%s: NULL img0, img1, weights, bwd_weights, taps, v_total or scratch", name);
        return MOBGS_E_INVALID;
    }
    if (!g_img0 && !g_img1) {
        set_error("%s: g_img0 and g_img1 are both NULL: no gradient is wanted", name);
        return MOBGS_E_INVALID;
    }
    if ((flags & MOBGS_LPIPS_QUANTIZE) && g_img1) {
        set_error("%s: MOBGS_LPIPS_QUANTIZE with g_img1: the 8-bit truncation of img1 has no gradient", name);
        return MOBGS_E_INVALID;
    }
    const float* lin[LP_LAYERS] = {weights->lin1, weights->lin2, weights->lin3, weights->lin4, weights->lin5};
    const float* bw[LP_LAYERS] = {weights->w1, bwd_weights->w2, bwd_weights->w3, bwd_weights->w4, bwd_weights->w5};
    for (int l = 0; l < LP_LAYERS; ++l) {
        if (!bw[l] || !lin[l] || !taps[l] || (tap_grads && !tap_grads[l])) {
            set_error("%s: NULL weight, head, tap or tap-gradient pointer of layer %d", name, l + 1);
            return MOBGS_E_INVALID;
        }
        if (((uintptr_t)bw[l] & 15) || ((uintptr_t)lin[l] & 3) || ((uintptr_t)taps[l] & 15) ||
            (tap_grads && ((uintptr_t)tap_grads[l] & 15))) {
            set_error("%s: layer %d: packed weights, taps and tap gradients must be 16-byte aligned, heads 4-byte", name,
                      l + 1);
            return MOBGS_E_INVALID;
        }
    }
    if (((uintptr_t)img0 & 3) || ((uintptr_t)img1 & 3) || ((uintptr_t)g_img0 & 3) || ((uintptr_t)g_img1 & 3) ||
        ((uintptr_t)v_total & 3) || ((uintptr_t)scratch & 255)) {
        set_error("%s: images, gradients and v_total must be 4-byte aligned, scratch 256-byte aligned", name);
        return MOBGS_E_INVALID;
    }
    if (scratch_bytes < bp.bytes) {
        set_error("%s: scratch_bytes = %zu, mobgs_lpips_bwd_scratch_bytes(%d, %d, %d) = %zu", name, scratch_bytes, B, H, W,
                  bp.bytes);
        return MOBGS_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    const int ns = (g_img0 ? 1 : 0) + (g_img1 ? 1 : 0);      // wanted sides
    const int n_stride = ns == 2 ? 1 : 2, n_off = ns == 2 ? 0 : (g_img1 ? 1 : 0);
    const int NQ = ns * B;
    float* grad[LP_LAYERS];
    for (int l = 0; l < LP_LAYERS; ++l) grad[l] = tap_grads ? tap_grads[l] : (float*)(base + bp.off_grad[l]);
    float* gpool[2] = {(float*)(base + bp.off_pool[0]), (float*)(base + bp.off_pool[1])};
    // the distance gradients of the five taps
    for (int l = 0; l < LP_LAYERS; ++l) {
        const int P = p.h[l] * p.w[l];
        hipLaunchKernelGGL(lpips_dist_bwd_kernel, dim3((unsigned)p.rows[l], (unsigned)NQ), dim3(LP_THREADS), 0, s, taps[l],
                           lin[l], v_total, P, LP_COUT[l], n_stride, n_off, grad[l]);
    }
    // layers 5 .. 2: the gradient of layer l's output -> the gradient of its input (tap l - 1, or the pooled map in front)
    for (int l = LP_LAYERS - 1; l >= 1; --l) {
        const bool pooled = l <= 2;                          // layers 3 and 2 read a pooled map
        LpConvArgs a = {};
        a.in = grad[l];
        a.w = bw[l];
        a.out = pooled ? gpool[l - 1] : grad[l - 1];
        a.tap = taps[l - 1];
        a.n_stride = n_stride;
        a.n_off = n_off;
        a.N = NQ;
        a.Hi = p.h[l];                                       // stride 1, k - 1 - pad = pad: input and output sizes agree
        a.Wi = p.w[l];
        a.Cin = LP_COUT[l];
        a.Ho = p.h[l];
        a.Wo = p.w[l];
        a.Cout = LP_CIN[l];
        a.ks = LP_KS[l];
        a.stride = 1;
        a.pad = LP_PAD[l];
        a.Kpad = lp_bwd_pack_k(l + 1);
        a.M = NQ * p.h[l] * p.w[l];
        a.flags = flags;
        const unsigned blocks = (unsigned)((a.M + LP_BM - 1) / LP_BM) * (unsigned)(a.Cout / LP_BN);
        if (pooled) {
            hipLaunchKernelGGL(lpips_conv_kernel<LP_BWD_POOL>, dim3(blocks), dim3(LP_THREADS), 0, s, a);
            const int t = l - 1, C4 = LP_COUT[t] / 4;        // the tap in front of the pool
            const size_t total = (size_t)NQ * p.h[t] * p.w[t] * C4;
            hipLaunchKernelGGL(lpips_pool_bwd_kernel, dim3((unsigned)((total + LP_THREADS - 1) / LP_THREADS)),
                               dim3(LP_THREADS), 0, s, taps[t], (const float*)gpool[t], grad[t], p.h[t], p.w[t], p.ph[t],
                               p.pw[t], C4, n_stride, n_off, total);
        } else {
            hipLaunchKernelGGL(lpips_conv_kernel<LP_BWD_TAP>, dim3(blocks), dim3(LP_THREADS), 0, s, a);
        }
    }
    // layer 1, per wanted side
    const unsigned cell_blocks = (unsigned)(((long long)((H + 3) / 4) * ((W + 3) / 4) + LP_THREADS - 1) / LP_THREADS);
    int k = 0;
    for (int side = 0; side < 2; ++side) {
        float* g = side ? g_img1 : g_img0;
        if (!g) continue;
        // the truncation of img1 (refused above when its gradient is wanted) does not touch img0's clamp
        hipLaunchKernelGGL(lpips_first_bwd_kernel, dim3(cell_blocks, 16, (unsigned)B), dim3(LP_THREADS), 0, s,
                           (const float*)grad[0], weights->w1, side ? img1 : img0, g, H, W, p.h[0], p.w[0], ns, k, flags);
        ++k;
    }
    return check_launch(name);
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

size_t mobgs_lpips_scratch_bytes(int B, int H, int W) {
    LpPlan p;
    return lp_plan(B, H, W, p) ? p.bytes : 0;
}

size_t mobgs_lpips_spatial_scratch_bytes(int B, int H, int W) {
    LpPlan p;
    LpSpatialPlan q;
    return lp_spatial_plan(B, H, W, p, q) ? q.bytes : 0;
}

int mobgs_lpips_pack_k(int layer) {
    if (layer < 1 || layer > LP_LAYERS) return 0;
    const int K = LP_CIN[layer - 1] * LP_KS[layer - 1] * LP_KS[layer - 1];
    return (K + LP_BK - 1) / LP_BK * LP_BK;
}

int mobgs_lpips_alex(int B, int H, int W, const float* img0, const float* img1, const MobgsLpipsWeights* weights,
                     int flags, void* scratch, size_t scratch_bytes, double* out, float* const* taps, void* stream) {
    LpPlan p;
    if (!lp_plan(B, H, W, p)) {
        set_error("mobgs_lpips_alex: B = %d, H = %d, W = %d outside 1 <= B <= %d, %d <= H, W <= %d, 2 B h1 w1 <= 2^30 (below "
                  "31 the second pool has no output)", B, H, W, LP_MAX_B, LP_MIN_EDGE, LP_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    return lp_run("mobgs_lpips_alex", p, nullptr, B, H, W, img0, img1, weights, nullptr, flags, scratch, scratch_bytes,
                  nullptr, out, taps, stream);
}

int mobgs_lpips_alex_spatial(int B, int H, int W, const float* img0, const float* img1, const MobgsLpipsWeights* weights,
                             const float* mask, int flags, void* scratch, size_t scratch_bytes, float* map, double* out,
                             void* stream) {
    LpPlan p;
    LpSpatialPlan q;
    if (!lp_spatial_plan(B, H, W, p, q)) {
        set_error("mobgs_lpips_alex_spatial: B = %d, H = %d, W = %d outside 1 <= B <= %d, %d <= H, W <= %d, 2 B h1 w1 <= 2^30 "
                  "(below 31 the second pool has no output)", B, H, W, LP_MAX_B, LP_MIN_EDGE, LP_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    return lp_run("mobgs_lpips_alex_spatial", p, &q, B, H, W, img0, img1, weights, mask, flags, scratch, scratch_bytes, map,
                  out, nullptr, stream);
}

size_t mobgs_lpips_bwd_scratch_bytes(int B, int H, int W) {
    LpPlan p;
    LpBwdPlan q;
    return lp_bwd_plan(B, H, W, p, q) ? q.bytes : 0;
}

int mobgs_lpips_bwd_pack_k(int layer) { return lp_bwd_pack_k(layer); }

int mobgs_lpips_alex_bwd(int B, int H, int W, const float* img0, const float* img1, const MobgsLpipsWeights* weights,
                         const MobgsLpipsBwdWeights* bwd_weights, int flags, const float* const* taps,
                         const float* v_total, void* scratch, size_t scratch_bytes, float* g_img0, float* g_img1,
                         float* const* tap_grads, void* stream) {
    LpPlan p;
    LpBwdPlan q;
    if (!lp_bwd_plan(B, H, W, p, q)) {
        set_error("mobgs_lpips_alex_bwd: B = %d, H = %d, W = %d outside 1 <= B <= %d, %d <= H, W <= %d, 2 B h1 w1 <= 2^30 "
                  "(below 31 the second pool has no output)", B, H, W, LP_MAX_B, LP_MIN_EDGE, LP_MAX_EDGE);
        return MOBGS_E_INVALID;
    }
    return lp_bwd_run("mobgs_lpips_alex_bwd", p, q, B, H, W, img0, img1, weights, bwd_weights, flags, taps, v_total, scratch,
                      scratch_bytes, g_img0, g_img1, tap_grads, stream);
}

}  // extern "C"


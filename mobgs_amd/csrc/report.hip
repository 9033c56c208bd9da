// K26: report sheets (the reference's utils/scene_utils.py:15-260 render_training_image, with flow_vis.flow_to_color):
// every panel of a sheet -- images, the dynamic mask, the error map, depth over its maximum, normals from the depth's
// forward differences, flow on the Middlebury colour wheel -- is converted to 8 bits and laid out on the device; the host
// copies the finished bytes once.  gfx950 only.  Two launches per sheet, no synchronisation, no read-back, no float atomic.
//
//   report_stats_kernel     grid (workgroups, maps): min and max of a map, of a squared error (a - b)^2 or of a flow's
//                           radius sqrt(u u + v v).  A workgroup reduces its grid-stride share in registers, by shuffles
//                           and through LDS, and merges ONE pair into the map's key words with integer atomics: an fp32
//                           value's bits, with the sign bit flipped (negative values: all bits), order as the values
//                           do.  Min and max are order-free, so the result is bit-equal to torch.amin / torch.amax.  The
//                           workgroup that draws a map's last ticket turns the keys back into two floats.
//   report_compose_kernel   a lane owns four consecutive pixels of the sheet = twelve bytes = three aligned dwords, which
//                           it stores as dwords; only the last lane of a sheet whose pixel count is no multiple of four
//                           stores bytes.  A row of 3 P W bytes need not be a multiple of four: a lane's run may cross a
//                           panel or a row, so every PIXEL looks up its own panel, row and column.
//
// Built with -ffp-contract=off: every panel is the reference's numpy / torch float32 statements, one rounding per written
// operation, so a byte can differ from the float64 restatement only where 255 x sits within a few ulp of an integer
// (tests/report_cases.py derives the band per panel kind).
#include "common.h"
#include "reduce_shared.h"

namespace mobgs {

constexpr int REPORT_BLOCK = 256;
constexpr int REPORT_STAT_GRID = 256;     // workgroups per map at most (one per CU); beyond: grid-stride
constexpr int REPORT_MAX_GRID = 4096;     // workgroups of the compose kernel at most; beyond: grid-stride
constexpr int REPORT_PIX = 4;             // pixels per lane: 12 bytes = 3 dwords

// ---- the colour wheel of flow_vis.make_colorwheel (Baker et al., "A Database and Evaluation Methodology for Optical
// Flow", ICCV 2007): 55 entries, segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 ------------------------------------------
struct Wheel {
    uint8_t c[MOBGS_REPORT_WHEEL][4];
};
constexpr Wheel make_wheel() {
    Wheel w = {};
    const int len[6] = {15, 6, 4, 11, 13, 6};
    // segment s: channel rise[s] rises, or channel fall[s] falls, while hold[s] stays at 255
    const int rise[6] = {1, -1, 2, -1, 0, -1}, fall[6] = {-1, 0, -1, 1, -1, 2}, hold[6] = {0, 1, 1, 2, 2, 0};
    int k = 0;
    for (int s = 0; s < 6; ++s)
        for (int i = 0; i < len[s]; ++i, ++k) {
            const int ramp = 255 * i / len[s];    // floor
            w.c[k][hold[s]] = 255;
            if (rise[s] >= 0) w.c[k][rise[s]] = (uint8_t)ramp;
            if (fall[s] >= 0) w.c[k][fall[s]] = (uint8_t)(255 - ramp);
        }
    return w;
}
__constant__ Wheel REPORT_WHEEL = make_wheel();

// ---- statistics ------------------------------------------------------------------------------------------------------
// order-preserving key of an fp32 value (no NaN): unsigned comparison of keys = comparison of values
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct StatArgs {
    MobgsReportStat s[MOBGS_REPORT_MAX_STATS];
};

// the value of element i of a map; flow: i is a pixel
__device__ __forceinline__ float stat_value(const MobgsReportStat& s, int64_t i) {
    if (s.kind == MOBGS_REPORT_STAT_SQERR) {
        const float d = s.a[i] - s.b[i];
        return d * d;
    }
    if (s.kind == MOBGS_REPORT_STAT_FLOW_RAD) {
        float2 f = reinterpret_cast<const float2*>(s.a)[i];
        if (s.clip >= 0.f) {
            f.x = fminf(fmaxf(f.x, 0.f), s.clip);
            f.y = fminf(fmaxf(f.y, 0.f), s.clip);
        }
        // sqrtf is the correctly rounded root under hipcc's defaults, as numpy's; __fsqrt_rn maps to the 1-ulp hardware root
        return sqrtf(f.x * f.x + f.y * f.y);
    }
    return s.a[i];
}

// words: [2 S] key words (~key of the minimum, key of the maximum: both grow, both start at 0), then [S] tickets
__global__ void __launch_bounds__(REPORT_BLOCK) report_stats_kernel(StatArgs args, float* __restrict__ out,
                                                                     uint32_t* __restrict__ words, int n_stats) {
    __shared__ float s_lo[REPORT_BLOCK / MOBGS_WAVE], s_hi[REPORT_BLOCK / MOBGS_WAVE];
    const int m = blockIdx.y;
    const MobgsReportStat& s = args.s[m];
    const int64_t n = s.n;
    // (every workgroup of a map's row runs, also those beyond its share: the ticket count is gridDim.x)
    float lo = __builtin_inff(), hi = -__builtin_inff();
    const int64_t stride = (int64_t)gridDim.x * REPORT_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * REPORT_BLOCK + threadIdx.x; i < n; i += stride) {
        const float v = stat_value(s, i);
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
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < REPORT_BLOCK / MOBGS_WAVE; ++w) {
        lo = fminf(lo, s_lo[w]);
        hi = fmaxf(hi, s_hi[w]);
    }
    uint32_t* keys = words + 2 * m;
    if (lo <= hi) {    // (false for a workgroup without elements)
        atomicMax(&keys[0], ~order_key(lo));
        atomicMax(&keys[1], order_key(hi));
    }
    __threadfence();
    const uint32_t ticket = atomicAdd(&words[2 * n_stats + m], 1u);
    if (ticket != gridDim.x - 1) return;
    __threadfence();
    // (read through the atomic unit, where every workgroup's merge happened)
    out[2 * m] = key_value(~atomicMax(&keys[0], 0u));
    out[2 * m + 1] = key_value(atomicMax(&keys[1], 0u));
}

// ---- panels ----------------------------------------------------------------------------------------------------------
struct ComposeArgs {
    MobgsReportPanel p[MOBGS_REPORT_MAX_PANELS];
};
struct ReportCam {
    float focal, cx, cy, skew, offset;
};

// the reference's (np.clip(x, 0, 1) * 255).astype('uint8'): truncation.  (NaN -> 0: the conversion stays defined)
__device__ __forceinline__ uint32_t byte_of(float x) {
    const float c = !(x > 0.f) ? 0.f : (x > 1.f ? 1.f : x);
    return (uint32_t)floorf(c * 255.f);
}

// camera-frame point of pixel (i, j) at depth z, scene_utils.py:130-141: z = depth + 1e-6, the direction from the single
// focal length (both axes) as csrc/normals.hip forms its own
__device__ __forceinline__ void fd_point(const ReportCam& c, const float* __restrict__ depth, int W, int i, int j,
                                         float p[3]) {
    const float z = depth[(size_t)i * W + j] + 1e-6f;
    const float y = (((float)i + c.offset) - c.cy) / c.focal;
    const float x = (((float)j + c.offset) - c.cx - y * c.skew) / c.focal;
    p[0] = x * z;
    p[1] = y * z;
    p[2] = 1.f * z;
}

// scene_utils.py:143-163, :185: forward differences (the last column / row repeats its neighbour's), cross product as
// written, F.normalize (eps 1e-12), (n + 1) / 2
__device__ __forceinline__ void normals_fd(const ReportCam& c, const float* __restrict__ depth, int H, int W, int i, int j,
                                           float rgb[3]) {
    const int ju = j < W - 1 ? j : W - 2, iv = i < H - 1 ? i : H - 2;
    float a[3], b[3], du[3], dv[3];
    fd_point(c, depth, W, i, ju + 1, a);
    fd_point(c, depth, W, i, ju, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) du[k] = a[k] - b[k];
    fd_point(c, depth, W, iv + 1, j, a);
    fd_point(c, depth, W, iv, j, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) dv[k] = a[k] - b[k];
    float n[3];
    n[0] = dv[1] * du[2] - du[1] * dv[2];
    n[1] = dv[2] * du[0] - du[2] * dv[0];
    n[2] = dv[0] * du[1] - du[0] * dv[1];
    const float len = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[k] = (n[k] / len + 1.f) / 2.f;
}

// flow_vis.flow_to_color / flow_uv_to_colors for one pixel, float32 as numpy evaluates it.  rad < 1 after the division by
// rad_max + 1e-5, so the package's `col * 0.75` arm (rad > 1) cannot be reached and is not here.
__device__ __forceinline__ void flow_colour(const MobgsReportPanel& p, float rad_max, size_t q, float rgb[3]) {
    float2 f = reinterpret_cast<const float2*>(p.a)[q];
    if (p.clip >= 0.f) {
        f.x = fminf(fmaxf(f.x, 0.f), p.clip);
        f.y = fminf(fmaxf(f.y, 0.f), p.clip);
    }
    const float den = rad_max + 1e-5f;
    const float u = f.x / den, v = f.y / den;
    const float rad = sqrtf(u * u + v * v);
    // a division by fp32 pi, not a product with 1 / pi: atan2f(-0, -u) = -pi_f gives a = -1 exactly (v = +0, u > 0: wheel
    // entry 0), and a zero flow (-0, -0) likewise
    const float a = atan2f(-v, -u) / 3.14159265358979323846f;
    const float fk = (a + 1.f) / 2.f * (float)(MOBGS_REPORT_WHEEL - 1);
    const float fl = floorf(fk);
    int k0 = (int)fl;
    k0 = k0 < 0 ? 0 : (k0 > MOBGS_REPORT_WHEEL - 1 ? MOBGS_REPORT_WHEEL - 1 : k0);   // (stays inside the table whatever fk)
    const int k1 = k0 + 1 == MOBGS_REPORT_WHEEL ? 0 : k0 + 1;
    const float w = fk - fl;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float c0 = (float)REPORT_WHEEL.c[k0][ch] / 255.f, c1 = (float)REPORT_WHEEL.c[k1][ch] / 255.f;
        // (1 - f) c0 + f c1 in the form that is exact where the two entries agree: on a channel both hold at 255 the package
        // (float64 wheel) returns exactly 1 and the byte 255; fp32's (1 - f) + f can be one ulp short of 1, i.e. 254
        const float col = c0 + w * (c1 - c0);
        rgb[ch] = 1.f - rad * (1.f - col);
    }
}

// the three bytes of pixel (i, j) of panel p, packed r | g << 8 | b << 16
__device__ __forceinline__ uint32_t panel_pixel(const MobgsReportPanel& p, const float* __restrict__ stats,
                                                const ReportCam& cam, int H, int W, int i, int j) {
    const size_t P = (size_t)H * W, q = (size_t)i * W + j;
    float rgb[3];
    switch (p.kind) {
    case MOBGS_REPORT_RGB:
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = p.a[k * P + q];
        break;
    case MOBGS_REPORT_GREY:
        rgb[0] = rgb[1] = rgb[2] = p.a[q];
        break;
    case MOBGS_REPORT_GREY_DIV_MAX: {
        // scene_utils.py:177-179: x / max.  The reference divides by zero where the map's maximum is 0; here the panel is 0.
        const float mx = stats[2 * p.slot + 1];
        rgb[0] = rgb[1] = rgb[2] = mx == 0.f ? 0.f : p.a[q] / mx;
        break;
    }
    case MOBGS_REPORT_ERROR: {
        // scene_utils.py:187-188
        const float lo = stats[2 * p.slot], hi = stats[2 * p.slot + 1];
        const float den = fmaxf(hi - lo, 1e-8f);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d = p.a[k * P + q] - p.b[k * P + q];
            rgb[k] = (d * d - lo) / den;
        }
        break;
    }
    case MOBGS_REPORT_SIGNED3:
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = (p.a[k * P + q] + 1.f) / 2.f;
        break;
    case MOBGS_REPORT_NORMALS_FD:
        normals_fd(cam, p.a, H, W, i, j, rgb);
        break;
    default:    // MOBGS_REPORT_FLOW (the host refuses any other kind)
        flow_colour(p, stats[2 * p.slot + 1], q, rgb);
        break;
    }
    return byte_of(rgb[0]) | (byte_of(rgb[1]) << 8) | (byte_of(rgb[2]) << 16);
}

// sheet: [H, P W, 3] (vertical == 0: panels side by side) or [P H, W, 3] (vertical: one below the other, every panel a
// contiguous [H, W, 3] image).  n_pix = P H W.
__global__ void __launch_bounds__(REPORT_BLOCK) report_compose_kernel(ComposeArgs args, const float* __restrict__ stats,
                                                                       ReportCam cam, int H, int W, int n_panels,
                                                                       int vertical, uint32_t n_pix,
                                                                       uint8_t* __restrict__ sheet) {
    const uint32_t n_runs = (n_pix + REPORT_PIX - 1) / REPORT_PIX;
    const uint32_t stride = gridDim.x * REPORT_BLOCK;
    const uint32_t row_pix = vertical ? (uint32_t)W : (uint32_t)n_panels * W;
    for (uint32_t r = blockIdx.x * REPORT_BLOCK + threadIdx.x; r < n_runs; r += stride) {
        const uint32_t q0 = r * REPORT_PIX;
        uint32_t px[REPORT_PIX];
#pragma unroll
        for (int k = 0; k < REPORT_PIX; ++k) {
            const uint32_t q = q0 + k;
            px[k] = 0u;
            if (q >= n_pix) continue;
            const uint32_t row = q / row_pix, col = q - row * row_pix;
            int panel, i, j;
            if (vertical) {
                panel = (int)(row / (uint32_t)H);
                i = (int)(row - (uint32_t)panel * H);
                j = (int)col;
            } else {
                panel = (int)(col / (uint32_t)W);
                i = (int)row;
                j = (int)(col - (uint32_t)panel * W);
            }
            px[k] = panel_pixel(args.p[panel], stats, cam, H, W, i, j);
        }
        uint8_t* dst = sheet + 3 * (size_t)q0;
        if (q0 + REPORT_PIX <= n_pix) {
            // 12 bytes r g b r | g b r g | b r g b at a multiple of 12 from a 4-byte aligned base
            uint32_t* d = reinterpret_cast<uint32_t*>(dst);
            d[0] = px[0] | (px[1] << 24);
            d[1] = (px[1] >> 8) | (px[2] << 16);
            d[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
#pragma unroll
            for (int k = 0; k < REPORT_PIX; ++k) {
                if (q0 + k >= n_pix) break;
                dst[3 * k] = (uint8_t)(px[k] & 255u);
                dst[3 * k + 1] = (uint8_t)((px[k] >> 8) & 255u);
                dst[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
        }
    }
}

// (pixel indices are 32-bit: a sheet has at most 2^30 pixels)
static bool report_size_ok(int H, int W, int n_panels) {
    return H >= 1 && W >= 1 && n_panels >= 1 && (int64_t)H * W * n_panels <= ((int64_t)1 << 30);
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

size_t mobgs_report_stats_floats(int n_stats) {
    if (n_stats < 1 || n_stats > MOBGS_REPORT_MAX_STATS) return 0;
    return 5 * (size_t)n_stats;
}

int mobgs_report_stats(int n_stats, const MobgsReportStat* stats_host, float* stats, void* stream) {
    if (n_stats < 1 || n_stats > MOBGS_REPORT_MAX_STATS || !stats_host || !stats) {
        set_error("mobgs_report_stats: n_stats = %d (1 .. %d), or a NULL buffer", n_stats, MOBGS_REPORT_MAX_STATS);
        return MOBGS_E_INVALID;
    }
    if (!aligned(stats, 4)) {
        set_error("mobgs_report_stats: stats must be 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    StatArgs args = {};
    int64_t n_max = 0;
    for (int m = 0; m < n_stats; ++m) {
        const MobgsReportStat& s = stats_host[m];
        const bool two = s.kind == MOBGS_REPORT_STAT_SQERR, flow = s.kind == MOBGS_REPORT_STAT_FLOW_RAD;
        if (s.kind != MOBGS_REPORT_STAT_MINMAX && !two && !flow) {
            set_error("mobgs_report_stats: map %d has the unknown kind %d", m, s.kind);
            return MOBGS_E_INVALID;
        }
        if (s.n < 1 || s.n > ((int64_t)1 << 32) || !s.a || (two && !s.b)) {
            set_error("mobgs_report_stats: map %d has n = %lld (1 .. 2^32) or a NULL pointer", m, (long long)s.n);
            return MOBGS_E_INVALID;
        }
        if (!aligned(s.a, flow ? 8 : 4) || !aligned(s.b, 4)) {
            set_error("mobgs_report_stats: map %d is misaligned (flow maps 8 bytes, others 4)", m);
            return MOBGS_E_INVALID;
        }
        args.s[m] = s;
        n_max = s.n > n_max ? s.n : n_max;
    }
    hipStream_t st = (hipStream_t)stream;
    uint32_t* words = reinterpret_cast<uint32_t*>(stats + 2 * (size_t)n_stats);
    if (hipMemsetAsync(words, 0, 3 * (size_t)n_stats * sizeof(uint32_t), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("mobgs_report_stats: hipMemsetAsync failed");
        return MOBGS_E_LAUNCH;
    }
    const int64_t g = (n_max + REPORT_BLOCK - 1) / REPORT_BLOCK;
    const dim3 grid((unsigned)(g < REPORT_STAT_GRID ? g : REPORT_STAT_GRID), (unsigned)n_stats);
    hipLaunchKernelGGL(report_stats_kernel, grid, dim3(REPORT_BLOCK), 0, st, args, stats, words, n_stats);
    return check_launch("mobgs_report_stats");
}

int mobgs_report_compose(int H, int W, int n_panels, const MobgsReportPanel* panels_host, const float* stats,
                         int n_stats, float focal, float cx, float cy, float skew, float pixel_offset, int vertical,
                         uint8_t* sheet, void* stream) {
    if (n_panels > MOBGS_REPORT_MAX_PANELS || !report_size_ok(H, W, n_panels) || !panels_host || !sheet) {
        set_error("mobgs_report_compose: H = %d, W = %d, n_panels = %d (1 .. %d, at most 2^30 pixels), or a NULL buffer", H, W, n_panels,
                  MOBGS_REPORT_MAX_PANELS);
        return MOBGS_E_INVALID;
    }
    if (!aligned(sheet, 4) || !aligned(stats, 4)) {
        set_error("mobgs_report_compose: sheet and stats must be 4-byte aligned");
        return MOBGS_E_INVALID;
    }
    ComposeArgs args = {};
    for (int k = 0; k < n_panels; ++k) {
        const MobgsReportPanel& p = panels_host[k];
        if (p.kind < MOBGS_REPORT_RGB || p.kind > MOBGS_REPORT_FLOW) {
            set_error("mobgs_report_compose: panel %d has the unknown kind %d", k, p.kind);
            return MOBGS_E_INVALID;
        }
        const bool needs_stat = p.kind == MOBGS_REPORT_GREY_DIV_MAX || p.kind == MOBGS_REPORT_ERROR ||
                                p.kind == MOBGS_REPORT_FLOW;
        if (!p.a || (p.kind == MOBGS_REPORT_ERROR && !p.b) ||
            (needs_stat && (!stats || p.slot < 0 || p.slot >= n_stats))) {
            set_error("mobgs_report_compose: panel %d (kind %d) has a NULL source or a statistics slot outside 0 .. %d",
                      k, p.kind, n_stats - 1);
            return MOBGS_E_INVALID;
        }
        if (!aligned(p.a, p.kind == MOBGS_REPORT_FLOW ? 8 : 4) || !aligned(p.b, 4)) {
            set_error("mobgs_report_compose: panel %d is misaligned (flow maps 8 bytes, others 4)", k);
            return MOBGS_E_INVALID;
        }
        if (p.kind == MOBGS_REPORT_NORMALS_FD && (H < 2 || W < 2 || !(focal != 0.f))) {
            set_error("mobgs_report_compose: the NORMALS_FD panel %d needs H, W >= 2 and a focal length (H = %d, W = %d)",
                      k, H, W);
            return MOBGS_E_INVALID;
        }
        args.p[k] = p;
    }
    const uint32_t n_pix = (uint32_t)n_panels * (uint32_t)H * (uint32_t)W;
    const uint32_t runs = (n_pix + REPORT_PIX - 1) / REPORT_PIX;
    const uint32_t g = (runs + REPORT_BLOCK - 1) / REPORT_BLOCK;
    const ReportCam cam = {focal, cx, cy, skew, pixel_offset};
    hipLaunchKernelGGL(report_compose_kernel, dim3((unsigned)(g < REPORT_MAX_GRID ? g : REPORT_MAX_GRID)),
                       dim3(REPORT_BLOCK), 0, (hipStream_t)stream, args, stats, cam, H, W, n_panels, vertical ? 1 : 0,
                       n_pix, sheet);
    return check_launch("mobgs_report_compose");
}

}  // extern "C"

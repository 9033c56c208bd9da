// K28: the HexPlane grid regularisers (the reference's scene/regulation.py:13-28 and scene/gaussian_model.py:1373-1415):
// second-difference smoothness along h, total variation, and |1 - t| of the time planes, for ALL planes of a call in one
// streaming launch, with the backward in one more.  gfx950 only.
//
//   gridreg_fwd_kernel     a workgroup owns GR_BLOCK units of four neighbouring columns and GR_ROWS rows of ONE plane of
//                          the table; a thread walks its rows with the previous row and the previous difference in
//                          registers and adds the squares (and |1 - t|) in float64: one row of two partial sums
//   gridreg_finish_kernel  one workgroup: per plane the rows of its workgroups in a fixed order (wave_rows_sum), times the
//                          reciprocal counts, added per output slot in table order; the slots rounded to fp32 once, then
//                          the weighted total in fp32 as the reference's statement forms it
//   gridreg_bwd_kernel     the same geometry in gather form: a thread slides a five-row window (TV: three rows) over
//                          its rows and writes every gradient element exactly once
//
// Two launches forward, one backward, on the caller's stream: no atomics, no zero-fill, no read-back, no allocation.  The
// summation order is a function of the table's shapes alone, so the same planes give the same bits.  A first or second
// difference is formed in fp32 exactly as the reference writes it -- (a - b), then the difference of the differences; this
// file is built with -ffp-contract=off -- and everything after it (squares, sums, the gradient's combination) in float64.
//
// Layouts.  A plane [C, h, w] comes with three element strides and must have one unit-stride direction:
//   channels-last (sc == 1)  inner = C, outer = w; with dense rows (sw == C) a row is ONE run of w C elements and the
//                            plane is walked as inner = w C, outer = 1, so four lanes' worth of channels never ends at C
//   NCHW          (sw == 1)  inner = w, outer = C
// The walk along h is the strided direction in both, so the lanes of a wave read one contiguous run per row.  A unit is
// loaded as one float4 when the plane's base is 16-byte aligned and its strides are multiples of four, and element by
// element otherwise (uniform per plane); the last unit of a run of length != 0 (mod 4) is always element by element.
// The gradient is written DENSE in the same arm's layout ([h][w][C], or [C][h][w]).
#include "reduce_shared.h"

namespace mobgs {

constexpr int GR_BLOCK = 256;
constexpr int GR_WAVES = GR_BLOCK / MOBGS_WAVE;
constexpr int GR_VEC = 4;
// rows per workgroup: the 256 x 256 x 32 plane of the trained configuration becomes 8 x 32 workgroups (1008 for its nine
// spatial planes: four per CU).  A thread has one row in flight at a time, so the launch is bound by latency and more,
// shorter segments win although a segment re-reads 2 of its neighbour's rows (backward 4), so a plane is requested 1.25
// times forward and 1.5 times backward (that the repeats are served by the L2 is supposed, not measured): on the 18
// planes forward / backward take 28.0 / 35.5 us with 32 rows, 18.5 / 25.0 with 16, 15.3 / 20.1 with 8 (MI355X, one visit,
// kernel trace, three builds; docs/MEASUREMENT_LOG.md).
constexpr int GR_ROWS = 8;
constexpr int GR_F_VEC_IN = 1, GR_F_VEC_OUT = 2, GR_F_W_OUTER = 4;

struct GrPlane {
    const float* t;
    float* g;
    double inv0, inv1;
    int32_t so, sh;     // element strides of the outer index and of h (the inner index has stride 1)
    int32_t gso, gsh;   // the same for the gradient
    int32_t ni, no, h;
    int32_t wd, ws;     // w-neighbour (TV): address distance; its distance along the inner index (inner arm)
    int32_t kind, slot, flags;
    int32_t first, ncb;  // first workgroup of the plane; workgroups along the units
};
struct GrTable {
    int32_t n, n_slots;
    GrPlane p[MOBGS_GRIDREG_MAX_PLANES];
};

struct GrVec {
    float v[GR_VEC];
};

// where a workgroup and a thread stand
struct GrPos {
    int p, h0, h1, nv;        // plane, rows [h0, h1), valid elements of the unit (0: the thread is idle)
    int o, i;                 // outer index, first inner index
};

__device__ __forceinline__ GrPos gr_locate(const GrTable& tb) {
    int p = 0;
    for (int q = 1; q < tb.n; ++q)
        if ((int)blockIdx.x >= tb.p[q].first) p = q;
    const GrPlane& pl = tb.p[p];
    const int b = (int)blockIdx.x - pl.first;
    const int cb = b % pl.ncb, seg = b / pl.ncb;
    const int ncu = (pl.ni + GR_VEC - 1) / GR_VEC;
    const int u = cb * GR_BLOCK + (int)threadIdx.x;
    GrPos r;
    r.p = p;
    r.h0 = seg * GR_ROWS;
    r.h1 = min(r.h0 + GR_ROWS, pl.h);
    r.o = u / ncu;
    r.i = (u - r.o * ncu) * GR_VEC;
    r.nv = r.o < pl.no ? min(GR_VEC, pl.ni - r.i) : 0;
    return r;
}

__device__ __forceinline__ GrVec gr_load(const float* __restrict__ a, int nv, bool vec) {
    GrVec x;
    if (vec && nv == GR_VEC) {
        const float4 q = *reinterpret_cast<const float4*>(a);
        x.v[0] = q.x, x.v[1] = q.y, x.v[2] = q.z, x.v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < GR_VEC; ++e) x.v[e] = e < nv ? a[e] : 0.f;
    }
    return x;
}

__device__ __forceinline__ void gr_store(float* __restrict__ a, const GrVec& x, int nv, bool vec) {
    if (vec && nv == GR_VEC) {
        *reinterpret_cast<float4*>(a) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < GR_VEC; ++e)
            if (e < nv) a[e] = x.v[e];
    }
}

// TV: has element (o, idx) a neighbour one step down / up w?
__device__ __forceinline__ bool gr_has_left(const GrPlane& pl, int o, int idx) {
    return (pl.flags & GR_F_W_OUTER) ? o >= 1 : idx >= pl.ws;
}
__device__ __forceinline__ bool gr_has_right(const GrPlane& pl, int o, int idx) {
    return (pl.flags & GR_F_W_OUTER) ? o + 1 < pl.no : idx + pl.ws < pl.ni;
}

__global__ void __launch_bounds__(GR_BLOCK) gridreg_fwd_kernel(GrTable tb, double* __restrict__ partial) {
    __shared__ double s_wave[GR_WAVES];
    const GrPos at = gr_locate(tb);
    const GrPlane& pl = tb.p[at.p];
    const int kind = pl.kind;
    const bool smooth = kind == MOBGS_GRIDREG_SMOOTH || kind == MOBGS_GRIDREG_SMOOTH_L1;
    const bool l1 = kind == MOBGS_GRIDREG_L1 || kind == MOBGS_GRIDREG_SMOOTH_L1;
    const bool tv = kind == MOBGS_GRIDREG_TV;
    double s0 = 0.0, s1 = 0.0;
    if (at.nv > 0) {
        const bool vec = (pl.flags & GR_F_VEC_IN) != 0;
        const float* base = pl.t + (size_t)at.o * pl.so + at.i;
        // the last row read: sd[k] = (t[k+2] - t[k+1]) - (t[k+1] - t[k]) is owned by the segment of k, dh[k] likewise
        const int last = l1 && !smooth ? at.h1 - 1 : min(tv ? at.h1 : at.h1 + 1, pl.h - 1);
        GrVec tm1 = {}, dm1 = {};
        for (int r = at.h0; r <= last; ++r) {
            const float* row = base + (size_t)r * pl.sh;
            const GrVec tr = gr_load(row, at.nv, vec);
            GrVec d;
#pragma unroll
            for (int e = 0; e < GR_VEC; ++e) {
                const bool live = e < at.nv;
                d.v[e] = r > at.h0 ? tr.v[e] - tm1.v[e] : 0.f;
                if (smooth && r >= at.h0 + 2) {
                    const float sd = d.v[e] - dm1.v[e];
                    s0 += (double)sd * (double)sd;
                }
                if (l1 && r < at.h1 && live) s1 += (double)fabsf(1.f - tr.v[e]);
                if (tv) {
                    if (r > at.h0) s0 += (double)d.v[e] * (double)d.v[e];
                    if (r < at.h1 && live && gr_has_left(pl, at.o, at.i + e)) {
                        const float dw = tr.v[e] - row[e - pl.wd];
                        s1 += (double)dw * (double)dw;
                    }
                }
            }
            tm1 = tr;
            dm1 = d;
        }
    }
    s0 = block_sum<GR_WAVES>(s0, s_wave);
    s1 = block_sum<GR_WAVES>(s1, s_wave);
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = s0;
        partial[2 * (size_t)blockIdx.x + 1] = s1;
    }
}

// out[0 .. n_slots): the terms; *total: sum_s weights[s] out[s] in fp32, left to right (weights != NULL).
// One workgroup of 16 waves: a wave adds one column of one plane's partial rows at a time (wave_rows_sum: no barrier, an
// order fixed by the row count), so the 36 sums of an 18-plane table take three rounds instead of 36; thread 0 then
// combines them in table order.
constexpr int GR_FIN_BLOCK = 1024;
__global__ void __launch_bounds__(GR_FIN_BLOCK) gridreg_finish_kernel(GrTable tb, int n_blocks,
                                                                      const double* __restrict__ partial,
                                                                      const float* __restrict__ weights,
                                                                      float* __restrict__ out, float* __restrict__ total_out) {
    __shared__ double s_sum[2 * MOBGS_GRIDREG_MAX_PLANES];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / MOBGS_WAVE), lane = (int)threadIdx.x & (MOBGS_WAVE - 1);
    for (int item = wave; item < 2 * tb.n; item += GR_FIN_BLOCK / MOBGS_WAVE) {
        const int p = item >> 1;
        const int first = tb.p[p].first;
        const int nb = (p + 1 < tb.n ? tb.p[p + 1].first : n_blocks) - first;
        const double s = wave_rows_sum(partial + 2 * (size_t)first + (item & 1), nb, 2, lane);
        if (lane == 0) s_sum[item] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double acc[MOBGS_GRIDREG_MAX_SLOTS + 1] = {};
    for (int p = 0; p < tb.n; ++p) {
        const GrPlane& pl = tb.p[p];
        const double S0 = s_sum[2 * p], S1 = s_sum[2 * p + 1];
        switch (pl.kind) {
            case MOBGS_GRIDREG_SMOOTH: acc[pl.slot] += S0 * pl.inv0; break;
            case MOBGS_GRIDREG_TV: acc[pl.slot] += 2.0 * (S0 * pl.inv0 + S1 * pl.inv1); break;
            case MOBGS_GRIDREG_L1: acc[pl.slot] += S1 * pl.inv1; break;
            default:
                acc[pl.slot] += S0 * pl.inv0;
                acc[pl.slot + 1] += S1 * pl.inv1;
                break;
        }
    }
    float total = 0.f;
    for (int s = 0; s < tb.n_slots; ++s) {
        const float v = (float)acc[s];
        out[s] = v;
        if (weights) total = s == 0 ? weights[0] * v : total + weights[s] * v;
    }
    if (weights) *total_out = total;
}

// the cotangent of slot s: v[s], or with weights v[0] weights[s] (v is then the cotangent of the weighted total)
__device__ __forceinline__ double gr_cot(const float* __restrict__ v, const float* __restrict__ weights, int s) {
    return weights ? (double)v[0] * (double)weights[s] : (double)v[s];
}

__global__ void __launch_bounds__(GR_BLOCK) gridreg_bwd_kernel(GrTable tb, const float* __restrict__ v,
                                                               const float* __restrict__ weights) {
    const GrPos at = gr_locate(tb);
    if (at.nv == 0) return;
    const GrPlane& pl = tb.p[at.p];
    const int kind = pl.kind;
    const bool vec = (pl.flags & GR_F_VEC_IN) != 0, gvec = (pl.flags & GR_F_VEC_OUT) != 0;
    const float* base = pl.t + (size_t)at.o * pl.so + at.i;
    float* gbase = pl.g + (size_t)at.o * pl.gso + at.i;
    if (kind == MOBGS_GRIDREG_TV) {
        // d/dt[j] of 2 (inv0 sum dh^2 + inv1 sum dw^2): 4 inv0 (dh[j-1] - dh[j]) + 4 inv1 (dw[i-1] - dw[i])
        const double g = gr_cot(v, weights, pl.slot);
        const double c0 = 4.0 * pl.inv0 * g, c1 = 4.0 * pl.inv1 * g;
        const int r0 = max(at.h0 - 1, 0);
        GrVec tm1 = {}, dm1 = {};
        for (int r = r0; r <= at.h1; ++r) {
            GrVec tr = {}, d;
            if (r < pl.h) tr = gr_load(base + (size_t)r * pl.sh, at.nv, vec);
#pragma unroll
            for (int e = 0; e < GR_VEC; ++e) d.v[e] = (r < pl.h && r > r0) ? tr.v[e] - tm1.v[e] : 0.f;   // dh[r-1]
            const int j = r - 1;
            if (j >= at.h0) {
                const float* row = base + (size_t)j * pl.sh;
                // (dm1 is dh[j-1], or was never formed: j = 0)
                GrVec out;
#pragma unroll
                for (int e = 0; e < GR_VEC; ++e) {
                    double a = (j > 0 ? (double)dm1.v[e] : 0.0) - (double)d.v[e];
                    double b = 0.0;
                    if (e < at.nv) {
                        if (gr_has_left(pl, at.o, at.i + e)) b += (double)(tm1.v[e] - row[e - pl.wd]);
                        if (gr_has_right(pl, at.o, at.i + e)) b -= (double)(row[e + pl.wd] - tm1.v[e]);
                    }
                    out.v[e] = (float)(c0 * a + c1 * b);
                }
                gr_store(gbase + (size_t)j * pl.gsh, out, at.nv, gvec);
            }
            tm1 = tr;
            dm1 = d;
        }
        return;
    }
    const bool smooth = kind != MOBGS_GRIDREG_L1, l1 = kind != MOBGS_GRIDREG_SMOOTH;
    // d/dt[j] of inv0 sum sd^2: 2 inv0 (sd[j-2] - 2 sd[j-1] + sd[j]); of inv1 sum |1 - t|: -inv1 sign(1 - t[j])
    const double c0 = smooth ? 2.0 * pl.inv0 * gr_cot(v, weights, pl.slot) : 0.0;
    const double c1 = l1 ? pl.inv1 * gr_cot(v, weights, kind == MOBGS_GRIDREG_L1 ? pl.slot : pl.slot + 1) : 0.0;
    const int r0 = smooth ? max(at.h0 - 2, 0) : at.h0;
    const int lag = smooth ? 2 : 0;   // row j = r - lag is written when row r has been read
    GrVec tm1 = {}, tm2 = {}, dm1 = {}, sdA = {}, sdB = {};
    for (int r = r0; r < at.h1 + lag; ++r) {
        GrVec tr = {}, d, sdC;
        const bool have = r < pl.h;
        if (have) tr = gr_load(base + (size_t)r * pl.sh, at.nv, vec);
#pragma unroll
        for (int e = 0; e < GR_VEC; ++e) {
            d.v[e] = (have && r >= r0 + 1) ? tr.v[e] - tm1.v[e] : 0.f;
            sdC.v[e] = (have && r >= r0 + 2) ? d.v[e] - dm1.v[e] : 0.f;    // sd[r-2]; 0 where the window is cut
        }
        const int j = r - lag;
        if (j >= at.h0) {
            GrVec out;
#pragma unroll
            for (int e = 0; e < GR_VEC; ++e) {
                const float tj = smooth ? tm2.v[e] : tr.v[e];
                const float one_minus = 1.f - tj;
                const double sgn = (double)((one_minus > 0.f) - (one_minus < 0.f));   // sign(0) = 0, as torch.abs has it
                // (a term the kind does not have is left out, not multiplied by 0: a non-finite value must not reach it)
                double g = l1 ? -(c1 * sgn) : 0.0;
                if (smooth) g += c0 * (((double)sdA.v[e] - 2.0 * (double)sdB.v[e]) + (double)sdC.v[e]);
                out.v[e] = (float)g;
            }
            gr_store(gbase + (size_t)j * pl.gsh, out, at.nv, gvec);
        }
        sdA = sdB, sdB = sdC, tm2 = tm1, tm1 = tr, dm1 = d;
    }
}

// The table the kernels read, from the caller's.  -> NULL, or what is wrong.  n_blocks: the workgroups of a launch.
static const char* gr_build(int n_planes, const MobgsGridPlane* planes, int n_slots, bool backward, GrTable& tb,
                            int& n_blocks) {
    if (n_planes < 1 || n_planes > MOBGS_GRIDREG_MAX_PLANES) return "n_planes outside 1 .. MOBGS_GRIDREG_MAX_PLANES";
    if (!planes) return "NULL plane table";
    if (n_slots < 1 || n_slots > MOBGS_GRIDREG_MAX_SLOTS) return "n_slots outside 1 .. MOBGS_GRIDREG_MAX_SLOTS";
    tb.n = n_planes;
    tb.n_slots = n_slots;
    int64_t first = 0;
    for (int k = 0; k < n_planes; ++k) {
        const MobgsGridPlane& in = planes[k];
        GrPlane& p = tb.p[k];
        if (!in.t || (backward && !in.grad)) return "NULL plane or gradient pointer";
        if (((uintptr_t)in.t & 3) || ((uintptr_t)in.grad & 3)) return "planes and gradients must be 4-byte aligned";
        if (in.C < 1 || in.h < 1 || in.w < 1) return "C, h and w must be positive";
        if (in.kind < MOBGS_GRIDREG_SMOOTH || in.kind > MOBGS_GRIDREG_SMOOTH_L1) return "unknown term kind";
        const bool smooth = in.kind == MOBGS_GRIDREG_SMOOTH || in.kind == MOBGS_GRIDREG_SMOOTH_L1;
        if (smooth && in.h < 3) return "the smoothness term needs h >= 3 (the reference yields NaN there)";
        if (in.slot < 0 || in.slot + (in.kind == MOBGS_GRIDREG_SMOOTH_L1 ? 1 : 0) >= n_slots) return "slot outside the outputs";
        if (in.sc < 0 || in.sh < 0 || in.sw < 0) return "negative stride";
        if (!(in.inv0 >= 0.0) || !(in.inv1 >= 0.0)) return "a reciprocal count is negative or NaN";
        const bool cl = in.C == 1 || in.sc == 1, nchw = in.w == 1 || in.sw == 1;
        if (!cl && !nchw) return "a plane needs a unit-stride direction (sc == 1 or sw == 1)";
        const int64_t n = (int64_t)in.C * in.h * in.w;
        const int64_t extent = (int64_t)(in.C - 1) * in.sc + (int64_t)(in.h - 1) * in.sh + (int64_t)(in.w - 1) * in.sw;
        if (n >= ((int64_t)1 << 31) || extent >= ((int64_t)1 << 31)) return "a plane must span fewer than 2^31 elements";
        int64_t so, gso, gsh;
        p.flags = 0;
        if (cl) {
            const bool flat = in.w == 1 || in.sw == in.C;   // dense rows: one run of w C elements
            p.ni = flat ? in.C * in.w : in.C;
            p.no = flat ? 1 : in.w;
            so = flat ? 0 : in.sw;
            gso = flat ? 0 : in.C;
            gsh = (int64_t)in.C * in.w;
            p.ws = in.C;
            p.wd = flat ? in.C : (int32_t)in.sw;
            if (!flat) p.flags |= GR_F_W_OUTER;
        } else {
            p.ni = in.w;
            p.no = in.C;
            so = in.sc;
            gso = (int64_t)in.h * in.w;
            gsh = in.w;
            p.ws = p.wd = 1;
        }
        p.t = in.t;
        p.g = backward ? in.grad : nullptr;
        p.inv0 = in.inv0;
        p.inv1 = in.inv1;
        p.so = (int32_t)so;
        p.sh = (int32_t)in.sh;
        p.gso = (int32_t)gso;
        p.gsh = (int32_t)gsh;
        p.h = in.h;
        p.kind = in.kind;
        p.slot = in.slot;
        if (aligned(in.t, 16) && (p.no == 1 || so % GR_VEC == 0) && (in.h == 1 || in.sh % GR_VEC == 0)) p.flags |= GR_F_VEC_IN;
        if (backward && aligned(in.grad, 16) && (p.no == 1 || gso % GR_VEC == 0) && (in.h == 1 || gsh % GR_VEC == 0))
            p.flags |= GR_F_VEC_OUT;
        const int64_t units = (int64_t)p.no * ((p.ni + GR_VEC - 1) / GR_VEC);
        p.ncb = (int32_t)((units + GR_BLOCK - 1) / GR_BLOCK);
        p.first = (int32_t)first;
        first += (int64_t)p.ncb * ((in.h + GR_ROWS - 1) / GR_ROWS);
        if (first >= ((int64_t)1 << 30)) return "too many workgroups";
    }
    n_blocks = (int)first;
    return nullptr;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_gridreg_blocks(int n_planes, const MobgsGridPlane* planes_host, int n_slots) {
    GrTable tb;
    int nb = 0;
    return gr_build(n_planes, planes_host, n_slots, false, tb, nb) ? 0 : nb;
}

int mobgs_gridreg_fwd(int n_planes, const MobgsGridPlane* planes_host, int n_slots, const float* weights,
                      double* partial, float* out, float* total, void* stream) {
    GrTable tb;
    int nb = 0;
    if (const char* why = gr_build(n_planes, planes_host, n_slots, false, tb, nb)) {
        set_error("mobgs_gridreg_fwd: %s", why);
        return MOBGS_E_INVALID;
    }
    if (!partial || !out || !aligned(partial, 8) || !aligned(out, 4) || !aligned(weights, 4) || !aligned(total, 4)) {
        set_error("mobgs_gridreg_fwd: NULL or misaligned partial (8 bytes), out, weights or total (4 bytes)");
        return MOBGS_E_INVALID;
    }
    if ((weights == nullptr) != (total == nullptr)) {
        set_error("mobgs_gridreg_fwd: weights and total must both be given or both be NULL");
        return MOBGS_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gridreg_fwd_kernel, dim3((unsigned)nb), dim3(GR_BLOCK), 0, s, tb, partial);
    hipLaunchKernelGGL(gridreg_finish_kernel, dim3(1), dim3(GR_FIN_BLOCK), 0, s, tb, nb, (const double*)partial, weights, out,
                       total);
    return check_launch("mobgs_gridreg_fwd");
}

int mobgs_gridreg_bwd(int n_planes, const MobgsGridPlane* planes_host, int n_slots, const float* weights,
                      const float* v_out, void* stream) {
    GrTable tb;
    int nb = 0;
    if (const char* why = gr_build(n_planes, planes_host, n_slots, true, tb, nb)) {
        set_error("mobgs_gridreg_bwd: %s", why);
        return MOBGS_E_INVALID;
    }
    if (!v_out || !aligned(v_out, 4) || !aligned(weights, 4)) {
        set_error("mobgs_gridreg_bwd: NULL or misaligned v_out, or misaligned weights");
        return MOBGS_E_INVALID;
    }
    hipLaunchKernelGGL(gridreg_bwd_kernel, dim3((unsigned)nb), dim3(GR_BLOCK), 0, (hipStream_t)stream, tb, v_out, weights);
    return check_launch("mobgs_gridreg_bwd");
}

}  // extern "C"

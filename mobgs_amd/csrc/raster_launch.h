// Host side of the compositing launches (raster.hip, raster_bwd_mfma.hip, raster_layers.hip): which kernel a pass takes
// (ONE record, which mobgs_raster_path() packs and every launcher reads), the channel counts kernels exist for, the tile
// grid of a launch, and the pointer bundles the launchers hand on.  No device code: the kernels keep their flat
// parameter lists, the launch helpers below expand a bundle into them.
#pragma once
#include <type_traits>

#include "raster_shared.h"

namespace mobgs {

// ---------------------------------------------------------------------------------------------------
// channel counts
// ---------------------------------------------------------------------------------------------------
// Total channel counts the compositors are compiled for (compile-time accumulators); other counts are zero-padded by
// the host wrapper (rendering._SUPPORTED lists the same counts, tests/test_raster_plan_cpu.py ties the two).
#define MOBGS_RASTER_CHANNELS(X) X(1) X(2) X(3) X(4) X(9) X(10) X(12) X(16) X(26)

// f(std::integral_constant<int, D>) for a supported D
template <typename F>
inline int dispatch_channels(int D, F&& f) {
    switch (D) {
#define MOBGS_CHANNEL_CASE(CD) case CD: f(std::integral_constant<int, CD>{}); return MOBGS_OK;
        MOBGS_RASTER_CHANNELS(MOBGS_CHANNEL_CASE)
#undef MOBGS_CHANNEL_CASE
        default: return MOBGS_E_UNSUPPORTED;
    }
}
inline bool raster_channels_supported(int D) { return dispatch_channels(D, [](auto) {}) == MOBGS_OK; }

// The counts with more than the quadrant kernels (class_filter: the class-restricted passes, built for 1 and 10 channels
// only).  Written as ranges: of the supported counts they select 9, 10, 12 / 9, 10 / 1, 3, 4, 9, 10; a count outside
// the table is refused by dispatch_channels whatever these say.
// block-walk forward raster_fwd_blocks_kernel.  Measured (profiles/r03): the block walk wins where a pixel's blend is
// wide -- 10 channels 256 -> 218 us, 12 channels 280 -> 255 us -- and loses where the per-step bookkeeping dominates
// (1 channel 86 -> 90 us) or the accumulators leave two waves per SIMD (16 channels 313 -> 335 us)
constexpr bool has_fwd_blocks(int D, bool class_filter) { return class_filter ? D == 10 : (D >= 7 && D <= 12); }
// block-walk backward raster_bwd_blocks_kernel (plain passes only)
constexpr bool has_bwd_blocks(int D) { return D >= 7 && D <= 10; }
// matrix-pipe backward raster_bwd_mfma_kernel (<= 10 total channels)
constexpr bool has_bwd_mfma(int D, bool class_filter) {
    return D == 1 || D == 10 || (!class_filter && (D == 3 || D == 4 || D == 9));
}

// ---------------------------------------------------------------------------------------------------
// the plan: which kernels a pass takes
// ---------------------------------------------------------------------------------------------------
enum RasterBwdKernel {   // (the values are bits 0-1 of mobgs_raster_path)
    BWD_QUADRANT = 0,    // raster_bwd_kernel: per-lane accumulators + wave reduction
    BWD_MFMA = 1,        // raster_bwd_mfma_kernel, one wave per tile + the four-wave team for the schedule's heavy tiles
    BWD_MFMA_TEAM = 2,   // raster_bwd_mfma_kernel, the team for every tile
    BWD_BLOCKS = 3,      // raster_bwd_blocks_kernel
};
struct RasterPlan {
    int bwd;          // RasterBwdKernel
    bool fwd_blocks;  // forward: raster_fwd_blocks_kernel (the decoder epilogue exists only there), else raster_fwd_kernel
    int heavy_len;    // list length from which the schedule marks a tile heavy (0 = never)
    bool gate;        // the backward may arm the zero-cotangent gate (MobgsTuning.gate_zero_cotangent decides whether it does)
    bool mfma() const { return bwd == BWD_MFMA || bwd == BWD_MFMA_TEAM; }
};
// class_filter: 1 for mobgs_raster_class_fwd / _bwd.  The only reader of the three kernel-choice knobs.
inline RasterPlan raster_plan(int D, int class_filter, int n_tiles, const MobgsTuning* tuning) {
    // a plain pass under bwd_block_walk never takes the matrix pipe and never arms the gate, also at counts without a
    // block-walk build (those run the quadrant kernel); the class backward ignores the knob
    const bool bwd_blocks = !class_filter && tuning_bwd_block_walk(tuning);
    const int mfma = tuning_bwd_mfma(tuning, n_tiles);
    RasterPlan p;
    p.bwd = BWD_QUADRANT;
    if (bwd_blocks) {
        if (has_bwd_blocks(D)) p.bwd = BWD_BLOCKS;
    } else if (mfma && has_bwd_mfma(D, class_filter)) {
        p.bwd = mfma;
    }
    p.fwd_blocks = tuning_block_walk(tuning) && has_fwd_blocks(D, class_filter);
    p.heavy_len = tuning_heavy_len(tuning, n_tiles);
    p.gate = !bwd_blocks;
    return p;
}

// ---------------------------------------------------------------------------------------------------
// the grid of a launch
// ---------------------------------------------------------------------------------------------------
struct RasterGrid {
    int width, height;
    int tile_w, tile_h, tiles_per_image;
    int nt;        // tiles of all C images
    int n_groups;  // workgroups that hold a tile
    int grid;      // workgroups launched
};
// tiles_per_wg: TILES_PER_WG for the compositors, 2 for the layered kernels.  With a schedule (tile_order) one
// workgroup per tiles_per_wg schedule slots; without, n_groups rounded up to the 8 XCDs (xcd_chunked).
inline RasterGrid raster_grid(int C, int width, int height, const int32_t* tile_order, int tiles_per_wg) {
    RasterGrid g;
    g.width = width;
    g.height = height;
    g.tile_w = (width + MOBGS_TILE - 1) / MOBGS_TILE;
    g.tile_h = (height + MOBGS_TILE - 1) / MOBGS_TILE;
    g.tiles_per_image = g.tile_w * g.tile_h;
    g.nt = C * g.tiles_per_image;
    g.n_groups = (g.nt + tiles_per_wg - 1) / tiles_per_wg;
    g.grid = tile_order ? (int)((sched_slots((size_t)g.nt) + tiles_per_wg - 1) / tiles_per_wg) : ((g.n_groups + 7) / 8) * 8;
    return g;
}
inline int tiles_per_image(int width, int height) { return raster_grid(1, width, height, nullptr, TILES_PER_WG).tiles_per_image; }

// ---------------------------------------------------------------------------------------------------
// argument bundles and the launch helpers that expand them
// ---------------------------------------------------------------------------------------------------
struct RasterFwdArgs {
    const float *records, *backgrounds;
    const int32_t *tile_offsets, *tile_order, *flatten_ids;
    float *render, *alphas;
    int32_t* last_ids;
    uint8_t* isect_reach;
};
struct RasterBwdArgs {
    const float *records, *backgrounds;
    const int32_t *radii, *cum_tiles, *keep_scan, *tile_offsets, *tile_order, *flatten_ids;
    const float* render_alphas;
    const int32_t* last_ids;
    const float *v_render, *v_alphas;
    float* grad_slots;
    const uint8_t* isect_reach;
    int32_t* any_record;
};
// raster_fwd_kernel, raster_fwd_blocks_kernel.  tail: the DecodeEpi of the block-walk kernel
template <typename K, typename... Tail>
inline void launch_raster_fwd(K kernel, const RasterGrid& g, const RasterFwdArgs& a, hipStream_t st, const ClassSel& cls,
                              Tail... tail) {
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(64 * TILES_PER_WG), 0, st, g.nt, g.n_groups, g.tile_w, g.tile_h, g.width,
                       g.height, a.records, a.backgrounds, a.tile_offsets, a.flatten_ids, a.render, a.alphas, a.last_ids,
                       a.tile_order, cls, a.isect_reach, tail...);
}
// raster_bwd_kernel, raster_bwd_mfma_kernel, raster_bwd_blocks_kernel.  sel: the ClassSel (block walk: its all_reach
// alone); tail: the DecodeBwd of the quadrant kernel
template <typename K, typename Sel, typename... Tail>
inline void launch_raster_bwd(K kernel, const RasterGrid& g, const RasterBwdArgs& a, hipStream_t st, const Sel& sel,
                              Tail... tail) {
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(64 * TILES_PER_WG), 0, st, g.nt, g.n_groups, g.tile_w, g.tile_h, g.width,
                       g.height, a.records, a.backgrounds, a.radii, a.cum_tiles, a.keep_scan, a.tile_offsets, a.flatten_ids,
                       a.render_alphas, a.last_ids, a.v_render, a.v_alphas, a.grad_slots, a.tile_order, sel, a.isect_reach,
                       a.any_record, tail...);
}

// raster_bwd_mfma.hip: the matrix-pipe backward the plan chose (kernel = BWD_MFMA or BWD_MFMA_TEAM)
int raster_bwd_mfma_launch(int kernel, int D, bool class_filter, const RasterGrid& g, const RasterBwdArgs& a,
                           const ClassSel& cls, hipStream_t st);

}  // namespace mobgs

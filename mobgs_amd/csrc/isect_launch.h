// Host side of projection -> tile lists -> per-tile sort (project.hip, isect.hip, pipeline.hip): the geometry of a binning
// call and its guards (ONE record, BinGrid), the layout of the scratch buffer the stages share (IsectScratch), which
// bin_kernel / sort build a call takes, and the pointer bundles the launchers hand on.  No device code: the kernels keep
// their flat parameter lists, the launch helpers in isect.hip expand a grid and the bundles into them.
#pragma once
#include "common.h"

namespace mobgs {

// ---------------------------------------------------------------------------------------------------
// constants the layout and the choices below share with the kernels
// ---------------------------------------------------------------------------------------------------
// stride of the per-tile list counters (1 = packed; giving each counter its own 128-byte line was measured: no gain
// for the atomics of a dense image region, +12 us in tile_scan)
constexpr int TC_STRIDE = 1;
// The rank counters exist TC_COPIES times ([copy][tile]); workgroup (chunk) c of bin_kernel uses copy c mod TC_COPIES.
// Device-scope atomics on one address are served one after the other at the memory side of the chip (~120 ns each:
// the L2s of the eight XCDs are not coherent with each other); every tile counter receives one atomic from almost
// every chunk that touches the tile -- ~200 per counter at 300 k splats, 150 at 30 k -- and that queue was 42 % /
// 62 % of bin_kernel (ablated build: 59.1 -> 34.4 us, 29.8 -> 11.3 us).  With the copies a counter's queue is 8 x
// shorter; tile_scan_kernel sums the copies into the list lengths and leaves every (copy, tile) pair's first
// position in tile_base, which is what emit_kernel adds the rank to.  Ranks only have to be distinct inside a list.
constexpr int TC_COPIES = 8;
constexpr int DENSE_MAX_TILES = 8192;      // LDS-ranked bin_kernel: one int per tile, 32 KiB of LDS
constexpr int SHORT_SORT_LDS_KEYS = 2048;  // 16 KiB: longer lists belong to the long-list launch (or sort in global memory)
constexpr int LONG_SORT_LDS_KEYS = 16384;  // 128 KiB of the 160 KiB LDS: the radix sort of tile_sort_kernel<1024>

// ---------------------------------------------------------------------------------------------------
// the geometry of a binning call
// ---------------------------------------------------------------------------------------------------
struct BinGrid {
    int C, N, width, height;
    int capacity;  // of the bounding-box arena (capacity_box)
    int tile_w, tile_h, tiles_per_cam;
    int n;          // C * N splats
    int nt;         // tiles of all C cameras
    int tile_bits;  // gsplat: tile_n_bits = floor(log2(tiles per camera)) + 1
    int n_chunks;   // keep_scan chunks of the arena = workgroups of bin_kernel
    int nb1;        // workgroups of the scan over the n bounding-box counts (one per KEEP_CHUNK = SCAN_BLOCK elements)
    bool sizes_ok;  // C >= 1, N >= 0, capacity >= 1, n and nt below 2^31 - 1 (else n, nt and what follows mean nothing)
};
inline int scan_blocks(size_t n) { return (int)((n + KEEP_CHUNK - 1) / KEEP_CHUNK); }
// the standalone entry points name their tile counts; bin_grid() below derives them from the image
inline BinGrid bin_grid_tiles(int C, int N, int tile_w, int tile_h, int width, int height, int capacity) {
    const long long n = (long long)C * N, nt = (long long)C * tile_w * tile_h;
    BinGrid g;
    g.C = C, g.N = N, g.width = width, g.height = height, g.capacity = capacity;
    g.tile_w = tile_w, g.tile_h = tile_h, g.tiles_per_cam = tile_w * tile_h;
    g.sizes_ok = C > 0 && N >= 0 && capacity >= 1 && n < (1ll << 31) - 1 && nt < (1ll << 31) - 1;
    g.n = (int)n, g.nt = (int)nt;
    g.tile_bits = 0;
    while (g.tile_bits < 31 && (1ll << g.tile_bits) <= (long long)g.tiles_per_cam) ++g.tile_bits;
    g.n_chunks = (capacity >> KEEP_CHUNK_LOG2) + 1;
    g.nb1 = g.sizes_ok ? scan_blocks((size_t)n) : 0;
    return g;
}
inline BinGrid bin_grid(int C, int N, int width, int height, int capacity) {
    return bin_grid_tiles(C, N, (width + MOBGS_TILE - 1) / MOBGS_TILE, (height + MOBGS_TILE - 1) / MOBGS_TILE, width, height,
                          capacity);
}
// The guards of every binning launcher.  `who` is the entry point the message names; bin_grid_ok is the same predicate
// without a message (pipeline.hip: may the projection kernel clear the counters on its way?).
inline bool bin_grid_ok(const BinGrid& g, const void* scratch) { return g.sizes_ok && ((uintptr_t)scratch & 7) == 0; }
inline int bin_grid_check(const char* who, const BinGrid& g, const void* scratch) {
    if (!g.sizes_ok) {
        set_error("%s: bad sizes C=%d N=%d tiles=%dx%d capacity=%d", who, g.C, g.N, g.tile_w, g.tile_h, g.capacity);
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)scratch & 7) != 0) {
        set_error("%s: scratch must be 8-byte aligned", who);
        return MOBGS_E_INVALID;
    }
    return MOBGS_OK;
}
// ... and what the fused single-pass lists ask on top: every counter copy on its own 128-byte line, room for the bin
// records in the (owner, tile, rank) region (12 floats per splat + the alignment slack <= 3 * capacity ints), and box
// origin / width / camera in 16 bits each (write_bin_record)
inline bool bin_grid_fused_ok(const BinGrid& g, const void* scratch) {
    return bin_grid_ok(g, scratch) && g.N > 0 && ((uintptr_t)scratch & 127) == 0 && (long long)g.capacity >= 4ll * g.n + 2 &&
           g.tile_w <= 0xFFFF && g.tile_h <= 0xFFFF && g.C <= 0xFFFF;
}

// ---------------------------------------------------------------------------------------------------
// the scratch buffer shared by the binning stages
// ---------------------------------------------------------------------------------------------------
// Layout (int32 units; cap = capacity of the bounding-box arena, nt_pad = count_stride(nt) * TC_COPIES):
//   [tile_count nt_pad | tickets 4 | status1 2 * (nb1 + 1)]                       <- zeroed once per call
//   [owner cap | tile_of_j cap | rank_of_j cap | chunk_cnt (cap >> 11) + 1]       (fused path: the bin records lie in
//                                                                                  the first three, see bin_records())
//   [chunk_owner (cap >> 11) + 2 | tile_base nt * TC_COPIES | cum_enum n + 1]
inline size_t count_stride(size_t n_tiles) { return (n_tiles * TC_STRIDE + 31) & ~(size_t)31; }
struct IntSpan {
    int32_t* ptr;
    size_t count;
};
struct IsectScratch {
    int32_t *tile_count, *tickets, *chunk_cnt, *owner, *tile_of_j, *rank_of_j, *chunk_owner, *tile_base, *cum_enum;
    int owner_slots;
    uint64_t* status1;
    size_t zeroed_ints, total_ints;
    int nb1;
    IsectScratch(void* scratch, size_t n_gauss, size_t n_tiles, size_t capacity) {
        nb1 = scan_blocks(n_gauss);
        // every counter copy of the fused path starts on its own 128-byte line; the two-pass path packs its copies at the start
        const size_t nt_pad = count_stride(n_tiles) * TC_COPIES;  // (even: the 64-bit status words stay 8-byte aligned)
        int32_t* p = (int32_t*)scratch;
        tile_count = p;
        tickets = p + nt_pad;
        status1 = (uint64_t*)(p + nt_pad + 4);
        zeroed_ints = nt_pad + 4 + 2 * (size_t)(nb1 + 1);
        owner = p + zeroed_ints;
        tile_of_j = owner + capacity;
        rank_of_j = tile_of_j + capacity;
        chunk_cnt = rank_of_j + capacity;
        owner_slots = (int)(capacity >> KEEP_CHUNK_LOG2) + 2;
        chunk_owner = chunk_cnt + (capacity >> KEEP_CHUNK_LOG2) + 1;
        tile_base = chunk_owner + owner_slots;
        cum_enum = tile_base + n_tiles * TC_COPIES;  // [n_gauss + 1]: the scan in the caller's enumeration order (fused path)
        total_ints = zeroed_ints + 3 * capacity + (capacity >> KEEP_CHUNK_LOG2) + 1 + (size_t)owner_slots +
                     n_tiles * TC_COPIES + n_gauss + 1;
    }
    IsectScratch(const void* scratch, const BinGrid& g)
        : IsectScratch(const_cast<void*>(scratch), (size_t)g.n, (size_t)g.nt, (size_t)g.capacity) {}
    // tile counters, tickets, status words: what a call starts from zero
    IntSpan zeroed() const { return IntSpan{tile_count, zeroed_ints}; }
    // fused path: the (owner, tile, rank) triples of the two-pass path are not written, the projection kernel leaves its
    // bin records there (bin_grid_fused_ok holds the room); rows are read as float4
    float* bin_records() const { return reinterpret_cast<float*>(((uintptr_t)owner + 15) & ~(uintptr_t)15); }
};

// ---------------------------------------------------------------------------------------------------
// argument bundles
// ---------------------------------------------------------------------------------------------------
struct ProjectIn {
    const float *means, *quats, *scales, *viewmats, *Ks;
    const float* opacities;  // [N] or [C,N] (opac_per_camera); read by the reach test and the optional side jobs only
    int opac_per_camera;
    float eps2d, near_plane, far_plane, radius_clip;
    int cull;
    const MobgsPrepInputs* prep;  // non-NULL: means / quats / scales / opacities are OUTPUTS, built in the projection kernel
};
struct ProjectOut {
    int32_t* radii;
    float *means2d, *depths, *conics;
    int32_t* tiles_per_gauss;
};
struct ListsOut {
    int32_t *cum_tiles, *keep_scan, *tile_offsets, *tile_order;
    int64_t* stats_dev;  // {I_box, I_listed, longest list}
    void* scratch;       // IsectScratch
    int64_t capacity_listed;  // 0: not checked on the device (the synchronous form reads the counts first)
    int32_t* flatten_ids;
    uint64_t* keys;  // two-pass: [capacity_listed] sort keys; fused: the strided arena [nt][TC_COPIES][seg_stride]
    uint64_t* isect_ids;
};
struct Speculation {
    int64_t max_tile_len_hint;  // longest list the caller expects (the previous frame's)
    int64_t* stats_mirror;      // device-visible host address that receives a copy of stats_dev[0..2] (or NULL) ...
    int64_t stats_seq;          // ... and then, in word 3, this sequence number (when non-zero)
};
struct FusedLists {
    int seg_stride;  // keys per (tile, counter copy) segment; 0 = the two-pass lists
    const int32_t* enum_order;
};

// ---------------------------------------------------------------------------------------------------
// which kernels a call takes
// ---------------------------------------------------------------------------------------------------
// bin_kernel: tiles in the workgroup's LDS rank table, 0 = direct atomics on the global counters.
// Two-pass lists: the LDS-ranked variant whenever one int per tile fits in LDS -- measured faster at every grid size that
// qualifies (scripts/ab/sweep_dense.sh: 576 tiles 47 -> 33 us, 1100 tiles 48 -> 40, 2040 tiles 50 -> 46, 5440 tiles 66.6
// -> 65.3), several times faster on dense image regions (long lists); larger grids keep the direct atomics.
constexpr int bin_window_two_pass(int nt) { return nt <= DENSE_MAX_TILES ? nt : 0; }
// Fused lists: small grids (every workgroup touches most tiles several times) and scenes with long lists (dense image
// regions: thousands of atomics on a few counters); on a large grid with short lists the plain returning atomics are
// ahead (47.4 against 50.2 us at 5440 tiles / 300 k splats)
// ... and with a (spatially coherent) enumeration order, whose whole point is that a workgroup's intersections
// concentrate on few tiles
// ... or with splats STORED in such an order (MobgsTuning.coherent_order: the caller's statement)
// ... for a batch of cameras the table covers ONE camera's tiles (bin_kernel, dense_window)
constexpr int bin_window_fused(int nt, int tiles_per_cam, int64_t max_tile_len_hint, bool enum_order, bool coherent_order) {
    const int window = nt < tiles_per_cam ? nt : tiles_per_cam;
    return window <= DENSE_MAX_TILES && (nt <= 2048 || max_tile_len_hint >= 1024 || enum_order || coherent_order) ? window : 0;
}

// The per-tile depth sort.  Lists <= SHORT_SORT_LDS_KEYS (all of them unless longer ones are expected): ONE launch, four
// tiles per workgroup, a wave per list of <= 64 * epl entries (registers), the workgroup for the few longer ones (16 KiB
// LDS); three builds because the register count of the longest network sets the occupancy of all of them.  Longer lists,
// when the previous frame had any (split): 1024 threads, 128 KiB LDS (<= LONG_SORT_LDS_KEYS keys; beyond that in place
// in global memory), in a separate launch over a compacted list of those tiles, so that the short lists keep their
// occupancy.  Lists beyond the LDS radix sort (huge): chunks + merge passes (huge_chunk_sort_kernel) when the previous
// frame's longest list says they are near -- and the dead (owner, tile, rank) triples of pass A, 12 bytes per
// bounding-box intersection, can hold a second copy of the keys; otherwise such a list takes the one-workgroup network in
// global memory (correct, slow; the next frame's hint then selects this path).
struct SortPlan {
    int epl;           // keys per lane of the short-sort build: 8, 16 or 32
    bool split, huge;
    int merge_passes;  // (huge) enough for one list holding every listed intersection
};
constexpr int short_sort_epl(int64_t max_tile_len) { return max_tile_len > 1024 ? 32 : max_tile_len > 512 ? 16 : 8; }
// max_tile_len: the previous frame's longest list, or this frame's in the synchronous form; listed_cap: the most
// intersections the lists can hold
constexpr SortPlan sort_plan(int64_t max_tile_len, int64_t listed_cap, int64_t capacity_box) {
    SortPlan p{short_sort_epl(max_tile_len), max_tile_len > SHORT_SORT_LDS_KEYS, false, 0};
    p.huge = p.split && max_tile_len > (3 * (int64_t)LONG_SORT_LDS_KEYS) / 4 && 8 * listed_cap <= 12 * capacity_box;
    while (p.huge && ((int64_t)LONG_SORT_LDS_KEYS << p.merge_passes) < listed_cap) ++p.merge_passes;
    return p;
}
static_assert(sort_plan(512, 1, 1).epl == 8 && sort_plan(513, 1, 1).epl == 16, "short sort: 64 x 8 keys in registers");
static_assert(sort_plan(1024, 1, 1).epl == 16 && sort_plan(1025, 1, 1).epl == 32, "short sort: 64 x 16 keys in registers");
static_assert(!sort_plan(SHORT_SORT_LDS_KEYS, 1, 1).split && sort_plan(SHORT_SORT_LDS_KEYS + 1, 1, 1).split, "split");
static_assert(!sort_plan(12288, 12, 8).huge && sort_plan(12289, 12, 8).huge, "huge: from 3/4 of the LDS radix sort");
static_assert(!sort_plan(12288, 13, 8).huge && !sort_plan(12289, 13, 8).huge, "huge: only with room for the second copy");
static_assert(!sort_plan(12289, 12, 8).merge_passes && sort_plan(12289, 16384, 16384).merge_passes == 0, "merge passes");
static_assert(sort_plan(12289, 16385, 16384).merge_passes == 1 && sort_plan(12289, 2 * 16384, 32768).merge_passes == 1 &&
                  sort_plan(12289, 2 * 16384 + 1, 32768).merge_passes == 2, "merge passes");

// ---------------------------------------------------------------------------------------------------
// launchers shared between translation units (the orchestrator in pipeline.hip fuses small steps)
// ---------------------------------------------------------------------------------------------------
// project.hip: project_fwd, with the option to clear `zero` on the way (the binning scratch counters), to pack the
// compositor's records and to write the bin records of the fused lists.  Reads C, N, the image and the tile counts of
// `g` (and checks those itself: mobgs_project_fwd has no arena, so no BinGrid guard applies).
int project_fwd_launch(const BinGrid& g, const ProjectIn& in, const ProjectOut& out, IntSpan zero, PackArgs pack, BinArgs bin,
                       int geometry_per_camera, void* stream);
// isect.hip: mobgs_isect_offsets (scan -> bin -> offsets / schedule / counts); scratch_zeroed: the counters were cleared
// by the caller
int isect_offsets_launch(const BinGrid& g, const ProjectIn& in, const ProjectOut& po, const ListsOut& lo, const Speculation& sp,
                         bool scratch_zeroed, const MobgsTuning* tuning, void* stream);
// isect.hip: mobgs_isect_emit_sort (emit -> per-tile sort).  counts_on_device: the speculative form -- n_isects is
// unknown (pass 1), the kernels read lo.stats_dev and stay inside lo.capacity_listed
int emit_sort(const BinGrid& g, const ListsOut& lo, const float* depths, int64_t n_isects, int64_t max_tile_len,
              bool counts_on_device, void* stream);
// isect.hip: the fused single-pass lists: scan -> bin (keys straight into the strided segments) -> offsets / schedule /
// counts -> per-tile sort
int isect_fused_launch(const BinGrid& g, const ProjectOut& po, const ListsOut& lo, const Speculation& sp, const FusedLists& fl,
                       const MobgsTuning* tuning, void* stream);

}  // namespace mobgs

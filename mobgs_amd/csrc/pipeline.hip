// Native orchestration of the first half of a rasterization: projection -> intersection offsets (+ reach test)
// -> [one 24-byte read-back] -> emit -> per-tile depth sort, as ONE C call.
//
// The stages are the same entry points a caller can drive one by one (mobgs_project_fwd, mobgs_isect_offsets,
// mobgs_isect_emit_sort); doing it here removes the host gaps a Python driver leaves between ~12 short kernels
// (allocation + ctypes + launch, 10-40 us each while the GPU idles -- profiles/r01: 0.2 ms of a 1.9 ms step).
// Buffers whose size depends on the intersection count live in a caller-owned arena sized from the previous call;
// when it is too small the function returns MOBGS_E_CAPACITY with the required sizes in `stats_host` and has
// written nothing past the arena.
#include "isect_launch.h"

using namespace mobgs;

static const PackArgs NO_PACK{nullptr, nullptr, nullptr, 0, 0, 0, 0};
static const BinArgs NO_BIN_RECORDS{nullptr, nullptr, 0, 0};

// fl.seg_stride > 0: the fused single-pass lists (isect.hip, isect_fused_launch) -- lo.keys is then the strided key
// arena [C * n_tiles][8][seg_stride]; 0: the two-pass path.  pack.records == NULL: no packed records.
static int project_and_bin_enqueue(const BinGrid& g, const ProjectIn& in, const ProjectOut& po, const ListsOut& lo,
                                   const FusedLists& fl, int64_t max_tile_len_hint, int64_t* stats_host_pinned,
                                   int64_t stats_seq, PackArgs pack, const MobgsTuning* tuning, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!stats_host_pinned || lo.capacity_listed < 1) {
        set_error("mobgs_project_and_bin_speculative: stats_host_pinned and capacity_listed are required");
        return MOBGS_E_INVALID;
    }
    // two launches fewer on the critical path: project_fwd clears the binning counters on the way, and tile_scan
    // writes the host's copy of the counts itself when the pinned slot is mapped into the device address space
    const bool fuse_zero = bin_grid_ok(g, lo.scratch) && g.N > 0;
    const IntSpan zero = fuse_zero ? IsectScratch(lo.scratch, g).zeroed() : IntSpan{nullptr, 0};
    if (pack.records) {
        if ((!pack.colors && !in.prep) || !in.opacities || pack.channels < 0) {
            set_error("mobgs_project_and_bin_speculative: pack_records needs pack_colors and opacities");
            return MOBGS_E_INVALID;
        }
        pack.opacities = in.opacities;
        pack.opac_per_camera = in.opac_per_camera;
        pack.stride = mobgs_record_stride(pack.channels + 1);
    } else {
        pack = NO_PACK;
    }
    BinArgs bin = NO_BIN_RECORDS;
    if (fl.seg_stride > 0) {
        if (!bin_grid_fused_ok(g, lo.scratch) || !in.opacities) {
            set_error("mobgs_project_and_bin_fused: needs N > 0, opacities, a 128-byte aligned scratch and capacity_box >= 4 C N + 2");
            return MOBGS_E_INVALID;
        }
        bin = BinArgs{IsectScratch(lo.scratch, g).bin_records(), in.opacities, in.opac_per_camera, in.cull};
    }
    int rc = project_fwd_launch(g, in, po, zero, pack, bin, tuning_geometry_per_camera(tuning), stream);
    if (rc != MOBGS_OK) return rc;
    Speculation sp{.max_tile_len_hint = max_tile_len_hint};
    void* mirror = nullptr;
    if (hipHostGetDevicePointer(&mirror, stats_host_pinned, 0) != hipSuccess) {
        (void)hipGetLastError();
        mirror = nullptr;
    }
    sp.stats_mirror = (int64_t*)mirror;
    sp.stats_seq = mirror ? stats_seq : 0;
    // the binning variant follows the caller's expectation of the longest list (max_tile_len_hint)
    if (fl.seg_stride > 0)
        rc = isect_fused_launch(g, po, lo, sp, fl, tuning, stream);
    else
        rc = isect_offsets_launch(g, in, po, lo, sp, fuse_zero, tuning, stream);
    if (rc != MOBGS_OK) return rc;
    if (!sp.stats_mirror) {
        hipError_t e = hipMemcpyAsync(stats_host_pinned, lo.stats_dev, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            set_error("mobgs_project_and_bin_speculative: statistics copy failed: %s", hipGetErrorString(e));
            return MOBGS_E_LAUNCH;
        }
    }
    if (fl.seg_stride == 0) {
        rc = emit_sort(g, lo, po.depths, /*n_isects (unknown, > 0)*/ 1, max_tile_len_hint, /*counts_on_device=*/true, stream);
        if (rc != MOBGS_OK) return rc;
    }
    // 1: the counts travel by an ordinary asynchronous copy (or no sequence number was asked for) -- the caller
    // records an event behind this call and waits on it; 0: poll stats_host_pinned[3] for stats_seq instead
    return (sp.stats_mirror && stats_seq) ? MOBGS_OK : 1;
}

extern "C" {

int mobgs_project_and_bin(int C, int N, const float* means, const float* quats, const float* scales,
                          const float* viewmats, const float* Ks, const float* opacities, int opac_per_camera,
                          int width, int height, float eps2d, float near_plane, float far_plane, float radius_clip,
                          int cull, int32_t* radii, float* means2d, float* depths, float* conics,
                          int32_t* tiles_per_gauss, int32_t* cum_tiles, int32_t* tile_offsets, int32_t* tile_order,
                          int64_t* stats_dev,
                          int capacity_box, int32_t* keep_scan, void* scratch, int64_t capacity_listed,
                          int32_t* flatten_ids, uint64_t* sort_keys, uint64_t* isect_ids, int64_t* stats_host,
                          const MobgsTuning* tuning, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const BinGrid g = bin_grid(C, N, width, height, capacity_box);
    const ProjectIn in{.means = means, .quats = quats, .scales = scales, .viewmats = viewmats, .Ks = Ks,
                       .opacities = opacities, .opac_per_camera = opac_per_camera, .eps2d = eps2d,
                       .near_plane = near_plane, .far_plane = far_plane, .radius_clip = radius_clip, .cull = cull};
    const ProjectOut po{.radii = radii, .means2d = means2d, .depths = depths, .conics = conics,
                        .tiles_per_gauss = tiles_per_gauss};
    // (capacity_listed is checked on the host below, not on the device)
    const ListsOut lo{.cum_tiles = cum_tiles, .keep_scan = keep_scan, .tile_offsets = tile_offsets, .tile_order = tile_order,
                      .stats_dev = stats_dev, .scratch = scratch, .capacity_listed = 0, .flatten_ids = flatten_ids,
                      .keys = sort_keys, .isect_ids = isect_ids};
    int rc = project_fwd_launch(g, in, po, IntSpan{nullptr, 0}, NO_PACK, NO_BIN_RECORDS, tuning_geometry_per_camera(tuning),
                                stream);
    if (rc != MOBGS_OK) return rc;
    rc = isect_offsets_launch(g, in, po, lo, Speculation{}, /*scratch_zeroed=*/false, tuning, stream);
    if (rc != MOBGS_OK) return rc;
    // the pipeline's one host synchronisation (upstream gsplat has the same one): {I_box, I_listed, longest list}
    // (busy-polling hipStreamQuery instead of a blocking hipStreamSynchronize: the wait is ~0.2 ms at most and a
    // blocking wait adds ~30 us of wake-up latency during which the GPU idles)
    hipError_t e = hipMemcpyAsync(stats_host, stats_dev, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) {
        while ((e = hipStreamQuery(st)) == hipErrorNotReady) {
        }
    }
    if (e != hipSuccess) {
        set_error("mobgs_project_and_bin: statistics read-back failed: %s", hipGetErrorString(e));
        return MOBGS_E_LAUNCH;
    }
    if (stats_host[0] > (int64_t)capacity_box || stats_host[1] > capacity_listed) {
        set_error("mobgs_project_and_bin: arena too small (box %lld > %d or listed %lld > %lld)",
                  (long long)stats_host[0], capacity_box, (long long)stats_host[1], (long long)capacity_listed);
        return MOBGS_E_CAPACITY;
    }
    return emit_sort(g, lo, depths, stats_host[1], stats_host[2], /*counts_on_device=*/false, stream);
}

int mobgs_project_and_bin_speculative(int C, int N, const float* means, const float* quats, const float* scales,
                                      const float* viewmats, const float* Ks, const float* opacities,
                                      int opac_per_camera, int width, int height, float eps2d, float near_plane,
                                      float far_plane, float radius_clip, int cull, int32_t* radii, float* means2d,
                                      float* depths, float* conics, int32_t* tiles_per_gauss, int32_t* cum_tiles,
                                      int32_t* tile_offsets, int32_t* tile_order, int64_t* stats_dev,
                                      int capacity_box, int32_t* keep_scan, void* scratch, int64_t capacity_listed,
                                      int32_t* flatten_ids, uint64_t* sort_keys, uint64_t* isect_ids,
                                      int64_t max_tile_len_hint, int64_t* stats_host_pinned, int64_t stats_seq,
                                      const float* pack_colors, int colors_per_camera, int pack_channels,
                                      float* pack_records, const MobgsTuning* tuning, void* stream) {
    const ProjectIn in{.means = means, .quats = quats, .scales = scales, .viewmats = viewmats, .Ks = Ks,
                       .opacities = opacities, .opac_per_camera = opac_per_camera, .eps2d = eps2d,
                       .near_plane = near_plane, .far_plane = far_plane, .radius_clip = radius_clip, .cull = cull};
    const ProjectOut po{.radii = radii, .means2d = means2d, .depths = depths, .conics = conics,
                        .tiles_per_gauss = tiles_per_gauss};
    const ListsOut lo{.cum_tiles = cum_tiles, .keep_scan = keep_scan, .tile_offsets = tile_offsets, .tile_order = tile_order,
                      .stats_dev = stats_dev, .scratch = scratch, .capacity_listed = capacity_listed,
                      .flatten_ids = flatten_ids, .keys = sort_keys, .isect_ids = isect_ids};
    const PackArgs pack{.colors = pack_colors, .records = pack_records, .colors_per_camera = colors_per_camera,
                        .channels = pack_channels};
    return project_and_bin_enqueue(bin_grid(C, N, width, height, capacity_box), in, po, lo, FusedLists{0, nullptr},
                                   max_tile_len_hint, stats_host_pinned, stats_seq, pack, tuning, stream);
}

int mobgs_project_and_bin_fused(int C, int N, const float* means, const float* quats, const float* scales,
                                const float* viewmats, const float* Ks, const float* opacities, int opac_per_camera,
                                int width, int height, float eps2d, float near_plane, float far_plane,
                                float radius_clip, int cull, int32_t* radii, float* means2d, float* depths,
                                float* conics, int32_t* tiles_per_gauss, int32_t* cum_tiles, int32_t* tile_offsets,
                                int32_t* tile_order, int64_t* stats_dev, int capacity_box, int32_t* keep_scan,
                                void* scratch, int64_t capacity_listed, int32_t* flatten_ids, uint64_t* seg_keys,
                                int seg_stride, const int32_t* enum_order, uint64_t* isect_ids, int64_t max_tile_len_hint,
                                int64_t* stats_host_pinned, int64_t stats_seq, const float* pack_colors,
                                int colors_per_camera, int pack_channels, float* pack_records,
                                const MobgsTuning* tuning, void* stream) {
    if (seg_stride < 1 || !seg_keys) {
        set_error("mobgs_project_and_bin_fused: seg_stride >= 1 and seg_keys are required");
        return MOBGS_E_INVALID;
    }
    const ProjectIn in{.means = means, .quats = quats, .scales = scales, .viewmats = viewmats, .Ks = Ks,
                       .opacities = opacities, .opac_per_camera = opac_per_camera, .eps2d = eps2d,
                       .near_plane = near_plane, .far_plane = far_plane, .radius_clip = radius_clip, .cull = cull};
    const ProjectOut po{.radii = radii, .means2d = means2d, .depths = depths, .conics = conics,
                        .tiles_per_gauss = tiles_per_gauss};
    const ListsOut lo{.cum_tiles = cum_tiles, .keep_scan = keep_scan, .tile_offsets = tile_offsets, .tile_order = tile_order,
                      .stats_dev = stats_dev, .scratch = scratch, .capacity_listed = capacity_listed,
                      .flatten_ids = flatten_ids, .keys = seg_keys, .isect_ids = isect_ids};
    const PackArgs pack{.colors = pack_colors, .records = pack_records, .colors_per_camera = colors_per_camera,
                        .channels = pack_channels};
    return project_and_bin_enqueue(bin_grid(C, N, width, height, capacity_box), in, po, lo, FusedLists{seg_stride, enum_order},
                                   max_tile_len_hint, stats_host_pinned, stats_seq, pack, tuning, stream);
}

int mobgs_prep_project_and_bin_fused(const MobgsPrepInputs* prep, float* means, float* quats, float* scales,
                                     const float* viewmats, const float* Ks, float* opacities, int width, int height,
                                     float eps2d, float near_plane, float far_plane, float radius_clip, int cull,
                                     int32_t* radii, float* means2d, float* depths, float* conics,
                                     int32_t* tiles_per_gauss, int32_t* cum_tiles, int32_t* tile_offsets,
                                     int32_t* tile_order, int64_t* stats_dev, int capacity_box, int32_t* keep_scan,
                                     void* scratch, int64_t capacity_listed, int32_t* flatten_ids, uint64_t* seg_keys,
                                     int seg_stride, const int32_t* enum_order, uint64_t* isect_ids,
                                     int64_t max_tile_len_hint, int64_t* stats_host_pinned, int64_t stats_seq,
                                     float* pack_records, const MobgsTuning* tuning, void* stream) {
    if (!prep || !means || !quats || !scales || !opacities || !pack_records) {
        set_error("mobgs_prep_project_and_bin_fused: prep, the four state outputs and pack_records are required");
        return MOBGS_E_INVALID;
    }
    if (prep->Ns < 0 || prep->Nd < 0 || prep->Ns + prep->Nd < 1) {
        set_error("mobgs_prep_project_and_bin_fused: bad sizes Ns=%d Nd=%d", prep->Ns, prep->Nd);
        return MOBGS_E_INVALID;
    }
    const ProjectIn in{.means = means, .quats = quats, .scales = scales, .viewmats = viewmats, .Ks = Ks,
                       .opacities = opacities, .opac_per_camera = 0, .eps2d = eps2d, .near_plane = near_plane,
                       .far_plane = far_plane, .radius_clip = radius_clip, .cull = cull, .prep = prep};
    const ProjectOut po{.radii = radii, .means2d = means2d, .depths = depths, .conics = conics,
                        .tiles_per_gauss = tiles_per_gauss};
    const ListsOut lo{.cum_tiles = cum_tiles, .keep_scan = keep_scan, .tile_offsets = tile_offsets, .tile_order = tile_order,
                      .stats_dev = stats_dev, .scratch = scratch, .capacity_listed = capacity_listed,
                      .flatten_ids = flatten_ids, .keys = seg_keys, .isect_ids = isect_ids};
    // the colours are built in the projection kernel: 9 channels; seg_stride 0: the two-pass lists (first frame of a
    // workload, or the caller's choice)
    const PackArgs pack{.records = pack_records, .channels = 9};
    return project_and_bin_enqueue(bin_grid(1, prep->Ns + prep->Nd, width, height, capacity_box), in, po, lo,
                                   FusedLists{seg_stride, enum_order}, max_tile_len_hint, stats_host_pinned, stats_seq, pack,
                                   tuning, stream);
}

}  // extern "C"

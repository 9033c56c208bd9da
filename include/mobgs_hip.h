/*
 * mobgs_hip.h -- C ABI of libmobgs_hip.so, the MI355X (gfx950) Gaussian-splatting hot path for MoBGS.
 *
 * Boundary (level B3).  Each entry point replaces one stage of the third-party
 * gsplat==1.4.0 operator pipeline that the reference drives from
 *   /root/reference/gaussian_renderer/__init__.py:143-156   rasterization(...)        (and :163,201,236,255,274,
 *                                                                                       379,437,456,473,538)
 *   /root/reference/gaussian_renderer/__init__.py:190-199   fully_fused_projection(...) (and :411,422,513,524)
 * plus the reference's own per-Gaussian / per-pixel torch glue on the same path:
 *   /root/reference/gaussian_renderer/__init__.py:23-56     interpolate_cubic_hermite
 *   /root/reference/gaussian_renderer/__init__.py:93-125    time offset, rotation, colour feature build
 *   /root/reference/helper_model.py:19-28                   Sandwich colour decoder
 * and, either side of the path:
 *   /root/reference/scene/deformation.py, scene/hexplane.py deform_network (HexPlane + MLP heads)
 *   /root/reference/utils/loss_utils.py:233-239,351-381     L1 + SSIM
 *   /root/reference/main_utils.py:95-141                    normals from depth
 *   /root/reference/scene/gaussian_model.py:1044-1244,1352-1356,1480-1506   densification / optimiser surgery
 *   /root/reference/scene/gaussian_model.py:420,514         simple_knn distCUDA2 (initial scales)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every buffer (outputs and scratch); the library never allocates device memory; its only
 *     mutable state is the thread-local last-error string -- scheduling policy and testing switches travel with
 *     each call (MobgsTuning), so calls are re-entrant across streams, devices and threads;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no call synchronises, except
 *     mobgs_project_and_bin (one documented read-back);
 *   - return value: 0 on success, negative MOBGS_E_* on failure (mobgs_last_error() gives the text);
 *   - tensors are row-major contiguous float32 / int32 exactly as gsplat lays them out
 *     (means [N,3], quats [N,4] wxyz, scales [N,3], viewmats [C,4,4] world->camera, Ks [C,3,3],
 *      radii [C,N], means2d [C,N,2], depths [C,N], conics [C,N,3], colors [C,N,D] or [N,D],
 *      images [C,H,W,D], alphas [C,H,W]);
 *   - "tile" is a 16x16 pixel square (tile_size is fixed to 16 in this build, as every reference call site
 *     uses gsplat's default); tiles are numbered cam*tile_h*tile_w + ty*tile_w + tx.
 */
#ifndef MOBGS_HIP_H
#define MOBGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBGS_OK 0
#define MOBGS_E_INVALID (-1)   /* bad argument (size, channel count, null pointer)            */
#define MOBGS_E_LAUNCH (-2)    /* hipLaunchKernel / hipMemsetAsync reported an error           */
#define MOBGS_E_UNSUPPORTED (-3)
#define MOBGS_E_CAPACITY (-4)   /* a caller-owned arena is too small; required sizes were reported         */

#define MOBGS_TILE 16
#define MOBGS_MAX_CHANNELS 32

/* Library identification.  Returns e.g. "mobgs_hip 0.2 gfx950". */
/* Per-call policy of the binning / compositing entry points.  The library keeps NO mutable state: what used to be
 * process-wide setters travels with each call (host pointer, may be NULL = all defaults; a negative field = default).
 *   heavy_tile_len     scheduling: a tile whose list has at least this many entries is composited by a whole
 *                      workgroup, one 8x8 quadrant per wave -- for at most an eighth of the tiles, or all of them
 *                      on grids of <= 1024 tiles (small images cannot fill the chip with one wave per tile).
 *                      Default 1024 (1 on grids of <= 1024 tiles); 0 = never.
 *   longest_list_hint  the longest per-tile list the caller expects (e.g. the previous frame's stats[2]).  Accepted
 *                      for compatibility: mobgs_isect_offsets now ranks through LDS on every grid of <= 8192 tiles
 *                      (it used to do so only with a hint >= 2048).  Default 0.
 *   quadrant_culling   testing aid, default 1: the compositors skip, per list entry, the 8x8 quadrants of the tile
 *                      the splat cannot reach (work that is predicated off at every pixel); 0 evaluates everything
 *                      -- results are identical.
 *   block_walk         forward compositor of the plain passes with <= 10 total channels, default 1: sixteen
 *                      independent 4x4-pixel workers per wave, each walking the entries that can reach ITS block
 *                      (raster.hip, "block-walk formulation"); 0 = the one-entry-at-a-time quadrant kernel.  Images,
 *                      alphas and last_ids are bit-identical either way.
 *   bwd_block_walk     experimental, default 0: 1 runs the same sixteen-worker formulation in the backward pass of the
 *                      7..10-channel plain passes (partial gradient records of the blocks combined in an LDS accumulator
 *                      under an integer claim).  Measured 9 % SLOWER than the quadrant kernel on the benchmark lists
 *                       -- kept as the A/B arm; gradients agree to summation order.
 *   geometry_per_camera  layout flag of mobgs_project_and_bin / _speculative (round 3), default 0: 1 = `means` is
 *                      [C,N,3] and `quats` [C,N,4] -- every camera sees its OWN positions / rotations of the N splats
 *                      (the K sub-frames of one blurry view: same Gaussians at K exposure times through K cameras,
 *                      projected, binned, sorted and composited as ONE C = K batch); scales / opacities stay [N,..].
 *   bwd_mfma           backward compositor of the passes with <= 10 total channels (round 4): the per-splat gradient
 *                      sums on the matrix pipe (raster_bwd_mfma.hip: the pair weights alpha*T and v_sigma are transposed
 *                      through LDS and summed over the pixels by v_mfma_f32_16x16x4_f32 against [colour cotangents |
 *                      pixel moments]; no per-entry wave reduction).  0 = OFF (the quadrant kernel with per-lane accumulators) -- NOT "default": a
 *                      zero-initialised struct selects the quadrant kernel on every grid, only a negative value defers to the library;
 *                      1 = one wave per tile, the four-wave team (one 8x8 quadrant per wave) for the schedule's heavy
 *                      tiles; 2 = the team for every tile.  Gradients agree to summation order (observed <= 2e-5 of
 *                      each tensor's maximum).  Default (-1): 1 on grids of <= 1024 tiles, else 0 (measured).
 *   gate_zero_cotangent  (round 5; was `reserved`) backward compositing passes, default 0 / -1 = off.  1: mobgs_raster_bwd
 *                      and mobgs_raster_class_bwd first ask, on the device, whether ANY element of v_render / v_alphas
 *                      is non-zero (one streaming kernel that stops at the first hit; NaN counts as non-zero).  If none
 *                      is, the compositing kernel returns at once, no gradient record is written, any_record stays 0
 *                      and mobgs_raster_bwd_reduce writes exact zeros without reading a slot: a loss term whose weight
 *                      is 0 (/root/reference/train.py:675 with arguments/stereo/seesaw.py lambda_flow_loss = 0) then
 *                      costs a probe instead of a backward pass.  No host synchronisation (HIP-graph safe).  Contract
 *                      in this mode: `any_record` points at TWO zeroed int32 words (the second is the gate; the usual
 *                      zero fill of grad_slots + the extra row behind them provides both).  One extra kernel launch per
 *                      call.  Ignored (treated as 0) with bwd_block_walk = 1.
 *   coherent_order     (round 5) mobgs_project_and_bin_fused, default 0 / -1 = unknown.  1: the caller states that the
 *                      splats are STORED in a spatially coherent order (neighbouring rows are neighbours in space, e.g.
 *                      rows along a Morton curve: mobgs_amd GaussianParams.spatial_sort_(), kept by TrainableGaussians
 *                      after every densification) -- the binning kernel then ranks through LDS on grids of up to 8192
 *                      tiles, as it does with an enum_order, without the order's indirection (measured at 300 k splats,
 *                      1352x1014: bin 49.6 -> 29.9 us; against an enum_order: scan 12.5 -> 7.1 us, slot reduction
 *                      38.9 -> 35.4 us).  A performance hint only: a wrong statement costs time, never correctness.
 *   static_rows        (round 6) mobgs_raster_bwd / mobgs_raster_class_bwd with 10 or 12 total channels, default 0 / -1 =
 *                      none.  S > 0: the caller states that the splats with (flat id % N) < S are MoBGS's STATIC set --
 *                      colour features cat(f_dc, 0.0 * f_t) (/root/reference/scene/gaussian_model.py:244-246; in
 *                      get_flow()'s 12-channel pass also a flow of exactly 0, gaussian_renderer/__init__.py:436-476) --
 *                      i.e. channels 6..8 (10 channels) / 6..10 (12 channels) of those rows are zero AND their gradient
 *                      is not wanted (the reference multiplies it by 0.0).  The backward compositor then runs a blend body
 *                      without those channels for such entries (one wave-uniform branch per list entry; 6 / 10 of ~50 VALU
 *                      per evaluated 8x8 quadrant) and v_colors[.., 6..] of those rows is written as 0.  Every other
 *                      output is BIT-identical (fma(0, v, acc) = acc).  The zeros are verified per staged entry (an entry
 *                      whose dead channels are not all +-0 takes the full body): a wrong statement about the DATA costs
 *                      nothing; a caller that does want d/d(colour 6..8) of such rows must leave this at 0.  Only
 *                      the quadrant kernel has such a body: the matrix-pipe (bwd_mfma) and block-walk kernels ignore the
 *                      field, and mobgs_amd's compositing nodes write the zeros themselves after the reduction, for every static
 *                      row (also one whose dead channels are not zero, where the quadrant kernel returns the gradient).
 *   cover_slots        (round 6) mobgs_raster_bwd / mobgs_raster_bwd_decode, default 0 / -1 = off.  1: the caller did NOT
 *                      zero-fill grad_slots (108 MB at 1352x1014 / 300 k splats: a 15-us fill per render, 9 of them per
 *                      blurry view) -- the kernel writes the slot of EVERY entry of its lists, zeros where no pixel blended
 *                      the splat (entries behind every pixel's last blended one included), so mobgs_raster_bwd_reduce
 *                      sums exactly what it would have; stage 1 takes any_record = NULL then (the flag would live in unwritten
 *                      memory), stage 2 takes as its any_record the address of tile_offsets[n_tiles] -- the lists' total, 0
 *                      when a speculative binning call overflowed an arena and emptied the lists: without a host in the
 *                      loop (a HIP-graph replay) keep_scan and the slot ranges of such a frame must not be read.  Honoured only where the quadrant kernel runs ((mobgs_raster_path(D, 0, n_tiles,
 *                      tuning) & 3) == 0; other selections return MOBGS_E_UNSUPPORTED) and not together with
 *                      gate_zero_cotangent (a gated-off pass writes nothing).  Gradients are bit-identical. */
typedef struct MobgsTuning {
    int32_t heavy_tile_len;
    int32_t longest_list_hint;
    int32_t quadrant_culling;
    int32_t block_walk;
    int32_t bwd_block_walk;
    int32_t geometry_per_camera;
    int32_t bwd_mfma;
    int32_t gate_zero_cotangent;
    int32_t coherent_order;
    int32_t static_rows;
    int32_t cover_slots;
} MobgsTuning;

const char* mobgs_version(void);
/* Is any element of any of `n_arrays` float arrays (device pointers in the HOST array `arrays`, element counts in
 * `counts`) non-zero?  -> *live (device int32) = 1 if so, else 0; NaN counts as non-zero, -0.0 as zero.  Streams every
 * array once when all are zero, stops at the first hit otherwise.  The device-side form of "is this loss term's weight
 * zero" (MobgsTuning.gate_zero_cotangent uses the same kernel for one pass; mobgs_amd.gaussian_renderer reads *live on
 * the host to drop the whole backward graph of a view's get_flow() calls, /root/reference/train.py:570-579, :675). */
int mobgs_cotangent_probe(int n_arrays, const float* const* arrays, const size_t* counts, int32_t* live, void* stream);
/* Integer that changes whenever a signature, a struct layout or the format of a scratch buffer handed between entry
 * points changes (round 4 inserted `records` into mobgs_raster_bwd_reduce and changed the gradient-slot format without
 * one: a stale host extension would have passed shifted pointers).  Bindings compare it with the MOBGS_ABI_VERSION
 * they were built against and refuse to run on a mismatch (mobgs_amd/_lib.py, csrc/fastpath.cpp). */
#define MOBGS_ABI_VERSION 16
int mobgs_abi_version(void);
/* Text of the last error raised on the calling thread ("" if none). */
const char* mobgs_last_error(void);

/* Number of floats in one packed splat record / gradient slot for `channels` colour channels:
 * {x, y, conic_a, conic_b, conic_c, opacity, colour[channels]} rounded up to a multiple of 4. */
int mobgs_record_stride(int channels);

/* ---- K1: projection forward (replaces gsplat fully_fused_projection fwd) -------------------------------
 * Also emits tiles_per_gauss[C,N] (number of 16x16 tiles the 3-sigma box touches; 0 when culled), which
 * gsplat computes in isect_tiles' first pass.  Culled entries get radii=0 and zeros in the other outputs. */
int mobgs_project_fwd(int C, int N, const float* means, const float* quats, const float* scales,
                      const float* viewmats, const float* Ks, int width, int height, float eps2d,
                      float near_plane, float far_plane, float radius_clip, int32_t* radii,
                      float* means2d, float* depths, float* conics, int32_t* tiles_per_gauss,
                      void* stream);

/* ---- K2: projection backward (replaces gsplat fully_fused_projection bwd, incl. v_viewmats) ------------
 * v_viewmats_partial: scratch [ceil(C*N/256), 16] floats; v_viewmats [C,4,4] is fully written.
 * v_means/v_quats/v_scales are [N,3]/[N,4]/[N,3], summed over cameras, fully written by the call.
 * geometry_per_camera (see MobgsTuning) = 1: means / v_means [C,N,3] and quats / v_quats [C,N,4] (every camera's rows
 * written once, nothing summed over cameras), v_scales [N,3] summed over cameras.
 * Any of v_means2d / v_depths / v_conics may be NULL (treated as zeros). */
size_t mobgs_project_bwd_scratch_floats(int C, int N);
int mobgs_project_bwd(int C, int N, int geometry_per_camera, const float* means, const float* quats,
                      const float* scales, const float* viewmats, const float* Ks, int width, int height,
                      float eps2d, const int32_t* radii, const float* conics, const float* v_means2d,
                      const float* v_depths, const float* v_conics, float* v_means, float* v_quats,
                      float* v_scales, float* v_viewmats, float* v_viewmats_partial, void* stream);
/* Projection backward + prep backward of ONE camera in one launch (round 5; the backward half of
 * mobgs_prep_project_and_bin_fused): what mobgs_project_bwd would store as v_means / v_quats / v_scales stays in the
 * thread's registers and goes through the arithmetic of mobgs_prep_bwd (bit for bit) to the 13 leaf gradients.
 * x_means / x_quats / x_scales (each may be NULL): cotangents that reach the activated state directly, added first.
 * v_opacities / v_colors (may be NULL): as mobgs_prep_bwd.  accumulate: as mobgs_prep_bwd.  v_viewmats [4,4] is fully
 * written (scratch v_viewmats_partial: mobgs_project_bwd_scratch_floats(1, N) floats); v_viewmats = NULL: the pose needs no
 * gradient (the training loop never optimises it; eval.py's test-time pose optimisation does) -- the per-workgroup partial
 * rows and the reduction launch are skipped.  float32 leaves only.
 * MobgsLeafGrads: the 13 leaf-gradient buffers (device pointers; a host struct, read before the call returns).  s_xyz and
 * d_control are float32; the eleven attribute members are float32 -- or IEEE binary16 where mobgs_prep_bwd is called with
 * grad_half = 1. */
typedef struct MobgsLeafGrads {
    float* s_xyz;
    void *s_scaling, *s_rotation, *s_opacity, *s_fdc, *s_ft;
    float* d_control;
    void *d_scaling, *d_rotation, *d_omega, *d_opacity, *d_fdc, *d_ft;
} MobgsLeafGrads;
int mobgs_project_prep_bwd_fused(int N, const float* means, const float* quats, const float* scales,
                                 const float* viewmats, const float* Ks, int width, int height, float eps2d,
                                 const int32_t* radii, const float* conics, const float* v_means2d,
                                 const float* v_depths, const float* v_conics, const float* x_means,
                                 const float* x_quats, const float* x_scales, float* v_viewmats,
                                 float* v_viewmats_partial, int Ns, int Nd, const float* times, const int64_t* d_ncp,
                                 const float* d_trbf, const float* opacities, const float* v_opacities,
                                 const float* v_colors, const MobgsLeafGrads* grads, int accumulate, void* stream);


/* ---- K3a: intersection offsets (replaces isect_tiles pass 1 + cumsum + isect_offset_encode) ------------
 * in : tiles_per_gauss [C*N] (bounding-box tile counts from mobgs_project_fwd), means2d, radii, conics,
 *      opacities ([C,N] when opac_per_camera else [N])
 * cull = 0: every bounding-box intersection is listed -- exactly upstream's lists.
 * cull = 1: a (tile, splat) pair is listed only if the splat can reach alpha >= 1/255 somewhere on the tile's
 *      pixel rectangle (min over the rectangle of sigma <= ln(255*opacity), conservative margin).  Pairs that
 *      fail are skipped by the compositor at all 256 pixels anyway, so every output pixel is bit-identical and every
 *      gradient keeps exactly its non-zero terms; lists, sort and gradient slots shrink (about 2x on anisotropic scenes).
 * out: cum_tiles [C*N+1] exclusive prefix sum of the BOX counts (cum_tiles[C*N] = I_box)
 *      keep_scan [mobgs_keep_scan_len(capacity)] exclusive prefix sum of the keep flags over the box
 *                intersections, stored in chunks of 2048 intersections, each preceded by one base word:
 *                chunk c = [base_c | local_0 .. local_2047], local_i = kept intersections before i inside the
 *                chunk, base_c = kept intersections in all earlier chunks.  The compact index of box intersection
 *                j (= its gradient slot in mobgs_raster_bwd) is
 *                    keep_scan[(j >> 11) * 2049] + keep_scan[(j >> 11) * 2049 + 1 + (j & 2047)],
 *                defined for 0 <= j <= min(I_box, capacity).
 *      tile_offsets [C*n_tiles+1] exclusive prefix sum of the per-tile list lengths
 *      tile_order [mobgs_tile_order_len(C*n_tiles)] (may be NULL) the schedule of the compositing kernels, 4
 *                slots per workgroup: tile ids by descending list length (1024 length classes; longest lists
 *                first, lists of similar length share a workgroup), -1 = unused slot.  Tiles whose list is at
 *                least MobgsTuning.heavy_tile_len long (capped, see there) appear as id | 1<<30 in
 *                the 4 slots of one workgroup, whose 4 waves then composite one 8x8 quadrant each.  A schedule
 *                only -- images do not depend on it; the compositing entry points accept NULL for raster order.
 *      stats int64[3] = {I_box, I_listed, longest per-tile list}; the caller reads them back to size the list
 *      buffers (the one host sync of the pipeline, as in gsplat).  If I_box > capacity the flags were
 *      truncated: call again with capacity >= I_box.
 * capacity_listed > 0 (speculative callers, see mobgs_isect_emit_sort_speculative): when I_box > capacity or
 *      I_listed > capacity_listed, tile_offsets is written as all zeros (every list empty) so that consumers
 *      already enqueued behind this call touch nothing; stats still hold the true counts.  <= 0: no such check.
 * scratch: mobgs_isect_scratch_bytes(C*N, C*n_tiles, capacity) bytes. */
size_t mobgs_isect_scratch_bytes(int n_gauss, int n_tiles, int capacity);
size_t mobgs_tile_order_len(int n_tiles);  /* int32 entries of tile_order */
size_t mobgs_keep_scan_len(int capacity); /* int32 entries of keep_scan for `capacity` box intersections */
int mobgs_isect_offsets(int C, int N, int tile_w, int tile_h, int width, int height, int cull, int capacity,
                        const int32_t* tiles_per_gauss, const float* means2d, const int32_t* radii,
                        const float* conics, const float* opacities, int opac_per_camera,
                        int32_t* cum_tiles, int32_t* keep_scan, int32_t* tile_offsets, int32_t* tile_order,
                        int64_t capacity_listed, int64_t* stats, void* scratch, const MobgsTuning* tuning,
                        void* stream);

/* ---- K3b/K4: emit + per-tile depth sort (replaces isect_tiles pass 2 + CUB DeviceRadixSort) ------------
 * Writes, per tile, its listed splats ordered by (float depth bits ascending, flat id ascending) -- the order a
 * stable LSD radix sort on gsplat's 64-bit key produces.
 * n_isects = stats[1], max_tile_len = stats[2] of mobgs_isect_offsets (lists longer than 4096 get a second launch
 * of the 1024-thread / 128-KiB-LDS sort variant over a compacted list of those tiles).
 * out: flatten_ids [n_isects] (cam*N+gaussian), isect_ids [n_isects] (gsplat's u64 key; may be NULL)
 * offsets_scratch: the SAME scratch buffer (and capacity) that was passed to mobgs_isect_offsets -- it holds the
 *   (flag, owner, tile, rank) of every bounding-box intersection (its dead per-tile counters are reused as
 *   scratch, so one call per mobgs_isect_offsets call); sort_keys [n_isects] u64 is scratch. */
int mobgs_isect_emit_sort(int C, int N, int tile_w, int tile_h, int capacity, int64_t n_isects,
                          int64_t max_tile_len, const float* depths, const int32_t* cum_tiles,
                          const int32_t* tile_offsets, const void* offsets_scratch, uint64_t* sort_keys,
                          int32_t* flatten_ids, uint64_t* isect_ids, void* stream);

/* The same stage enqueued BEFORE the counts are known on the host: the kernels read them from stats_dev (the
 * buffer mobgs_isect_offsets filled, called with the same capacity / capacity_listed) and do nothing when the
 * arena is too small.  max_tile_len_hint only selects the sort variant (any list length sorts correctly with
 * either; pass the previous frame's longest list).  sort_keys / flatten_ids / isect_ids hold capacity_listed
 * entries. */
int mobgs_isect_emit_sort_speculative(int C, int N, int tile_w, int tile_h, int capacity, int64_t capacity_listed,
                                      int64_t max_tile_len_hint, const float* depths, const int32_t* cum_tiles,
                                      const int32_t* tile_offsets, const int64_t* stats_dev,
                                      const void* offsets_scratch, uint64_t* sort_keys, int32_t* flatten_ids,
                                      uint64_t* isect_ids, void* stream);

/* ---- K1 + K3-K5 in one call: projection -> offsets (+ reach test) -> read-back -> emit -> per-tile sort ------
 * Same stages and buffers as mobgs_project_fwd + mobgs_isect_offsets + mobgs_isect_emit_sort, driven natively so
 * that no host gap separates the ~12 short kernels.  Arena: keep_scan [mobgs_keep_scan_len(capacity_box)], scratch
 * (mobgs_isect_scratch_bytes(C*N, C*n_tiles, capacity_box)), flatten_ids [capacity_listed], sort_keys
 * [capacity_listed], isect_ids [capacity_listed] or NULL.  stats_dev: 3 x int64 device scratch; stats_host: 3 x int64
 * HOST output {I_box, I_listed, longest list}.  Returns MOBGS_E_CAPACITY (stats_host valid, nothing written past
 * the arena) when I_box > capacity_box or I_listed > capacity_listed: grow and call again.  This function
 * synchronises `stream` once (the intersection-count read-back that upstream gsplat also performs). */
int mobgs_project_and_bin(int C, int N, const float* means, const float* quats, const float* scales,
                          const float* viewmats, const float* Ks, const float* opacities, int opac_per_camera,
                          int width, int height, float eps2d, float near_plane, float far_plane,
                          float radius_clip, int cull, int32_t* radii, float* means2d, float* depths,
                          float* conics, int32_t* tiles_per_gauss, int32_t* cum_tiles, int32_t* tile_offsets,
                          int32_t* tile_order, int64_t* stats_dev, int capacity_box, int32_t* keep_scan, void* scratch,
                          int64_t capacity_listed, int32_t* flatten_ids, uint64_t* sort_keys, uint64_t* isect_ids,
                          int64_t* stats_host, const MobgsTuning* tuning, void* stream);

/* mobgs_project_and_bin WITHOUT the host synchronisation: every stage is enqueued, the three counts are copied
 * asynchronously into stats_host_pinned (page-locked host memory, valid once the caller has waited on an event
 * recorded after this call) and the function returns.  When the arena turns out too small (counts exceed
 * capacity_box / capacity_listed) every per-tile list was written EMPTY: compositing kernels enqueued in the
 * meantime are harmless no-ops, and the caller redoes the binning with a larger arena (mobgs_isect_offsets +
 * mobgs_isect_emit_sort on the projection outputs, which do not depend on the arena).
 * stats_host_pinned holds FOUR words: {I_box, I_listed, longest list, sequence}.  With stats_seq != 0 and a pinned
 * buffer that is mapped into the device address space, the last binning kernel stores the three counts and then
 * stats_seq into word 3 (system-scope release): the caller clears word 3 beforehand and simply polls it -- no event,
 * hence no marker packet between the binning and the compositing kernels.  Return value 0 says so; 1 means the
 * counts travel by an asynchronous copy and the caller waits on an event recorded after this call, as before.
 * pack_records (optional, else NULL): [C*N, mobgs_record_stride(pack_channels + 1)] -- the projection kernel also
 * writes the compositor's packed records {means2d, conic, opacity, pack_colors, depth as the extra channel} of the
 * visible splats (what mobgs_pack_records / mobgs_raster_fwd would do in a launch of its own); hand them to
 * mobgs_raster_fwd with colors = NULL.  pack_colors: [C,N,ch] (colors_per_camera = 1) or [N,ch]. */
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
                                      float* pack_records, const MobgsTuning* tuning, void* stream);

/* mobgs_project_and_bin_speculative with SINGLE-PASS lists (round 5).  The two-pass form ranks every kept intersection,
 * scans the per-tile counts, and only then scatters the sort keys (scan -> bin -> tile_scan -> emit -> sort, with a
 * second pass over the kept intersections in between).  Here the projection kernel also leaves one 48-byte "bin
 * record" per visible splat inside `scratch`, the binning kernel reads that one row per intersection and writes each
 * kept intersection's 64-bit key STRAIGHT into its tile's segment of a strided arena,
 *     seg_keys [C * n_tiles][8][seg_stride] u64   (mobgs_fused_seg_keys_len(C * n_tiles, seg_stride) entries; the 8
 *                                                  counter copies of the binning kernel each own a sub-segment),
 * and the per-tile sort reads the segments and writes flatten_ids / isect_ids PACKED at tile_offsets -- every output
 * is identical to the two-pass path's (same lists, same order, same keep_scan / cum_tiles / tile_order semantics).
 * seg_stride: capacity of a tile's list, 1 .. mobgs_fused_max_seg_stride(); the caller sizes it from the longest list
 * it expects (the previous frame's stats[2] plus slack).  A tile whose list is longer makes the call behave like an
 * arena overflow: every list is written EMPTY, stats still hold the true counts (stats[2] > seg_stride tells), and
 * the caller redoes the binning with the two-pass entry points.  Requires N > 0, capacity_box >= 4 C N + 2 and a
 * 128-byte aligned scratch.  Everything else as mobgs_project_and_bin_speculative (including the return value).
 * enum_order (optional, else NULL): [C*N] int32, a PERMUTATION of the flat splat ids 0 .. C*N-1 -- the order in which the
 *   splats' bounding-box intersections are enumerated (cum_tiles / keep_scan / gradient-slot numbering).  Any permutation
 *   gives the same lists, images and gradients (each splat's intersections stay consecutive and in the same order); a
 *   SPATIALLY COHERENT one (e.g. a Morton order of the positions, recomputed now and then by the caller) makes
 *   neighbouring intersections hit neighbouring tiles, so the binning kernel ranks them in LDS and issues an order of
 *   magnitude fewer returning atomics (48 -> 27 us at 300 k splats).  With a permutation cum_tiles[g + 1] is no longer
 *   the END of splat g's intersections: pass tiles_per_gauss to mobgs_raster_bwd_reduce / mobgs_raster_layers_bwd. */
size_t mobgs_fused_seg_keys_len(int n_tiles, int seg_stride);
int mobgs_fused_max_seg_stride(void);
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
                                const MobgsTuning* tuning, void* stream);
/* The same call with the per-splat state built INSIDE the projection kernel (round 5): what
 * mobgs_prep_fwd computes from the raw parameters of the two sets -- /root/reference/gaussian_renderer/__init__.py:93-125,
 * :181-185 (spline position, rotation + t * omega, exp / sigmoid activations, colour features) -- is evaluated by the
 * thread that projects the splat, bit for bit the arithmetic of mobgs_prep_fwd, so the activated state is not written
 * by one launch and read back by the next.  One camera (C = 1), float attributes, N = prep->Ns + prep->Nd.
 * `means` [N,3], `quats` [N,4], `scales` [N,3] and `opacities` [N] are OUTPUTS here (the backward pass and the caller's
 * result dict need them); the 9 colour features only exist inside `pack_records` (stride mobgs_record_stride(10): the
 * depth is the tenth channel), which is required.
 * MobgsPrepInputs: the raw parameters of the two sets (see K8, mobgs_prep_fwd).  A host struct, read before the call
 * returns; all pointers in it are device pointers.  The eleven attribute members are float32 -- or IEEE binary16 where
 * mobgs_prep_fwd is called with attr_half = 1 (this entry point reads them as float32). */
typedef struct MobgsPrepInputs {
    int32_t Ns, Nd;
    const float* times;      /* [K,2]: {t_feat, t_curve} per instant (K = 1 here) */
    const float* s_xyz;
    const void *s_scaling, *s_rotation, *s_opacity, *s_fdc, *s_ft;
    const float* d_control;
    const int64_t* d_ncp;
    const void *d_scaling, *d_rotation, *d_omega, *d_opacity, *d_fdc, *d_ft;
    const float* d_trbf;
} MobgsPrepInputs;
int mobgs_prep_project_and_bin_fused(const MobgsPrepInputs* prep, float* means, float* quats, float* scales,
                                     const float* viewmats, const float* Ks, float* opacities, int width, int height,
                                     float eps2d, float near_plane, float far_plane, float radius_clip, int cull,
                                     int32_t* radii, float* means2d, float* depths, float* conics,
                                     int32_t* tiles_per_gauss, int32_t* cum_tiles, int32_t* tile_offsets,
                                     int32_t* tile_order, int64_t* stats_dev, int capacity_box, int32_t* keep_scan,
                                     void* scratch, int64_t capacity_listed, int32_t* flatten_ids, uint64_t* seg_keys,
                                     int seg_stride, const int32_t* enum_order, uint64_t* isect_ids,
                                     int64_t max_tile_len_hint, int64_t* stats_host_pinned, int64_t stats_seq,
                                     float* pack_records, const MobgsTuning* tuning, void* stream);


/* ---- K6: rasterise forward (replaces gsplat rasterize_to_pixels fwd) -----------------------------------
 * colors   : [C,N,channels] (colors_per_camera=1) or [N,channels] (0); NULL: `records` are already packed (by
 *            mobgs_project_and_bin_speculative or mobgs_pack_records) and only `extra != NULL` is looked at
 * opacities: [C,N] (opac_per_camera=1) or [N] (0)
 * extra    : optional [C,N] channel appended after `channels` (gsplat's "+D"/"+ED" depth channel), or NULL
 * backgrounds: [C, channels(+1 if extra)] or NULL
 * records  : scratch/out [C*N, mobgs_record_stride(D)] packed splat records (kept for backward; an OPAQUE format of
 *            the kernels: {x, y, A, B, C, L, colours..} with conic and opacity in exponent form,
 *            opacity exp(-sigma) = exp2(A dx^2 + C dy^2 + B dx dy + L) -- csrc/common.h write_splat_record), D = total
 * out: render [C,H,W,D], alphas [C,H,W], last_ids [C,H,W] (index into flatten_ids of the last blended splat)
 * isect_reach (optional out, else NULL): [I_listed] bytes -- per list entry, the 8x8 quadrants of its tile the splat
 *   can reach (what the kernel computes anyway to skip the others); hand it to mobgs_raster_bwd for the same lists and
 *   the backward pass does not recompute it */
int mobgs_raster_fwd(int C, int N, int channels, int width, int height, const float* means2d,
                     const float* conics, const float* colors, int colors_per_camera,
                     const float* opacities, int opac_per_camera, const float* extra,
                     const float* backgrounds, const int32_t* radii, const int32_t* tile_offsets,
                     const int32_t* tile_order, const int32_t* flatten_ids, float* records, float* render,
                     float* alphas, int32_t* last_ids, uint8_t* isect_reach, const MobgsTuning* tuning,
                     void* stream);

/* mobgs_raster_fwd + the Sandwich decoder as the compositor's EPILOGUE (round 5): for the 9-feature + depth pass of
 * render() (channels = 9, extra != NULL, MobgsTuning.block_walk on) the kernel also writes what mobgs_decoder_fwd_many
 * would compute from `render` / `alphas` -- rgb [C,3,H,W] and the expected depth [C,H,W] -- while the pixel's features are
 * still in registers: no decoder launch and no re-read of the feature image (which is written all the same: the backward
 * passes read it).  Pinhole rays only: ray_intr [fx, fy, cx, cy] and ray_c2w (the first 12 entries of the row-major
 * camera-to-world matrix) per camera, intr_stride / c2w_stride floats apart (0 = shared); w1 [6,12], w2 [3,6] as
 * /root/reference/helper_model.py:19-28.  Bit-identical to the two separate calls.  Other channel counts / the quadrant
 * kernel: MOBGS_E_UNSUPPORTED (call mobgs_raster_fwd and mobgs_decoder_fwd_many). */
int mobgs_raster_fwd_decode(int C, int N, int channels, int width, int height, const float* means2d,
                            const float* conics, const float* colors, int colors_per_camera, const float* opacities,
                            int opac_per_camera, const float* extra, const float* backgrounds, const int32_t* radii,
                            const int32_t* tile_offsets, const int32_t* tile_order, const int32_t* flatten_ids,
                            float* records, float* render, float* alphas, int32_t* last_ids, uint8_t* isect_reach,
                            const float* ray_intr, int intr_stride, const float* ray_c2w, int c2w_stride, const float* w1,
                            const float* w2, float* rgb, float* depth, const MobgsTuning* tuning, void* stream);

/* ---- K7: rasterise backward (replaces gsplat rasterize_to_pixels bwd) ----------------------------------
 * Deterministic two-stage gradient reduction, no floating-point atomics:
 *   stage 1 (mobgs_raster_bwd) walks every tile back to front and writes ONE gradient record
 *     {A, B, Sxx, Sxy, Syy, S, v_colour[..]} per (tile, splat) intersection -- the geometry and opacity terms as raw
 *     sums over the tile's pixels, with d = mean2d - pixel centre and v_sigma the cotangent of the exponent:
 *     A = sum v_sigma dx, B = sum v_sigma dy, Sxx = sum v_sigma dx^2, Sxy = sum v_sigma dx dy, Syy = sum v_sigma dy^2,
 *     S = sum v_sigma -- into
 *     grad_slots [I_listed, stride]; slot = compact index (see keep_scan) of cum_tiles[flat id] + position of the tile inside the
 *     splat's tile rectangle].  grad_slots must be zero-filled by the caller (intersections that no pixel blended stay 0).
 *   stage 2 (mobgs_raster_bwd_reduce) sums each splat's contiguous slots and applies the splat's conic (a, b, c) of
 *     `records` (the packed records stage 1 read) once: v_means2d = (a A + b B, b A + c B), v_conics = (Sxx / 2, Sxy,
 *     Syy / 2), v_opacity = -S / opacity (a pair's v_sigma is -opacity vis v_alpha) -- conic and opacity are constant
 *     per splat, so this equals summing gsplat's per-pixel terms -- into the dense
 *     gradients v_means2d [C,N,2], v_conics [C,N,3], v_opacities [C,N], v_colors [C,N,channels], v_extra [C,N] (NULL
 *     when there was no extra channel); all fully written.
 *   any_record (optional, both stages the same zero-initialised int32; NULL = off): stage 1 sets it when it writes
 *     its first record, stage 2 reads no slot when it is still 0 -- a pass whose cotangents are all exactly zero (a
 *     loss term with weight 0, e.g. lambda_flow_loss = 0 in arguments/stereo/seesaw.py) then costs no reduction. */
int mobgs_raster_bwd(int C, int N, int channels, int has_extra, int width, int height,
                     const float* records, const float* backgrounds, const int32_t* radii,
                     const float* means2d, const int32_t* cum_tiles, const int32_t* keep_scan,
                     const int32_t* tile_offsets, const int32_t* tile_order, const int32_t* flatten_ids,
                     const float* render_alphas, const int32_t* last_ids, const float* v_render,
                     const float* v_alphas, float* grad_slots, const uint8_t* isect_reach,
                     int32_t* any_record, const MobgsTuning* tuning, void* stream);
/* Stage 1 with the Sandwich decoder's BACKWARD pass as its prologue (round 6; the counterpart of mobgs_raster_fwd_decode;
 * replaces, for the lean render() of /root/reference/gaussian_renderer/__init__.py:201-227, the chain
 * [helper_model.py:19-28 backward -> gsplat rasterize_to_pixels backward]): 9 feature channels + the depth channel,
 * pinhole rays.  The kernel reads the decoder's inputs -- `render` [C,H,W,10] (the composited image mobgs_raster_fwd[_decode]
 * wrote), `render_alphas`, the cotangents v_rgb [C,3,H,W] of the decoded colour and v_depth [C,H,W] (NULL = none) of the
 * expected depth -- and forms the cotangent of the composited image in registers (bit for bit what mobgs_decoder_bwd_many
 * would have written to v_feat_hw / v_alphas; v_alphas here = an ADDITIONAL cotangent of the alpha output, NULL = none).
 * The weight and pose gradients leave the kernel as ONE row of 102 sums per tile in w_partial (scratch of
 * mobgs_raster_bwd_decode_scratch_floats(C, width, height) floats, contents irrelevant on entry: the rows, then chunk sums
 * and a ticket word); mobgs_raster_bwd_decode_finish -- any time later on the same stream -- adds them in a fixed order
 * (deterministic) into g_w1 [6,12], g_w2 [3,6] (accumulate_wgrad != 0: added to what is there; sums over all images) and
 * g_c2w [C, g_c2w_floats = 12 | 16] (NULL = not wanted; per image, fully written).  Only where the quadrant kernel is the
 * selection ((mobgs_raster_path(10, 0, n_tiles, tuning) & 3) == 0), else MOBGS_E_UNSUPPORTED: callers then run
 * mobgs_decoder_bwd_many + mobgs_raster_bwd.  Everything else as mobgs_raster_bwd (channels = 9, has_extra = 1). */
int mobgs_raster_bwd_decode(int C, int N, int width, int height, const float* records, const float* backgrounds,
                            const int32_t* radii, const int32_t* cum_tiles, const int32_t* keep_scan,
                            const int32_t* tile_offsets, const int32_t* tile_order, const int32_t* flatten_ids,
                            const float* render, const float* render_alphas, const int32_t* last_ids, const float* v_rgb,
                            const float* v_depth, const float* v_alphas, const float* ray_intr, int intr_stride,
                            const float* ray_c2w, int c2w_stride, const float* w1, const float* w2, float* grad_slots,
                            const uint8_t* isect_reach, int32_t* any_record, float* w_partial, const MobgsTuning* tuning,
                            void* stream);
int mobgs_raster_bwd_decode_finish(int C, int width, int height, float* w_partial, int c2w_stride, float* g_w1,
                                   float* g_w2, float* g_c2w, int g_c2w_floats, int accumulate_wgrad, void* stream);
/* mobgs_raster_bwd_reduce (channels = 9, has_extra = 1) and mobgs_raster_bwd_decode_finish in ONE launch: the weight / pose
 * sums run as extra leading workgroups of the slot reduction (no launch of their own).  Same results as the two calls
 * (weight / pose gradients to summation order). */
int mobgs_raster_bwd_reduce_decode(int C, int N, const float* records, const int32_t* cum_tiles, const int32_t* keep_scan,
                                   const float* grad_slots, const int32_t* any_record, float* v_means2d, float* v_conics,
                                   float* v_opacities, float* v_colors, float* v_extra, const int32_t* tiles_per_gauss,
                                   int width, int height, const float* w_partial, int c2w_stride, float* g_w1, float* g_w2,
                                   float* g_c2w, int g_c2w_floats, int accumulate_wgrad, void* stream);
size_t mobgs_raster_bwd_decode_scratch_floats(int C, int width, int height);
/* tiles_per_gauss (optional, else NULL): [C*N] -- splat g's intersections are then [cum_tiles[g], cum_tiles[g] +
 *     tiles_per_gauss[g]) instead of [cum_tiles[g], cum_tiles[g + 1]): REQUIRED when the lists were built with an enum_order
 *     (mobgs_project_and_bin_fused), equivalent otherwise. */
int mobgs_raster_bwd_reduce(int C, int N, int channels, int has_extra, const float* records,
                            const int32_t* cum_tiles, const int32_t* keep_scan, const float* grad_slots,
                            const int32_t* any_record, float* v_means2d, float* v_conics, float* v_opacities,
                            float* v_colors, float* v_extra, const int32_t* tiles_per_gauss, void* stream);

/* Packs the compositor's per-splat inputs into records [C*N, mobgs_record_stride(D)] (the first step of
 * mobgs_raster_fwd, exposed for mobgs_raster_layers_fwd). */
int mobgs_pack_records(int C, int N, int channels, const float* means2d, const float* conics, const float* colors,
                       int colors_per_camera, const float* opacities, int opac_per_camera, const float* extra,
                       const int32_t* radii, float* records, void* stream);

/* ---- K6'/K7': layered compositing (train-mode render(): combined + static-only + dynamic-only in one pass) ----
 * Replaces the 5 rasterization() calls of /root/reference/gaussian_renderer/__init__.py:143-176,201-214,236-268
 * that share one camera: splats with (flat id % N) < Ns are "static", the others "dynamic".
 * layer_mask (non-zero): bit 0 = all, bit 1 = static-only, bit 2 = dynamic-only.  10 total channels only
 * (9 features + depth).  Per-layer tensors are passed as HOST arrays of 3 device pointers (index = layer;
 * entries of layers that are not requested may be NULL): render [C,H,W,10], alphas [C,H,W], last_ids [C,H,W].
 * Backward: v_render3 / v_alphas3 entries may be NULL (zero cotangent); grad_slots [I_listed, 2, 16] and
 * grad_xy0 [I_listed, 2, 2] are zero-filled scratch (one record per HALF tile and splat); the dense gradients
 * are fully written.  v_means2d is the total over the layers, v_means2d_layer0 the share of the combined render
 * alone (what the reference's `viewspace_points.grad` holds, gaussian_renderer/__init__.py:218-223). */
int mobgs_raster_layers_fwd(int C, int N, int Ns, int layer_mask, int channels_total, int width, int height,
                            const float* records, const float* backgrounds, const int32_t* tile_offsets,
                            const int32_t* tile_order, const int32_t* flatten_ids, float* const* render3_host,
                            float* const* alphas3_host,
                            int32_t* const* last_ids3_host, void* stream);
int mobgs_raster_layers_bwd(int C, int N, int Ns, int layer_mask, int channels, int has_extra, int width,
                            int height, const float* records, const float* backgrounds, const int32_t* radii,
                            const int32_t* cum_tiles, const int32_t* keep_scan, const int32_t* tile_offsets,
                            const int32_t* tile_order, const int32_t* flatten_ids,
                            const float* const* render_alphas3_host,
                            const int32_t* const* last_ids3_host, const float* const* v_render3_host,
                            const float* const* v_alphas3_host, float* grad_slots, float* grad_xy0,
                            float* v_means2d_layer0, float* v_means2d, float* v_conics, float* v_opacities,
                            float* v_colors, float* v_extra, const int32_t* tiles_per_gauss, void* stream);

/* ---- K13: densification ---------------------------------------------------------------
 * The per-splat table (14 optimiser groups + their Adam moments + 5 statistics arrays) of
 * /root/reference/scene/gaussian_model.py:598-617 is resized by clone / split / prune
 * (:1044-1155, :1207-1244, :1480-1506).  The reference does it with ~50 torch index/cat/repeat calls per
 * operation; here a resize is: masks (mobgs_densify_select) -> row list (mobgs_mask_indices + list arithmetic) ->
 * ONE mobgs_rows_gather launch that moves every field into a second buffer set -> mobgs_split_children.
 *
 * mobgs_densify_stats: the per-iteration statistics of helper_train.py:263-264 + gaussian_model.py:1352-1356,
 *   for rows with visible[i] != 0 (visible == NULL: radii[i] > 0): max_radii2D[i] = max(., radii[i]) (skipped when
 *   radii or max_radii2D is NULL), xyz_gradient_accum[i] += |viewspace_grad[i, 0:2]|, denom[i] += 1.
 *   viewspace_grad is [n, grad_stride] (2 for means2d.grad, 3 for the reference's screenspace tensor).
 * mobgs_densify_select: g = accum/denom (NaN -> 0; rows >= n_grads count as 0), big = max_k exp(scaling[i,k]) >
 *   size_threshold (= percent_dense * scene_extent): clone_sel = |g| >= thr && !big, split_sel = g >= thr && big.
 * mobgs_mask_indices: indices[0..count) = ascending rows with (mask[i] != 0) == (want != 0); count is a device int.
 * mobgs_rows_gather: for every field f (host arrays of n_fields device pointers / row sizes in bytes / flags) and
 *   output row r: dst_f[dst_offset + r] = src_f[index[r]] if index[r] >= 0; a negative index marks a NEW copy of
 *   row -(index[r]+1): fields with zero_new[f] != 0 (Adam moments) get zeros there, the others the copy.
 * mobgs_split_children: rows [first_row, first_row + n_children) hold copies of their parents;
 *   xyz += R(rotation) * sample, scaling = log(exp(scaling) / (0.8 * n_split))  (gaussian_model.py:1218-1221). */
int mobgs_densify_stats(int n, const float* viewspace_grad, int grad_stride, const uint8_t* visible,
                        const int32_t* radii, float* xyz_gradient_accum, float* denom, float* max_radii2D,
                        void* stream);
int mobgs_densify_select(int n, int n_grads, const float* xyz_gradient_accum, const float* denom,
                         const float* scaling, float grad_threshold, float size_threshold, uint8_t* clone_sel,
                         uint8_t* split_sel, void* stream);
int mobgs_mask_indices(int n, const uint8_t* mask, int want, int32_t* indices, int32_t* count, void* stream);
int mobgs_rows_gather(int n_fields, const void* const* src_host, void* const* dst_host,
                      const int32_t* row_bytes_host, const int32_t* zero_new_host, const int32_t* index, int n_out,
                      int dst_offset, void* stream);
int mobgs_split_children(int n_children, int first_row, int n_split, const float* samples, const float* rotation,
                         float* xyz, float* scaling, void* stream);

/* ---- K14: normals from a depth map (replaces /root/reference/main_utils.py:95-141 get_normals, train.py:590) ----
 * z [H,W] -> normals [3,H,W]: every pixel is back-projected with its view direction
 *   y = (i + pixel_offset - cy) / fy,  x = (j + pixel_offset - cx - y * skew) / fx,  point = (x, y, 1) * z,
 * n = normalize(cross(right - left, top - bottom), eps 1e-12) on the interior, zeros on the 1-pixel border.
 * pixel_offset = 0.5 for dycheck cameras with use_center (the default).  Backward: v_z [H,W] fully written. */
int mobgs_normals_fwd(int H, int W, float fx, float fy, float cx, float cy, float skew, float pixel_offset,
                      const float* z, float* normals, void* stream);
int mobgs_normals_bwd(int H, int W, float fx, float fy, float cx, float cy, float skew, float pixel_offset,
                      const float* z, const float* v_normals, float* v_z, void* stream);

/* ---- K6''/K7'': class-restricted passes of the single-set compositor -----------------------------------------
 * Replaces the static-only / dynamic-only rasterization() calls of
 * /root/reference/gaussian_renderer/__init__.py:201-214 (dynamic), :236-250 (static) and their ones-colour alpha
 * passes :163-177, :255-269, for splat sets that are the two halves of one projected set.
 * The static-only (class_sel = 1: flat id % N < Ns) or dynamic-only (class_sel = 2) "RGB+D" render over the lists
 * of the WHOLE set: entries of the other class are dropped as each 64-entry batch is staged.  Every splat belongs
 * to exactly one class, so the two passes together blend each (tile, splat) pair once and their backward passes
 * write disjoint records of ONE grad_slots buffer (zero-filled [I_listed, stride]), reduced by one
 * mobgs_raster_bwd_reduce.  channels_total = 10 (9 features + depth), or 1 (one colour channel, no extra: the
 * dynamic-only coverage of get_flow(), /root/reference/gaussian_renderer/__init__.py:477-490, where only the alpha
 * output matters); records from mobgs_pack_records; last_ids index the whole set's lists; any_record as in
 * mobgs_raster_bwd. */
int mobgs_raster_class_fwd(int C, int N, int Ns, int class_sel, int channels_total, int width, int height,
                           const float* records, const float* backgrounds, const int32_t* tile_offsets,
                           const int32_t* tile_order, const int32_t* flatten_ids, float* render, float* alphas,
                           int32_t* last_ids, uint8_t* isect_reach, const MobgsTuning* tuning, void* stream);
int mobgs_raster_class_bwd(int C, int N, int Ns, int class_sel, int channels_total, int width, int height,
                           const float* records, const float* backgrounds, const int32_t* radii,
                           const int32_t* cum_tiles, const int32_t* keep_scan, const int32_t* tile_offsets,
                           const int32_t* tile_order, const int32_t* flatten_ids, const float* render_alphas,
                           const int32_t* last_ids, const float* v_render, const float* v_alphas, float* grad_slots,
                           const uint8_t* isect_reach, int32_t* any_record, const MobgsTuning* tuning, void* stream);

/* 1 if raster kernels are compiled for `total_channels` (colour channels + optional extra channel). */
int mobgs_raster_channels_supported(int total_channels);

/* Which compositing kernels a pass of `total_channels` over a grid of `n_tiles` tiles (all cameras) takes under
 * `tuning` -- the decision functions the launchers themselves use, exported so that a test can ASSERT which kernels a
 * comparison exercised (round-5 review: every reference-generated fixture ran the small-grid selection, the benchmark
 * the other one).  class_filter: 1 for mobgs_raster_class_fwd/bwd.  Returns a bit field:
 *   bits 0-1  backward kernel: 0 = quadrant kernel raster_bwd_kernel (per-lane accumulators + wave reduction),
 *             1 = matrix-pipe backward, one wave per tile + four-wave team for heavy tiles, 2 = team for every tile,
 *             3 = block-walk backward (MobgsTuning.bwd_block_walk)
 *   bit 2     forward: 1 = block-walk kernel raster_fwd_blocks_kernel (the decoder epilogue exists only there)
 *   bit 3     the tile schedule may mark tiles heavy (four waves per tile) -- whether any IS heavy depends on the list
 *             lengths: count the entries of tile_order with bit 30 set
 *   bits 8-.. the list length from which a tile is scheduled heavy (0 = never)
 * Not a launch: no device work, no error state. */
int mobgs_raster_path(int total_channels, int class_filter, int n_tiles, const MobgsTuning* tuning);

/* ---- K8: per-splat state build (replaces the reference's per-Gaussian torch glue) -----------------------
 * /root/reference/gaussian_renderer/__init__.py:23-56 (interpolate_cubic_hermite), :93-125 (time offset,
 * rotation, colour features), :181-185 (cat static|dynamic); scene/gaussian_model.py:209-254 (activations).
 * Rows [0,Ns) of every output are the static splats, [Ns,Ns+Nd) the dynamic ones.
 * K time instants in ONE launch (K = 1: a plain render; K > 1: the K sub-frames of a blurry view, train.py:502-518 --
 * the same Gaussians at K exposure times), 1 <= K <= 65535.
 * in (host struct, see MobgsPrepInputs; read before the call returns):
 *   times (device, [K,2] floats): per instant {t_feat = time + delta/max_time, t_curve = clamp(t_feat,0,1)}.
 *   static leaves : xyz [Ns,3], scaling [Ns,3] (log), rotation [Ns,4], opacity [Ns] (logit), f_dc [Ns,6], f_t [Ns,3]
 *   dynamic leaves: control [Nd,12,3] (x100 units), ncp [Nd] int64 active knots (4..12), scaling, rotation,
 *                   omega [Nd,4], opacity, f_dc, f_t, trbf [Nd]
 * attr_half = 1: the ATTRIBUTES (scaling, rotation, omega, opacity, f_dc, f_t) are stored as IEEE binary16 (BASELINE
 *   config #5; no such mode exists in the reference, whose GaussianModel keeps fp32 nn.Parameters,
 *   scene/gaussian_model.py:1044-1090): the kernels read the halves from HBM and widen them in registers, arithmetic and
 *   outputs stay fp32.  xyz / control / trbf stay fp32.  0: float32.
 * out: means [K,N,3], quats [K,N,4] (un-normalised; the projection normalises), colors [K,N,9] (row block k = instant
 *      k); scales [N,3] and opacities [N] do not depend on time and exist once. */
int mobgs_prep_fwd(int K, const MobgsPrepInputs* in, int attr_half, float* means, float* quats, float* scales,
                   float* opacities, float* colors, void* stream);
/* Backward of mobgs_prep_fwd.  Of `in`, only Ns, Nd, times, d_ncp and d_trbf are read.  v_means / v_quats / v_colors
 * [K,...], v_scales / v_opacities once; cotangent pointers may be NULL (zeros).  Every gradient buffer of `grads` (host
 * struct, see MobgsLeafGrads) is fully written -- or, with accumulate != 0, added to: the leaf gradients are the sums over
 * the instants, accumulated in instant order (the result of K single-instant calls in a row, bit for bit).  trbf and the
 * times get no gradient (the reference detaches the time offset, :102).
 * grad_half = 1: the attribute gradients are written as binary16 (what a half leaf's .grad must be); accumulation across
 * renders in fp32 buffers uses grad_half = 0 -- the backward pass does not read the attributes. */
int mobgs_prep_bwd(int K, const MobgsPrepInputs* in, const float* scales, const float* opacities, const float* v_means,
                   const float* v_quats, const float* v_scales, const float* v_opacities, const float* v_colors,
                   const MobgsLeafGrads* grads, int grad_half, int accumulate, void* stream);

/* ---- K9: colour decoder + expected-depth normalisation (replaces Sandwich.forward + gsplat's "ED" step) ---
 * /root/reference/helper_model.py:19-28; /root/reference/gaussian_renderer/__init__.py:216-227.
 * feat_hw [P,CF] channels-last compositor output (CF >= 9; channel 9 = accumulated depth when has_depth),
 * alphas [P], w1 [6,12], w2 [3,6]  ->  rgb [3,P] planar, depth [P].
 * Camera rays, one of:
 *   rays   [6,P] planar (the reference's cam_ray map, /root/reference/scene/cameras.py:132-146), ray_* = NULL;
 *   rays = NULL, ray_intr = device float[4] {fx, fy, cx, cy}, ray_c2w = device float[12] (the first three rows of
 *          the row-major camera-to-world matrix: a [3,4] or a [4,4] array), width = image width: the origin and
 *          the unit view direction through each pixel centre are generated in registers.
 * Backward: w_partial: scratch [C * mobgs_decoder_bwd_blocks(P), 102] floats.  v_depth / v_rays may be NULL.
 * g_c2w (may be NULL): gradient of ray_c2w (in-kernel-ray mode only), g_c2w_floats = 12 ([3,4]) or 16 ([4,4]: the
 * fourth row is written as zeros).  accumulate_wgrad != 0: the weight gradients are added to g_w1 / g_w2 instead
 * of overwriting them (fixed summation order either way).
 * A BATCH of C images in one launch (C = 1: one image; C > 1: the K sub-frames of a blurry view): feat_hw [C,P,CF],
 * alphas [C,P], rgb [C,3,P], depth [C,P] (and the cotangents alike); *_stride = floats between consecutive images' ray
 * maps / intrinsics / poses, 0 = shared by all images.  The weight gradients are sums over all images (one fixed-order
 * reduction); g_c2w [C, g_c2w_floats].  A shared ray map / pose cannot receive a gradient when C > 1. */
int mobgs_decoder_bwd_blocks(int P);
int mobgs_decoder_fwd_many(int C, int P, int CF, int has_depth, int width, const float* feat_hw, const float* alphas,
                           const float* rays, int64_t rays_stride, const float* ray_intr, int intr_stride,
                           const float* ray_c2w, int c2w_stride, const float* w1, const float* w2, float* rgb,
                           float* depth, void* stream);
int mobgs_decoder_bwd_many(int C, int P, int CF, int has_depth, int width, const float* feat_hw, const float* alphas,
                           const float* rays, int64_t rays_stride, const float* ray_intr, int intr_stride,
                           const float* ray_c2w, int c2w_stride, const float* w1, const float* w2, const float* v_rgb,
                           const float* v_depth, float* v_feat_hw, float* v_alphas, float* v_rays, float* w_partial,
                           float* g_w1, float* g_w2, float* g_c2w, int g_c2w_floats, int accumulate_wgrad,
                           void* stream);

/* The batched decoder with `n` further channels [c0, c0 + n) of the image -- behind the ones the decoder reads -- handed
 * out as an array of their own, chan_out [C,P,n] (forward), and their cotangent v_chan [C,P,n] written into those
 * channels of v_feat_hw (backward; the other unread channels get 0 as before).  get_flow()
 * (/root/reference/gaussian_renderer/__init__.py:436-476) composites 9 features + 2 flow channels in one pass; taking the
 * two channels off the 12-channel image with a PyTorch slice is a strided copy of the whole image each way.
 * chan_out / v_chan = NULL: exactly mobgs_decoder_fwd_many / mobgs_decoder_bwd_many. */
int mobgs_decoder_fwd_channels(int C, int P, int CF, int has_depth, int width, const float* feat_hw, const float* alphas,
                               const float* rays, int64_t rays_stride, const float* ray_intr, int intr_stride,
                               const float* ray_c2w, int c2w_stride, const float* w1, const float* w2, float* rgb,
                               float* depth, float* chan_out, int c0, int n, void* stream);
int mobgs_decoder_bwd_channels(int C, int P, int CF, int has_depth, int width, const float* feat_hw, const float* alphas,
                               const float* rays, int64_t rays_stride, const float* ray_intr, int intr_stride,
                               const float* ray_c2w, int c2w_stride, const float* w1, const float* w2, const float* v_rgb,
                               const float* v_depth, float* v_feat_hw, float* v_alphas, float* v_rays, float* w_partial,
                               float* g_w1, float* g_w2, float* g_c2w, int g_c2w_floats, int accumulate_wgrad,
                               const float* v_chan, int c0, int n, void* stream);

/* ---- K10: deformation network (the API the reference exposes as scene.deformation.deform_network) -----
 * /root/reference/scene/hexplane.py:75-108,165-187 (HexPlane multi-resolution bilinear planes, product over the
 * 6 planes of a level, concat over 3 levels -> 96 features); /root/reference/scene/deformation.py:158-199
 * (Linear 96->128, three ReLU-Linear(128,128)-ReLU-Linear(128,{7,3,4}) heads, point/scale/rotation update).
 *
 * planes_host / gplanes_host: HOST arrays of 18 device pointers, index level*6 + plane with plane order
 *   (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); every plane is CHANNELS-LAST [rb][ra][32] (ra = resolution of the first
 *   axis of the pair, rb of the second) -- the host permutes the reference's [1,32,rb,ra] parameters.
 * ra_host / rb_host: HOST int32[18].   aabb: device [2,3] = {xyz_max, xyz_min} (the reference's convention).
 * mobgs_hexplane_fwd : pts [N,3], times [N]  ->  feat [N,96]
 * mobgs_hexplane_bwd : v_feat [N,96] -> gplanes (ACCUMULATED; zero them first), v_pts [N,3] (ADDED to its current
 *                      content), v_times [N] (written).  The (point, plane) contributions are counting-sorted by
 *                      plane cell (integer atomics) and runs of equal cells are summed in registers before they
 *                      leave as float atomics, instead of torch's one global float atomic per (point, plane, tap,
 *                      channel) (grid_sampler_2d_backward).  scratch: mobgs_hexplane_bwd_scratch_bytes(N, ra, rb)
 *                      bytes, 16-byte aligned (per-cell counters + entry lists of 144 B per point and plane).
 * mobgs_deform_mlp_fwd: feat + pts/scales/rots [N,3]/[N,3]/[N,4] -> out_pts, out_scales, out_rots (MFMA fp32).
 *   Weights K-major: W0t [96,128], b0 [128], W1t [3,128,128], b1 [3,128], W2t [3,128,32] (7/3/4 real columns,
 *   zero padded), b2 [3,32]; head order: position, scale, rotation.
 *   o_raw [N,16] (may be NULL): the 14 raw head outputs per point (position 0..6, scale 7..9, rotation 10..13),
 *   all the backward pass keeps of the forward pass.
 * mobgs_deform_mlp_bwd: replaces torch autograd over the reference's nn.Sequential heads
 *   (/root/reference/scene/deformation.py:56-73,158-199).  Recomputes the hidden activations from `feat`, then
 *   data gradients (v_feat [N,96], v_pts [N,3], v_rots [N,4], all WRITTEN; the scale input's cotangent is
 *   v_out_scales itself) and weight gradients, everything on fp32 MFMA.  Besides the K-major W0t / W1t it reads
 *   the weights in their original (out, in) layouts: W0 [128,96], W1 [3,128,128], W2pad [3,8,128] (rows >= 7/3/4
 *   zero).  v_out_* may be NULL (zero cotangent).  v_o: scratch [N,16] (cotangents of the raw head outputs).
 *   partials: scratch of mobgs_deform_mlp_bwd_blocks(N) x
 *   mobgs_deform_mlp_grad_floats() floats (one block of partial sums per workgroup, reduced in workgroup order:
 *   deterministic).  grads (mobgs_deform_mlp_grad_floats() = 66 080 floats, WRITTEN): W0 [128,96] | b0 [128] |
 *   W1 [3,128,128] | b1 [3,128] | W2 [32,128] (row 8h + o = output o of head h) | b2 [32] (same indexing). */
int mobgs_hexplane_fwd(int N, const float* pts, const float* times, const float* aabb,
                       const float* const* planes_host, const int32_t* ra_host, const int32_t* rb_host,
                       float* feat, void* stream);
int mobgs_hexplane_bwd(int N, const float* pts, const float* times, const float* aabb,
                       const float* const* planes_host, const int32_t* ra_host, const int32_t* rb_host,
                       const float* v_feat, float* const* gplanes_host, float* v_pts, float* v_times,
                       void* scratch, void* stream);
size_t mobgs_hexplane_bwd_scratch_bytes(int N, const int32_t* ra_host, const int32_t* rb_host);
int mobgs_deform_mlp_fwd(int N, const float* feat, const float* pts, const float* scales, const float* rots,
                         const float* W0t, const float* b0, const float* W1t, const float* b1, const float* W2t,
                         const float* b2, float* out_pts, float* out_scales, float* out_rots, float* o_raw,
                         void* stream);
int mobgs_deform_mlp_bwd_blocks(int N);
size_t mobgs_deform_mlp_grad_floats(void);
int mobgs_deform_mlp_bwd(int N, const float* feat, const float* pts, const float* rots, const float* o_raw,
                         const float* W0t, const float* b0, const float* W1t, const float* b1, const float* W0,
                         const float* W1, const float* W2pad, const float* v_out_pts, const float* v_out_scales,
                         const float* v_out_rots, float* v_feat, float* v_pts, float* v_rots, float* v_o,
                         float* partials, float* grads, void* stream);

/* ---- K10b: BLCE of one view (latent camera poses of the K = 9 sub-frames), forward and backward ----------
 * /root/reference/scene/blce.py:374-478 (BLCE.forward) + :150-152 (inverse of the warped poses), which the reference
 * runs as ~180 + ~350 tiny torch launches per view.  One single-wave kernel each way.
 * params_host / grads_host: HOST arrays of 22 device pointers in the order documented in csrc/blce.hip (the
 *   reference's parameter tensors of view `idx`: view_embedder table, Rt_encoder, view_encoder, blur_feature_encoder
 *   0/2/4, wv_derivative.{time_embedder, w_linear, v_linear}, rot/trans/theta decoders; weight then bias).
 * Rt [4,4] c2w of the view, blur_feature: device scalar.  c2w / w2c [9,4,4]: warped poses and their inverses.
 * saved: mobgs_blce_saved_floats() floats kept for the backward pass (NULL when no gradient is needed).
 * bwd: v_c2w / v_w2c [9,4,4] cotangents (either may be NULL); every gradient tensor is fully written (the
 *   view_embedder table gets zeros outside row idx). */
size_t mobgs_blce_saved_floats(void);
int mobgs_blce_fwd(const float* const* params_host, int idx, int num_views, const float* Rt,
                   const float* blur_feature, float* c2w, float* w2c, float* saved, void* stream);
int mobgs_blce_bwd(const float* const* params_host, float* const* grads_host, int idx, int num_views, const float* Rt,
                   const float* saved, const float* v_c2w, const float* v_w2c, void* stream);

/* ---- K11: fused photometric loss (L1 + SSIM), forward and backward -------------------------------------
 * /root/reference/utils/loss_utils.py:233-239 (l1_loss, mask=None), :251-260 + :351-381 (ssim: 11x11 Gaussian
 * window sigma 1.5, zero padding, per channel, mean over all elements); /root/reference/train.py:621-628.
 * img1, img2 [C,H,W].  fwd: partial [mobgs_ssim_l1_blocks(C,H,W), 2] = per-workgroup {sum ssim_map, sum |img1-img2|}
 * (the caller sums and divides by C*H*W); dmaps [3,C,H,W] = d ssim_map / d{mu1, E[x^2], E[xy]} (NULL when no
 * backward is needed).  bwd: scales = device float[C,2], per channel {d loss / d sum-of-ssim_map, d loss / d sum-of-|diff|}
 * (i.e. the mean's 1/(C*H*W) already applied); v_img1 [C,H,W] is fully written (gradient w.r.t. img1 only). */
int mobgs_ssim_l1_blocks(int C, int H, int W);
int mobgs_ssim_l1_fwd(int C, int H, int W, const float* img1, const float* img2, float* partial, float* dmaps,
                      void* stream);
int mobgs_ssim_l1_bwd(int C, int H, int W, const float* img1, const float* img2, const float* dmaps,
                      const float* scales, float* v_img1, void* stream);

/* ---- K17: flow-consistency loss (the consumer of get_flow()'s outputs in a training iteration) ---------------------
 * /root/reference/train.py:651-671 with utils/loss_utils.py:233-237 (masked l1_loss):
 *   loss = l1(grid_sample(ori expanded over K, norm(exp2mid)), latent, mask = latent_alpha)
 *        + l1(grid_sample(latent,             norm(mid2exp)), ori,    mask = d_alpha)
 * norm(c) = 2 c / (size - 1) - 1 per axis; grid_sample bilinear, padding_mode = 'border', align_corners = False;
 * l1(a, b, m) = sum |(a - b) m| / (3 sum(m) + 1e-8).  lambda_flow_loss is the caller's.
 * ori [B,3,H,W]; latent [B,K,3,H,W]; exp2mid, mid2exp [B,K,H,W,2] PIXEL coordinates (what get_flow returns; the
 * reference normalises them in place, this entry point leaves its inputs alone); latent_alpha [B,K,H,W]; d_alpha
 * [B,H,W].  H, W >= 2.
 * fwd: partial = scratch [mobgs_flow_warp_loss_blocks(B,H,W), 4]; sums [4] (kept for bwd) = {N1, S1, N2, S2};
 *      loss [1].  Deterministic (fixed summation order).
 * bwd: v_loss = device scalar.  g_ori [B,3,H,W] and g_latent [B,K,3,H,W] are ADDED to with float atomics (bilinear
 *      scatter, as torch's grid_sampler_2d_backward: summation order not fixed) -- zero-fill them; g_exp2mid /
 *      g_mid2exp [B,K,H,W,2], g_latent_alpha [B,K,H,W], g_d_alpha [B,H,W] are fully written.  Any may be NULL.
 *      scratch: mobgs_flow_warp_loss_bwd_scratch_floats(B,K,H,W) floats (needed when g_ori or g_latent is wanted: the
 *      images' gradients as TARGETS of the other term are written there and added at the end).
 *      combine_taps != 0: coinciding taps of neighbouring pixels (next lane, next row) are merged in registers before
 *      the atomics (same sums, a quarter of the atomics).
 * mobgs_flow_warp_loss_bwd_rows: the rows of a wave's strip (4 or 8) in the build of the backward kernel that
 *      mobgs_flow_warp_loss_bwd launches for these sizes -- 8 when combine_taps != 0 and ceil(W / 64) ceil(H / 32) B
 *      >= 1024, else 4; the launcher chooses its kernel by this very function.  A size query: no device is touched.
 *      Bad sizes (B <= 0, H < 2, W < 2): MOBGS_E_INVALID with a message, as the other flow entry points. */
int mobgs_flow_warp_loss_blocks(int B, int H, int W);
int mobgs_flow_warp_loss_bwd_rows(int B, int H, int W, int combine_taps);
int mobgs_flow_warp_loss_fwd(int B, int K, int H, int W, const float* ori, const float* latent, const float* exp2mid,
                             const float* mid2exp, const float* latent_alpha, const float* d_alpha, float* partial,
                             float* sums, float* loss, void* stream);
int mobgs_flow_warp_loss_bwd(int B, int K, int H, int W, const float* ori, const float* latent, const float* exp2mid,
                             const float* mid2exp, const float* latent_alpha, const float* d_alpha, const float* sums,
                             const float* v_loss, float* g_ori, float* g_latent, float* g_exp2mid, float* g_mid2exp,
                             float* g_latent_alpha, float* g_d_alpha, float* scratch, int combine_taps, void* stream);
size_t mobgs_flow_warp_loss_bwd_scratch_floats(int B, int K, int H, int W);

/* ---- K16: one Adam step over MANY parameter tensors in one launch ------------------------------------------------
 * The reference steps three torch.optim.Adam optimisers per iteration (train.py:790-807: static Gaussians, dynamic
 * Gaussians + decoder, blur kernel), ~14 one-tensor parameter groups each: ~26 groups x 8 multi-tensor launches =
 * 3.3 ms of device time per iteration at 300 k Gaussians for 0.48 GB of traffic.  One launch over all of them:
 *   m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2;  p = p - step_size * m / (sqrt(v) / bias2_sqrt + eps)
 * (torch.optim.Adam, amsgrad = False, weight_decay = 0, maximize = False; step_size = lr / (1 - beta1^t) and
 * bias2_sqrt = sqrt(1 - beta2^t) are computed by the caller per tensor, as torch does on the host; the betas arrive as
 * doubles and 1 - beta is formed in double before it is rounded to fp32, again as torch does: 1.f - 0.999f is off by 1e-5).
 * tensors_host: HOST array of n_tensors descriptors (device pointers, fp32, contiguous); n_tensors <= 64. */
typedef struct MobgsAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    float step_size;
    float bias2_sqrt;
} MobgsAdamTensor;
int mobgs_adam_step(int n_tensors, const MobgsAdamTensor* tensors_host, double beta1, double beta2, double eps,
                    void* stream);

/* ---- K17: exact 3-nearest-neighbour mean squared distance (scene initialisation) ---------------------------------
 * Replaces simple_knn._C.distCUDA2, the CUDA-only extension behind every initial scale of
 * /root/reference/scene/gaussian_model.py:420,514 (create_from_pcd_dynamic / create_from_pcd).
 *   dist2[i] = (d0 + d1 + d2) / 3, the three smallest |p_i - p_j|^2 over j != i (self excluded by INDEX: a duplicate
 *   point counts with distance 0), each evaluated in fp32 as (dx dx + dy dy) + dz dz without FMA contraction.
 * Exact for every row order: rows are pruned in boxes of consecutive rows, and a box is skipped only when its fp32
 * distance bound proves that it cannot change the result; the order decides the speed only (callers pass rows sorted
 * along a Morton curve, mobgs_amd.scene_init).  Bit-reproducible; no atomics.
 * n < 4 (fewer than three neighbours) and n > 2^30 are refused before any launch; mobgs_knn3_scratch_bytes returns
 * 0 for them.  scratch: 16-byte aligned, at least mobgs_knn3_scratch_bytes(n) bytes. */
size_t mobgs_knn3_scratch_bytes(int n);
int mobgs_knn3_mean_dist2(int n, const float* points, float* dist2, void* scratch, size_t scratch_bytes, void* stream);

/* ---- K18: drop one spline control point per dynamic Gaussian (motion-adaptive splines) -----------------------------
 * The reference's scene/gaussian_model.py:274-371 (onedown_control_pts: inverse_cubic_hermite_for_prune,
 * compute_prune_error and the commit) in ONE launch.  A row with n = control_num[i] in 5..12 points is refitted with
 * m = n - 1 points, new[j] = sum_k P_n[j][k] old[k] with P_n = pinv_table[n - 5] (float32 [8,11,12], zero-padded: the
 * float64 pseudo-inverse of the [n, m] Hermite design matrix at the old knot times k / (n - 1); the caller builds it,
 * mobgs_amd.scene_init.one_down_tables).  Both splines are evaluated at times[v] of the interior views v = 1..V-2,
 * scaled by 1e-2, transformed with viewmats[v] (row-major world-to-camera, column vectors, divide by w + 1e-7),
 * projected with K = [focal, 0, cx; 0, focal, cy; 0, 0, 1] (divide by z + 1e-7), and the pixel distances averaged into
 * err_out[i].  new_control_out (or NULL) receives the m fitted points followed by zeros up to slot 10.
 * commit != 0: where err_out[i] <= threshold, slots 0..10 of control_xyz[i] := the fitted points and zeros (slot 11
 * stays), control_num[i] := m, and counters[0] grows by the number of such rows.  commit == 0 writes no input.
 * Rows with n == 4 are not candidates (deliberately unlike the reference, whose floor at 4 halves the fourth point):
 * error 0, never written, their own points in new_control_out.  A count outside 4..12 is never used as an index: the
 * row is skipped and counted in counters[1].  The caller clears counters[0..1] beforehand; nothing synchronises.
 * Refused before any launch: n_views < 3, n_rows < 0, a NULL table or buffer.  n_rows == 0 is a no-op. */
int mobgs_control_onedown(int n_rows, int n_views, const float* viewmats, const float* times, float focal, float cx,
                          float cy, const float* pinv_table, float threshold, float* control_xyz, int64_t* control_num,
                          float* err_out, float* new_control_out, int* counters, int commit, void* stream);

/* ---- K19: seeding both Gaussian sets from depth maps, poses and 2-D tracks (scene initialisation) -------------------
 * The numerical part of the reference's scene_initialization (/root/reference/train.py:58-199) in three launches on
 * the caller's stream, with no float atomics and no host synchronisation.  V views of H x W pixels, 2 <= V <= 4096,
 * H, W >= 2, H * W <= 2^28 (anything else is refused before any launch; mobgs_seed_scratch_bytes returns 0 for it).
 *
 * mobgs_seed_consistency: images [V,3,H,W], depths [V,H,W], pair_table [V,V,12]; entry (i, j) is the row-major 3x4
 *   matrix K_j [R_j R_i^T | t_j - R_j R_i^T t_i] K_i^-1 that takes (d u, d v, d, 1) of pixel (u, v) with depth d in view
 *   i to the homogeneous pixel (x, y, z) of view j (the caller builds it in float64: mobgs_amd.scene_init.pair_table).
 *   Per (pixel of i, view j), as inverse_warp_rt1_rt2 + train.py:105-106: |z| < 1e-6 -> 1e-6; normalise 2 (x / z) /
 *   (W - 1) - 1, 2 (y / z) / (H - 1) - 1; either coordinate outside [-1, 1] -> the sample is zero; else the 4-tap bilinear
 *   sample (align_corners, zero padding) of the 3 channels of image j; out_mask = (sum of channels > 0);
 *   accum_error[i] += mean_c(out_mask |sample - image_i|), j = i included.  scratch receives one partial sum of
 *   accum_error per workgroup: mobgs_seed_scratch_bytes(V, H, W) bytes, 4-byte aligned.
 * mobgs_seed_classify: reads that scratch; mean[i] = sum of view i's partials (fixed order: deterministic) / (H W);
 *   inconsistent = accum_error > mean[i] (uint8); cls = 0 (static candidate: !inconsistent and motion == 0), 1 (dynamic
 *   candidate: inconsistent and motion == 1) or 2 (neither; any other motion byte lands here); points [V,H,W,3] =
 *   unproject_table[i] (d u, d v, d, 1), unproject_table [V,12] holding the row-major 3x4 [R_i^T K_i^-1 | -R_i^T t_i].
 * mobgs_seed_trajectories: coords [N,2] pixel coordinates, tracklet [T,M,2] with T == V (refused otherwise), points as
 *   above.  track_index[n] = argmin_m |coords[n] - tracklet[0][m]|^2, evaluated in fp32 as (dx dx + dy dy) without FMA
 *   contraction, ties to the lowest m; trajectory [N,T,3]: points[t] at the pixel (nearbyint(u - 0.5), nearbyint(v - 0.5))
 *   (ties to even) of (u, v) = tracklet[t][track_index[n]] -- grid_sample(mode="nearest", align_corners=False,
 *   padding_mode="zeros") after the reference's / W, / H, * 2 - 1 -- and zeros outside the image.  N == 0 is a no-op. */
size_t mobgs_seed_scratch_bytes(int V, int H, int W);
int mobgs_seed_consistency(int V, int H, int W, const float* images, const float* depths, const float* pair_table,
                           float* accum_error, void* scratch, size_t scratch_bytes, void* stream);
int mobgs_seed_classify(int V, int H, int W, const float* accum_error, const void* scratch, size_t scratch_bytes,
                        const float* depths, const uint8_t* motion, const float* unproject_table,
                        uint8_t* inconsistent, uint8_t* cls, float* points, float* mean, void* stream);
int mobgs_seed_trajectories(int N, int T, int M, int V, int H, int W, const float* coords, const float* tracklet,
                            const float* points, int32_t* track_index, float* trajectory, void* stream);

/* ---- K20: exposure-time estimate from two rendered flow maps ------------------------------------------------------
 * What /root/reference/train.py:482-492 computes from its two get_flow_static images, on the caller's stream, without a
 * sort, a read-back or a float atomic (csrc/exposure.hip: radix select on the fp32 bit patterns).  cam_flow and
 * latent_flow are [n,2] (8-byte aligned), 1 <= n <= 2^30.  In fp32, every operation as written and correctly rounded:
 *   cam_mag = sqrt(x x + y y), lat_mag likewise; ratio = lat_mag / cam_mag;
 *   threshold = torch.quantile(cam_mag, q), linear: pos = q * float(n - 1) (fp32), lo = floor(pos), hi = ceil(pos),
 *     w = pos - lo, a / b = the order statistics of rank lo / hi, threshold = w < 0.5 ? a + w (b - a)
 *     : b - (b - a)(1 - w);
 *   valid = cam_mag > threshold, n_valid = its count;
 *   *slot = scale * (the LOWER median of ratio over the valid pixels: rank (n_valid - 1) / 2, as torch.median).
 * stats (device, 4 x int32) = {n_valid, n_nonfinite, updated, 0}; n_nonfinite counts inf / NaN magnitudes of both maps.
 * Unlike the reference, which would store NaN: if n_valid == 0 or n_nonfinite > 0, *slot is left untouched and
 * updated = 0 (n_valid is then the count against whatever threshold the non-finite keys produced).
 * scratch: mobgs_exposure_scratch_bytes(n) bytes, 4-byte aligned, contents irrelevant on entry (the call zeroes what it
 * accumulates into); 0 is returned for an n outside the range.  The inputs are only read.
 * Refused with MOBGS_E_INVALID before any launch: n outside the range, a NULL or misaligned pointer, q outside [0, 1]
 * (NaN included). */
size_t mobgs_exposure_scratch_bytes(int64_t n);
int mobgs_exposure_estimate(int64_t n, const float* cam_flow, const float* latent_flow, float q, float scale,
                            float* slot, int32_t* stats, void* scratch, void* stream);

/* ---- K21: depth, entropy and sparsity terms of the training loss, and the PSNR next to them ------------------------
 * /root/reference/train.py:651-655 with utils/loss_utils.py:233-239 (l1_loss, mask=None), :264-276 (entropy_loss),
 * :285-295 (sparsity_loss), and train.py:622 with utils/image_utils.py:17-38 (psnr, mask=None), on the caller's stream,
 * without a float atomic (csrc/regterms.hip: per-workgroup partial rows, a one-workgroup finishing launch).  All maps are
 * flattened fp32, 4-byte aligned (16-byte alignment is NOT needed: heads and tails are handled), at most 2^40 elements.
 * Every term is evaluated in fp32 as written below; the terms are ADDED in float64 and each sum is rounded to fp32 once:
 *   S_d = sum |depth - gt_depth|                                        depth_loss = S_d / n_d
 *   S_e = sum [a log(a + eps) + (1 - a) log(1 - a + eps)], eps = 1e-6   entropy    = -S_e
 *   S_s = sum a a                                                       sparsity   = S_s
 *   mask_loss = w_e entropy + w_s sparsity;   reg_loss = (0 + w_d depth_loss) + mask_loss
 *   psnr[b]   = 20 log10(1 / sqrt(sum (image[b] - gt_image[b])^2 / (3 H W)))      (fp32 squares; the rest in float64,
 *                                                                                   rounded to fp32 at the end)
 * Nothing is clamped: an alpha outside [-eps, 1 + eps] gives NaN, as in the reference.
 * terms: MOBGS_REG_ENTROPY | MOBGS_REG_SPARSITY, the alpha terms that are evaluated; one that is not contributes a sum
 *   of 0 (and no NaN), forward and backward.
 * fwd: depth and gt_depth [n_d] may both be NULL (n_d = 0: depth_loss = 0); alpha [n_a] may be NULL (n_a = 0, terms = 0);
 *   not both.  image and gt_image [B,3,H,W] may both be NULL (B = 0; H, W ignored), else 1 <= B <= MOBGS_REG_MAX_IMAGES.
 *   partial: scratch, [mobgs_reg_terms_blocks(max(n_d, n_a, 3 H W)), 3 + B] doubles, contents irrelevant on entry.
 *   out [5 + B] (device) = {reg_loss, depth_loss, mask_loss, entropy, sparsity, psnr[0..B)}.  Two launches; the result is
 *   bit-identical from run to run.  The inputs are only read.
 * bwd: v_loss = device scalar, d L / d reg_loss.  Recomputed from the inputs (forward saves nothing):
 *   v_depth [n_d] = v_loss w_d sgn(depth - gt_depth) / n_d                                  (sgn(0) = 0)
 *   v_alpha [n_a] = v_loss (-w_e [log(a + eps) + a / (a + eps) - log(1 - a + eps) - (1 - a) / (1 - a + eps)] + w_s 2 a)
 *   Either may be NULL (that side is not computed; not both); what is given is fully written.  One launch.
 * mobgs_reg_terms_blocks(n): workgroups of the streaming launch for a largest map of n elements (a host computation:
 *   no device is touched); 0 for an n outside [1, 2^40].
 * Refused with MOBGS_E_INVALID before any launch: a size <= 0 with a non-NULL map or != 0 with a NULL one, one of a pair
 * of maps without the other, no map at all, terms that do not match alpha, images without B, H, W >= 1, a gradient for a
 * map that is not given, a NULL partial / out / v_loss, a misaligned pointer. */
#define MOBGS_REG_ENTROPY 1
#define MOBGS_REG_SPARSITY 2
#define MOBGS_REG_MAX_IMAGES 64
int mobgs_reg_terms_blocks(int64_t n);
int mobgs_reg_terms_fwd(int64_t n_d, const float* depth, const float* gt_depth, int64_t n_a, const float* alpha,
                        int terms, float w_d, float w_e, float w_s, int B, int H, int W, const float* image,
                        const float* gt_image, double* partial, float* out, void* stream);
int mobgs_reg_terms_bwd(int64_t n_d, const float* depth, const float* gt_depth, int64_t n_a, const float* alpha,
                        int terms, float w_d, float w_e, float w_s, const float* v_loss, float* v_depth,
                        float* v_alpha, void* stream);

/* ---- K22: evaluation metrics of a batch of image pairs -------------------------------------------------------------
 * What /root/reference/metrics.py:54-79, :123-125 (scikit-image), dycheck_metrics.py:67-200 (jax) and train.py:918-919
 * compute per image, for B pairs at once, on the caller's stream, forward only (csrc/metrics.hip: 16x16 tiles, the halo
 * patch in LDS, a separable window; per-workgroup partial rows and a one-workgroup finishing launch; no float atomic, so
 * a result is bit-identical from run to run and an image's row does not depend on the batch around it).
 * pred, gt [B,3,H,W] fp32; mask [B,H,W] fp32 in {0, 1}, or NULL (= all ones).  flags: MOBGS_METRICS_CLAMP clamps both
 * images to [0, 1] first (train.py:903-907); MOBGS_METRICS_QUANTIZE then replaces pred by floor(clip(pred, 0, 1) * 255)
 * / 255, evaluated in fp32 (eval.py:162 and the / 255 of metrics.py:100: the 8-bit image without writing it).  All
 * arithmetic after that is float64.  With d = pred - gt, n = 3 H W and M = 3 sum(mask) (the mask broadcast over the
 * channels), out [B, MOBGS_METRICS_COLUMNS] float64 (device) =
 *   0 l1              sum |d| / n
 *   1 mse             sum d^2 / n
 *   2 psnr            20 log10(1 / sqrt(mse))                                              (utils/image_utils.py:30-31)
 *   3 psnr_masked     -10 / ln 10 * ln(sum d^2 mask / max(M, 1e-6))                        (dycheck_metrics.py:57-64, :91)
 *   4 ssim_box        skimage structural_similarity(multichannel=True): 7x7 uniform window with `reflect` borders, sample
 *                     covariance (x 49 / 48), C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = data_range; per channel the mean of
 *                     the map cropped by 3 on every side, then the mean of the three
 *   5 ssim_box_masked sum(map x mask) / (M + 1e-8) over the uncropped map                  (metrics.py:62-64)
 *   6 ssim_gauss      dycheck's partial-convolution SSIM: 11 taps, sigma 1.5, `valid`; the horizontal pass over z x mask,
 *                     renormalised by 11 / m_ where the window's mask count m_ != 0 and 0 elsewhere; the vertical pass
 *                     over that with the mask (m_ != 0), renormalised the same way; variances clipped at 0, the covariance
 *                     limited to sqrt(s00 s11); the mean of the whole (H - 10) x (W - 10) x 3 map, unmasked
 *   7 sum d^2 mask    8 M
 * arms: MOBGS_METRICS_BOX | MOBGS_METRICS_GAUSS, the windows that are evaluated (at least one); the columns of the other
 *   are NaN.  partial: scratch, mobgs_image_metrics_scratch_doubles(B, H, W) doubles, contents irrelevant on entry.
 * mobgs_image_metrics_scratch_doubles: a host computation; 0 for a shape outside 1 <= B <= 16384, 1 <= H, W <= 32768.
 * Refused with MOBGS_E_INVALID before any launch: a shape outside that range, H or W < 7 with the box arm or < 11 with the
 * Gaussian arm, arms = 0, an unknown bit, a data_range that is not positive and finite, a NULL pred / gt / partial / out,
 * a misaligned pointer.  The inputs are only read; two or three launches, no synchronisation. */
#define MOBGS_METRICS_BOX 1
#define MOBGS_METRICS_GAUSS 2
#define MOBGS_METRICS_CLAMP 1
#define MOBGS_METRICS_QUANTIZE 2
#define MOBGS_METRICS_COLUMNS 9
size_t mobgs_image_metrics_scratch_doubles(int B, int H, int W);
int mobgs_image_metrics(int B, int H, int W, const float* pred, const float* gt, const float* mask, int arms, int flags,
                        double data_range, double* partial, double* out, void* stream);

/* ---- K23: test-time pose refinement: pose head, -PSNR loss, optimiser step ----------------------------------------
 * The pieces of /root/reference/eval.py:43-166 (render_test_tto) around the render, on the caller's stream, without a
 * float atomic and without a read-back (csrc/pose.hip, built with -ffp-contract=off).  All pointers are device pointers,
 * fp32 unless stated, 4-byte aligned.  Entry points only: no struct, signature or scratch format of an earlier ABI
 * version changes, and MOBGS_ABI_VERSION stays as it is.
 *
 * mobgs_pose_head_fwd: q [4] = (r, i, j, k), real part first and NOT normalised; t [3] -> w2c [16], row-major
 *   [[R, t], [0 0 0 1]] with pytorch3d's quaternion_to_matrix as written (eval.py:122-123): two_s = 2 / (q . q),
 *   R = [[1 - two_s (jj + kk), two_s (ij - kr), two_s (ik + jr)], [two_s (ij + kr), 1 - two_s (ii + kk), two_s (jk - ir)],
 *        [two_s (ik - jr), two_s (jk + ir), 1 - two_s (ii + jj)]].  One wave.
 * mobgs_pose_head_bwd: v_w2c [16] -> v_q [4], v_t [3] = v_w2c[3], [7], [11]: the exact Jacobian of the expression above,
 *   two_s included, so the component of v_q along q is zero up to rounding.  q = 0 gives NaN, as the reference.  One wave.
 * mobgs_pose_step: one wave, in this order: (v_q, v_t) = mobgs_pose_head_bwd(q, v_w2c); the Adam update of K16 on the seven
 *   values with their moments exp_avg, exp_avg_sq [7] (q's four, then t's three), the SAME device code as
 *   mobgs_adam_step (csrc/adam_shared.h), step_size_q for q and step_size_t for t (lr / (1 - beta1^step), formed by the
 *   caller as for K16, like bias2_sqrt = sqrt(1 - beta2^step)); w2c = mobgs_pose_head_fwd(q, t) of the updated values;
 *   v_w2c := 0 (the next step's zero_grad).  q, t, the moments and v_w2c are updated in place; bit-identical with the
 *   three separate calls.
 * mobgs_neg_psnr_fwd: pred, gt [n], n = 3 H W values of a [3,H,W] image pair, 1 <= n <= 2^40.
 *   *mse (float64) = sum (pred - gt)^2 / n, differences and squares in fp32 as eval.py:137 forms them, added in float64;
 *   *loss (fp32) = -20 log10(1 / sqrt(mse)) (eval.py:138-139), evaluated in float64 and rounded once; -inf for mse == 0.
 *   Each workgroup adds a fixed contiguous range and a one-workgroup finishing launch adds the partial sums in a
 *   fixed order that depends on their number alone: which element is added where depends on n alone, so the result is bit-identical from run to run AND from
 *   address to address.  A 16-byte aligned array is read 16 bytes at a time, another one element by element.
 *   partial: scratch, mobgs_neg_psnr_scratch_doubles(n) doubles (a host computation; 0 for n outside the range), contents
 *   irrelevant on entry.  Two launches.  The inputs are only read.
 * mobgs_neg_psnr_bwd: v_pred [n] = v_loss 20 / (ln 10 n mse) (pred - gt): the factor from *mse (device, as the forward
 *   left it) and *v_loss (device; NULL = 1) in float64, rounded once; the product in fp32.  mse == 0 gives NaN everywhere,
 *   as autograd does.  v_pred is fully written.  One launch.
 * Refused with MOBGS_E_INVALID before any launch: a NULL pointer (v_loss excepted), a misaligned one (partial and mse:
 * 8 bytes), n outside the range. */
int mobgs_pose_head_fwd(const float* q, const float* t, float* w2c, void* stream);
int mobgs_pose_head_bwd(const float* q, const float* v_w2c, float* v_q, float* v_t, void* stream);
int mobgs_pose_step(float* q, float* t, float* v_w2c, float* exp_avg, float* exp_avg_sq, float step_size_q,
                    float step_size_t, float bias2_sqrt, double beta1, double beta2, double eps, float* w2c,
                    void* stream);
size_t mobgs_neg_psnr_scratch_doubles(int64_t n);
int mobgs_neg_psnr_fwd(int64_t n, const float* pred, const float* gt, double* partial, double* mse, float* loss,
                       void* stream);
int mobgs_neg_psnr_bwd(int64_t n, const float* pred, const float* gt, const double* mse, const float* v_loss,
                       float* v_pred, void* stream);

/* ---- K24: LPIPS (net-lin, AlexNet trunk, v0.1, spatial average, no mask) of a batch of image pairs -----------------
 * What /root/reference/metrics.py:84-85, :127-131 and eval.py:76 evaluate (models/networks_basic.py:68-105,
 * models/pretrained_networks.py:57-95), forward only, on the caller's stream (csrc/lpips.hip).  Entry points only:
 * MOBGS_ABI_VERSION stays as it is.  All device pointers fp32 unless stated.
 *
 * The computation, per pair (img0, img1), both [3,H,W]:
 *   x = img (MOBGS_LPIPS_UNIT_RANGE: 2 img - 1), then (x - shift_c) / scale_c with shift (-.030, -.088, -.188) and scale
 *   (.458, .448, .450); the trunk conv(3->64, k 11, stride 4, pad 2) ReLU [tap 1] maxpool(3, 2) conv(64->192, k 5, pad 2) ReLU
 *   [tap 2] maxpool(3, 2) conv(192->384, k 3, pad 1) ReLU [tap 3] conv(384->256, k 3, pad 1) ReLU [tap 4] conv(256->256, k 3,
 *   pad 1) ReLU [tap 5], every convolution with a bias and zero padding of its own input (the first one pads the SCALED
 *   tensor); per tap and pixel n = f / (sqrt(sum_c f^2) + 1e-10) for both images, sum_c lin_c (n0 - n1)^2, the mean over
 *   the tap's pixels; the total is the sum of the five layer values.
 * The convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32: every output is one k-ordered fmaf chain over
 * K = (ky, kx, ci), whatever tile it falls into); activations are channel-last [2B, h, w, C] with image 2b = img0 of pair b
 * and 2b + 1 = img1.  Norms, differences and the head dot product are fp32; a workgroup's sum over its 64 pixels and
 * everything after it is float64, in an order that depends on the tap's size alone; no float atomics.  So a pair's row
 * is bit-identical from run to run, whatever B is and wherever the pair sits in the batch, and exactly 0 for equal images.
 *
 * MobgsLpipsWeights (host struct, read before the call returns; device pointers, 16-byte aligned):
 *   w1 .. w5    the convolution weights PACKED [Kpad, Cout]: row k = (ky * ks + kx) * Cin + ci for layers 2 .. 5, row
 *               k = (ci * 11 + ky) * 11 + kx for layer 1 (Cin = 3: the image is read channel-first), rows K .. Kpad - 1
 *               zero.  Kpad = mobgs_lpips_pack_k(layer): K rounded up to the kernel's K step (363 -> 384; the others are
 *               multiples of it already).  layer = 1 .. 5; 0 for another value.
 *   b1 .. b5    the biases [Cout];  lin1 .. lin5: the head weights [Cout] (>= 0).
 * flags: MOBGS_LPIPS_UNIT_RANGE: the images are in [0, 1] and are mapped to [-1, 1] inside (without it they are taken as
 *   [-1, 1] already); MOBGS_LPIPS_CLAMP: both images are clamped to [0, 1] first; MOBGS_LPIPS_QUANTIZE: img1, the
 *   prediction in the reference's call order, is then replaced by floor(clip(img1, 0, 1) * 255) / 255 in fp32 (eval.py:162,
 *   as K22 does).  Clamp and quantize act on the values as given, before the 2 x - 1.
 * scratch: mobgs_lpips_scratch_bytes(B, H, W) bytes, 256-byte aligned, contents irrelevant on entry (two activation
 *   regions the layers alternate between, and the float64 partial sums).  A host computation; 0 for a shape that is
 *   refused.  Scratch grows with B: callers with a budget split the batch, which does not change a bit of any pair's row.
 * out [B, MOBGS_LPIPS_COLUMNS] float64 (device): the total, then the five layer values.
 * taps: NULL, or a HOST array of five device pointers (16-byte aligned) that receive the ReLU maps [2B, h_l, w_l, C_l] of
 *   all images, channel-last; the layers then read their input from there.  Sizes: h_1 = (H - 7) / 4 + 1, pooled
 *   p = (h - 3) / 2 + 1, h_2 = p(h_1), h_3 = h_4 = h_5 = p(h_2) (integer division; widths alike); C = 64, 192, 384, 256, 256.
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: a NULL pointer (taps excepted, but not one
 *   of its five), B < 1 or B > 4096, H or W < 31 (below that the second pool has no output) or > 16384, 2 B h_1 w_1 > 2^30,
 *   an unknown flag, a misaligned pointer, scratch_bytes smaller than the size query's answer.
 * 13 launches (5 convolutions, 2 pools, 5 distance kernels, one finishing workgroup), no synchronisation, no read-back. */
#define MOBGS_LPIPS_UNIT_RANGE 1
#define MOBGS_LPIPS_CLAMP 2
#define MOBGS_LPIPS_QUANTIZE 4
#define MOBGS_LPIPS_COLUMNS 6
typedef struct MobgsLpipsWeights {
    const float *w1, *w2, *w3, *w4, *w5;
    const float *b1, *b2, *b3, *b4, *b5;
    const float *lin1, *lin2, *lin3, *lin4, *lin5;
} MobgsLpipsWeights;
size_t mobgs_lpips_scratch_bytes(int B, int H, int W);
int mobgs_lpips_pack_k(int layer);
int mobgs_lpips_alex(int B, int H, int W, const float* img0, const float* img1, const MobgsLpipsWeights* weights,
                     int flags, void* scratch, size_t scratch_bytes, double* out, float* const* taps, void* stream);

/* ---- K24, spatial and masked forms: the per-pixel LPIPS map and the two masked averages ---------------------------------
 * What PNetLin.forward computes under spatial=True (models/networks_basic.py:24-28, :79-80) and with mask= (:16-22, :82),
 * and what dycheck's compute_lpips reduces the map to (dycheck_metrics.py:203-244).  Same trunk, weights, flags, layout and
 * per-pixel arithmetic as mobgs_lpips_alex, whose results keep their bits.  Entry points only: MOBGS_ABI_VERSION stays.
 *
 * Let d_l [h_l, w_l] be the head-weighted squared difference of the channel-normalised taps of a pair (the value
 * mobgs_lpips_alex averages), l = 1 .. 5, fp32.
 *   map [H, W] = up(d_1) + up(d_2) + ... + up(d_5), added in fp32 in that order; up is bilinear, align_corners = False, onto
 *     H x W: source coordinate max(s (dst + 0.5) - 0.5, 0) with s = (float)h / (float)H formed on the host (one fp32 fma),
 *     i0 = (int)src, i1 = i0 + (i0 < h - 1), t = src - i0, value (1 - ty) ((1 - tx) a + tx b) + ty ((1 - tx) c + tx d).  This
 *     is nn.Upsample(size = (H, W)): defined for every size (the reference's scale_factor form yields H - 1 rows for some).
 *   m_l = the mask resized to (h_l, w_l) by nearest neighbour: row min((int)floorf(i sH), H - 1) with sH = (float)H /
 *     (float)h_l and the product rounded to fp32; columns alike.  d_l m_l is formed in fp32, every sum is float64.
 * mask [B, H, W] fp32 in [0, 1], or NULL = all ones (the same bits as a mask of ones).
 * map [B, H, W] fp32 or NULL: receives the map; the row in `out` has the same bits with and without it.
 * out [B, MOBGS_LPIPS_SPATIAL_COLUMNS] float64 (device), per pair:
 *   0        mean of the map, sum(map) / (H W)
 *   1        dycheck's masked mean, sum(map m) / max(sum(m), 1e-6)   (map m exact in float64)
 *   2, 3, 4  sum(map m), sum(m), sum(map)
 *   5        the sum of the five masked layer values (columns 6 .. 10, added in that order)
 *   6 .. 10  the reference's masked average per layer, numerator_l / (denominator_l + 1e-8)
 *   11 .. 15 numerator_l = sum(d_l m_l);  16 .. 20 denominator_l = sum(m_l)
 *   An empty mask gives 0 in columns 1 and 5 .. 10, never NaN; equal images give a map of +0 and 0 in every column but 3
 *   and 16 .. 20.  (The reference's mask= form divides sums over the WHOLE batch: callers form that from 11 .. 20.)
 * scratch: mobgs_lpips_spatial_scratch_bytes(B, H, W) bytes, 256-byte aligned, contents irrelevant on entry (the scratch of
 *   mobgs_lpips_alex, the five d maps -- sum h_l w_l floats per pair -- and the float64 partial sums).  0 for a refused shape.
 * Every sum has a fixed order that depends on the sizes alone; a pair is a grid index; no atomics.  So a pair's row and map
 * are bit-identical from run to run, whatever B is and wherever the pair sits in the batch.
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: as mobgs_lpips_alex (mask and map may be
 *   NULL; 4-byte aligned otherwise).
 * 15 launches (5 convolutions, 2 pools, 5 distance-map kernels, the masked sums, the upsample-and-reduce kernel, one finish),
 * no synchronisation, no read-back. */
#define MOBGS_LPIPS_SPATIAL_COLUMNS 21
size_t mobgs_lpips_spatial_scratch_bytes(int B, int H, int W);
int mobgs_lpips_alex_spatial(int B, int H, int W, const float* img0, const float* img1, const MobgsLpipsWeights* weights,
                             const float* mask, int flags, void* scratch, size_t scratch_bytes, float* map, double* out,
                             void* stream);

/* ---- K24, backward: the gradient of the LPIPS total with respect to the images (LPIPS as a training loss) -----------
 * What autograd gives the reference's lpips_loss (utils/loss_utils.py:228-230) through PNetLin.forward, for the images only
 * (the trunk and the heads are constants).  Same trunk, weights, flags and layout as mobgs_lpips_alex, whose results keep
 * their bits (csrc/lpips.hip).  Entry points only: MOBGS_ABI_VERSION stays.
 *
 * taps: a HOST array of the five device pointers that a mobgs_lpips_alex call with the same B, H, W, images, weights and
 *   flags filled ([2B, h_l, w_l, C_l], channel-last); only read.
 * v_total [B] fp32: the cotangent of column 0 of the forward's row, per pair.
 * g_img0 / g_img1 [B,3,H,W] fp32, fully written: the gradient with respect to img0 / img1 as the caller passed them (through
 *   the scaling layer, the 2 x - 1 of MOBGS_LPIPS_UNIT_RANGE and the clamp of MOBGS_LPIPS_CLAMP, which passes the gradient
 *   where 0 <= img <= 1, bounds included, as torch.clamp does).  NULL = that side is not wanted: only the wanted images are
 *   walked.  Both NULL is refused.  MOBGS_LPIPS_QUANTIZE with a wanted g_img1 is refused: the truncation has no gradient.
 * bwd_weights (host struct, device pointers, 16-byte aligned): w2 .. w5, the weights of layers 2 .. 5 packed for the
 *   backward-data pass [Cout k k, Cin]: row (ky k + kx) Cout + co holds weight[co, ci, k - 1 - ky, k - 1 - kx] in column ci
 *   (the taps flipped, the channel axes exchanged).  mobgs_lpips_bwd_pack_k(layer) = Cout k k for layer = 2 .. 5 (4800, 3456,
 *   2304, 2304: multiples of the K step), 0 for another value.  Layer 1 reads the forward's w1.
 * tap_grads: NULL, or a HOST array of five device pointers (16-byte aligned) that receive the gradient with respect to the
 *   five pre-activations (the ReLU mask applied), [n B, h_l, w_l, C_l] channel-last, n = the number of wanted sides: image
 *   n b + k is the k-th wanted side of pair b.  The image gradients have the same bits with and without it.
 * scratch: mobgs_lpips_bwd_scratch_bytes(B, H, W) bytes, 256-byte aligned, contents irrelevant on entry; 0 for a refused
 *   shape.
 *
 * Per tap and pixel, with u the wanted side's vector and v the other one: a = |u| + 1e-10, b = |v| + 1e-10,
 *   e = u / a - v / b, s = 2 lin e, dd/du = s / a - u (sum s u) / (a^2 |u|), times v_total / (h_l w_l); fp32, one wave per
 *   pixel.  Where |u| = 0 the second term is DEFINED as 0 (autograd's sqrt gives inf 0 = NaN there); the ReLU mask u > 0
 *   removes the first.  The backward-data pass of layers 5 .. 2 is the forward's implicit GEMM (rows = the wanted images'
 *   pixels) with an epilogue that adds the tap's own distance gradient and applies the mask; max-pool backward is a gather:
 *   a position takes the gradient of each of its <= 2 x 2 windows whose maximum it is, the FIRST one in row-major order on
 *   ties (torch's rule); layer 1 is a direct gather per image pixel.  No float atomics, no hand-off between workgroups; every
 *   sum has an order fixed by the shapes: a pair's gradient is bit-identical from run to run, whatever B, the pair's place in
 *   the batch and the set of wanted sides, and exactly +0 for equal images (v_total >= 0).  Pixels in no window of the first
 *   convolution and pixels the clamp cuts get exactly 0.
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: as mobgs_lpips_alex, and the above.
 * 11 launches and one per wanted side (5 distance kernels, 4 GEMMs, 2 pool gathers; the image kernel), no
 * synchronisation, no read-back. */
typedef struct MobgsLpipsBwdWeights {
    const float *w2, *w3, *w4, *w5;
} MobgsLpipsBwdWeights;
size_t mobgs_lpips_bwd_scratch_bytes(int B, int H, int W);
int mobgs_lpips_bwd_pack_k(int layer);
int mobgs_lpips_alex_bwd(int B, int H, int W, const float* img0, const float* img1, const MobgsLpipsWeights* weights,
                         const MobgsLpipsBwdWeights* bwd_weights, int flags, const float* const* taps,
                         const float* v_total, void* scratch, size_t scratch_bytes, float* g_img0, float* g_img1,
                         float* const* tap_grads, void* stream);

/* ---- K25: tOF, the temporal optical-flow metric: dense Farneback flow and the distance of two flow fields -----------
 * What the reference's metrics.py:14-47 and :108-120 evaluate: cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15,
 * 3, 5, 1.2, 0) between consecutive 8-bit grey frames, for the prediction and for the ground truth, and the mean of
 * |flow_gt - flow_pred|_2 over the crop_8x8 window.  Forward only, on the caller's stream (csrc/tof.hip, built with
 * -ffp-contract=off).  Entry points only: MOBGS_ABI_VERSION stays as it is.  OpenCV could not be run where this was
 * written: the algorithm is a restatement (README, "UNPINNED"; tests/tof_restatement.py is the same text in float64).
 * Device pointers are fp32 unless stated, 4-byte aligned; every input is only read; no call synchronises, allocates or
 * reads back, so all of them can be recorded into a graph.  A frame pair is a grid index and there is no float atomic: a
 * pair's result is bit-identical from run to run and does not depend on the batch around it.
 * x = column; flow channel 0 = u along x, channel 1 = v along y, from the pair's first frame to its second.
 *
 * mobgs_tof_levels: a host computation (no device is touched).  scale = 1; for k = 0, 1, 2: scale *= 0.5, stop if W scale
 *   < 32 or H scale < 32; L = the k reached.  out[i], i = 0 .. L, COARSEST FIRST (k = L - i, s = 0.5^k): width = rint(W s),
 *   height = rint(H s) (half to even), sigma = (1 / s - 1) / 2, taps = max(rint(5 sigma) | 1, 3).  Returns L + 1 (1 .. 4),
 *   or 0 for a NULL out or a size outside 48 <= H, W <= 16384 (below 48 the crop window is empty).  out holds 4 records.
 * mobgs_tof_crop: yxhw (HOST, 4 x int32) = crop_8x8's window (metrics.py:32-47): h = (H / 32) 32, minus 32 while h > H - 16,
 *   y = (H - h) / 2; w and x alike.  A host computation.
 * mobgs_tof_grey: rgb [F,3,H,W] -> grey [F,H,W], 8-bit values held as fp32.  Per channel: with MOBGS_METRICS_CLAMP, clip to
 *   [0, 1]; with MOBGS_METRICS_QUANTIZE, floor(clip(x) * 255) / 255 in fp32 (the written PNG read back, metrics.py:100);
 *   then trunc(fl32(x * 255)), saturated to 0 .. 255 (metrics.py:109-110: the product is formed in fp32 as numpy forms
 *   it; on k / 255 that round trip is the identity for all 256 k, tests/test_tof_cpu.py); then OpenCV's 8-bit COLOR_RGB2GRAY, (4899 R + 9617 G + 1868 B + 8192) >> 14.  1 launch.
 * mobgs_tof_pyramid_level: grey [F,H,W] -> out [F,height,width]: the Gaussian blur of the full-size image (taps, sigma;
 *   the taps exp(-t^2 / (2 sigma^2)) normalised to sum 1, [1/4, 1/2, 1/4] for sigma = 0; reflect-101 border) resized
 *   bilinearly (sx = (dx + 0.5) W / width - 0.5, clamped to [0, W - 1]).  level: one HOST record as mobgs_tof_levels fills
 *   them (odd taps in 3 .. 19, sigma >= 0, a size not above the image's).  1 launch.
 * mobgs_tof_polyexp: img [F,h,w] -> R [F,5,h,w] = (r_x, r_y, r_xx, r_yy, r_xy): per pixel the coefficients of x, y, x^2, y^2,
 *   xy of the least-squares fit of (1, x, y, x^2, y^2, xy) over the 11x11 window under the weight g(x) g(y), g ~ exp(-t^2 /
 *   (2 1.2^2)) normalised to sum 1; samples outside the image are replicated.  1 launch; run it once per frame and level.
 * mobgs_tof_update_matrices: R [P+1,5,h,w] (pair p = frames p, p + 1) -> M [P,5,h,w] = (G11, G12, G22, h1, h2).  The flow
 *   (u, v) of a pixel: 0 if flow is NULL; flow [P,src_h,src_w,2] itself if (src_h, src_w) = (h, w); otherwise that field
 *   resized bilinearly to (h, w) (as above) and multiplied by 2.  flow_out [P,h,w,2] or NULL receives the flow used.  With
 *   S = R1 sampled bilinearly at (x + u, y + v) if 0 <= floor(x + u) < w - 1 and 0 <= floor(y + v) < h - 1:
 *     in bounds: a_xx = (R0.xx + S.xx) / 2, a_yy alike, a_xy = (R0.xy + S.xy) / 4, b_x = (R0.x - S.x) / 2, b_y alike;
 *     otherwise: a_xx = R0.xx, a_yy = R0.yy, a_xy = R0.xy / 2, b_x = R0.x / 2, b_y = R0.y / 2;
 *     b_x += a_xx u + a_xy v, b_y += a_xy u + a_yy v; all five times the product of the border factors of the four sides,
 *     t[d] = (0.14, 0.14, 0.4472, 0.4472, 0.4472) for a distance d = 0 .. 4 to that side, 1 beyond;
 *     G11 = a_xx^2 + a_xy^2, G12 = (a_xx + a_yy) a_xy, G22 = a_yy^2 + a_xy^2, h1 = a_xx b_x + a_xy b_y, h2 = a_xy b_x + a_yy b_y.
 *   A flow that is not finite, or beyond 1e6 pixels, counts as out of bounds.  1 launch.
 * mobgs_tof_blur_solve: M_in [P,5,h,w] -> flow [P,h,w,2] (fully written): the 15x15 box MEAN of the five values (replicate
 *   border, float64), det = G11 G22 - G12^2 + 1e-3, u = (G22 h1 - G12 h2) / det, v = (G11 h2 - G12 h1) / det.  With M_out
 *   (and R) not NULL the update matrices of the NEW flow are written to M_out in the same launch, bit-identical with a
 *   mobgs_tof_update_matrices call on that flow; M_out must not be M_in.  1 launch.
 * mobgs_tof_flow: grey [F,H,W] -> flow_out [F-1,H,W,2], the flows of the F - 1 consecutive pairs.  Per level, coarsest
 *   first: the level image and the expansion of every FRAME once, the first update matrices from the coarser level's flow
 *   (zero at the coarsest), three rounds of mobgs_tof_blur_solve, the first two with the next update fused in.  6 launches
 *   per level, at most 24.  scratch: mobgs_tof_scratch_bytes(F, H, W) bytes (a host computation; 0 for a shape that is
 *   refused), 256-byte aligned, contents irrelevant on entry.  It grows with F: a caller with a budget splits the frames
 *   into runs that overlap by one, which does not change a bit of any pair's flow.
 * mobgs_tof_score: flow_a, flow_b [P,H,W,2], mask [P,H,W] or NULL -> out [P] float64 (device): over crop_8x8's window,
 *   the mean of sqrt(du^2 + dv^2) (float64 from the differences on), or sum(. mask) / sum(mask) (NaN for
 *   an empty mask, as the reference's 0 / 0).  partial: scratch, mobgs_tof_score_scratch_doubles(P, H, W) float64 (a host
 *   computation; 0 for a refused shape), contents irrelevant on entry.  Fixed summation order; 2 launches.
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: a NULL pointer (the optional ones
 *   excepted) or a misaligned one (scratch 256 bytes, partial and out 8), a count outside 1 .. 4096 (mobgs_tof_flow: F < 2),
 *   an image below 48 or above 16384 on a side (grey, the stage calls on a level: below 2), an unknown flag, a level record
 *   outside the ranges above, a src size above the level's. */
typedef struct MobgsTofLevel {
    int width, height, taps;
    double sigma;
} MobgsTofLevel;
int mobgs_tof_levels(int H, int W, MobgsTofLevel* out);
int mobgs_tof_crop(int H, int W, int32_t* yxhw);
size_t mobgs_tof_scratch_bytes(int F, int H, int W);
size_t mobgs_tof_score_scratch_doubles(int P, int H, int W);
int mobgs_tof_grey(int F, int H, int W, const float* rgb, int flags, float* grey, void* stream);
int mobgs_tof_pyramid_level(int F, int H, int W, const float* grey, const MobgsTofLevel* level, float* out, void* stream);
int mobgs_tof_polyexp(int F, int h, int w, const float* img, float* R, void* stream);
int mobgs_tof_update_matrices(int P, int h, int w, const float* R, const float* flow, int src_h, int src_w,
                              float* flow_out, float* M, void* stream);
int mobgs_tof_blur_solve(int P, int h, int w, const float* M_in, float* flow, const float* R, float* M_out, void* stream);
int mobgs_tof_flow(int F, int H, int W, const float* grey, void* scratch, float* flow_out, void* stream);
int mobgs_tof_score(int P, int H, int W, const float* flow_a, const float* flow_b, const float* mask, double* partial,
                    double* out, void* stream);

/* ---- K26: report sheets: the panels of render_training_image composed as 8-bit images on the device -----------------
 * What the reference's utils/scene_utils.py:15-260 builds on the host, one .cpu().numpy() round trip per panel: here a
 * sheet is laid out as uint8 on the device and copied once (csrc/report.hip, built with -ffp-contract=off).  Entry points
 * only: MOBGS_ABI_VERSION stays as it is.  Two launches per sheet on the caller's stream; neither synchronises,
 * allocates or reads back, so both can be recorded into a graph.  Every input is fp32, only read, finite (NaN handling is
 * not defined), 4-byte aligned (flow maps, [H,W,2]: 8).  The records are HOST arrays; their pointers are device pointers.
 *
 * mobgs_report_stats: for map m of stats_host, stats[2 m] = its minimum and stats[2 m + 1] = its maximum, bit-equal to
 *   torch.amin / torch.amax of the same fp32 expression (min and max do not depend on an order; integer atomics on the
 *   ordered bit patterns).  kind MINMAX: the n values of a.  SQERR: (a[i] - b[i])^2, the difference and the square each
 *   rounded to fp32; the error map is not stored.  FLOW_RAD: a is [n,2]; sqrt(u u + v v) with every operation rounded as
 *   numpy's float32 statements round it (no fused multiply-add, the correctly rounded root), after clipping u and v to
 *   [0, clip] if clip >= 0 (flow_vis' clip_flow); the maximum is flow_to_color's rad_max.
 *   stats: mobgs_report_stats_floats(n_stats) floats (a host computation; 0 for a count outside 1 .. MAX_STATS): the
 *   2 n_stats results, then words the call zeroes and merges into.  1 memset + 1 launch.
 * mobgs_report_compose: sheet (uint8, fully written) = the n_panels panels side by side, [H, n_panels W, 3] (row-major,
 *   channel-last, as PIL.Image.fromarray takes it), or with vertical != 0 one below the other, [n_panels H, W, 3], so that
 *   every panel is a contiguous [H,W,3] image.  Every panel ends in (np.clip(x, 0, 1) * 255).astype('uint8'), i.e.
 *   floor(clamp01(x) 255).  kind:
 *     RGB           a [3,H,W]
 *     GREY          a [1,H,W], repeated over the three channels
 *     GREY_DIV_MAX  a [1,H,W] / max, max = stats[2 slot + 1] (scene_utils.py:177-179); 0 where max is 0 (the reference
 *                   divides by zero there)
 *     ERROR         (e - min) / max(max - min, 1e-8), e = (a - b)^2 per channel, a and b [3,H,W], (min, max) = the slot's
 *                   pair (scene_utils.py:187-188)
 *     SIGNED3       (a + 1) / 2, a [3,H,W]
 *     NORMALS_FD    a = depth [1,H,W]; scene_utils.py:130-163, :185: z = depth + 1e-6; directions ((px - cx - y skew) /
 *                   focal, y = (py - cy) / focal, 1), px = column + pixel_offset; forward differences along the row and
 *                   the column, the last column / row repeating its neighbour's; the cross product as written,
 *                   F.normalize (eps 1e-12), (n + 1) / 2.  Needs H, W >= 2.  (Not main_utils.get_normals: K15.)
 *     FLOW          a [H,W,2]; flow_vis.flow_to_color (convert_to_bgr = False): with rad_max = stats[2 slot + 1],
 *                   u, v (clipped to [0, clip] if clip >= 0) divided by rad_max + 1e-5; rad = sqrt(u u + v v);
 *                   a = atan2f(-v, -u) / pi_f; fk = (a + 1) / 2 * 54; k0 = floor(fk), k1 = k0 + 1 (55 -> 0), f = fk - k0;
 *                   per channel col = (1 - f) wheel[k0] / 255 + f wheel[k1] / 255, then 1 - rad (1 - col).  The wheel: 55
 *                   entries, segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6.  flow_vis could not be run where this was
 *                   written: a restatement (README, "UNPINNED"; tests/report_restatement.py is the same text in float64).
 *   A sheet has at most 2^30 pixels.  1 launch; a lane stores 12 bytes as three aligned dwords.
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: a count or size outside its range, an
 *   unknown kind, a NULL or misaligned pointer (b and stats may be NULL where no panel reads them), a statistics slot
 *   outside 0 .. n_stats - 1, a NORMALS_FD panel with H < 2, W < 2 or focal == 0. */
#define MOBGS_REPORT_RGB 0
#define MOBGS_REPORT_GREY 1
#define MOBGS_REPORT_GREY_DIV_MAX 2
#define MOBGS_REPORT_ERROR 3
#define MOBGS_REPORT_SIGNED3 4
#define MOBGS_REPORT_NORMALS_FD 5
#define MOBGS_REPORT_FLOW 6
#define MOBGS_REPORT_MAX_PANELS 16
#define MOBGS_REPORT_STAT_MINMAX 0
#define MOBGS_REPORT_STAT_SQERR 1
#define MOBGS_REPORT_STAT_FLOW_RAD 2
#define MOBGS_REPORT_MAX_STATS 32
#define MOBGS_REPORT_WHEEL 55
typedef struct MobgsReportStat {
    int32_t kind;
    int64_t n;
    const float *a, *b;
    float clip;
} MobgsReportStat;
typedef struct MobgsReportPanel {
    int32_t kind, slot;
    const float *a, *b;
    float clip;
} MobgsReportPanel;
size_t mobgs_report_stats_floats(int n_stats);
int mobgs_report_stats(int n_stats, const MobgsReportStat* stats_host, float* stats, void* stream);
int mobgs_report_compose(int H, int W, int n_panels, const MobgsReportPanel* panels_host, const float* stats,
                         int n_stats, float focal, float cx, float cy, float skew, float pixel_offset, int vertical,
                         uint8_t* sheet, void* stream);

/* ---- K27: the Adam step of K16 with its factors formed ON THE DEVICE, from tables and counters in device memory ------
 * mobgs_adam_step (K16) takes step_size = lr / (1 - beta1^t) and bias2_sqrt = sqrt(1 - beta2^t) per tensor from the host:
 * recorded into a graph they freeze, and so does a learning rate set on the host.  Here the host tabulates once -- the
 * learning rate of every iteration, and 1 - beta1^t and sqrt(1 - beta2^t) for every step count t, all as float64, each
 * formed by the host statements the eager path uses -- and the device only indexes (csrc/adam_dev.hip).  Entry points
 * and structs only: MOBGS_ABI_VERSION stays as it is.  Two launches per step on the caller's stream; neither synchronises,
 * allocates or reads back, and no argument changes between steps, so both can be recorded into a graph and replayed.
 * Every pointer below is a DEVICE pointer, the descriptor arrays included.
 *
 * mobgs_adam_dev_factors: counters = [iteration, step_0 .. step_{n-1}] (int32).  For tensor i, with row = iteration
 *   clamped to 0 .. lr_rows - 1 and t = step_i + 1 clamped to 0 .. bc_rows - 1:
 *     factors[2 i]     = (float)(lr[row * lr_stride] / bc1[t])      (the correctly rounded double quotient, rounded to
 *     factors[2 i + 1] = (float)bc2s[t]                              fp32 as a host c_float is: K16's host factors, bit for bit)
 *   then step_i and iteration advance by one.  lr_stride = 0: a constant rate (one value).  The clamps keep every read
 *   inside the tables; refusing a step past the last row is the caller's job.  One workgroup, integer state, no atomics.
 * mobgs_adam_dev_step: K16's update (csrc/adam_shared.h: the same float4 body, scalar tail and alignment test) on
 *   n_tensors tensors, descriptor and factors read from device memory by the block's tensor index: no limit of 64.
 *   w1 = (float)(1 - beta1), beta2, w2 = (float)(1 - beta2) and eps travel in the descriptor, so tensors of several
 *   (betas, eps) classes share a launch.  longest: the largest n among the descriptors (sizes the grid; a tensor is
 *   never accessed at or beyond its own n whatever longest says).  n = 0: nothing is read or written.
 * Refused with MOBGS_E_INVALID before any launch: a negative count, n_tensors > 65535 (the grid's second dimension), a
 *   NULL array with n_tensors > 0, a negative longest or one that needs more than 2^31 - 1 workgroups. */
typedef struct MobgsAdamDevSchedule {
    const double *lr, *bc1, *bc2s;
    int32_t lr_stride, lr_rows, bc_rows, reserved;
} MobgsAdamDevSchedule;
typedef struct MobgsAdamDevTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    float w1, beta2, w2, eps;
} MobgsAdamDevTensor;
int mobgs_adam_dev_factors(int n_tensors, const MobgsAdamDevSchedule* schedules_dev, int32_t* counters_dev,
                           float* factors_dev, void* stream);
int mobgs_adam_dev_step(int n_tensors, const MobgsAdamDevTensor* tensors_dev, const float* factors_dev, int64_t longest,
                        void* stream);

/* ---- K28: the HexPlane grid regularisers: smoothness along h, total variation, |1 - t| of the time planes -------------
 * The reference's scene/regulation.py:13-28 (compute_plane_tv, compute_plane_smoothness) and scene/gaussian_model.py:
 * 1373-1415 (_plane_regulation, _time_regulation, _l1_regulation, compute_regulation) for ALL planes of a call at once
 * (csrc/gridreg.hip, built with -ffp-contract=off).  Entry points and a struct only: MOBGS_ABI_VERSION stays as it is.
 * Two launches forward, one backward, on the caller's stream; none synchronises, allocates, zero-fills or reads back and
 * there are no atomics, so all can be recorded into a graph, and the same planes give the same bits.
 *
 * planes_host: a HOST array of n_planes records; t and grad are DEVICE pointers.  A plane is [C, h, w] fp32 with element
 *   strides sc, sh, sw, one of which must be the unit direction: sc == 1 (channels-last; C == 1 counts) or sw == 1 (NCHW;
 *   w == 1 counts); anything else is the caller's to copy.  h is the direction the differences run along.  kind:
 *     SMOOTH     S0 = sum of sd^2, sd[k] = (t[k+2] - t[k+1]) - (t[k+1] - t[k]) along h, every difference rounded to fp32 as
 *                the reference's statements round it, the square and the sum in float64; out[slot] += S0 inv0
 *                (inv0 = 1 / (C (h - 2) w) for the reference's mean).  Needs h >= 3: the reference yields NaN below.
 *     TV         S0 = sum of squared first differences along h, S1 = along w; out[slot] += 2 (S0 inv0 + S1 inv1)
 *                (compute_plane_tv: inv0 = 1 / (C (h - 1) w + 1e-6), inv1 = 1 / (C h (w - 1) + 1e-6))
 *     L1         S1 = sum of |1 - t| (the difference in fp32); out[slot] += S1 inv1
 *     SMOOTH_L1  both on one read of the plane: out[slot] += S0 inv0, out[slot + 1] += S1 inv1
 *   Several records may share a slot (the planes of a term; the images of a batch, each with the batch's count).
 * mobgs_gridreg_blocks: workgroups of the streaming launch for this table (a host computation; 0 for a table that
 *   would be refused).  partial: scratch, [blocks, 2] doubles, contents irrelevant on entry.
 * mobgs_gridreg_fwd: out[0 .. n_slots) = the slots' float64 sums rounded to fp32 once.  weights (DEVICE, [n_slots]) and
 *   total (one float), both given or both NULL: *total = ((weights[0] out[0]) + weights[1] out[1]) + ... in fp32, left to
 *   right.  grad is not read.
 * mobgs_gridreg_bwd: grad of every record, fully written (no zero-fill needed), DENSE in the plane's arm: [h][w][C] for a
 *   channels-last plane, [C][h][w] for an NCHW one.  The cotangent of slot s is v_out[s], or with weights
 *   v_out[0] weights[s] (v_out is then the cotangent of the weighted total); read from device memory.  An element is
 *   (float)(2 inv0 cot (sd[j-2] - 2 sd[j-1] + sd[j]) - inv1 cot' sign(1 - t[j])), the combination in float64 and rounded
 *   once, with sd = 0 where the window leaves the plane and sign(0) = 0 as torch.abs has it; TV:
 *   (float)(4 inv0 cot (dh[j-1] - dh[j]) + 4 inv1 cot (dw[i-1] - dw[i])).
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: n_planes outside 1 .. MAX_PLANES,
 *   n_slots outside 1 .. MAX_SLOTS, a NULL table, plane, partial, out or v_out (grad: backward only), a misaligned
 *   pointer, a non-positive C, h or w, a negative stride, no unit-stride direction, an unknown kind, a slot outside the
 *   outputs, h < 3 with a smoothness kind, a negative or NaN reciprocal, a plane spanning 2^31 elements or more. */
#define MOBGS_GRIDREG_SMOOTH 0
#define MOBGS_GRIDREG_TV 1
#define MOBGS_GRIDREG_L1 2
#define MOBGS_GRIDREG_SMOOTH_L1 3
#define MOBGS_GRIDREG_MAX_PLANES 32
#define MOBGS_GRIDREG_MAX_SLOTS 4
typedef struct MobgsGridPlane {
    const float* t;
    float* grad;
    int32_t C, h, w, kind, slot, reserved;
    int64_t sc, sh, sw;
    double inv0, inv1;
} MobgsGridPlane;
int mobgs_gridreg_blocks(int n_planes, const MobgsGridPlane* planes_host, int n_slots);
int mobgs_gridreg_fwd(int n_planes, const MobgsGridPlane* planes_host, int n_slots, const float* weights,
                      double* partial, float* out, float* total, void* stream);
int mobgs_gridreg_bwd(int n_planes, const MobgsGridPlane* planes_host, int n_slots, const float* weights,
                      const float* v_out, void* stream);

/* ---- K29: one-launch snapshot / restore of a per-splat table (training checkpoints, mobgs_amd/checkpoint.py) -----------
 * The table of K13 (parameters, Adam moments, statistics, the uint8 deformation table, the integer knot counts) as ONE
 * packed block and back (csrc/snapshot.hip).  Entry points and a struct only: MOBGS_ABI_VERSION stays as it is.  One launch
 * each on the caller's stream; neither synchronises, allocates or reads back.  Not meant to be recorded into a graph: n
 * changes with every densification.  fields_dev is a DEVICE array of n_fields records; rows, block and sum_dev are device
 * pointers.
 *
 * Packed layout: field f occupies the slot [offset, offset + round16(n row_bytes)) of the block; every offset and the
 *   block's base are multiples of 16, slots do not overlap (the caller lays them out: checkpoint.pack_layout).  The copy
 *   is byte-wise, whatever the element type.  A 16-byte lane is one access where the field's base is 16-byte aligned, four
 *   4-byte accesses where it is 4-byte aligned, bytes otherwise; the lane with the field's last bytes goes byte by byte.
 * mobgs_rows_snapshot: slot_f = rows_f[0, n row_bytes) followed by zeros to the slot's end (< 16 bytes), for every field;
 *   nothing of a field is read at or beyond n row_bytes and nothing of the block is written outside the slots.
 *   *sum_dev += the sum of the 32-bit words of all slots as an unsigned 64-bit integer (one atomic add per workgroup; an
 *   integer sum has no order); the caller zeroes it beforehand.  zero_new is not read.
 * mobgs_rows_restore: rows_f[0, n row_bytes) = the slot's first n row_bytes bytes; a field with zero_new != 0 also gets
 *   zeros in rows [n, capacity); rows [n, capacity) of every other field are not written.
 * longest_row_bytes: the largest row_bytes among the records (sizes the grid; a field is never touched beyond its own
 *   size whatever this says).  n = 0 or row_bytes = 0: nothing of that field is read or written.
 * Refused with MOBGS_E_INVALID before any launch: n_fields outside 0 .. 65535, a negative n or longest_row_bytes, capacity
 *   below n, a NULL table, block or sum, a block that is not 16-byte aligned, sizes that overflow 63 bits, more than
 *   2^31 - 1 workgroups.  The records live in device memory and are the caller's to get right. */
typedef struct MobgsRowsField {
    void* rows;
    int64_t row_bytes, offset;
    int32_t zero_new, reserved;
} MobgsRowsField;
int mobgs_rows_snapshot(int n_fields, const MobgsRowsField* fields_dev, int64_t n, int64_t longest_row_bytes, void* block,
                        uint64_t* sum_dev, void* stream);
int mobgs_rows_restore(int n_fields, const MobgsRowsField* fields_dev, int64_t n, int64_t capacity,
                       int64_t longest_row_bytes, const void* block, void* stream);

/* ---- K33: probes of the cross-lane primitives and the fixed-order sums (test support) ------------------------------------
 * One launch of a thin kernel that loads per-thread values, calls ONE function of csrc/wave_shared.h or
 * csrc/reduce_shared.h and stores what every thread holds afterwards (csrc/lane_probe.hip), so that lane coverage,
 * placement and summation order of each primitive can be compared bit for bit with tests/lane_model.py.  Not part of the
 * drop-in surface.  An entry point and constants only: MOBGS_ABI_VERSION stays as it is.  One launch on the caller's
 * stream; it does not synchronise, allocate or read back.  in and out are device pointers.
 *
 * op selects the function and the instantiation (MOBGS_LANE_*, below).  A group is one full wave (T = 64 threads), for
 *   BLOCK_SUM, ROWS_SUM and BLOCK_SUM4 one workgroup of T = 256 threads; the launch runs n_groups independent groups.
 *   Thread t of group g reads in[(g T + t) KI + i], i < KI, and writes out[(g T + t) KO + j], j < KO; nothing else of out
 *   is written.  Elements are 8 bytes (double) for WAVE_SUM_F64, BLOCK_SUM, ROWS_SUM and WAVE_ROWS_SUM, 4 bytes (float,
 *   int32 or uint32 as the name says; the DPP moves and the fence carry uint32 payloads) for the others.
 *   KI -> KO is 1 -> 1 except: REDUCE_COMPONENTS_<NVP> NVP -> NVP / 4 (the registers v[0 .. NVP / 4) the header
 *   documents), REDUCE_PAIR 2 -> 1 (e0, e1), WAVE_FENCE 1 -> 2 (lane l writes LDS slot l; fence; reads slot 63 - l and
 *   writes that value to slot (l + 17) & 63; fence; reads slot l: the two reads), BLOCK_SUM and BLOCK_SUM4 2 -> 2 (two
 *   calls in a row on the same LDS array, value i to call i).
 *   ROWS_SUM: group g sums the n values at stride `stride` from in + (2 g) n stride, then at once those from
 *   in + (2 g + 1) n stride, with rows_sum<256>; KO = 2.  WAVE_ROWS_SUM: the n values from in + g n stride; KO = 1.
 * n, stride: read by ROWS_SUM and WAVE_ROWS_SUM only (the others: pass 0 and 1).
 * Refused with MOBGS_E_INVALID before any launch, under the entry point's name: an unknown op, a NULL pointer,
 *   n_groups < 1, n < 0, stride < 1, a pointer that is not a multiple of the element size, n_groups n stride > 2^40. */
#define MOBGS_LANE_WAVE_SUM_F32 0
#define MOBGS_LANE_WAVE_SUM_I32 1
#define MOBGS_LANE_WAVE_SUM_F64 2
#define MOBGS_LANE_WAVE_MIN_F32 3
#define MOBGS_LANE_WAVE_MIN_I32 4
#define MOBGS_LANE_WAVE_MAX_F32 5
#define MOBGS_LANE_WAVE_MAX_I32 6
#define MOBGS_LANE_FOLD_MAX_I32 7            /* MOBGS_WAVE_FOLD(v, max)            */
#define MOBGS_LANE_FOLD_ADD_I32 8            /* MOBGS_WAVE_FOLD(v, MOBGS_WAVE_ADD) */
#define MOBGS_LANE_FOLD_ADD_F32 9
#define MOBGS_LANE_DPP_MOV_XOR1 10           /* dpp_mov<0xB1>                      */
#define MOBGS_LANE_DPP_MOV_XOR2 11           /* dpp_mov<0x4E>                      */
#define MOBGS_LANE_DPP_MOV_QUAD_REVERSE 12   /* dpp_mov<0x1B>                      */
#define MOBGS_LANE_DPP_MOV_HALF_MIRROR 13    /* dpp_mov<0x141>                     */
#define MOBGS_LANE_DPP_MOV_ROR8 14           /* dpp_mov<0x128>                     */
#define MOBGS_LANE_DPP_MOV_XOR4 15           /* dpp_mov<0x1B>(dpp_mov<0x141>(v))   */
#define MOBGS_LANE_DPP_ADD_XOR1 16           /* dpp_add<0xB1>                      */
#define MOBGS_LANE_DPP_ADD_XOR2 17           /* dpp_add<0x4E>                      */
#define MOBGS_LANE_DPP_ADD_HALF_MIRROR 18    /* dpp_add<0x141>                     */
#define MOBGS_LANE_DPP_ADD_ROR8 19           /* dpp_add<0x128>                     */
#define MOBGS_LANE_DPP_ADD_ROR4 20           /* dpp_add<0x124>                     */
#define MOBGS_LANE_DPP_ADD_XOR4 21           /* dpp_add_xor4                       */
#define MOBGS_LANE_ROW_ALLREDUCE 22
#define MOBGS_LANE_HALF_WAVE_SUM 23
#define MOBGS_LANE_WAVE_ALLREDUCE 24
#define MOBGS_LANE_REDUCE_COMPONENTS_8 25
#define MOBGS_LANE_REDUCE_COMPONENTS_16 26
#define MOBGS_LANE_REDUCE_COMPONENTS_32 27
#define MOBGS_LANE_REDUCE_COMPONENTS_64 28
#define MOBGS_LANE_REDUCE_PAIR 29
#define MOBGS_LANE_WAVE_FENCE 30
#define MOBGS_LANE_BLOCK_SUM 31              /* block_sum<4>, twice                */
#define MOBGS_LANE_ROWS_SUM 32               /* rows_sum<256>, twice               */
#define MOBGS_LANE_WAVE_ROWS_SUM 33
#define MOBGS_LANE_BLOCK_SUM4 34             /* block_sum4, twice                  */
#define MOBGS_LANE_OPS 35
int mobgs_lane_probe(int op, int n_groups, int n, int stride, const void* in, void* out, void* stream);

/* ---- K34: densification controller (mobgs_amd/helper_train.py; csrc/densify_ctl.hip, built with -ffp-contract=off) -------
 * The statistics of one training iteration over the views of its batch, and the row list of a resize as one plan.  Entry
 * points and an enum only: MOBGS_ABI_VERSION stays as it is, and the five entry points of K13 keep their behaviour.  None
 * of the calls synchronises, allocates or reads back.  The kernels validate neither row indices nor buffer sizes.
 *
 * mobgs_densify_stats_batch: train.py:634-648 and :813-817 for ONE set, in one launch.  grads_host / radii_host: HOST
 *   arrays of n_views (1 .. MOBGS_STATS_MAX_VIEWS = 16) device pointers to [N_total, grad_stride] fp32 gradients and [N_total] int32 radii; row i
 *   of the set (i < n) is row row0 + i of each.  All arithmetic fp32, in view order:
 *     gx = (((0 + g_0.x) + g_1.x) + ...) sx,  gy likewise with sy   (sx = W * 0.5f, sy = H * 0.5f)
 *     r = max_v radii_v,  vis = r > 0 (any view's radius is positive)
 *     vis: max_radii2D[i] = max(max_radii2D[i], float(r)); xyz_gradient_accum[i] += sqrt(gx gx + gy gy), each operation
 *          rounded (as mobgs_densify_stats); denom[i] += 1.  A row that is not visible is not written.
 *   grad_sum [n,2] fp32 (8-byte aligned), radii_max [n] int32, visible [n] uint8: optional outputs (NULL: not written),
 *   written for every row.  n = 0 launches nothing.  MOBGS_E_INVALID before any launch: n_views outside 1 .. 16, n < 0,
 *   row0 < 0, grad_stride < 2, a NULL pointer among the views or the three statistics arrays.
 *
 * mobgs_densify_stats_sets: the statistics of mobgs_densify_stats_batch for up to TWO sets in ONE launch (the static rows
 *   and the dynamic rows of a render, or of a gradient message), bit-equal to one mobgs_densify_stats_batch call per set on
 *   the same numbers.  Set a is rows [row0_a, row0_a + n_a) of every view's arrays with its own three statistics arrays, set
 *   b likewise; either may have n = 0 (its pointers are then not read).  radii_host: HOST array of n_views device pointers
 *   to [N_total] radii in the encoding radii_encoding names: MOBGS_RADII_INT32 (contiguous int32, what render() returns) or
 *   MOBGS_RADII_FP32 (fp32-coded integers, the last N floats of a gradient message's slot whose first 2 N floats are the
 *   [N, 2] gradient rows; |r| < 2^24, so the conversion is exact).  Both tables are copied into the kernel's arguments: the
 *   call can be recorded in a graph.  No optional outputs.  MOBGS_E_INVALID before any launch: n_views outside 1 .. 16, an
 *   unknown encoding, a negative n or row0, grad_stride < 2, a NULL table, a NULL pointer among the views (n_a + n_b > 0) or
 *   among the statistics arrays of a set with n > 0.
 *
 * mobgs_densify_plan: ONE row list for mobgs_rows_gather (a negative entry -(row + 1) is a new copy of that row), in two
 *   launches without atomics: per-block counts (1024 rows a block), then every block sums the counts before it and the
 *   totals and writes its rows to their final places.  Meant for tables of up to a few million rows: every block of the
 *   write pass reads all per-block counts (12 bytes per 1024 rows), so those reads grow with the square of n -- 1 MB in
 *   all at 300 k rows, 1 GB at 10 M -- and nothing but the 2^31 - 1 bound on the list refuses a larger n.
 *   op (MobgsDensifyPlanOp) selects the list and the inputs it reads;
 *   the other input pointers may be NULL.  Every comparison is false on NaN, so a NaN row is kept.
 *     PRUNECLONE     [rows not split, ascending | -(clone + 1), ascending | -(split + 1), ascending, the run n_split times]
 *                    with clone / split the selection of mobgs_densify_select at n_grads = n on xyz_gradient_accum, denom
 *                    [n], scaling [n,3], grad_threshold, size_threshold
 *     PRUNE_OPACITY  rows with !(1 / (1 + expf(-opacity[i])) < min_opacity), ascending; opacity [n].  The quotient is this
 *                    kernel's fp32 evaluation, not torch.sigmoid's: a row whose sigmoid lies within a few ulp of
 *                    min_opacity may be decided differently from torch's (sigmoid(x) < t) mask
 *     PRUNE_BOUNDS   rows with none of x > max.x, y > max.y, z > max.z, x < min.x, y < min.y, z < min.z (strict), ascending;
 *                    xyz [n,3], bounds = {max.x, max.y, max.z, min.x, min.y, min.z} six fp32 ON THE DEVICE
 *     PRUNE_MASK     rows with mask[i] == 0, ascending; mask [n] uint8
 *   index [n max(2, n_split)] int32: the list; entries at and beyond counts[3] are not written.
 *   counts [4] int32: kept rows, clones, split parents, n_out = kept + clones + n_split parents (the prunes: kept, 0, 0,
 *   kept), written by the last block.  scratch: 3 int32 per block of 1024 rows, (n + 1023) / 1024 blocks.
 *   n = 0: counts = 0 (a memset on the stream), no launch, no list.  MOBGS_E_INVALID before any launch: n_split outside
 *   1 .. 8 (for every op), an unknown op, n < 0, n max(2, n_split) > 2^31 - 1, NULL counts, and for n > 0 a NULL list,
 *   scratch or input of the op. */
#define MOBGS_STATS_MAX_VIEWS 16
#define MOBGS_RADII_INT32 0
#define MOBGS_RADII_FP32 1
typedef enum MobgsDensifyPlanOp {
    MOBGS_PLAN_PRUNECLONE = 0,
    MOBGS_PLAN_PRUNE_OPACITY = 1,
    MOBGS_PLAN_PRUNE_BOUNDS = 2,
    MOBGS_PLAN_PRUNE_MASK = 3
} MobgsDensifyPlanOp;
int mobgs_densify_stats_batch(int n_views, const float* const* grads_host, int grad_stride,
                              const int32_t* const* radii_host, int row0, int n, float sx, float sy,
                              float* xyz_gradient_accum, float* denom, float* max_radii2D, float* grad_sum,
                              int32_t* radii_max, uint8_t* visible, void* stream);
int mobgs_densify_stats_sets(int n_views, const float* const* grads_host, int grad_stride, const void* const* radii_host,
                             int radii_encoding, float sx, float sy, int row0_a, int n_a, float* xyz_gradient_accum_a,
                             float* denom_a, float* max_radii2D_a, int row0_b, int n_b, float* xyz_gradient_accum_b,
                             float* denom_b, float* max_radii2D_b, void* stream);
int mobgs_densify_plan(int op, int n, int n_split, const float* xyz_gradient_accum, const float* denom,
                       const float* scaling, float grad_threshold, float size_threshold, const float* opacity,
                       float min_opacity, const float* xyz, const float* bounds, const uint8_t* mask, int32_t* index,
                       int32_t* counts, int32_t* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOBGS_HIP_H */

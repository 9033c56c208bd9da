// K29: one-launch snapshot / restore of a per-splat table for training checkpoints (mobgs_amd/checkpoint.py).  gfx950 only.
//
//   rows_snapshot_kernel   rows [0, n) of every field of the table -> ONE packed block, plus the integer sum of the block's
//                          32-bit words (one 64-bit atomic add per workgroup: an integer sum does not depend on the order)
//   rows_restore_kernel    the inverse: the packed block -> rows [0, n) of capacity-sized buffers; rows [n, capacity) of the
//                          fields flagged zero_new are written as zeros in the same launch, those of the others are left
//
// Packed layout.  Field f occupies the SLOT [offset_f, offset_f + round16(n row_bytes_f)) of the block; offsets are
// multiples of 16 and so is the block's base, so every 16-byte lane of the block is aligned whatever the field's row size.
// The snapshot writes the whole slot: the field's n row_bytes bytes, then zeros up to the slot's end (at most 15 bytes), so
// that every byte the checksum covers is defined.  Nothing outside the slots is written.  The copy is byte-wise: fp32
// fields, fp16 storage, the uint8 table and integer counts pass through the same kernel.
//
// Lanes.  A thread moves one 16-byte lane of a slot per round.  On the field's side (the source of a snapshot, the
// destination of a restore) the lane is one 16-byte access when the field's base is 16-byte aligned, four 4-byte accesses
// when it is only 4-byte aligned (a view that starts some rows into its buffer), single bytes otherwise -- uniform per
// field -- and the lane that holds the field's last bytes (or, restoring, the end of the zeroed rows) is always moved byte
// by byte and never touches a byte at or beyond the field's end.  mobgs_rows_gather (csrc/densify.hip) cannot express this
// copy: it addresses rows through an index list, one 4-byte word and one division per thread, into a buffer of the same
// row pitch; here source and destination are contiguous runs and there is no row arithmetic at all, so its body is not
// shared.
//
// Grid (workgroups over the longest slot, field): a workgroup owns SNAP_ROUNDS x 256 consecutive lanes (16 KiB) of one
// field; workgroups past a shorter field's end return at once.  Neither launch synchronises, allocates or reads back.
#include "common.h"

namespace mobgs {

constexpr int SNAP_BLOCK = 256;
constexpr int SNAP_ROUNDS = 4;
constexpr int64_t SNAP_LANE = 16;
constexpr int64_t SNAP_SPAN = (int64_t)SNAP_BLOCK * SNAP_ROUNDS * SNAP_LANE;   // bytes of a slot per workgroup

__host__ __device__ inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// the 16 bytes of a field at byte p (a multiple of 16), bytes at or beyond `end` read as zero and are not touched
__device__ inline uint4 load_lane(const uint8_t* __restrict__ base, int64_t p, int64_t end, unsigned align) {
    if (p + SNAP_LANE <= end) {
        if (align == 16) return *reinterpret_cast<const uint4*>(base + p);
        if (align == 4) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(base + p);
            return make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (p + k < end) w[k >> 2] |= (uint32_t)base[p + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the inverse: bytes at or beyond `end` are not written
__device__ inline void store_lane(uint8_t* __restrict__ base, int64_t p, int64_t end, unsigned align, uint4 v) {
    if (p + SNAP_LANE <= end) {
        if (align == 16) {
            *reinterpret_cast<uint4*>(base + p) = v;
            return;
        }
        if (align == 4) {
            uint32_t* w = reinterpret_cast<uint32_t*>(base + p);
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
            return;
        }
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (p + k < end) base[p + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

__device__ inline unsigned lane_alignment(const void* p) {
    const uintptr_t a = (uintptr_t)p;
    return (a & 15) == 0 ? 16u : ((a & 3) == 0 ? 4u : 1u);
}

__global__ void __launch_bounds__(SNAP_BLOCK)
rows_snapshot_kernel(const MobgsRowsField* __restrict__ fields, int64_t n, uint8_t* __restrict__ block,
                     unsigned long long* __restrict__ sum) {
    const MobgsRowsField F = fields[blockIdx.y];
    const int64_t bytes = n * F.row_bytes, slot = round16(bytes);
    const int64_t first = (int64_t)blockIdx.x * SNAP_SPAN;
    if (first >= slot) return;   // (uniform over the workgroup)
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(F.rows);
    uint8_t* __restrict__ dst = block + F.offset;
    const unsigned align = lane_alignment(src);
    unsigned long long acc = 0ull;
#pragma unroll
    for (int r = 0; r < SNAP_ROUNDS; ++r) {
        const int64_t p = first + ((int64_t)r * SNAP_BLOCK + threadIdx.x) * SNAP_LANE;
        if (p < slot) {
            const uint4 v = load_lane(src, p, bytes, align);
            *reinterpret_cast<uint4*>(dst + p) = v;   // block base and offset are multiples of 16, p + 16 <= slot
            acc += (unsigned long long)v.x + v.y + v.z + v.w;
        }
    }
    __shared__ unsigned long long part[SNAP_BLOCK];
    part[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = SNAP_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(sum, part[0]);
}

__global__ void __launch_bounds__(SNAP_BLOCK)
rows_restore_kernel(const MobgsRowsField* __restrict__ fields, int64_t n, int64_t capacity,
                    const uint8_t* __restrict__ block) {
    const MobgsRowsField F = fields[blockIdx.y];
    const int64_t bytes = n * F.row_bytes;
    const int64_t end = F.zero_new ? capacity * F.row_bytes : bytes;   // the last byte this launch may write, exclusive
    const int64_t first = (int64_t)blockIdx.x * SNAP_SPAN;
    if (first >= end) return;
    const uint8_t* __restrict__ src = block + F.offset;
    uint8_t* __restrict__ dst = static_cast<uint8_t*>(F.rows);
    const unsigned align = lane_alignment(dst);
#pragma unroll
    for (int r = 0; r < SNAP_ROUNDS; ++r) {
        const int64_t p = first + ((int64_t)r * SNAP_BLOCK + threadIdx.x) * SNAP_LANE;
        if (p < end) {
            // (a lane of the slot is read whole only where all of it is the field's; the slot's padding is not relied on)
            const uint4 v = p < bytes ? load_lane(src, p, bytes, 16u) : make_uint4(0u, 0u, 0u, 0u);
            store_lane(dst, p, end, align, v);
        }
    }
}

static int snapshot_grid(const char* who, int n_fields, const void* fields_dev, int64_t n, int64_t longest_row_bytes,
                         const void* block, dim3* grid) {
    if (n_fields < 0 || n_fields > 65535 || n < 0 || longest_row_bytes < 0 || (n_fields > 0 && (!fields_dev || !block))) {
        set_error("%s: bad arguments n_fields=%d (0..65535) n=%lld longest_row_bytes=%lld, or a NULL table / block", who,
                  n_fields, (long long)n, (long long)longest_row_bytes);
        return MOBGS_E_INVALID;
    }
    if (((uintptr_t)block & 15) != 0 || ((uintptr_t)fields_dev & 7) != 0) {
        set_error("%s: the block must be 16-byte aligned and the field table 8-byte aligned", who);
        return MOBGS_E_INVALID;
    }
    if (n > 0 && longest_row_bytes > INT64_MAX / 2 / n) {
        set_error("%s: n=%lld rows of %lld bytes overflow", who, (long long)n, (long long)longest_row_bytes);
        return MOBGS_E_INVALID;
    }
    const int64_t blocks = (round16(n * longest_row_bytes) + SNAP_SPAN - 1) / SNAP_SPAN;
    if (blocks > 2147483647LL) {
        set_error("%s: %lld workgroups (at most 2^31 - 1)", who, (long long)blocks);
        return MOBGS_E_INVALID;
    }
    *grid = dim3((unsigned)blocks, (unsigned)n_fields);
    return MOBGS_OK;
}

}  // namespace mobgs

using namespace mobgs;

extern "C" {

int mobgs_rows_snapshot(int n_fields, const MobgsRowsField* fields_dev, int64_t n, int64_t longest_row_bytes, void* block,
                        uint64_t* sum_dev, void* stream) {
    dim3 grid;
    const int rc = snapshot_grid("mobgs_rows_snapshot", n_fields, fields_dev, n, longest_row_bytes, block, &grid);
    if (rc != MOBGS_OK) return rc;
    if (n_fields > 0 && (!sum_dev || ((uintptr_t)sum_dev & 7) != 0)) {
        set_error("mobgs_rows_snapshot: the sum must be a non-NULL, 8-byte aligned device pointer");
        return MOBGS_E_INVALID;
    }
    if (grid.x == 0 || grid.y == 0) return MOBGS_OK;
    hipLaunchKernelGGL(rows_snapshot_kernel, grid, dim3(SNAP_BLOCK), 0, (hipStream_t)stream, fields_dev, n,
                       static_cast<uint8_t*>(block), reinterpret_cast<unsigned long long*>(sum_dev));
    return check_launch("rows_snapshot_kernel");
}

int mobgs_rows_restore(int n_fields, const MobgsRowsField* fields_dev, int64_t n, int64_t capacity,
                       int64_t longest_row_bytes, const void* block, void* stream) {
    if (capacity < n) {
        set_error("mobgs_rows_restore: capacity=%lld is below n=%lld", (long long)capacity, (long long)n);
        return MOBGS_E_INVALID;
    }
    dim3 grid;   // (sized by the capacity: the zeroed rows of a zero_new field reach that far)
    const int rc = snapshot_grid("mobgs_rows_restore", n_fields, fields_dev, capacity, longest_row_bytes, block, &grid);
    if (rc != MOBGS_OK) return rc;
    if (grid.x == 0 || grid.y == 0) return MOBGS_OK;
    hipLaunchKernelGGL(rows_restore_kernel, grid, dim3(SNAP_BLOCK), 0, (hipStream_t)stream, fields_dev, n, capacity,
                       static_cast<const uint8_t*>(block));
    return check_launch("rows_restore_kernel");
}

}  // extern "C"

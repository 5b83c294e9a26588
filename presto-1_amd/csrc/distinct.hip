// distinct.hip -- the marking kernels of MarkDistinctOperator (M/operator/MarkDistinctHash.java:52-69) and DistinctLimitOperator
// (M/operator/DistinctLimitOperator.java:178-210).
//
// Input is what GroupByHashGpu::get_group_ids delivers: the page's int32 group ids and the group count before (G0) and after (G1) the
// page.  The reference's loop `id == nextDistinctId -> true, nextDistinctId++` marks row i if and only if gid[i] >= G0 and i is the
// smallest row of the page with that id.  Two facts follow from the ids being handed out in first-seen order:
//   - G1 == G0: no row is marked.  Nothing is launched but the fill of the column.
//   - first_row[g - G0], the smallest row of new group g, grows with g: the array IS the list of marked rows in row order.
// So one streaming pass over the ids (distinct_first_row_kernel, 4 B read per row, atomicMin for rows of new groups only) leaves
// everything both operators need.  MarkDistinct scatters G1 - G0 bytes into a zero-filled column (1 B written per row by the fill);
// DistinctLimit uses the first min(remaining, G1 - G0) entries as the position list of its gathers: no scan, no compaction, no read-back.
#include "distinct.h"
#include "kernels.h"

#include <algorithm>

namespace tgpu {

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 4;   // rows in flight per lane
constexpr int32_t kNoRow = 0x7fffffff;

// first_row[g - g0] = min(row : gids[row] == g) for every g in [g0, g0 + count).  A run of equal ids over neighbouring lanes sends its
// first lane only (rows grow with the lane, so that is the run's minimum), as the group-by probe dedupes its runs.  Ids that repeat
// further apart meet in memory: first_row only ever falls, so a row that reads a value at or below its own number has nothing to add
// and skips the atomic -- a stale read is a larger value and costs one atomic too many, never a wrong minimum.
__global__ void __launch_bounds__(kBlock) distinct_first_row_kernel(const int32_t *__restrict__ gids, int64_t n, int32_t g0, uint32_t count, int32_t *first_row)
{
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)kBlock * kRows;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        int32_t g[kRows];
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            const int64_t r = base + u * kBlock + threadIdx.x;
            g[u] = r < n ? gids[r] : -1;
        }
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            const int64_t r = base + u * kBlock + threadIdx.x;
            const uint32_t idx = (uint32_t)g[u] - (uint32_t)g0;
            const bool fresh = g[u] >= g0 && idx < count;   // rows past n carry -1
            const int32_t before = __shfl_up(g[u], 1, 64);
            if (fresh && (lane == 0 || before != g[u])) {
                if (*(const volatile int32_t *)&first_row[idx] > (int32_t)r) atomicMin(&first_row[idx], (int32_t)r);
            }
        }
    }
}

// mark[first_row[k]] = 1: first_row grows with k, so neighbouring lanes store to ascending addresses
__global__ void __launch_bounds__(kBlock) distinct_scatter_kernel(const int32_t *__restrict__ first_row, int64_t count, int64_t n, uint8_t *__restrict__ mark)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (int64_t)gridDim.x * kBlock) {
        const int64_t r = first_row[k];
        if (r < n) mark[r] = 1;   // every new group has a row; kNoRow would mean it had none
    }
}

}  // namespace

DistinctMarkerGpu::DistinctMarkerGpu(Context *ctx, std::vector<int32_t> types, bool has_input_hash, int32_t expected_size)
    : ctx_(ctx), hash_(ctx, std::move(types), has_input_hash, expected_size)
{
}

int64_t DistinctMarkerGpu::new_groups(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n)
{
    TG_CHECK_ARG(n >= 0 && n <= 0x7fffffffLL, "a page of 2^31 rows or more: row numbers are int32");
    if (n == 0) return 0;
    grow(ctx_, gids_, (size_t)n * 4);
    const int64_t g0 = hash_.group_count();
    hash_.get_group_ids(keys, hashes, n, gids_->as<int32_t>());
    const int64_t count = hash_.group_count() - g0;
    if (count == 0) return 0;   // the steady state of a low-cardinality stream: every key has been seen
    grow(ctx_, first_row_, (size_t)count * 4);
    ProfileScope ps(ctx_, "distinct_first_row");
    k::fill_i32(ctx_, first_row_->as<int32_t>(), kNoRow, count);
    distinct_first_row_kernel<<<grid_for(ctx_, n, (int64_t)kBlock * kRows), kBlock, 0, ctx_->stream()>>>(gids_->as<int32_t>(), n, (int32_t)g0, (uint32_t)count,
                                                                                                          first_row_->as<int32_t>());
    check_launch("distinct_first_row");
    return count;
}

DeviceColumn DistinctMarkerGpu::mark(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n)
{
    const int64_t count = new_groups(keys, hashes, n);
    DeviceColumn out;
    out.type = TGPU_BOOLEAN;
    out.n = n;
    ProfileScope ps(ctx_, "distinct_mark");
    out.values_buf = ctx_->alloc_zero((size_t)std::max<int64_t>(n, 1));
    out.values = out.values_buf->ptr();
    if (count == 0) return out;
    distinct_scatter_kernel<<<grid_for(ctx_, count, kBlock), kBlock, 0, ctx_->stream()>>>(first_row_->as<int32_t>(), count, n, out.values_buf->as<uint8_t>());
    check_launch("distinct_scatter");
    return out;
}

int64_t DistinctMarkerGpu::first_rows(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n, int64_t limit, const int32_t **positions)
{
    const int64_t count = new_groups(keys, hashes, n);
    *positions = count > 0 ? first_row_->as<int32_t>() : nullptr;
    return std::min(count, limit);
}

}  // namespace tgpu

// rownumber.hip -- the ranking kernels of RowNumberOperator (M/operator/RowNumberOperator.java:301-311 createRowNumberBlock, :313-342
// getSelectedRows).
//
// Input is what GroupByHashGpu::get_group_ids delivers: the page's int32 group ids and the group count after the page (G1).  The
// reference walks the page in row order and does count[partition]++ per row; the device computes the same numbers as
//   rn[i] = count_before[gid[i]] + |{ j < i : gid[j] == gid[i] }| + 1
// with a stable per-group running rank.  There are no atomic tickets anywhere on the way to a row number: equal-key rows are numbered
// in row order, and with a limit the kept rows of a group are its FIRST max - count_before rows.  Two paths, chosen per page by G1:
//
//   G1 <= kLdsGroups: the unit of work is a wave that owns one contiguous chunk of the page.
//     row_number_count_kernel       each wave histograms its chunk into its own LDS slice (G1 x 4 B) and stores it as row w of a
//                                   waves x G1 int32 matrix
//     row_number_chunk_scan_kernel  one lane per group walks the matrix down the waves (neighbouring lanes = neighbouring groups: every
//                                   step a coalesced load; 16 slices of the waves per block, combined through LDS), leaves the exclusive
//                                   per-chunk bases in place, saves count[g] as before[g] and writes the new count[g] (saturated at max)
//     row_number_assign_kernel      each wave reloads its row of bases into LDS and walks its chunk 64 rows at a time: peer mask of the
//                                   lanes with the same id from one ballot per id bit, rank = popcount(peers below), rn = before[g] +
//                                   base[g] + rank + 1; the highest lane of each peer set then adds popcount(peers) to base[g]
//   G1 > kLdsGroups: stable radix sort of (gid, row) pairs over the ceil(log2 G1) bits in use (rocPRIM, as partition.hip drives it), then
//     run_start (head rows record start[g]), run_number (rn[row[i]] = count[g] + i - start[g] + 1) and, in a launch of its own because
//     every row of a run reads count[g], run_count (the last row of each run writes count[g]).
#include "rownumber.h"
#include "kernels.h"

#include <algorithm>

#include <rocprim/rocprim.hpp>

namespace tgpu {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kScanBlock = 1024;
constexpr int kScanSlices = kScanBlock / 64;
constexpr int64_t kMinChunk = 512;               // rows per wave below which a wave is not worth its row of the matrix
constexpr int64_t kMatrixBytes = 8ll << 20;      // waves x G1 x 4 B stays within this

// ---- few groups -----------------------------------------------------------------------------------------------------------------------
// wave w owns rows [w * chunk, min(n, (w + 1) * chunk)); chunk is a multiple of 64.  A wave whose chunk is empty stores a row of zeros.
__global__ void __launch_bounds__(kBlock) row_number_count_kernel(const int32_t *__restrict__ gids, int64_t n, int64_t chunk, int32_t groups,
                                                                  int32_t *__restrict__ matrix)
{
    extern __shared__ int32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t *hist = lds + (size_t)wave * groups;
    for (int32_t g = lane; g < groups; g += 64) hist[g] = 0;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * kWaves + wave;
    const int64_t begin = w * chunk, end = std::min(n, begin + chunk);
#pragma unroll 4
    for (int64_t r = begin + lane; r < end; r += 64) {
        const uint32_t g = (uint32_t)gids[r];
        if (g < (uint32_t)groups) atomicAdd(&hist[g], 1);
    }
    __syncthreads();
    int32_t *row = matrix + w * groups;
    for (int32_t g = lane; g < groups; g += 64) row[g] = hist[g];
}

// block b owns groups [64 b, 64 b + 64), one per lane; its 16 waves each own a slice of the matrix' rows.  In place: counts -> exclusive
// bases down each column.  before[g] = count[g] for the assign kernel, count[g] advances by the column's total.
__global__ void __launch_bounds__(kScanBlock) row_number_chunk_scan_kernel(int32_t *__restrict__ matrix, int64_t waves, int32_t groups, int64_t *__restrict__ count,
                                                                           int64_t *__restrict__ before, int64_t max_rows)
{
    __shared__ int32_t part[kScanSlices][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 64 + lane;
    const bool live = g < groups;
    const int64_t per = (waves + kScanSlices - 1) / kScanSlices, w0 = std::min(waves, slice * per), w1 = std::min(waves, w0 + per);
    int32_t sum = 0;
    if (live) {
#pragma unroll 8
        for (int64_t w = w0; w < w1; w++) sum += matrix[w * groups + g];
    }
    part[slice][lane] = sum;
    __syncthreads();
    int32_t run = 0, total = 0;
#pragma unroll
    for (int s = 0; s < kScanSlices; s++) {
        const int32_t v = part[s][lane];
        if (s < slice) run += v;
        total += v;
    }
    if (!live) return;
#pragma unroll 8
    for (int64_t w = w0; w < w1; w++) {
        const int32_t v = matrix[w * groups + g];
        matrix[w * groups + g] = run;
        run += v;
    }
    if (slice == 0) {
        int64_t c = count[g];
        before[g] = c;
        c += total;
        if (max_rows >= 0 && c > max_rows) c = max_rows;   // RowNumberOperator.java:323-325: the count stops at the limit
        count[g] = c;
    }
}

template <bool LIMIT>
__global__ void __launch_bounds__(kBlock) row_number_assign_kernel(const int32_t *__restrict__ gids, int64_t n, int64_t chunk, int32_t groups, int bits,
                                                                   const int32_t *__restrict__ matrix, const int64_t *__restrict__ before, int64_t max_rows,
                                                                   int64_t *__restrict__ rn, int32_t *__restrict__ keep)
{
    extern __shared__ int32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    volatile int32_t *base = lds + (size_t)wave * groups;   // rows of group g in the chunks before this wave's + in the rows it has walked
    const int64_t w = (int64_t)blockIdx.x * kWaves + wave;
    const int32_t *row = matrix + w * groups;
    for (int32_t g = lane; g < groups; g += 64) base[g] = row[g];
    __syncthreads();
    const int64_t begin = w * chunk, end = std::min(n, begin + chunk);
    const uint64_t below = (1ull << lane) - 1;
    for (int64_t r0 = begin; r0 < end; r0 += 64) {   // wave-uniform trip count: every lane takes part in the ballots
        const int64_t r = r0 + lane;
        uint32_t g = r < end ? (uint32_t)gids[r] : 0u;
        const bool valid = r < end && g < (uint32_t)groups;
        uint64_t peers = __ballot(valid);
        for (int b = 0; b < bits; b++) {
            const bool bit = (g >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        int32_t b0 = 0;
        if (valid) {
            b0 = base[g];
            const int64_t v = before[g] + b0 + __popcll(peers & below) + 1;
            rn[r] = v;
            if (LIMIT) keep[r] = v <= max_rows ? 1 : 0;
        }
        __builtin_amdgcn_wave_barrier();   // every lane has read its base before a peer set's highest lane moves it
        if (valid && (peers >> lane) == 1ull) base[g] = b0 + __popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- many groups ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) row_number_pairs_kernel(const int32_t *__restrict__ gids, int64_t n, unsigned int *__restrict__ keys, int32_t *__restrict__ rows)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        keys[i] = (unsigned int)gids[i];
        rows[i] = (int32_t)i;
    }
}

__global__ void __launch_bounds__(kBlock) row_number_run_start_kernel(const unsigned int *__restrict__ keys, int64_t n, int64_t groups, int32_t *__restrict__ start)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned int g = keys[i];
        if (g < groups && (i == 0 || keys[i - 1] != g)) start[g] = (int32_t)i;
    }
}

template <bool LIMIT>
__global__ void __launch_bounds__(kBlock) row_number_run_number_kernel(const unsigned int *__restrict__ keys, const int32_t *__restrict__ rows, int64_t n, int64_t groups,
                                                                       const int32_t *__restrict__ start, const int64_t *__restrict__ count, int64_t max_rows,
                                                                       int64_t *__restrict__ rn, int32_t *__restrict__ keep)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned int g = keys[i];
        const int64_t r = rows[i];
        if (g >= groups || r < 0 || r >= n) continue;
        const int64_t v = count[g] + (i - start[g]) + 1;
        rn[r] = v;
        if (LIMIT) keep[r] = v <= max_rows ? 1 : 0;
    }
}

// after run_number: the last row of each run is the only writer of count[g], and nothing reads it any more in this page
__global__ void __launch_bounds__(kBlock) row_number_run_count_kernel(const unsigned int *__restrict__ keys, int64_t n, int64_t groups, const int32_t *__restrict__ start,
                                                                      int64_t *__restrict__ count, int64_t max_rows)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned int g = keys[i];
        if (g >= groups || (i + 1 < n && keys[i + 1] == g)) continue;
        int64_t c = count[g] + (i - start[g]) + 1;
        if (max_rows >= 0 && c > max_rows) c = max_rows;
        count[g] = c;
    }
}

// ---- shared ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) row_number_iota_kernel(int64_t *__restrict__ out, int64_t base, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) out[i] = base + i + 1;
}

int bits_of(int64_t groups)
{
    int bits = 0;
    while (bits < 32 && (1ll << bits) < groups) bits++;
    return bits;
}

DeviceColumn bigint_column(Context *ctx, int64_t n)
{
    DeviceColumn out;
    out.type = TGPU_BIGINT;
    out.n = n;
    out.values_buf = ctx->alloc((size_t)std::max<int64_t>(n, 1) * 8);
    out.values = out.values_buf->ptr();
    return out;
}

}  // namespace

RowNumbererGpu::RowNumbererGpu(Context *ctx, std::vector<int32_t> partition_types, bool has_input_hash, int32_t expected_size, int64_t max_rows)
    : ctx_(ctx), max_rows_(max_rows)
{
    if (!partition_types.empty()) hash_ = std::make_unique<GroupByHashGpu>(ctx, std::move(partition_types), has_input_hash, expected_size);
}

int64_t RowNumbererGpu::group_ids(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n)
{
    TG_CHECK_ARG(n >= 0 && n <= 0x7fffffffLL, "a page of 2^31 rows or more: row numbers inside a page are int32");
    TG_CHECK_STATE(hash_ != nullptr, "no partition channels");
    if (n == 0) return hash_->group_count();
    grow(ctx_, gids_, (size_t)n * 4);
    hash_->get_group_ids(keys, hashes, n, gids_->as<int32_t>());
    const int64_t groups = hash_->group_count();
    // partitionRowCount.ensureCapacity(groupCount) (:279): new entries are zero
    if (!count_ || (int64_t)(count_->bytes() / 8) < groups) {
        const size_t cap = std::max<size_t>((size_t)groups * 2, 1024);
        BufferPtr bigger = ctx_->alloc_zero(cap * 8);
        if (count_ && counted_groups_ > 0)
            HIP_CHECK(hipMemcpyAsync(bigger->ptr(), count_->ptr(), (size_t)counted_groups_ * 8, hipMemcpyDeviceToDevice, ctx_->stream()));
        count_ = bigger;
    }
    counted_groups_ = groups;
    return groups;
}

void RowNumbererGpu::rank_lds(int64_t n, int32_t groups, int64_t *rn, int32_t *keep)
{
    // waves: enough rows per wave to be worth a row of the matrix, at most two blocks per CU, the matrix within kMatrixBytes
    int64_t waves = ceil_div(n, kMinChunk);
    waves = std::min(waves, (int64_t)ctx_->cu_count() * 2 * kWaves);
    waves = std::min(waves, std::max<int64_t>(kWaves, kMatrixBytes / ((int64_t)groups * 4)));
    const int blocks = (int)ceil_div(std::max<int64_t>(waves, 1), kWaves);
    waves = (int64_t)blocks * kWaves;
    const int64_t chunk = ceil_div(ceil_div(n, waves), 64) * 64;
    const size_t lds_bytes = (size_t)kWaves * groups * 4;   // <= 32 KiB at kLdsGroups
    grow(ctx_, matrix_, (size_t)waves * groups * 4);
    grow(ctx_, before_, (size_t)kLdsGroups * 8);
    ProfileScope ps(ctx_, "row_number_lds");
    row_number_count_kernel<<<blocks, kBlock, lds_bytes, ctx_->stream()>>>(gids_->as<int32_t>(), n, chunk, groups, matrix_->as<int32_t>());
    check_launch("row_number_count");
    row_number_chunk_scan_kernel<<<(int)ceil_div(groups, 64), kScanBlock, 0, ctx_->stream()>>>(matrix_->as<int32_t>(), waves, groups, count_->as<int64_t>(),
                                                                                                before_->as<int64_t>(), max_rows_);
    check_launch("row_number_chunk_scan");
    if (keep)
        row_number_assign_kernel<true><<<blocks, kBlock, lds_bytes, ctx_->stream()>>>(gids_->as<int32_t>(), n, chunk, groups, bits_of(groups), matrix_->as<int32_t>(),
                                                                                       before_->as<int64_t>(), max_rows_, rn, keep);
    else
        row_number_assign_kernel<false><<<blocks, kBlock, lds_bytes, ctx_->stream()>>>(gids_->as<int32_t>(), n, chunk, groups, bits_of(groups), matrix_->as<int32_t>(),
                                                                                        before_->as<int64_t>(), max_rows_, rn, nullptr);
    check_launch("row_number_assign");
}

void RowNumbererGpu::rank_sort(int64_t n, int64_t groups, int64_t *rn, int32_t *keep)
{
    grow(ctx_, keys_, (size_t)n * 4);
    grow(ctx_, rows_, (size_t)n * 4);
    grow(ctx_, keys_sorted_, (size_t)n * 4);
    grow(ctx_, rows_sorted_, (size_t)n * 4);
    grow(ctx_, start_, (size_t)groups * 4);
    ProfileScope ps(ctx_, "row_number_sort");
    const int g = grid_for(ctx_, n);
    row_number_pairs_kernel<<<g, kBlock, 0, ctx_->stream()>>>(gids_->as<int32_t>(), n, keys_->as<unsigned int>(), rows_->as<int32_t>());
    check_launch("row_number_pairs");
    const unsigned int end_bit = (unsigned int)std::max(1, bits_of(groups));
    size_t temp_bytes = 0;
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_->as<unsigned int>(), keys_sorted_->as<unsigned int>(), rows_->as<int>(), rows_sorted_->as<int>(), (size_t)n, 0,
                                        end_bit, ctx_->stream()));
    grow(ctx_, sort_temp_, temp_bytes > 0 ? temp_bytes : 1);
    HIP_CHECK(rocprim::radix_sort_pairs(sort_temp_->ptr(), temp_bytes, keys_->as<unsigned int>(), keys_sorted_->as<unsigned int>(), rows_->as<int>(), rows_sorted_->as<int>(),
                                        (size_t)n, 0, end_bit, ctx_->stream()));
    const unsigned int *sorted = keys_sorted_->as<unsigned int>();
    row_number_run_start_kernel<<<g, kBlock, 0, ctx_->stream()>>>(sorted, n, groups, start_->as<int32_t>());
    check_launch("row_number_run_start");
    if (keep)
        row_number_run_number_kernel<true><<<g, kBlock, 0, ctx_->stream()>>>(sorted, rows_sorted_->as<int32_t>(), n, groups, start_->as<int32_t>(), count_->as<int64_t>(),
                                                                              max_rows_, rn, keep);
    else
        row_number_run_number_kernel<false><<<g, kBlock, 0, ctx_->stream()>>>(sorted, rows_sorted_->as<int32_t>(), n, groups, start_->as<int32_t>(), count_->as<int64_t>(),
                                                                               max_rows_, rn, nullptr);
    check_launch("row_number_run_number");
    row_number_run_count_kernel<<<g, kBlock, 0, ctx_->stream()>>>(sorted, n, groups, start_->as<int32_t>(), count_->as<int64_t>(), max_rows_);
    check_launch("row_number_run_count");
}

void RowNumbererGpu::rank(int64_t n, int64_t groups, int64_t *rn, int32_t *keep)
{
    if (!force_sort_ && groups <= kLdsGroups) rank_lds(n, (int32_t)groups, rn, keep);
    else rank_sort(n, groups, rn, keep);
}

DeviceColumn RowNumbererGpu::number(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n)
{
    const int64_t groups = group_ids(keys, hashes, n);
    DeviceColumn out = bigint_column(ctx_, n);
    if (n > 0) rank(n, groups, out.values_buf->as<int64_t>(), nullptr);
    return out;
}

int64_t RowNumbererGpu::select(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n, const int32_t **positions, DeviceColumn *rn)
{
    TG_CHECK_STATE(max_rows_ >= 0, "select needs a limit");
    const int64_t groups = group_ids(keys, hashes, n);
    *positions = nullptr;
    if (n == 0 || max_rows_ == 0) return 0;   // a limit of 0 keeps nothing: count[g] == max from the start (:323)
    DeviceColumn all = bigint_column(ctx_, n);
    grow(ctx_, keep_, (size_t)n * 4);
    grow(ctx_, rank_, (size_t)n * 4);
    grow(ctx_, positions_, (size_t)n * 4);
    if (!total_) total_ = ctx_->alloc(8);
    rank(n, groups, all.values_buf->as<int64_t>(), keep_->as<int32_t>());
    {
        ProfileScope ps(ctx_, "row_number_compact");
        k::exclusive_scan_i32(ctx_, keep_->as<int32_t>(), rank_->as<int32_t>(), n, total_->as<int64_t>());
        k::compact_positions(ctx_, keep_->as<int32_t>(), rank_->as<int32_t>(), n, positions_->as<int32_t>());
        check_launch("row_number_compact");
    }
    const int64_t kept = ctx_->read_scalar(total_->as<int64_t>());
    TG_CHECK_STATE(kept >= 0 && kept <= n, "kept-row count out of range");
    if (kept == 0) return 0;
    *positions = positions_->as<int32_t>();
    *rn = k::gather_column(ctx_, all, *positions, kept, false);
    return kept;
}

DeviceColumn RowNumbererGpu::iota(int64_t base, int64_t n)
{
    TG_CHECK_ARG(n >= 0 && n <= 0x7fffffffLL, "a page of 2^31 rows or more");
    DeviceColumn out = bigint_column(ctx_, n);
    if (n == 0) return out;
    ProfileScope ps(ctx_, "row_number_iota");
    row_number_iota_kernel<<<grid_for(ctx_, n), kBlock, 0, ctx_->stream()>>>(out.values_buf->as<int64_t>(), base, n);
    check_launch("row_number_iota");
    return out;
}

}  // namespace tgpu

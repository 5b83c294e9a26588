// rownumber.h -- the step after the group ids of RowNumberOperator (M/operator/RowNumberOperator.java:301-342), in HBM: for every row of a
// page, how many earlier rows of the stream carry the same partition id.
#pragma once

#include "common.h"
#include "groupby.h"

namespace tgpu {

// One GroupByHashGpu (none without partition channels) plus count_[group], the reference's `LongBigArray partitionRowCount`, and the
// scratch of the ranking kernels (rownumber.hip).  The reference walks the page in row order and does count[partition]++ per row; here
//   rn[i] = count_before[gid[i]] + |{ j < i : gid[j] == gid[i] }| + 1
// comes out of a stable per-group running rank -- no atomic tickets, so equal-key rows are numbered in row order.
class RowNumbererGpu {
public:
    // pages whose group count after the page is at most this take the LDS path, the others the sort path.
    // tools/exp_row_number.py reads this line to decide which group counts it also forces down the sort path.
    static constexpr int32_t kLdsGroups = 2048;

    // partition_types empty = one partition, no hash; max_rows < 0 = no limit
    RowNumbererGpu(Context *ctx, std::vector<int32_t> partition_types, bool has_input_hash, int32_t expected_size, int64_t max_rows);

    // Without a limit: the page's row numbers as a BIGINT column without nulls; count_ advanced by the page.  No read-back.
    DeviceColumn number(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n);
    // With a limit: the kept rows (rn <= max) in row order.  *positions = their row numbers in the page (dense device list, valid until
    // the next call), *rn = their row numbers, already compacted; returns how many there are (the page's one read-back).
    int64_t select(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n, const int32_t **positions, DeviceColumn *rn);
    // No partition channels: base + 1 .. base + n
    DeviceColumn iota(int64_t base, int64_t n);

    bool partitioned() const { return hash_ != nullptr; }
    int64_t estimated_size() const { return (hash_ ? hash_->estimated_size() : 0) + (int64_t)(count_ ? count_->bytes() : 8); }   // :266
    // every page down the sort path, whatever its group count: the baseline of tools/exp_row_number.py, and how the tests reach the sort
    // path with few groups
    void force_sort(bool on) { force_sort_ = on; }

private:
    // the page's group ids in gids_, count_ grown to the new group count; returns G1
    int64_t group_ids(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n);
    // rn[n] (and keep[n] with a limit) of the page in gids_; count_ advanced
    void rank(int64_t n, int64_t groups, int64_t *rn, int32_t *keep);
    void rank_lds(int64_t n, int32_t groups, int64_t *rn, int32_t *keep);
    void rank_sort(int64_t n, int64_t groups, int64_t *rn, int32_t *keep);

    Context *ctx_;
    std::unique_ptr<GroupByHashGpu> hash_;
    int64_t max_rows_;
    int64_t counted_groups_ = 0;   // entries of count_ in use (all others zero)
    bool force_sort_ = false;
    BufferPtr count_;                                    // int64 per group
    BufferPtr gids_, matrix_, before_, start_, keys_, rows_, keys_sorted_, rows_sorted_, sort_temp_;   // reused from page to page, grown by doubling
    BufferPtr keep_, rank_, positions_, total_;
};

}  // namespace tgpu

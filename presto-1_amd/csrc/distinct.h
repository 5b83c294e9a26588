// distinct.h -- the step after the group ids of MarkDistinctOperator (M/operator/MarkDistinctHash.java:52-69) and DistinctLimitOperator
// (M/operator/DistinctLimitOperator.java:178-210), in HBM: which rows of a page start a key the stream has not shown before.
#pragma once

#include "common.h"
#include "groupby.h"

namespace tgpu {

// One GroupByHashGpu plus the scratch of the marking kernels (distinct.hip).  Both of the reference's loops walk the page's group ids with
// `nextDistinctId`; ids are assigned in first-seen order, so row i passes `id == nextDistinctId` if and only if its id is new in this page
// (>= the group count before the page) and i is the smallest row of the page with that id.
class DistinctMarkerGpu {
public:
    DistinctMarkerGpu(Context *ctx, std::vector<int32_t> types, bool has_input_hash, int32_t expected_size);

    // MarkDistinctHash.markDistinctRows: a BOOLEAN column without a null vector, 1 = the row starts a new key.  No read-back of its own.
    DeviceColumn mark(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n);
    // DistinctLimitOperator.getOutput's loop: the rows that start a new key, in row order, cut after `limit` of them.  *positions is a
    // dense device list of their row numbers, valid until the next call; returns its length.  No read-back of its own.
    int64_t first_rows(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n, int64_t limit, const int32_t **positions);

    int64_t group_count() const { return hash_.group_count(); }
    int64_t estimated_size() const { return hash_.estimated_size(); }   // MarkDistinctHash.getEstimatedSize: the hash's

private:
    // group ids of the page, then first_row_[g - G0] = smallest row with id g for every new id g; returns the number of new ids
    int64_t new_groups(const std::vector<const DeviceColumn *> &keys, const int64_t *hashes, int64_t n);

    Context *ctx_;
    GroupByHashGpu hash_;
    BufferPtr gids_, first_row_;   // reused from page to page, grown by doubling
};

}  // namespace tgpu

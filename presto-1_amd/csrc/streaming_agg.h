// streaming_agg.h -- group detection for StreamingAggregationOperator (M/operator/StreamingAggregationOperator.java:277-347): the groups of a
// page are its runs of consecutive rows whose key rows are NOT DISTINCT from each other (PagesHashStrategy.rowNotDistinctFromRow), the
// first run possibly continuing the group the previous page left open.  No table, no order among the groups, nulls and VARCHAR legal.
#pragma once

#include "common.h"

namespace tgpu {

// rows of one tile of the detection kernels (256 threads x 8 rows): page sizes and run starts around it are what the tests aim at
constexpr int kSaggTile = 2048;

struct SaggGroups {
    BufferPtr gids;         // int32[n]: page-local ascending group ids; id 0 is the open group when one is carried
    BufferPtr starts;       // int32[segments]: first row of every segment of the page in row order (row 0 always starts one)
    int64_t segments = 0;   // >= 1 for a page with rows
    bool shift = false;     // a group is carried and row 0 is distinct from it: the carried group has no row here, segment j is group j + 1
    int64_t groups() const { return segments + (shift ? 1 : 0); }
};

// keys: the page's group-by columns; carry: the one-row key columns of the open group, or null at the start of the stream.
// Two launches around one scan of the tile counts, and ONE read-back (segments, shift).
SaggGroups sagg_detect(Context *ctx, const std::vector<const DeviceColumn *> &keys, int64_t n, const std::vector<DeviceColumn> *carry);

}  // namespace tgpu

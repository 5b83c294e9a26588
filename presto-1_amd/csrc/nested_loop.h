// nested_loop.h -- the product of a nested loop join (M/operator/NestedLoopJoinOperator.java:247-274, NestedLoopPageBuilder :319-397),
// materialised piece by piece.  For one probe page and one build page the reference emits one page per row of the SMALL side, each holding
// every row of the LARGE side (L rows) with the small row repeated: row r of that sequence is (small row r / L, large row r % L).  A column
// of the large side is therefore TILED, out[r] = src[r % L], and a column of the small side REPEATED, out[r] = src[r / L].
#pragma once

#include "common.h"

namespace tgpu {

// a page kept for the product: its columns in HBM as delivered and, per VARCHAR channel, the offsets on the host (the output offsets of a
// piece are closed-form in them, and so is where a piece must end for its pool to stay below 2^31 bytes)
struct NlPage {
    DevicePage page;
    std::vector<std::vector<int32_t>> host_offsets;   // per channel; empty unless VARCHAR
};
// the columns get buffers of their own where they borrowed the caller's; one read-back per VARCHAR channel
NlPage nl_keep(Context *ctx, DevicePage page);

// bytes of VARCHAR channel `col` in rows [0, r) of the sequence (r <= rows of the small side * L)
int64_t nl_varchar_bytes_before(const NlPage &pg, int col, bool tiled, int64_t L, int64_t r);
// the largest n in [1, want] for which no VARCHAR channel of `cols` reaches 2^31 bytes in rows [r0, r0 + n)
int64_t nl_cut_rows(const NlPage &pg, const std::vector<int32_t> &cols, bool tiled, int64_t L, int64_t r0, int64_t want);
// rows [r0, r0 + n) of channel `col` in the sequence; a null vector only when the source has one
DeviceColumn nl_product_column(Context *ctx, const NlPage &pg, int col, bool tiled, int64_t L, int64_t r0, int64_t n);

}  // namespace tgpu

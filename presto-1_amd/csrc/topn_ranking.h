// topn_ranking.h -- the top n rows per partition in HBM: what TopNRankingOperator keeps between its pages.
// Reference: M/operator/TopNRankingOperator.java:170-310 over GroupedTopNRowNumberBuilder.java:99-188 / GroupedTopNRankBuilder.java, the row
// order of SimplePageWithPositionComparator.java:58-79.  Rows that compare equal rank in arrival order, as in topn.h.
#pragma once

#include "common.h"
#include "groupby.h"
#include "join.h"

namespace tgpu {

// One GroupByHashGpu (none without partition channels), a candidate store over all source channels with one int32 group id per candidate,
// and cut_[group]: the order code above which a row of the group can no longer win (all ones = the group is not full yet).  The kernels
// and the invariant of the cutoff are in topn_ranking.hip.
class GroupedTopNGpu {
public:
    static constexpr int64_t kSliceRows = 1 << 20;      // a larger page is prefiltered and selected slice by slice (TGPU_TOP_N_RANKING_SLICE_ROWS replaces it)
    static constexpr int64_t kCompactFloor = 1 << 16;   // the store is not compacted below this many rows (TGPU_TOP_N_RANKING_COMPACT_ROWS replaces it)

    GroupedTopNGpu(Context *ctx, std::vector<int32_t> types, std::vector<int32_t> partition_channels, std::vector<int32_t> sort_channels,
                   std::vector<int32_t> sort_orders, int32_t ranking_type, int64_t max_rank, int32_t hash_channel, int32_t expected_positions);

    // keeps the rows of the page that can still be among a partition's top n; the page itself is not retained
    void add_page(const DevicePage &page);
    // Every source channel of the kept rows: partitions in group-id order, inside a partition the comparator's order, equal rows in
    // arrival order; *ranking = their BIGINT ranking column.  The store is left compacted.
    DevicePage result(DeviceColumn *ranking);

    int64_t position_count() const { return store_.position_count(); }
    int64_t estimated_size() const;
    void set_prefilter(bool on) { prefilter_ = on; }
    void set_compact_floor(int64_t rows) { compact_floor_ = rows; }
    void set_slice_rows(int64_t rows) { slice_rows_ = rows; }

private:
    struct Selection {
        BufferPtr rows, gids, rank;   // the kept rows (numbers in the source), their group ids and rankings, in output order
        int64_t count = 0;
    };
    // step 4 over `m` rows of `src` (rows_in[i] + row_base = their numbers, nullptr = row_base .. row_base + m - 1); gids / codes are indexed by source row, keys_dev = the
    // sort keys of `src` on the device (order_codes)
    Selection select(const DevicePage &src, const BufferPtr &keys_dev, const int32_t *gids, const unsigned long long *codes, const int32_t *rows_in, int64_t row_base,
                     int64_t m);
    BufferPtr order_codes(const DevicePage &src, BufferPtr &keys_dev);
    BufferPtr upload_keys(const DevicePage &src);
    void grow_cut(int64_t groups);
    void append_gids(const int32_t *gids, int64_t n);
    Selection compact();

    Context *ctx_;
    std::vector<int32_t> types_, partition_channels_, sort_channels_, sort_orders_;
    int32_t ranking_type_, hash_channel_;
    int64_t max_rank_;
    std::unique_ptr<GroupByHashGpu> hash_;
    PagesIndexGpu store_;
    BufferPtr store_gids_;   // int32 per candidate, parallel to store_
    BufferPtr cut_;          // one order code per group
    int64_t cut_groups_ = 0;
    bool prefilter_ = true;
    int64_t compact_floor_ = kCompactFloor, after_compaction_ = 0, slice_rows_ = kSliceRows;
    BufferPtr gids_, flags_, offsets_, positions_, total_;   // reused from page to page, grown by doubling
};

}  // namespace tgpu

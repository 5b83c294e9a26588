// merge.h -- the k-way merge of sorted page streams (M/util/MergeSortedPages.java:41-142 behind MergeOperator.java:44-256 and
// LocalMergeSourceOperator.java:39-): one ROUND merges the settled prefixes of the streams' buffered rows.
//   merge_bound   the smallest (last buffered row, stream) over the unfinished streams and, by a binary search per stream, how many of
//                 each stream's buffered rows are settled against it
//   merge_path    an (order code, stream, row) pair per settled row, the k runs merged pairwise in ceil(log2 k) two-way merge-path passes
//   merge_gather  the output channels read straight from the streams' buffers through the final (stream, row) refs
// Row order = device_order.h (SimplePageWithPositionComparator); rows that compare equal come out lower stream first, inside a stream
// in arrival order (the left run wins every tie, and the left run is the lower stream).
#pragma once

#include "common.h"

namespace tgpu {

// Rows of one round over all streams that the operator aims at when it pulls: a stream is read ahead to kMergeRoundRows / k rows, at
// least kMergeMinReadAheadRows.  A guess (DESIGN.md section 5 "Merge"): large enough that a round over 8,192-row pages is a few
// full-width launches and not a handful of tiny ones, small enough that the buffered rows and the two pair buffers stay in the hundreds of MB.
constexpr int64_t kMergeRoundRows = 1ll << 23;
constexpr int64_t kMergeMinReadAheadRows = 1ll << 16;
// settled rows of one round (a page's position count is an int32); the rest comes out in the next round
constexpr int64_t kMergeMaxRoundRows = 0x7fffffffLL;

// the two-way merge-path kernel: a workgroup of kMergeBlock lanes owns kMergeTile = kMergeBlock x kMergeItems = 2,304 pairs of the output
// (tests/test_gpu_merge.py states kMergeTile and kMergeItems as T and I for its tile-edge cases: change them together)
constexpr int kMergeBlock = 256;
constexpr int kMergeItems = 9;
constexpr int kMergeTile = kMergeBlock * kMergeItems;

// one stream's buffered rows as the kernels see them
struct MergeStreamView {
    TgKeyCols keys;        // the sort channels, in priority order
    long long head;        // first buffered row that has not been emitted
    long long rows;        // rows of the buffer, [head, rows) are buffered
    long long window;      // rows of [head, head + window) take part in this round
    int open;              // more rows may follow the window (the stream is unfinished, or the window was cut)
    int pad;
};

// a settled row: its order code and where it lives
struct alignas(16) MergePair {
    unsigned long long code;
    unsigned int stream, row;
};

// one tile of one pass: output [a_begin + tile * kMergeTile, ...) of the merge of [a_begin, a_end) with [a_end, b_end)
struct MergeTile {
    long long a_begin, a_end, b_end, tile;
};

struct MergeKeySpec {
    int n;
    int pad;
    int order[TG_MAX_KEY_CHANNELS];
};

class MergeGpu {
public:
    MergeGpu(Context *ctx, std::vector<int32_t> types, std::vector<int32_t> output_channels, std::vector<int32_t> sort_channels, std::vector<int32_t> sort_orders);

    // One round over `pages` (stream s buffers rows [head[s], pages[s].n); window[s] of them take part, open[s]: more may follow).
    // settled[s] receives the count of stream s's rows the round emits; the return value is the merged page of the output channels
    // (n == 0: nothing settled).  A round in which one stream alone has settled rows passes them through by region (shared owners) and
    // launches no merge-path kernel.
    DevicePage round(const std::vector<const DevicePage *> &pages, const std::vector<int64_t> &head, const std::vector<int64_t> &window, const std::vector<bool> &open,
                     std::vector<int64_t> &settled);

private:
    DevicePage gather(const std::vector<const DevicePage *> &pages, const MergePair *refs, int64_t n);
    Context *ctx_;
    std::vector<int32_t> types_, output_channels_, sort_channels_;
    MergeKeySpec spec_{};
    BufferPtr spec_dev_, views_, counts_, pairs_[2], tiles_, out_views_;   // scratch that persists between rounds (stream-ordered reuse)
};

}  // namespace tgpu

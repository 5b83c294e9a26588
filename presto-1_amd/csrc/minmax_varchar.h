// minmax_varchar.h -- min / max over VARCHAR for the grouped accumulators (agg.h): the extreme byte string of every group in
// Slice.compareTo order (unsigned bytes left to right, a proper prefix first; AbstractMinMaxAggregationFunction.java:245,269,325 keep the
// block position the comparison prefers).  The 16-byte state word cannot hold a value, so a group's state is its count, a two-word slot
// that holds the ROUND CODES while a page is looked at, and a place in a value store that lives across pages.
//
// Per page, order-independent, no locks and no compare-and-swap loops over strings:
//   round k   looks at bytes [7k, 7k + 7) of a candidate row's value: code = those bytes big-endian and zero-padded in the high 56 bits,
//             min(length - 7k, 8) in the low byte (8 = more follows) -- it orders as the strings do within the window, a proper prefix
//             below its extensions.  One unsigned atomicMax per row (min: of ~code; a plain read first, device_agg.h tg_minmax_update)
//             finds the group's winning code; round 0 runs over every taken row of the page.
//   select    the rows whose code equals their group's winner survive.  Survivors whose winning code says "ends here" are byte-identical:
//             the first one to claim the group is the page's candidate.  The others go, compacted, to round k + 1.  One read-back per
//             round (the length of the next list, and what the store must have room for); a page whose values differ within their first
//             7 bytes -- or end there -- costs ONE.  The rounds are bounded by (longest tied value) / 7 + 1, each over a shrinking list.
//   install   one candidate row per group the page touched is compared with the group's stored value (one comparison per group and
//             page) and, when it is better, copied to the end of the store; the group's two words and its claim are cleared again.
// The store is an append-only arena with (position, length) per group; what a replaced value leaves behind is garbage, and the arena is
// compacted when the garbage exceeds the live bytes.  It never keeps an input page alive: values are copied.
#pragma once
#include "common.h"

namespace tgpu {

class VarcharExtremes {
public:
    VarcharExtremes(Context *ctx, bool is_min) : ctx_(ctx), is_min_(is_min) {}

    // One page.  gids == nullptr: every row belongs to group 0.  Raw input: a row is taken when its mask cell (if any) is true and not
    // null and its value is not null, and counts 1.  Intermediate input (icounts != nullptr): a row is taken when icounts[r] > 0, whatever
    // its value cell's null flag says, and counts icounts[r].  No byte outside [offsets[r], offsets[r + 1]) of a taken row is read.
    void add(const int32_t *gids, int64_t n, const DeviceColumn &values, const uint8_t *mask, const uint8_t *mask_nulls, const long long *icounts, int64_t groups);
    // appends the output channels for groups [0, groups): the VARCHAR value, NULL (and empty) where the count is 0; partial: count BIGINT first
    void evaluate(int64_t groups, bool partial, std::vector<DeviceColumn> &out);
    int64_t estimated_size() const;
    // what add() needed (tests): rounds run and read-backs made so far
    int64_t rounds() const { return rounds_; }

private:
    void ensure(int64_t groups);
    void reserve_arena(int64_t cursor, int64_t garbage, int64_t need, int64_t groups);

    Context *ctx_;
    bool is_min_;
    int64_t cap_ = 0;
    BufferPtr counts_;     // int64[g]
    BufferPtr words_;      // uint64[g][2]: the round codes of even / odd rounds; zero between pages
    BufferPtr claim_;      // int32[g]: candidate row + 1 of the page at hand; zero between pages
    BufferPtr vpos_;       // int64[g]: position in the arena + 1; 0 = no value yet
    BufferPtr vlen_;       // int32[g]
    BufferPtr arena_;      // the value bytes
    BufferPtr counters_;   // uint64[4]: next list length, bytes the candidates need, arena cursor, garbage bytes
    int64_t rounds_ = 0;
};

}  // namespace tgpu

// semijoin.h -- the set of a semi join in HBM: ChannelSet (M/operator/ChannelSet.java) built by SetBuilderOperator and probed by
// HashSemiJoinOperator (M/operator/HashSemiJoinOperator.java:166-218), one BOOLEAN per probe row.
#pragma once

#include "common.h"
#include "groupby.h"
#include "join.h"

namespace tgpu {

class SemiSetGpu {
public:
    // tgpu_set_supplier_stats' layout codes
    enum Layout { kBitmap = 0, kHash = 1, kGeneric = 2 };

    SemiSetGpu(Context *ctx, int32_t type);
    // build side, one page at a time: the key column is copied (BIGINT / INTEGER / DATE) or inserted into the group-by hash (other types)
    void add_keys(const DeviceColumn &keys);
    // picks the layout from the exact key range and row count and builds it (one read-back); the set is immutable afterwards
    void finish();

    // the BOOLEAN column HashSemiJoinOperator appends for `keys` (:191-216): null key -> false for an empty set, else null; key in the
    // set -> true; else null when the set contains a null, else false.  No read-back: the launches are only enqueued.
    DeviceColumn probe(const DeviceColumn &keys) const;

    int32_t type() const { return type_; }
    int64_t size() const { return size_; }             // distinct keys, the null key counted (ChannelSet.size)
    bool contains_null() const { return contains_null_; }
    bool empty() const { return positions_ == 0; }     // ChannelSet.isEmpty: no build position at all
    int layout() const { return layout_; }
    int64_t estimated_size() const;                    // HBM bytes held (while building: the collected keys)

private:
    Context *ctx_;
    int32_t type_;
    bool integer_;                                     // BIGINT / INTEGER / DATE: bitmap or key-only hash layout
    bool finished_ = false;
    int64_t positions_ = 0, size_ = 0;
    bool contains_null_ = false;
    int layout_ = kGeneric;
    BufferPtr null_seen_;                              // one device word: a build page held a null key
    std::unique_ptr<PagesIndexGpu> keys_;              // integer keys until finish()
    std::unique_ptr<GroupByHashGpu> groups_;           // other types
    mutable std::mutex generic_mu_;                    //   (its lookup is not re-entrant; probe operators may run on several threads)
    BufferPtr bitmap_;                                 // kBitmap: one bit per value of [key_min_, key_min_ + span_]
    long long key_min_ = 0;
    unsigned long long span_ = 0;
    BufferPtr slots_;                                  // kHash: int64 keys, kEmptyKey = free
    uint64_t mask_ = 0;
    bool has_empty_key_ = false;                       // kHash: the key equal to kEmptyKey is in the set (it is never stored)
};

}  // namespace tgpu

// semijoin.hip -- ChannelSet in HBM (SetBuilderOperator, M/operator/SetBuilderOperator.java:137-233; ChannelSet.java:62-108) and the
// membership probe of HashSemiJoinOperator (M/operator/HashSemiJoinOperator.java:166-218).
//
// A set only answers "is this key present": no group ids, no positions, no first-seen order.  Its layout is chosen once the build side
// has finished, from the exact key range and row count:
//   - BIGINT / INTEGER / DATE keys over a dense range: an exact bitmap over [min, max] -- the DIRECT idea of the join without its rank
//     structure; a probe is one word load and a bit test;
//   - the same keys over a sparse range: a key-only open-address table (power-of-two capacity, fill <= 0.5, 8-byte slots, CAS insert);
//     kEmptyKey marks a free slot, so that one key value is never stored: its presence is a flag of its own;
//   - any other type: GroupByHashGpu, whose equality is the reference's (DOUBLE NaN / -0.0 as the group-by hash, VARCHAR bytewise).
// The three-valued result (null probe key, null in the set) is applied inside the probe kernels; set_empty / contains_null are known
// on the host after the build and passed as arguments, so a probe page costs no read-back.
#include "semijoin.h"
#include "kernels.h"

#include <algorithm>

namespace tgpu {

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 4;   // probe rows in flight per lane (their dependent word / slot loads overlap)
constexpr unsigned long long kEmptyKey = 0x8000000000000000ull;   // INT64_MIN: never an INTEGER / DATE key

__device__ __forceinline__ long long key_at(const ColView &c, int64_t r)
{
    return c.type == TGPU_BIGINT || c.type == TGPU_TIMESTAMP ? ((const long long *)c.values)[r] : (long long)((const int *)c.values)[r];
}

// HashSemiJoinOperator.java:191-215 for one row
__device__ __forceinline__ void semi_store(uint8_t *__restrict__ out, uint8_t *__restrict__ out_nulls, int64_t r, bool key_null, bool found, int set_empty,
                                           int contains_null)
{
    out[r] = (!key_null && found) ? 1 : 0;
    if (out_nulls) out_nulls[r] = (key_null ? !set_empty : (!found && contains_null)) ? 1 : 0;
}

// a build page holds a null key (ChannelSet.containsNull): an idempotent store of 1
__global__ void __launch_bounds__(kBlock) semi_null_flag_kernel(const uint8_t *__restrict__ nulls, int64_t n, unsigned long long *flag)
{
    bool any = false;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) any = any || nulls[r] != 0;
    if (__any(any) && (threadIdx.x & 63) == 0) *flag = 1;
}

// smallest / largest non-null key: one pair of atomics per wave
__global__ void __launch_bounds__(kBlock) semi_range_kernel(ColView key, int64_t n, long long *minmax)
{
    long long lo = 0x7fffffffffffffffLL, hi = -0x7fffffffffffffffLL - 1;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        if (key.nulls && key.nulls[r]) continue;
        const long long v = key_at(key, r);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long l2 = __shfl_down(lo, d, 64), h2 = __shfl_down(hi, d, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&minmax[0], lo);
        atomicMax(&minmax[1], hi);
    }
}

// Bitmap layout: one bit per key.  As in join.hip's build_direct_kernel, the lanes of a contiguous run that falls into one bitmap word
// OR their bits together and only the run's first lane issues the atomicOr (build sides clustered by key would otherwise serialise
// on one cache line).  Repeated keys are legal: they set a bit that is already set.
__global__ void __launch_bounds__(kBlock) semi_bitmap_build_kernel(ColView key, int64_t n, long long key_min, unsigned long long *bitmap)
{
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
        const int64_t r = base + threadIdx.x;
        const bool active = r < n && !(key.nulls && key.nulls[r]);
        const unsigned long long d = active ? (unsigned long long)key_at(key, r) - (unsigned long long)key_min : 0ull;
        const unsigned int word = active ? (unsigned int)(d >> 6) : 0xffffffffu;   // span < 2^32 bits: word < 2^26
        unsigned long long bits = active ? (1ull << (d & 63)) : 0ull;
        const unsigned int word_prev = __shfl_up(word, 1, 64);
        const bool head = lane == 0 || word_prev != word;
        const unsigned long long heads = __ballot(head);
        const int run = __popcll(heads & ((2ull << lane) - 1ull));
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {   // segmented suffix OR: the run's first lane ends up with the whole run
            const unsigned long long b2 = __shfl_down(bits, k, 64);
            const int run2 = __shfl_down(run, k, 64);
            if (lane + k < 64 && run2 == run) bits |= b2;
        }
        if (head && active) atomicOr(&bitmap[word], bits);
    }
}

// distinct keys of the bitmap layout
__global__ void __launch_bounds__(kBlock) semi_popcount_kernel(const unsigned long long *__restrict__ bitmap, int64_t words, unsigned long long *count)
{
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (int64_t)gridDim.x * kBlock) c += (unsigned long long)__popcll(bitmap[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

__global__ void __launch_bounds__(kBlock) semi_fill_kernel(unsigned long long *__restrict__ slots, int64_t capacity)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < capacity; i += (int64_t)gridDim.x * kBlock) slots[i] = kEmptyKey;
}

// Hash layout: CAS insert with linear probing.  counters[0] += keys inserted (= distinct keys), counters[1] = 1 when the key equal to
// kEmptyKey was seen (it is kept as that flag, not in a slot)
__global__ void __launch_bounds__(kBlock) semi_hash_insert_kernel(ColView key, int64_t n, unsigned long long *slots, unsigned long long mask,
                                                                   unsigned long long *counters)
{
    unsigned long long inserted = 0;
    bool empty_key = false;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        if (key.nulls && key.nulls[r]) continue;
        const unsigned long long k = (unsigned long long)key_at(key, r);
        if (k == kEmptyKey) {
            empty_key = true;
            continue;
        }
        unsigned long long h = tg_fmix64(k) & mask;
        for (;;) {   // fill <= 0.5: a free slot always ends the walk
            const unsigned long long seen = slots[h];
            if (seen == k) break;
            if (seen == kEmptyKey) {
                const unsigned long long old = atomicCAS(&slots[h], kEmptyKey, k);
                if (old == kEmptyKey) {
                    inserted++;
                    break;
                }
                if (old == k) break;
            }
            h = (h + 1) & mask;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) inserted += __shfl_down(inserted, d, 64);
    const bool any_empty = __any(empty_key);
    if ((threadIdx.x & 63) == 0) {
        if (inserted) atomicAdd(&counters[0], inserted);
        if (any_empty) counters[1] = 1;
    }
}

// ---- probes: kRows rows per lane, loads of all of them first (keys, then words / slots), stores last ------------------------------
__global__ void __launch_bounds__(kBlock) semi_probe_bitmap(ColView key, int64_t n, long long key_min, unsigned long long span,
                                                             const unsigned long long *__restrict__ bitmap, int set_empty, int contains_null,
                                                             uint8_t *__restrict__ out, uint8_t *__restrict__ out_nulls)
{
    const int64_t tile = (int64_t)kBlock * kRows;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        unsigned long long d[kRows], w[kRows];
        bool live[kRows], knull[kRows], in[kRows];
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            const int64_t r = base + u * kBlock + threadIdx.x;
            live[u] = r < n;
            knull[u] = live[u] && key.nulls && key.nulls[r];
            d[u] = live[u] ? (unsigned long long)key_at(key, r) - (unsigned long long)key_min : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            in[u] = bitmap && live[u] && !knull[u] && d[u] <= span;
            w[u] = in[u] ? bitmap[d[u] >> 6] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            const int64_t r = base + u * kBlock + threadIdx.x;
            if (live[u]) semi_store(out, out_nulls, r, knull[u], in[u] && ((w[u] >> (d[u] & 63)) & 1ull), set_empty, contains_null);
        }
    }
}

__global__ void __launch_bounds__(kBlock) semi_probe_hash(ColView key, int64_t n, const unsigned long long *__restrict__ slots, unsigned long long mask,
                                                           int has_empty_key, int set_empty, int contains_null, uint8_t *__restrict__ out,
                                                           uint8_t *__restrict__ out_nulls)
{
    const int64_t tile = (int64_t)kBlock * kRows;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        unsigned long long k[kRows], h[kRows], s[kRows];
        bool live[kRows], knull[kRows], walk[kRows];
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            const int64_t r = base + u * kBlock + threadIdx.x;
            live[u] = r < n;
            knull[u] = live[u] && key.nulls && key.nulls[r];
            k[u] = live[u] ? (unsigned long long)key_at(key, r) : kEmptyKey;
        }
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            walk[u] = live[u] && !knull[u] && k[u] != kEmptyKey;
            h[u] = tg_fmix64(k[u]) & mask;
            s[u] = walk[u] ? slots[h[u]] : kEmptyKey;
        }
#pragma unroll
        for (int u = 0; u < kRows; u++) {
            if (!live[u]) continue;
            bool found = !knull[u] && k[u] == kEmptyKey && has_empty_key;
            if (walk[u]) {
                while (s[u] != k[u] && s[u] != kEmptyKey) {   // fill <= 0.5: the walk ends
                    h[u] = (h[u] + 1) & mask;
                    s[u] = slots[h[u]];
                }
                found = s[u] == k[u];
            }
            semi_store(out, out_nulls, base + u * kBlock + threadIdx.x, knull[u], found, set_empty, contains_null);
        }
    }
}

// generic layout: the rule over GroupByHashGpu::lookup's group ids (-1 = not in the set)
__global__ void __launch_bounds__(kBlock) semi_probe_generic(const int32_t *__restrict__ gids, const uint8_t *__restrict__ key_nulls, int64_t n, int set_empty,
                                                              int contains_null, uint8_t *__restrict__ out, uint8_t *__restrict__ out_nulls)
{
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock)
        semi_store(out, out_nulls, r, key_nulls && key_nulls[r], gids[r] >= 0, set_empty, contains_null);
}

}  // namespace

SemiSetGpu::SemiSetGpu(Context *ctx, int32_t type) : ctx_(ctx), type_(type)
{
    TG_CHECK_ARG(valid_type(type), "unknown type");
    integer_ = type == TGPU_BIGINT || type == TGPU_INTEGER || type == TGPU_DATE || type == TGPU_TIMESTAMP;
    if (integer_) keys_ = std::make_unique<PagesIndexGpu>(ctx, std::vector<int32_t>{type});
    else groups_ = std::make_unique<GroupByHashGpu>(ctx, std::vector<int32_t>{type}, false, 1024);
    null_seen_ = ctx->alloc_zero(8);
}

void SemiSetGpu::add_keys(const DeviceColumn &keys)
{
    TG_CHECK_STATE(!finished_, "the set has already been built");
    TG_CHECK_ARG(keys.type == type_, "key type does not match the set's type");
    const int64_t n = keys.n;
    if (n == 0) return;
    positions_ += n;
    ProfileScope ps(ctx_, "semi_build_collect");
    if (keys.nulls) {
        semi_null_flag_kernel<<<grid_for(ctx_, n), kBlock, 0, ctx_->stream()>>>(keys.nulls, n, null_seen_->as<unsigned long long>());
        check_launch("semi_null_flag");
    }
    if (integer_) {   // collected per page like the hash builder's PagesIndex: the layout needs the range of ALL keys
        DevicePage p;
        p.n = n;
        p.cols.push_back(keys);
        keys_->add_page(p);
        return;
    }
    BufferPtr gids = ctx_->alloc((size_t)n * 4);
    groups_->get_group_ids({&keys}, nullptr, n, gids->as<int32_t>());   // ChannelSetBuilder.addPage (ChannelSet.java:120-135)
}

void SemiSetGpu::finish()
{
    if (finished_) return;
    finished_ = true;
    if (!integer_) {
        contains_null_ = ctx_->read_scalar(null_seen_->as<unsigned long long>()) != 0;
        size_ = groups_->group_count();   // the null key is a group of its own
        layout_ = kGeneric;
        return;
    }
    const int64_t n = keys_->position_count();
    const DeviceColumn key = n > 0 ? keys_->column(0) : DeviceColumn{};
    BufferPtr mm = ctx_->alloc(24);   // [min, max, a null key was seen]
    const long long init[2] = {0x7fffffffffffffffLL, -0x7fffffffffffffffLL - 1};
    ctx_->upload(mm->ptr(), init, 16);
    HIP_CHECK(hipMemcpyAsync(mm->as<long long>() + 2, null_seen_->ptr(), 8, hipMemcpyDeviceToDevice, ctx_->stream()));
    {
        ProfileScope ps(ctx_, "semi_build_range");
        if (n > 0) semi_range_kernel<<<std::min(grid_for(ctx_, n), ctx_->cu_count() * 2), kBlock, 0, ctx_->stream()>>>(view_of(key), n, mm->as<long long>());
        check_launch("semi_range");
    }
    long long host[3];
    ctx_->download(host, mm->ptr(), 24);
    contains_null_ = host[2] != 0;
    const bool has_keys = host[0] <= host[1];
    key_min_ = has_keys ? host[0] : 0;
    span_ = has_keys ? (unsigned long long)host[1] - (unsigned long long)host[0] : 0ull;
    int64_t capacity = 64;   // the hash layout's size for these rows (fill <= 0.5)
    while (capacity < 2 * n) capacity <<= 1;
    const unsigned long long words = (span_ >> 6) + 1;
    const bool bitmap = !has_keys || (span_ < (1ull << 32) && words * 8ull <= (unsigned long long)capacity * 8ull);
    ProfileScope ps(ctx_, "semi_build_insert");
    if (bitmap) {
        layout_ = kBitmap;
        if (has_keys) {
            bitmap_ = ctx_->alloc_zero((size_t)words * 8);
            semi_bitmap_build_kernel<<<grid_for(ctx_, n), kBlock, 0, ctx_->stream()>>>(view_of(key), n, key_min_, bitmap_->as<unsigned long long>());
            check_launch("semi_bitmap_build");
            BufferPtr count = ctx_->alloc_zero(8);
            semi_popcount_kernel<<<grid_for(ctx_, (int64_t)words), kBlock, 0, ctx_->stream()>>>(bitmap_->as<unsigned long long>(), (int64_t)words,
                                                                                                 count->as<unsigned long long>());
            check_launch("semi_popcount");
            size_ = (int64_t)ctx_->read_scalar(count->as<unsigned long long>());
        }
    }
    else {
        layout_ = kHash;
        mask_ = (uint64_t)capacity - 1;
        slots_ = ctx_->alloc((size_t)capacity * 8);
        semi_fill_kernel<<<grid_for(ctx_, capacity), kBlock, 0, ctx_->stream()>>>(slots_->as<unsigned long long>(), capacity);
        check_launch("semi_fill");
        BufferPtr counters = ctx_->alloc_zero(16);
        semi_hash_insert_kernel<<<grid_for(ctx_, n), kBlock, 0, ctx_->stream()>>>(view_of(key), n, slots_->as<unsigned long long>(), mask_,
                                                                                  counters->as<unsigned long long>());
        check_launch("semi_hash_insert");
        unsigned long long c[2];
        ctx_->download(c, counters->ptr(), 16);
        has_empty_key_ = c[1] != 0;
        size_ = (int64_t)c[0] + (has_empty_key_ ? 1 : 0);
    }
    if (contains_null_) size_++;
    keys_.reset();   // the collected keys go back to the allocator: the set is all that is kept
}

DeviceColumn SemiSetGpu::probe(const DeviceColumn &keys) const
{
    TG_CHECK_STATE(finished_, "the set has not been built yet");
    TG_CHECK_ARG(keys.type == type_, "probe key type does not match the set's type");
    const int64_t n = keys.n;
    const bool set_empty = empty();
    DeviceColumn out;
    out.type = TGPU_BOOLEAN;
    out.n = n;
    out.values_buf = set_empty ? ctx_->alloc_zero((size_t)std::max<int64_t>(n, 1)) : ctx_->alloc((size_t)std::max<int64_t>(n, 1));
    out.values = out.values_buf->ptr();
    // a null vector only when the rule can produce a null: a null probe key against a non-empty set, or a set holding a null
    if ((keys.nulls && !set_empty) || contains_null_) {
        out.nulls_buf = ctx_->alloc((size_t)std::max<int64_t>(n, 1));
        out.nulls = out.nulls_buf->as<uint8_t>();
    }
    if (n == 0 || set_empty) return out;   // an empty set: every row false, never null (:193-195)
    uint8_t *values = out.values_buf->as<uint8_t>(), *nulls = out.nulls_buf ? out.nulls_buf->as<uint8_t>() : nullptr;
    const int se = set_empty ? 1 : 0, cn = contains_null_ ? 1 : 0;
    const int g = grid_for(ctx_, n, (int64_t)kBlock * kRows);
    if (layout_ == kBitmap) {
        ProfileScope ps(ctx_, "semi_probe_bitmap");
        semi_probe_bitmap<<<g, kBlock, 0, ctx_->stream()>>>(view_of(keys), n, key_min_, span_, bitmap_ ? bitmap_->as<unsigned long long>() : nullptr, se, cn, values,
                                                           nulls);
        check_launch("semi_probe_bitmap");
        return out;
    }
    if (layout_ == kHash) {
        ProfileScope ps(ctx_, "semi_probe_hash");
        semi_probe_hash<<<g, kBlock, 0, ctx_->stream()>>>(view_of(keys), n, slots_->as<unsigned long long>(), mask_, has_empty_key_ ? 1 : 0, se, cn, values, nulls);
        check_launch("semi_probe_hash");
        return out;
    }
    BufferPtr gids = ctx_->alloc((size_t)n * 4);
    {
        std::lock_guard<std::mutex> lk(generic_mu_);
        groups_->lookup({&keys}, nullptr, n, gids->as<int32_t>());
    }
    ProfileScope ps(ctx_, "semi_probe_generic");
    semi_probe_generic<<<grid_for(ctx_, n), kBlock, 0, ctx_->stream()>>>(gids->as<int32_t>(), keys.nulls, n, se, cn, values, nulls);
    check_launch("semi_probe_generic");
    return out;
}

int64_t SemiSetGpu::estimated_size() const
{
    int64_t s = null_seen_ ? 8 : 0;
    if (keys_) s += keys_->estimated_size();
    if (groups_) s += groups_->estimated_size();
    if (bitmap_) s += (int64_t)bitmap_->bytes();
    if (slots_) s += (int64_t)slots_->bytes();
    return s;
}

}  // namespace tgpu

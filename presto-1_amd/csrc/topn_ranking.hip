// topn_ranking.hip -- the top n rows per partition (GroupedTopNRowNumberBuilder.java:99-188, GroupedTopNRankBuilder.java), streamed.
//
// The reference keeps one heap of n rows per group and compares every arriving row with the heap's root
// (GroupedTopNRowNumberAccumulator.java:112).  Here a page goes through four steps; the memory held between pages is groups x n rows
// (plus RANK ties) within a constant factor, not the input:
//   1. group ids from GroupByHashGpu (first-arrival order, as RowNumbererGpu obtains them); none without partition channels (all 0);
//   2. the ORDER CODE of the first sort key per row (device_order.h: code(a) < code(b) implies a sorts before b, equal codes decide
//      nothing);
//   3. PREFILTER  top_n_ranking_prefilter_kernel flags the rows with code <= cut[gid]; flags + scan + compact_positions leave the
//      survivors in row order.  cut[g] starts at all ones ("not full yet").
//      INVARIANT of cut[g]: it is only ever set to the code of a row X of group g that has at least n - 1 rows of g sorting before or
//      equal to it (X is the n-th row of g in some selection).  A row is dropped only if its code is STRICTLY greater than cut[g]:
//      it then sorts strictly after X, so at least n rows of g sort strictly before it -- its row number and its rank both exceed n.
//      Rows whose code EQUALS the cutoff are always kept: the code decides nothing between them and X (VARCHAR keys that share their
//      first 8 bytes, later sort keys, RANK peers of the n-th row).
//   4. SELECT over the survivors:
//      top_n_ranking_sort_keys_kernel   one 16-byte sort key per survivor: (code, gid, row)
//      rocPRIM merge_sort               by gid, then code, then -- only between equal codes -- the full comparator, then the row number:
//                                       a total order in which rows that compare equal keep their arrival order
//      top_n_ranking_heads_kernel       against the predecessor: head of a group, head of a peer run (the comparator says "different")
//      rocPRIM inclusive_scan (max)     carries the index of the latest group head and peer-run head to every row: a segmented scan
//      top_n_ranking_keep_kernel        position in the group = i - group head + 1 (ROW_NUMBER), rank = peer head - group head + 1 (RANK);
//                                       keep = ranking <= n.  The one row per group at position n lowers cut[g] to its code (single
//                                       writer per group and launch: a plain store).
//      scan + top_n_ranking_emit_kernel the kept rows, their group ids and rankings in sorted order
//      No atomic tickets anywhere on the way to a ranking, for the reason rownumber.hip gives: the arrival order of equal rows survives.
//      A page of more than kSliceRows rows goes through steps 3 - 6 slice by slice (the codes and group ids are the page's): its first slice
//      sets the cutoffs that filter the later ones, so a first page of 2^24 rows does not sort 2^24 keys.
//   5. the kept rows are gathered and appended to the store, their group ids to store_gids_.  Appending in sorted order keeps equal
//      rows of one page in arrival order, and pages are appended in arrival order: the store position is the arrival tie-break.
//   6. COMPACTION when the store exceeds max(2 x its size after the last compaction, floor): cut[] back to all ones, step 4 over the
//      whole store (which sets cut[g] from the n-th row of every full group), survivors gathered into a fresh store in sorted order.
//      result() is one last compaction; its ranking column comes out of the same selection.
#include "topn_ranking.h"
#include "kernels.h"
#include "device_order.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>

namespace tgpu {

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kNotFull = ~0ULL;

struct SortKey {
    unsigned long long code;
    int gid, row;
};

// index of the latest group head / peer-run head at or before a row
struct Starts {
    int group, peer;
};
struct MaxStarts {
    __host__ __device__ Starts operator()(const Starts &a, const Starts &b) const
    {
        return Starts{a.group > b.group ? a.group : b.group, a.peer > b.peer ? a.peer : b.peer};
    }
};

struct KeyLess {
    const TopNKeys *k;
    __device__ bool operator()(const SortKey &a, const SortKey &b) const
    {
        if (a.gid != b.gid) return a.gid < b.gid;
        if (a.code != b.code) return a.code < b.code;
        const int cmp = compare_rows(*k, a.row, b.row);
        return cmp ? cmp < 0 : a.row < b.row;
    }
};

__global__ void __launch_bounds__(kBlock) top_n_ranking_codes_kernel(const TopNKeys *kp, int64_t n, unsigned long long *__restrict__ codes)
{
    const TopNKeys &k = *kp;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) codes[r] = order_code(k, r);
}

// cut == nullptr: keep everything (TGPU_TOP_N_RANKING_PREFILTER=off)
__global__ void __launch_bounds__(kBlock) top_n_ranking_prefilter_kernel(const unsigned long long *__restrict__ codes, const int32_t *__restrict__ gids, int64_t n,
                                                                         const unsigned long long *__restrict__ cut, int64_t groups, int32_t *__restrict__ flags)
{
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        const int64_t g = gids[r];
        const bool known = g >= 0 && g < groups;
        flags[r] = known && (!cut || codes[r] <= cut[g]) ? 1 : 0;
    }
}

// rows_in[i] + row_base = the i-th row's number in the source (rows_in == nullptr: row i)
__global__ void __launch_bounds__(kBlock) top_n_ranking_sort_keys_kernel(const int32_t *__restrict__ rows_in, int64_t row_base, const int32_t *__restrict__ gids,
                                                                         const unsigned long long *__restrict__ codes, int64_t m, int64_t source_rows,
                                                                         SortKey *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        int64_t r = row_base + (rows_in ? rows_in[i] : i);
        if (r < 0 || r >= source_rows) r = 0;   // (never: the positions come from compact_positions over source_rows flags)
        out[i] = SortKey{codes[r], gids[r], (int)r};
    }
}

__global__ void __launch_bounds__(kBlock) top_n_ranking_heads_kernel(const SortKey *__restrict__ sorted, int64_t m, const TopNKeys *kp, Starts *__restrict__ heads)
{
    const TopNKeys &k = *kp;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        bool group_head = i == 0, peer_head = i == 0;
        if (i > 0) {
            const SortKey a = sorted[i - 1], b = sorted[i];
            group_head = a.gid != b.gid;
            peer_head = group_head || a.code != b.code || compare_rows(k, a.row, b.row) != 0;
        }
        heads[i] = Starts{group_head ? (int)i : 0, peer_head ? (int)i : 0};
    }
}

// rank_peers: RANK (the ranking of a row is that of its peer run's head); otherwise ROW_NUMBER
__global__ void __launch_bounds__(kBlock) top_n_ranking_keep_kernel(const SortKey *__restrict__ sorted, const Starts *__restrict__ starts, int64_t m, int64_t max_rank,
                                                                    bool rank_peers, int32_t *__restrict__ flags, unsigned long long *__restrict__ cut, int64_t groups)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        const Starts s = starts[i];
        const int64_t position = i - s.group + 1;
        const int64_t ranking = rank_peers ? (int64_t)s.peer - s.group + 1 : position;
        flags[i] = ranking <= max_rank ? 1 : 0;
        if (position == max_rank) {   // the n-th row of its group in this selection: the only writer of cut[g] in this launch
            const SortKey key = sorted[i];
            if (key.gid >= 0 && key.gid < groups && key.code < cut[key.gid]) cut[key.gid] = key.code;
        }
    }
}

__global__ void __launch_bounds__(kBlock) top_n_ranking_emit_kernel(const SortKey *__restrict__ sorted, const Starts *__restrict__ starts, const int32_t *__restrict__ flags,
                                                                    const int32_t *__restrict__ offsets, int64_t m, bool rank_peers, int32_t *__restrict__ rows_out,
                                                                    int32_t *__restrict__ gids_out, int64_t *__restrict__ rank_out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        if (!flags[i]) continue;
        const int64_t o = offsets[i];
        if (o < 0 || o >= m) continue;   // (never: an exclusive scan of m flags)
        const SortKey key = sorted[i];
        const Starts s = starts[i];
        rows_out[o] = key.row;
        gids_out[o] = key.gid;
        rank_out[o] = rank_peers ? (int64_t)s.peer - s.group + 1 : i - s.group + 1;
    }
}

}  // namespace

GroupedTopNGpu::GroupedTopNGpu(Context *ctx, std::vector<int32_t> types, std::vector<int32_t> partition_channels, std::vector<int32_t> sort_channels,
                               std::vector<int32_t> sort_orders, int32_t ranking_type, int64_t max_rank, int32_t hash_channel, int32_t expected_positions)
    : ctx_(ctx), types_(std::move(types)), partition_channels_(std::move(partition_channels)), sort_channels_(std::move(sort_channels)),
      sort_orders_(std::move(sort_orders)), ranking_type_(ranking_type), hash_channel_(hash_channel), max_rank_(max_rank), store_(ctx, types_)
{
    if (!partition_channels_.empty()) {
        std::vector<int32_t> partition_types;
        for (int32_t ch : partition_channels_) partition_types.push_back(types_[(size_t)ch]);
        hash_ = std::make_unique<GroupByHashGpu>(ctx, std::move(partition_types), hash_channel_ >= 0, expected_positions);
    }
    total_ = ctx_->alloc(8);
}

int64_t GroupedTopNGpu::estimated_size() const
{
    return (hash_ ? hash_->estimated_size() : 0) + store_.estimated_size() + (int64_t)(store_gids_ ? store_gids_->bytes() : 0) + (int64_t)(cut_ ? cut_->bytes() : 0);
}

void GroupedTopNGpu::grow_cut(int64_t groups)
{
    if (groups <= cut_groups_) return;
    if (!cut_ || (int64_t)(cut_->bytes() / 8) < groups) {
        BufferPtr bigger = ctx_->alloc(std::max<size_t>((size_t)groups * 2, 1024) * 8);
        if (cut_ && cut_groups_ > 0) HIP_CHECK(hipMemcpyAsync(bigger->ptr(), cut_->ptr(), (size_t)cut_groups_ * 8, hipMemcpyDeviceToDevice, ctx_->stream()));
        cut_ = bigger;
    }
    k::fill_u64(ctx_, cut_->as<uint64_t>() + cut_groups_, kNotFull, groups - cut_groups_);   // new groups are not full yet
    cut_groups_ = groups;
}

void GroupedTopNGpu::append_gids(const int32_t *gids, int64_t n)
{
    const int64_t have = store_.position_count() - n;   // called after the rows themselves were appended
    if (!store_gids_ || (int64_t)(store_gids_->bytes() / 4) < have + n) {
        BufferPtr bigger = ctx_->alloc(std::max<size_t>((size_t)(have + n) * 2, 1024) * 4);
        if (store_gids_ && have > 0) HIP_CHECK(hipMemcpyAsync(bigger->ptr(), store_gids_->ptr(), (size_t)have * 4, hipMemcpyDeviceToDevice, ctx_->stream()));
        store_gids_ = bigger;
    }
    HIP_CHECK(hipMemcpyAsync(store_gids_->as<int32_t>() + have, gids, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx_->stream()));
}

BufferPtr GroupedTopNGpu::upload_keys(const DevicePage &src)
{
    TopNKeys host{};
    host.cols.n = (int32_t)sort_channels_.size();
    for (size_t i = 0; i < sort_channels_.size(); i++) {
        host.cols.c[i] = view_of(src.cols[(size_t)sort_channels_[i]]);
        host.order[i] = sort_orders_[i];
    }
    BufferPtr keys = ctx_->alloc(sizeof(TopNKeys));
    ctx_->upload(keys->ptr(), &host, sizeof(TopNKeys));
    return keys;
}

BufferPtr GroupedTopNGpu::order_codes(const DevicePage &src, BufferPtr &keys_dev)
{
    keys_dev = upload_keys(src);
    BufferPtr codes = ctx_->alloc((size_t)std::max<int64_t>(src.n, 1) * 8);
    top_n_ranking_codes_kernel<<<grid_for(ctx_, src.n), kBlock, 0, ctx_->stream()>>>(keys_dev->as<TopNKeys>(), src.n, codes->as<unsigned long long>());
    check_launch("top_n_ranking_codes");
    return codes;
}

GroupedTopNGpu::Selection GroupedTopNGpu::select(const DevicePage &src, const BufferPtr &keys_dev, const int32_t *gids, const unsigned long long *codes,
                                                 const int32_t *rows_in, int64_t row_base, int64_t m)
{
    Selection s;
    if (m == 0) return s;
    TG_CHECK_ARG(m <= 0x7fffffffLL && src.n <= 0x7fffffffLL, "2^31 candidate rows or more: row numbers are int32");
    BufferPtr keys = ctx_->alloc((size_t)m * sizeof(SortKey)), sorted = ctx_->alloc((size_t)m * sizeof(SortKey));
    BufferPtr heads = ctx_->alloc((size_t)m * sizeof(Starts)), starts = ctx_->alloc((size_t)m * sizeof(Starts));
    BufferPtr flags = ctx_->alloc((size_t)m * 4), offsets = ctx_->alloc((size_t)m * 4);
    const int g = grid_for(ctx_, m);
    const bool rank_peers = ranking_type_ == TGPU_RANKING_RANK;
    top_n_ranking_sort_keys_kernel<<<g, kBlock, 0, ctx_->stream()>>>(rows_in, row_base, gids, codes, m, src.n, keys->as<SortKey>());
    check_launch("top_n_ranking_sort_keys");
    {
        KeyLess less{keys_dev->as<TopNKeys>()};
        size_t temp_bytes = 0;
        HIP_CHECK(rocprim::merge_sort(nullptr, temp_bytes, keys->as<SortKey>(), sorted->as<SortKey>(), (size_t)m, less, ctx_->stream()));
        BufferPtr temp = ctx_->alloc(temp_bytes ? temp_bytes : 1);
        HIP_CHECK(rocprim::merge_sort(temp->ptr(), temp_bytes, keys->as<SortKey>(), sorted->as<SortKey>(), (size_t)m, less, ctx_->stream()));
    }
    top_n_ranking_heads_kernel<<<g, kBlock, 0, ctx_->stream()>>>(sorted->as<SortKey>(), m, keys_dev->as<TopNKeys>(), heads->as<Starts>());
    check_launch("top_n_ranking_heads");
    {
        size_t temp_bytes = 0;
        HIP_CHECK(rocprim::inclusive_scan(nullptr, temp_bytes, heads->as<Starts>(), starts->as<Starts>(), (size_t)m, MaxStarts{}, ctx_->stream()));
        BufferPtr temp = ctx_->alloc(temp_bytes ? temp_bytes : 1);
        HIP_CHECK(rocprim::inclusive_scan(temp->ptr(), temp_bytes, heads->as<Starts>(), starts->as<Starts>(), (size_t)m, MaxStarts{}, ctx_->stream()));
    }
    top_n_ranking_keep_kernel<<<g, kBlock, 0, ctx_->stream()>>>(sorted->as<SortKey>(), starts->as<Starts>(), m, max_rank_, rank_peers, flags->as<int32_t>(),
                                                                cut_->as<unsigned long long>(), cut_groups_);
    check_launch("top_n_ranking_keep");
    k::exclusive_scan_i32(ctx_, flags->as<int32_t>(), offsets->as<int32_t>(), m, total_->as<int64_t>());
    s.rows = ctx_->alloc((size_t)m * 4);
    s.gids = ctx_->alloc((size_t)m * 4);
    s.rank = ctx_->alloc((size_t)m * 8);
    top_n_ranking_emit_kernel<<<g, kBlock, 0, ctx_->stream()>>>(sorted->as<SortKey>(), starts->as<Starts>(), flags->as<int32_t>(), offsets->as<int32_t>(), m, rank_peers,
                                                                s.rows->as<int32_t>(), s.gids->as<int32_t>(), s.rank->as<int64_t>());
    check_launch("top_n_ranking_emit");
    s.count = ctx_->read_scalar(total_->as<int64_t>());
    TG_CHECK_STATE(s.count > 0 && s.count <= m, "kept-row count out of range");   // the first row of every group is always kept
    return s;
}

void GroupedTopNGpu::add_page(const DevicePage &page)
{
    TG_CHECK_ARG(page.cols.size() == types_.size(), "page channel count does not match the operator's types");
    for (size_t i = 0; i < types_.size(); i++) TG_CHECK_ARG(page.cols[i].type == types_[i], "page channel type does not match the operator's types");
    const int64_t n = page.n;
    TG_CHECK_ARG(n >= 0 && n <= 0x7fffffffLL, "a page of 2^31 rows or more: row numbers inside a page are int32");
    if (n == 0) return;
    // 1. group ids
    grow(ctx_, gids_, (size_t)n * 4);
    int64_t groups = 1;
    if (hash_) {
        std::vector<const DeviceColumn *> keys;
        for (int32_t ch : partition_channels_) keys.push_back(&page.cols[(size_t)ch]);
        const int64_t *hashes = hash_channel_ >= 0 ? (const int64_t *)page.cols[(size_t)hash_channel_].values : nullptr;
        hash_->get_group_ids(keys, hashes, n, gids_->as<int32_t>());
        groups = hash_->group_count();
    }
    else {
        k::fill_i32(ctx_, gids_->as<int32_t>(), 0, n);
    }
    grow_cut(groups);
    // 2. order codes of the whole page
    BufferPtr keys_dev, codes;
    {
        ProfileScope ps(ctx_, "top_n_ranking_prefilter");
        codes = order_codes(page, keys_dev);
    }
    // 3. - 6. slice by slice: the first slice of a large page sets the cutoffs the later ones are filtered with
    const int64_t slice = std::min(n, slice_rows_);
    grow(ctx_, flags_, (size_t)slice * 4);
    grow(ctx_, offsets_, (size_t)slice * 4);
    grow(ctx_, positions_, (size_t)slice * 4);
    for (int64_t first = 0; first < n; first += slice) {
        const int64_t len = std::min(slice, n - first);
        int64_t m = 0;
        {
            ProfileScope ps(ctx_, "top_n_ranking_prefilter");
            top_n_ranking_prefilter_kernel<<<grid_for(ctx_, len), kBlock, 0, ctx_->stream()>>>(codes->as<unsigned long long>() + first, gids_->as<int32_t>() + first, len,
                                                                                               prefilter_ ? cut_->as<unsigned long long>() : nullptr, cut_groups_,
                                                                                               flags_->as<int32_t>());
            check_launch("top_n_ranking_prefilter");
            k::exclusive_scan_i32(ctx_, flags_->as<int32_t>(), offsets_->as<int32_t>(), len, total_->as<int64_t>());
            k::compact_positions(ctx_, flags_->as<int32_t>(), offsets_->as<int32_t>(), len, positions_->as<int32_t>());
            check_launch("top_n_ranking_compact_positions");
            m = ctx_->read_scalar(total_->as<int64_t>());
        }
        TG_CHECK_STATE(m >= 0 && m <= len, "survivor count out of range");
        // what tools/exp_top_n_ranking.py reports next to the times: rows the prefilter saw and dropped, the store's largest size
        ctx_->profile_note("top_n_ranking_rows_seen", len);
        ctx_->profile_note("top_n_ranking_rows_dropped", len - m);
        if (m == 0) continue;
        Selection kept;
        {
            ProfileScope ps(ctx_, "top_n_ranking_select");
            kept = select(page, keys_dev, gids_->as<int32_t>(), codes->as<unsigned long long>(), positions_->as<int32_t>(), first, m);
        }
        DevicePage winners;
        winners.n = kept.count;
        {
            ProfileScope ps(ctx_, "top_n_ranking_gather");
            for (auto &c : page.cols) winners.cols.push_back(k::gather_column(ctx_, c, kept.rows->as<int32_t>(), kept.count, false));
        }
        store_.add_page(winners);
        append_gids(kept.gids->as<int32_t>(), kept.count);
        ctx_->profile_note("top_n_ranking_store_rows", store_.position_count());
        if (store_.position_count() > std::max<int64_t>(2 * after_compaction_, compact_floor_)) compact();
    }
}

GroupedTopNGpu::Selection GroupedTopNGpu::compact()
{
    DevicePage all;
    all.n = store_.position_count();
    for (size_t i = 0; i < types_.size(); i++) all.cols.push_back(store_.column((int)i));
    Selection kept;
    if (all.n == 0) return kept;
    DevicePage compacted;
    {
        ProfileScope ps(ctx_, "top_n_ranking_compact");
        BufferPtr keys_dev;
        BufferPtr codes = order_codes(all, keys_dev);
        k::fill_u64(ctx_, cut_->as<uint64_t>(), kNotFull, cut_groups_);   // reset: the selection below sets cut[g] of every full group
        kept = select(all, keys_dev, store_gids_->as<int32_t>(), codes->as<unsigned long long>(), nullptr, 0, all.n);
        compacted.n = kept.count;
        for (auto &c : all.cols) compacted.cols.push_back(k::gather_column(ctx_, c, kept.rows->as<int32_t>(), kept.count, false));
    }
    PagesIndexGpu fresh(ctx_, types_);
    fresh.add_page(compacted);
    store_ = std::move(fresh);
    store_gids_ = kept.gids;
    after_compaction_ = kept.count;
    return kept;
}

DevicePage GroupedTopNGpu::result(DeviceColumn *ranking)
{
    Selection kept = compact();
    DevicePage out;
    out.n = store_.position_count();
    for (size_t i = 0; i < types_.size(); i++) out.cols.push_back(store_.column((int)i));
    DeviceColumn rank;
    rank.type = TGPU_BIGINT;
    rank.n = out.n;
    rank.values_buf = kept.rank ? kept.rank : ctx_->alloc(8);
    rank.values = rank.values_buf->ptr();
    *ranking = std::move(rank);
    return out;
}

}  // namespace tgpu

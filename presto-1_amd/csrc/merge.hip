// merge.hip -- the kernels of one merge round (merge.h).  Every kernel is its own launch: no signalling between workgroups, no
// persistent kernel, no wait on another workgroup anywhere.  The streams' views and the key spec live in device memory (read through
// pointers: run-time stream and key indices are then plain loads).  No kernel trusts the input to be sorted: every binary search runs
// over a fixed index range that halves, and every index is clamped to the range it was derived from.
#include "merge.h"

#include "device_order.h"
#include "kernels.h"

namespace tgpu {
namespace {

struct alignas(16) Chunk16 { unsigned int w[4]; };

// ---- merge_bound: ONE workgroup.  Lane 0 walks the open streams for B = the smallest (last row of the window, stream); then lane s
// counts by binary search the rows of stream s's window that are settled: (row, s) <= (B, t_B), i.e. the upper bound of B for the
// streams up to and including t_B and the lower bound for the ones after it.  With no open stream every row of every window settles.
// counts[0, k) = the settled counts, counts[k, 2k] = their exclusive prefix sum (the runs of the merge) and the total.
// Reads: rows [head, head + window) of each stream's key columns, window <= rows - head (MergeGpu::round checks it).
__global__ void __launch_bounds__(256) merge_bound_kernel(const MergeStreamView *__restrict__ views, int k, const MergeKeySpec *__restrict__ spec, long long *__restrict__ counts)
{
    __shared__ int s_tb;
    if (threadIdx.x == 0) {
        int tb = -1;
        for (int s = 0; s < k; s++) {
            const MergeStreamView &v = views[s];
            if (!v.open || v.window <= 0) continue;
            if (tb < 0 || compare_rows(v.keys, v.head + v.window - 1, views[tb].keys, views[tb].head + views[tb].window - 1, spec->order) < 0) tb = s;
        }
        s_tb = tb;
    }
    __syncthreads();
    const int tb = s_tb;
    for (int s = threadIdx.x; s < k; s += 256) {
        const MergeStreamView &v = views[s];
        long long c = v.window > 0 ? v.window : 0;
        if (tb >= 0 && c > 0) {
            const MergeStreamView &b = views[tb];
            const long long rb = b.head + b.window - 1;
            long long lo = 0, hi = c;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                const int cmp = compare_rows(v.keys, v.head + mid, b.keys, rb, spec->order);
                if (s <= tb ? cmp <= 0 : cmp < 0) lo = mid + 1;
                else hi = mid;
            }
            c = lo;
        }
        counts[s] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long at = 0;
        for (int s = 0; s < k; s++) {
            counts[k + s] = at;
            at += counts[s];
        }
        counts[2 * k] = at;
    }
}

// ---- merge_path, step 1: pair i of the n settled rows = (order code, stream, row); the settled prefixes lie one after the other,
// stream s at [begin[s], begin[s + 1]) (begin = counts + k of merge_bound).  Writes pairs[0, n), n = begin[k] as the host read it.
__global__ void __launch_bounds__(256) merge_pairs_kernel(const MergeStreamView *__restrict__ views, int k, const MergeKeySpec *__restrict__ spec,
                                                          const long long *__restrict__ begin, long long n, MergePair *__restrict__ pairs)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int lo = 0, hi = k - 1;   // the last s with begin[s] <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (begin[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const MergeStreamView &v = views[lo];
        long long r = v.head + (i - begin[lo]);
        if (r >= v.rows) r = v.rows - 1;   // (cannot happen: i - begin[lo] < counts[lo] <= window)
        MergePair p;
        p.code = order_code(v.keys.c[0], spec->order[0], r);
        p.stream = (unsigned int)lo;
        p.row = (unsigned int)r;
        pairs[i] = p;
    }
}

// does y (of the right run) come strictly before x (of the left run)?  Codes first; on equal codes the full comparator through the
// refs (the code drops the lowest order bit of the first key, so equal codes never prove equal rows); a full tie keeps x in front: the
// left run is the lower stream, so the merge is stable.
__device__ __forceinline__ bool right_first(const MergeStreamView *__restrict__ views, const MergeKeySpec *__restrict__ spec, unsigned long long cx, unsigned int sx,
                                            unsigned int rx, unsigned long long cy, unsigned int sy, unsigned int ry)
{
    if (cy != cx) return cy < cx;
    return compare_rows(views[sy].keys, ry, views[sx].keys, rx, spec->order) < 0;
}

// ---- merge_path, step 2: one two-way merge-path pass.  Workgroup b owns tile tiles[b]: outputs [d0, d1) of the merge of run A =
// src[a_begin, a_end) with run B = src[a_end, b_end), d0 = tile * kMergeTile.  Lanes 0 and 1 find the splits of the diagonals d0 and
// d1 by binary search in global memory; the two sub-ranges (together d1 - d0 <= kMergeTile pairs) are staged in LDS, codes and refs in
// arrays of their own; every lane then finds the split of its own diagonal in LDS and merges kMergeItems outputs sequentially, each
// stored as one 16-byte pair to dst[a_begin + d0, a_begin + d1) as soon as it is decided (a lane's 9 pairs are 144 contiguous bytes).
// LDS: 16 B x kMergeTile = 36 KiB per workgroup.  kMergeItems is odd: the lanes of a group start 9 codes = 18 banks apart, which
// spreads the 8-byte loads of a lane group over all banks where an even count would fold them onto a few.
// An empty run B makes the pass a copy (a run that changes buffers without a partner).
__global__ void __launch_bounds__(kMergeBlock) merge_path_kernel(const MergeStreamView *__restrict__ views, const MergeKeySpec *__restrict__ spec,
                                                                 const MergeTile *__restrict__ tiles, const MergePair *__restrict__ src, MergePair *__restrict__ dst)
{
    __shared__ unsigned long long s_code[kMergeTile];
    __shared__ uint2 s_ref[kMergeTile];
    __shared__ long long s_split[2];
    const MergeTile t = tiles[blockIdx.x];
    const long long na = t.a_end - t.a_begin, nb = t.b_end - t.a_end, len = na + nb;
    const long long d0 = t.tile * kMergeTile, d1 = d0 + kMergeTile < len ? d0 + kMergeTile : len;
    const MergePair *__restrict__ A = src + t.a_begin, *__restrict__ B = src + t.a_end;
    if (threadIdx.x < 2) {
        const long long d = threadIdx.x ? d1 : d0;
        long long lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
        while (lo < hi) {   // mid in [max(0, d - nb), min(d, na)): mid < na and 0 <= d - 1 - mid < nb
            const long long mid = (lo + hi) >> 1;
            const MergePair x = A[mid], y = B[d - 1 - mid];
            if (right_first(views, spec, x.code, x.stream, x.row, y.code, y.stream, y.row)) hi = mid;
            else lo = mid + 1;
        }
        s_split[threadIdx.x] = lo;
    }
    __syncthreads();
    const long long a0 = s_split[0], b0 = d0 - a0;
    long long a1 = s_split[1];
    // on sorted runs a0 <= a1 <= a0 + (d1 - d0) holds by itself; on unsorted input it is enforced (both ends stay inside the runs:
    // a0 <= min(d0, na) and a0 + d1 - d0 >= d1 - nb)
    if (a1 < a0) a1 = a0;
    if (a1 > a0 + (d1 - d0)) a1 = a0 + (d1 - d0);
    const int ta = (int)(a1 - a0), n = (int)(d1 - d0), tb = n - ta;
    for (int i = threadIdx.x; i < n; i += kMergeBlock) {
        const MergePair p = i < ta ? A[a0 + i] : B[b0 + (i - ta)];
        s_code[i] = p.code;
        s_ref[i] = make_uint2(p.stream, p.row);
    }
    __syncthreads();
    // this lane's outputs [d, d + cnt) of the tile
    const int d = (int)threadIdx.x * kMergeItems < n ? (int)threadIdx.x * kMergeItems : n;
    const int cnt = n - d < kMergeItems ? n - d : kMergeItems;
    int lo = d > tb ? d - tb : 0, hi = d < ta ? d : ta;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, y = ta + d - 1 - mid;
        if (right_first(views, spec, s_code[mid], s_ref[mid].x, s_ref[mid].y, s_code[y], s_ref[y].x, s_ref[y].y)) hi = mid;
        else lo = mid + 1;
    }
    int ai = lo, bi = d - lo;   // ai + bi = d + j < n = ta + tb below: never both runs exhausted
    unsigned long long ca = 0, cb = 0;
    uint2 ra = make_uint2(0, 0), rb = make_uint2(0, 0);
    if (ai < ta) { ca = s_code[ai]; ra = s_ref[ai]; }
    if (bi < tb) { cb = s_code[ta + bi]; rb = s_ref[ta + bi]; }
    // LDS is only read from here on; every output is stored as soon as it is decided: dst[a_begin + d0 + d + j], j < cnt
    MergePair *__restrict__ out = dst + t.a_begin + d0 + d;
#pragma unroll
    for (int j = 0; j < kMergeItems; j++) {
        if (j < cnt) {
            const bool take_b = ai >= ta || (bi < tb && right_first(views, spec, ca, ra.x, ra.y, cb, rb.x, rb.y));
            MergePair p;
            if (take_b) {
                p.code = cb;
                p.stream = rb.x;
                p.row = rb.y;
                bi++;
                if (bi < tb) { cb = s_code[ta + bi]; rb = s_ref[ta + bi]; }
            }
            else {
                p.code = ca;
                p.stream = ra.x;
                p.row = ra.y;
                ai++;
                if (ai < ta) { ca = s_code[ai]; ra = s_ref[ai]; }
            }
            out[j] = p;
        }
    }
}

// ---- merge_gather: out[i] = cell refs[i].row of the channel in stream refs[i].stream, read straight from that stream's buffer.
// cols[s * stride] = the channel's column in stream s.  A lane assembles 16 bytes of consecutive outputs and stores them at once (the
// last elements one by one).  NULLS: the null bytes instead of the values (a stream without a null array holds no null).
template <typename T, bool NULLS>
__global__ void __launch_bounds__(256) merge_gather_kernel(const TgColView *__restrict__ cols, int stride, const MergePair *__restrict__ refs, long long n, T *__restrict__ out)
{
    constexpr int E = 16 / (int)sizeof(T);
    const long long chunks = (n + E - 1) / E;
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (long long)gridDim.x * 256) {
        const long long i0 = c * E;
        union { Chunk16 chunk; T v[E]; } u;
#pragma unroll
        for (int e = 0; e < E; e++) {
            T x = T(0);
            if (i0 + e < n) {
                const MergePair p = refs[i0 + e];
                const TgColView &col = cols[(long long)p.stream * stride];
                if (NULLS) x = col.nulls ? (T)col.nulls[p.row] : T(0);
                else x = ((const T *)col.values)[p.row];
            }
            u.v[e] = x;
        }
        if (i0 + E <= n) *reinterpret_cast<Chunk16 *>(out + i0) = u.chunk;
        else
            for (int e = 0; i0 + e < n; e++) out[i0 + e] = u.v[e];
    }
}

__global__ void __launch_bounds__(256) merge_varchar_len_kernel(const TgColView *__restrict__ cols, int stride, const MergePair *__restrict__ refs, long long n, int32_t *__restrict__ len)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const MergePair p = refs[i];
        const TgColView &col = cols[(long long)p.stream * stride];
        len[i] = col.offsets[p.row + 1] - col.offsets[p.row];
    }
}

// one row per lane; writes out_pool[out_offsets[i], out_offsets[i] + the row's length) and the closing offset
__global__ void __launch_bounds__(256) merge_varchar_bytes_kernel(const TgColView *__restrict__ cols, int stride, const MergePair *__restrict__ refs, long long n,
                                                                  int32_t *__restrict__ out_offsets, const long long *__restrict__ total, uint8_t *__restrict__ out_pool)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const MergePair p = refs[i];
        const TgColView &col = cols[(long long)p.stream * stride];
        const int32_t a = col.offsets[p.row], b = col.offsets[p.row + 1], o = out_offsets[i];
        const uint8_t *pool = (const uint8_t *)col.values;
        for (int32_t x = a; x < b; x++) out_pool[o + (x - a)] = pool[x];
        if (i == n - 1) out_offsets[n] = (int32_t)(*total);
    }
}

}  // namespace

MergeGpu::MergeGpu(Context *ctx, std::vector<int32_t> types, std::vector<int32_t> output_channels, std::vector<int32_t> sort_channels, std::vector<int32_t> sort_orders)
    : ctx_(ctx), types_(std::move(types)), output_channels_(std::move(output_channels)), sort_channels_(std::move(sort_channels))
{
    for (int32_t t : types_) TG_CHECK_ARG(valid_type(t), "unknown channel type");
    TG_CHECK_ARG(!sort_channels_.empty() && (int)sort_channels_.size() <= kMaxKeyChannels, "between 1 and 8 sort channels are supported");
    TG_CHECK_ARG(sort_orders.size() == sort_channels_.size(), "one sort order per sort channel");
    for (int32_t ch : sort_channels_) TG_CHECK_ARG(ch >= 0 && ch < (int)types_.size(), "sort channel out of range");
    for (int32_t ch : output_channels_) TG_CHECK_ARG(ch >= 0 && ch < (int)types_.size(), "output channel out of range");
    spec_.n = (int)sort_channels_.size();
    for (size_t i = 0; i < sort_orders.size(); i++) {
        TG_CHECK_ARG(sort_orders[i] >= TGPU_SORT_ASC_NULLS_FIRST && sort_orders[i] <= TGPU_SORT_DESC_NULLS_LAST, "unknown sort order");
        spec_.order[i] = sort_orders[i];
    }
}

DevicePage MergeGpu::round(const std::vector<const DevicePage *> &pages, const std::vector<int64_t> &head, const std::vector<int64_t> &window, const std::vector<bool> &open,
                           std::vector<int64_t> &settled)
{
    const int k = (int)pages.size();
    settled.assign((size_t)k, 0);
    DevicePage out;
    if (k == 0) return out;
    TG_CHECK_STATE((int64_t)k <= 0x7fffffff / 2 - 1, "too many streams");
    std::vector<MergeStreamView> hv((size_t)k);
    bool any_open = false;
    int64_t in_windows = 0;
    for (int s = 0; s < k; s++) {
        MergeStreamView &v = hv[(size_t)s];
        memset(&v, 0, sizeof(v));
        const int64_t rows = pages[(size_t)s] ? pages[(size_t)s]->n : 0;
        TG_CHECK_STATE(head[(size_t)s] >= 0 && window[(size_t)s] >= 0 && head[(size_t)s] + window[(size_t)s] <= rows && rows <= 0xffffffffLL, "merge: window outside the stream's buffer");
        TG_CHECK_STATE(!open[(size_t)s] || window[(size_t)s] > 0, "merge: an open stream without a buffered row");
        if (pages[(size_t)s]) {
            std::vector<const DeviceColumn *> keys;
            for (int32_t ch : sort_channels_) keys.push_back(&pages[(size_t)s]->cols[(size_t)ch]);
            v.keys = key_cols_of(keys);
        }
        v.head = head[(size_t)s];
        v.rows = rows;
        v.window = window[(size_t)s];
        v.open = open[(size_t)s] ? 1 : 0;
        any_open = any_open || open[(size_t)s];
        in_windows += window[(size_t)s];
    }
    TG_CHECK_STATE(in_windows <= kMergeMaxRoundRows, "merge: the windows of one round exceed a page");
    if (in_windows == 0) return out;
    if (!spec_dev_) {
        spec_dev_ = ctx_->alloc(sizeof(MergeKeySpec));
        ctx_->upload(spec_dev_->ptr(), &spec_, sizeof(MergeKeySpec));
    }
    grow(ctx_, views_, (size_t)k * sizeof(MergeStreamView));
    grow(ctx_, counts_, (size_t)(2 * k + 1) * 8);
    ctx_->upload(views_->ptr(), hv.data(), (size_t)k * sizeof(MergeStreamView));
    const MergeStreamView *views = views_->as<MergeStreamView>();
    const MergeKeySpec *spec = spec_dev_->as<MergeKeySpec>();
    {
        ProfileScope ps(ctx_, "merge_bound");
        merge_bound_kernel<<<1, 256, 0, ctx_->stream()>>>(views, k, spec, counts_->as<long long>());
        check_launch("merge_bound");
        // with every stream closed each window settles whole: the counts are known without the read-back
        if (any_open) ctx_->download(settled.data(), counts_->ptr(), (size_t)k * 8);
        else settled = window;
    }
    int64_t total = 0;
    int with_rows = 0, only = -1;
    for (int s = 0; s < k; s++) {
        TG_CHECK_STATE(settled[(size_t)s] >= 0 && settled[(size_t)s] <= window[(size_t)s], "merge: settled count outside the window");
        total += settled[(size_t)s];
        if (settled[(size_t)s] > 0) {
            with_rows++;
            only = s;
        }
    }
    if (total == 0) return out;
    out.n = total;
    if (with_rows == 1) {   // one stream's rows alone: passed through by region, owners shared
        for (int32_t ch : output_channels_) out.cols.push_back(k::region_of(ctx_, pages[(size_t)only]->cols[(size_t)ch], head[(size_t)only], total));
        return out;
    }
    int final_buf = 0;
    {
        ProfileScope ps(ctx_, "merge_path");
        grow(ctx_, pairs_[0], (size_t)total * sizeof(MergePair));
        grow(ctx_, pairs_[1], (size_t)total * sizeof(MergePair));
        merge_pairs_kernel<<<grid_for(ctx_, total), 256, 0, ctx_->stream()>>>(views, k, spec, counts_->as<long long>() + k, total, pairs_[0]->as<MergePair>());
        check_launch("merge_pairs");
        // the runs and, pass by pass, the tiles of their pairwise merges.  All runs but the last always lie in one buffer; a last run
        // without a partner stays where it is, and changes buffers (a copy pass of its own tiles) only when the NEXT pass merges it
        // and it is not in that pass's source yet.
        struct Run { int64_t b, e; int buf; };
        std::vector<Run> runs;
        int64_t at = 0;
        for (int s = 0; s < k; s++) {
            if (settled[(size_t)s] > 0) runs.push_back({at, at + settled[(size_t)s], 0});
            at += settled[(size_t)s];
        }
        struct Pass { size_t first, count; int src; };
        std::vector<Pass> passes;
        std::vector<MergeTile> tiles;
        auto add_tiles = [&](int64_t a_begin, int64_t a_end, int64_t b_end) {
            for (int64_t t = 0; t * kMergeTile < b_end - a_begin; t++) tiles.push_back({a_begin, a_end, b_end, t});
        };
        while (runs.size() > 1) {
            const int src = runs[0].buf, dst = 1 - src;
            const size_t m = runs.size(), first = tiles.size();
            std::vector<Run> next;
            for (size_t j = 0; j + 1 < m; j += 2) {
                add_tiles(runs[j].b, runs[j].e, runs[j + 1].e);
                next.push_back({runs[j].b, runs[j + 1].e, dst});
            }
            if (m % 2 == 1) {
                Run z = runs[m - 1];
                if (next.size() % 2 == 1 && z.buf != dst) {   // merged by the next pass, whose source is this pass's destination
                    add_tiles(z.b, z.e, z.e);
                    z.buf = dst;
                }
                next.push_back(z);
            }
            passes.push_back({first, tiles.size() - first, src});
            runs = std::move(next);
        }
        final_buf = runs[0].buf;
        grow(ctx_, tiles_, tiles.size() * sizeof(MergeTile));
        ctx_->upload(tiles_->ptr(), tiles.data(), tiles.size() * sizeof(MergeTile));
        for (const Pass &p : passes) {
            if (p.count == 0) continue;
            TG_CHECK_STATE(p.count <= 0x7fffffffu, "merge: too many tiles");
            merge_path_kernel<<<(unsigned int)p.count, kMergeBlock, 0, ctx_->stream()>>>(views, spec, tiles_->as<MergeTile>() + p.first, pairs_[p.src]->as<MergePair>(),
                                                                                       pairs_[1 - p.src]->as<MergePair>());
        }
        check_launch("merge_path");
    }
    return gather(pages, pairs_[final_buf]->as<MergePair>(), total);
}

DevicePage MergeGpu::gather(const std::vector<const DevicePage *> &pages, const MergePair *refs, int64_t n)
{
    const int k = (int)pages.size(), stride = (int)output_channels_.size();
    DevicePage out;
    out.n = n;
    if (stride == 0) return out;
    std::vector<TgColView> hv((size_t)k * (size_t)stride);
    std::vector<bool> any_nulls((size_t)stride, false);
    for (int s = 0; s < k; s++)
        for (int c = 0; c < stride; c++) {
            TgColView v{};
            if (pages[(size_t)s]) {
                v = view_of(pages[(size_t)s]->cols[(size_t)output_channels_[(size_t)c]]);
                any_nulls[(size_t)c] = any_nulls[(size_t)c] || v.nulls != nullptr;
            }
            hv[(size_t)s * (size_t)stride + (size_t)c] = v;
        }
    grow(ctx_, out_views_, hv.size() * sizeof(TgColView));
    ctx_->upload(out_views_->ptr(), hv.data(), hv.size() * sizeof(TgColView));
    // the VARCHAR channels' byte totals come back in one read after every length scan has been enqueued
    struct Var { size_t col; BufferPtr total; };
    std::vector<Var> vars;
    {
        ProfileScope ps(ctx_, "merge_gather");
        for (int c = 0; c < stride; c++) {
            const TgColView *cols = out_views_->as<TgColView>() + c;
            DeviceColumn col;
            col.type = types_[(size_t)output_channels_[(size_t)c]];
            col.n = n;
            if (any_nulls[(size_t)c]) {
                col.nulls_buf = ctx_->alloc((size_t)n);
                col.nulls = col.nulls_buf->as<uint8_t>();
                merge_gather_kernel<uint8_t, true><<<grid_for(ctx_, ceil_div(n, 16)), 256, 0, ctx_->stream()>>>(cols, stride, refs, n, col.nulls_buf->as<uint8_t>());
            }
            if (col.type == TGPU_VARCHAR) {
                col.offsets_buf = ctx_->alloc((size_t)(n + 1) * 4);
                col.offsets = col.offsets_buf->as<int32_t>();
                BufferPtr len = ctx_->alloc((size_t)n * 4), total = ctx_->alloc(8);
                merge_varchar_len_kernel<<<grid_for(ctx_, n), 256, 0, ctx_->stream()>>>(cols, stride, refs, n, len->as<int32_t>());
                k::exclusive_scan_i32(ctx_, len->as<int32_t>(), col.offsets_buf->as<int32_t>(), n, total->as<int64_t>());
                vars.push_back({out.cols.size(), total});
            }
            else {
                const int w = type_width(col.type);
                col.values_buf = ctx_->alloc((size_t)n * (size_t)w);
                col.values = col.values_buf->ptr();
                const int g = grid_for(ctx_, ceil_div(n * w, 16));
                if (w == 8) merge_gather_kernel<uint64_t, false><<<g, 256, 0, ctx_->stream()>>>(cols, stride, refs, n, col.values_buf->as<uint64_t>());
                else if (w == 4) merge_gather_kernel<uint32_t, false><<<g, 256, 0, ctx_->stream()>>>(cols, stride, refs, n, col.values_buf->as<uint32_t>());
                else merge_gather_kernel<uint8_t, false><<<g, 256, 0, ctx_->stream()>>>(cols, stride, refs, n, col.values_buf->as<uint8_t>());
            }
            check_launch("merge_gather");
            out.cols.push_back(std::move(col));
        }
        if (!vars.empty()) {
            std::vector<int64_t> totals(vars.size());
            std::vector<Context::Transfer> reads;
            for (size_t i = 0; i < vars.size(); i++) reads.push_back({&totals[i], vars[i].total->ptr(), 8});
            ctx_->download_batch(reads);
            for (size_t i = 0; i < vars.size(); i++) {
                if (totals[i] > 0x7fffffffLL) fail(TGPU_ERR_INSUFFICIENT_RESOURCES, "variable width block cannot exceed 2GB");
                DeviceColumn &col = out.cols[vars[i].col];
                col.values_buf = ctx_->alloc((size_t)(totals[i] > 0 ? totals[i] : 1));
                col.values = col.values_buf->ptr();
                col.pool_bytes = totals[i];
                col.pool_exact = true;
                merge_varchar_bytes_kernel<<<grid_for(ctx_, n), 256, 0, ctx_->stream()>>>(out_views_->as<TgColView>() + (int)vars[i].col, stride, refs, n,
                                                                                        col.offsets_buf->as<int32_t>(), vars[i].total->as<long long>(), col.values_buf->as<uint8_t>());
                check_launch("merge_gather_varchar");
            }
        }
    }
    return out;
}

}  // namespace tgpu

// window.hip -- window functions over the sorted pages index (WindowOperator.java:205-310; the row loop of WindowPartition.java:184-214).
//
// The reference walks the sorted index row by row: it finds the partition's end, then per row the peer group (updatePeerGroup,
// WindowPartition.java:238-247) and the frame (:281-345), and feeds every function.  Here, with i = a row's index in the sorted order:
//   1. ORDER       positions[i] = TopNGpu::sorted_positions over (partition channels ASC_NULLS_LAST, sort channels); no keys: the identity.
//   2. HEADS       window_heads_kernel compares rows positions[i - 1] and positions[i] with tg_rows_not_distinct (IS NOT DISTINCT FROM, not
//                  the comparator: -0.0 and +0.0 are one partition and peers) -> one byte per row: bit 0 = partition head, bit 1 = peer head.
//   3. SCAN        ONE forward scan in sorted order carries, fused:
//                    part_start, peer_start   max over "head ? i : 0"                 (the index of the latest head)
//                    part_ord, peer_ord       sum over the head bits                  (how many heads at or before i)
//                    per aggregate            (non-null count, 128-bit sum | max of the order code of device_agg.h), RESET at partition heads
//                  The element is (head, state); (a, x) . (b, y) = b ? (1, y) : (a, x + y) for the aggregates -- associative, so the scan is
//                  done in three launches (reduce, then scan), none of which waits for another workgroup:
//                    launch 1  window_scan_tiles_kernel<K, false>   one workgroup per tile of T rows: reads every argument through positions
//                              ONCE, leaves the row's (count, word) in the aggregate's running arrays and writes the tile's summary
//                    launch 2  window_scan_carries_kernel<K>        one workgroup scans the summaries, 256 tiles per trip
//                    launch 3  window_scan_tiles_kernel<K, true>    every tile again, seeded with the summary scan of the tile before it: reads
//                              the running arrays back (coalesced), overwrites them with the running values, writes the four index arrays,
//                              scatters the head indices (heads[ord - 1] = i) and raises the overflow word
//                  A workgroup scans 256 rows at a time: wave64 __shfl_up steps inside a wave, the four wave totals through LDS, the running
//                  carry in registers.  K = the aggregates one launch carries (at most kAggsPerLaunch = 4: ~30 state registers); an operator
//                  with more runs launches 1 - 3 again for the next four (the index arrays are written by the first run only).
//                  sum(bigint) overflow: the running 128-bit sum at row i IS the prefix of the partition's non-null values up to i, so
//                  "some prefix leaves int64" = "some row's running sum does not fit", checked where launch 3 writes it.  A tile-local sum
//                  beyond int64 is nothing: it lives in two words.
//   4. ENDS        part_end[i] = heads[part_ord[i]] - 1 (the next head; n - 1 behind the last one), peer_end alike: no reverse scan.
//   5. EVALUATE    window_evaluate_kernel, one launch per function: rankings from the index arrays, aggregates = the running value at the
//                  frame's end (i, peer_end[i] or part_end[i]), first / last / lag / lead = a row number per output row (negative = null),
//                  which k::gather_column turns into the column.  lag / lead with a default channel gather from the value column with the
//                  default column appended behind it (one PagesIndexGpu of two pages): "the default of the current row" is row N + positions[i],
//                  so every type, VARCHAR included, takes the one gather.
// Frames with offsets (tgpu_window_factory_create_framed; ROWS / GROUPS with k PRECEDING / k FOLLOWING, RANGE by peers) add, between 4 and 5:
//   4a. FRAMES     window_frame_bounds_kernel, once per distinct frame: frame_start[i] / frame_end[i] as indices of the sorted order (-1 = empty),
//                  the offsets read through positions at the current row (getFrameValue, WindowPartition.java:601-607).  GROUPS finds group g of a
//                  partition by index in the scattered peer heads.  A null / negative offset raises a bit of error word 2.
//   4b. EXTREMES   min / max over a frame [s, e] that does not start at its partition's first row is a range-maximum query over the per-row order
//                  codes (launch 1 leaves them in `raw`), answered from an index of 4 n words + (n / 64) log2(n / 64) words built by
//                  window_extreme_chunks_kernel (one wave per chunk of 64 rows) and one window_extreme_level_kernel launch per level:
//                    pre[i], suf[i]   the maximum from the chunk's first row to i / from i to the chunk's last row (one wave-shuffle scan each)
//                    mask[i]          bit j: row j of the chunk is greater than every row of (j, i] -- the stack of candidates; the maximum of
//                                     [s, i] inside one chunk is the row of the lowest set bit at or above s
//                    top[k][c]        the maximum of chunks c .. c + 2^k - 1 (a sparse table)
//                  so a query reads two to four words, whatever the frame's width.  Frames never cross a partition: nothing is segmented.
//                  count and sum take the difference of the running arrays at e and s - 1; the sum's running value is kept in both words (`hi`),
//                  and launch 3 raises no prefix overflow for it: only a frame's own sum outside int64 does, in the evaluate kernel.
// RANGE frames with a k PRECEDING / k FOLLOWING bound (tgpu_window_factory_create_ranged) fill the same frame_start / frame_end arrays in 4a:
//   4a'. KEYS      window_range_keys_kernel, once per distinct comparison key channel: codes[i] = the order code (device_order.h) of the comparison
//                  key of row positions[i], complemented under a descending sort, and key_null[i] = the SORT key of that row is null: one gather,
//                  after which every comparison is an unsigned compare of neighbouring words of one contiguous array.
//        BOUNDS    window_range_bounds_kernel, once per distinct frame: the row's bound values read through positions and encoded the same way, the
//                  partition's run of non-null keys from the null peer group (the nulls of ONE sort channel are one peer group at the partition's
//                  head or tail: two loads, no search), then per bound a gallop outward from the row's own position and a bisection
//                  (device_range_frame.h, which a host program compiles as it stands).  No row reads another row's result.
#include "window.h"
#include "kernels.h"
#include "topn.h"
#include "device_agg.h"
#include "device_order.h"
#include "device_range_frame.h"

#include <algorithm>

namespace tgpu {

namespace {

constexpr int kBlock = WindowGpu::kBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxAggs = WindowGpu::kAggsPerLaunch;

// the partition and the sort channels in device memory (read through a pointer: run-time column indices are then plain scalar loads)
struct WindowKeys {
    TgKeyCols part, order;
};

enum { kOpCount = 0, kOpSum = 1, kOpMax = 2 };

// one running aggregate of a scan launch; cnt == nullptr: the slot is unused
struct ScanAgg {
    TgColView arg;             // the argument column in arrival order (values == nullptr: count(*))
    int op, function;          // kOp*, tgpu_agg_function
    long long *cnt;            // [n] launch 1: the row's own count, launch 3: the running count
    unsigned long long *val;   // [n] the sum's low word / the extreme's order code (nullptr for the counts)
    unsigned long long *hi;    // [n] launch 3: the running sum's high word (nullptr: not kept)
    unsigned long long *raw;   // [n] launch 1: the row's own order code again, which launch 3 leaves alone (nullptr: not kept)
    int check_prefix;          // launch 3 raises the overflow word for a running sum outside int64 (the frames that grow from the partition's start)
};
template <int K> struct ScanArgs {
    ScanAgg a[K > 0 ? K : 1];
};

template <int K> struct State {
    int head;                      // the span holds a partition head
    int part_start, peer_start;    // the largest head index of the span (0: none, or row 0)
    int part_ord, peer_ord;        // heads in the span
    long long cnt[K > 0 ? K : 1];
    unsigned long long w0[K > 0 ? K : 1], w1[K > 0 ? K : 1];   // sum: low / high word; extreme: the code / 0
};

template <int K> __device__ __forceinline__ State<K> identity()
{
    State<K> s;
    s.head = s.part_start = s.peer_start = s.part_ord = s.peer_ord = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        s.cnt[k] = 0;
        s.w0[k] = s.w1[k] = 0;
    }
    return s;
}

// a in front of b
template <int K> __device__ __forceinline__ State<K> combine(const State<K> &a, const State<K> &b, const ScanArgs<K> &args)
{
    State<K> r;
    r.head = a.head | b.head;
    r.part_start = a.part_start > b.part_start ? a.part_start : b.part_start;
    r.peer_start = a.peer_start > b.peer_start ? a.peer_start : b.peer_start;
    r.part_ord = a.part_ord + b.part_ord;
    r.peer_ord = a.peer_ord + b.peer_ord;
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (b.head) {
            r.cnt[k] = b.cnt[k];
            r.w0[k] = b.w0[k];
            r.w1[k] = b.w1[k];
        }
        else if (args.a[k].op == kOpSum) {
            r.cnt[k] = a.cnt[k] + b.cnt[k];
            r.w0[k] = a.w0[k] + b.w0[k];
            r.w1[k] = a.w1[k] + b.w1[k] + (r.w0[k] < a.w0[k] ? 1ULL : 0ULL);
        }
        else {
            r.cnt[k] = a.cnt[k] + b.cnt[k];
            r.w0[k] = a.w0[k] > b.w0[k] ? a.w0[k] : b.w0[k];
            r.w1[k] = 0;
        }
    }
    return r;
}

template <int K> __device__ __forceinline__ State<K> shuffle_up(const State<K> &s, int d)
{
    State<K> o;
    o.head = __shfl_up(s.head, d, 64);
    o.part_start = __shfl_up(s.part_start, d, 64);
    o.peer_start = __shfl_up(s.peer_start, d, 64);
    o.part_ord = __shfl_up(s.part_ord, d, 64);
    o.peer_ord = __shfl_up(s.peer_ord, d, 64);
#pragma unroll
    for (int k = 0; k < K; k++) {
        o.cnt[k] = __shfl_up(s.cnt[k], d, 64);
        o.w0[k] = __shfl_up(s.w0[k], d, 64);
        o.w1[k] = __shfl_up(s.w1[k], d, 64);
    }
    return o;
}

// Inclusive scan over the workgroup's kBlock elements (thread t holds element t), `carry` in front of them; afterwards carry = carry . all of
// them.  Every thread of the workgroup calls it (two barriers).
template <int K> __device__ __forceinline__ void block_scan(State<K> &s, State<K> &carry, State<K> *wave_totals, const ScanArgs<K> &args)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const State<K> o = shuffle_up(s, d);
        if (lane >= d) s = combine(o, s, args);
    }
    if (lane == 63) wave_totals[wave] = s;
    __syncthreads();
    State<K> before = carry, total = carry;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const State<K> t = wave_totals[w];
        if (w < wave) before = combine(before, t, args);
        total = combine(total, t, args);
    }
    s = combine(before, s, args);
    carry = total;
    __syncthreads();
}

__global__ void __launch_bounds__(kBlock) window_heads_kernel(const WindowKeys *kp, const int32_t *__restrict__ positions, int64_t n, unsigned char *__restrict__ heads)
{
    const WindowKeys &k = *kp;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        unsigned char h = 3;
        if (i > 0) {
            const long long a = positions ? positions[i - 1] : i - 1, b = positions ? positions[i] : i;
            const bool part_head = !tg_rows_not_distinct(k.part, a, k.part, b);
            const bool peer_head = part_head || !tg_rows_not_distinct(k.order, a, k.order, b);
            h = (unsigned char)((part_head ? 1 : 0) | (peer_head ? 2 : 0));
        }
        heads[i] = h;
    }
}

struct ScanBounds {   // written by launch 3 when part_start != nullptr; all [n]
    int32_t *part_start, *peer_start, *part_ord, *peer_ord, *part_heads, *peer_heads;
};

// launches 1 (FINAL = false) and 3 (FINAL = true): workgroup b owns rows [b * tile_rows, (b + 1) * tile_rows)
template <int K, bool FINAL>
__global__ void __launch_bounds__(kBlock) window_scan_tiles_kernel(ScanArgs<K> args, const unsigned char *__restrict__ heads, const int32_t *__restrict__ positions, int64_t n,
                                                                   int64_t tile_rows, State<K> *__restrict__ summaries, ScanBounds bounds, unsigned int *__restrict__ errors)
{
    __shared__ State<K> wave_totals[kWaves];
    const int64_t tile = blockIdx.x, first = tile * tile_rows;
    const int64_t end = first + tile_rows < n ? first + tile_rows : n;
    State<K> carry = identity<K>();
    if (FINAL && tile > 0) carry = summaries[tile - 1];
    for (int64_t sub = first; sub < end; sub += kBlock) {
        const int64_t i = sub + threadIdx.x;
        const bool live = i < end;
        State<K> s = identity<K>();
        unsigned char h = 0;
        if (live) {
            h = heads[i];
            s.head = h & 1;
            s.part_start = (h & 1) ? (int)i : 0;
            s.peer_start = (h & 2) ? (int)i : 0;
            s.part_ord = h & 1;
            s.peer_ord = (h >> 1) & 1;
            if (!FINAL) {
                const long long r = positions ? positions[i] : i;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const ScanAgg &a = args.a[k];
                    if (!a.cnt) continue;
                    const bool present = !a.arg.values || !(a.arg.nulls && a.arg.nulls[r]);
                    unsigned long long w = 0;
                    if (present && a.op != kOpCount) {
                        const unsigned long long raw = ((const unsigned long long *)a.arg.values)[r];
                        w = a.op == kOpSum ? raw : tg_minmax_encode(a.function, raw);
                    }
                    s.cnt[k] = present ? 1 : 0;
                    s.w0[k] = w;
                    a.cnt[i] = s.cnt[k];
                    if (a.val) a.val[i] = w;
                    if (a.raw) a.raw[i] = w;
                }
            }
            else {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const ScanAgg &a = args.a[k];
                    if (!a.cnt) continue;
                    s.cnt[k] = a.cnt[i];
                    s.w0[k] = a.val ? a.val[i] : 0ULL;
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) s.w1[k] = args.a[k].op == kOpSum ? (unsigned long long)((long long)s.w0[k] >> 63) : 0ULL;
        }
        block_scan(s, carry, wave_totals, args);
        if (FINAL && live) {
            if (bounds.part_start) {
                bounds.part_start[i] = s.part_start;
                bounds.peer_start[i] = s.peer_start;
                bounds.part_ord[i] = s.part_ord;
                bounds.peer_ord[i] = s.peer_ord;
                // ord counts the heads at or before i: 1 <= ord <= i + 1
                if ((h & 1) && s.part_ord >= 1 && s.part_ord <= n) bounds.part_heads[s.part_ord - 1] = (int)i;
                if ((h & 2) && s.peer_ord >= 1 && s.peer_ord <= n) bounds.peer_heads[s.peer_ord - 1] = (int)i;
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                const ScanAgg &a = args.a[k];
                if (!a.cnt) continue;
                a.cnt[i] = s.cnt[k];
                if (a.val) a.val[i] = s.w0[k];
                if (a.hi) a.hi[i] = s.w1[k];
                // the prefix of the partition's non-null values up to this row does not fit an int64 (addExact would have thrown)
                if (a.op == kOpSum && a.check_prefix && s.w1[k] != (unsigned long long)((long long)s.w0[k] >> 63)) atomicOr(&errors[0], 1u);
            }
        }
    }
    if (!FINAL && threadIdx.x == 0) summaries[tile] = carry;
}

// launch 2: one workgroup; summaries[t] becomes the scan of summaries[0 .. t]
template <int K> __global__ void __launch_bounds__(kBlock) window_scan_carries_kernel(ScanArgs<K> args, State<K> *__restrict__ summaries, int64_t tiles)
{
    __shared__ State<K> wave_totals[kWaves];
    State<K> carry = identity<K>();
    for (int64_t chunk = 0; chunk < tiles; chunk += kBlock) {
        const int64_t t = chunk + threadIdx.x;
        State<K> s = t < tiles ? summaries[t] : identity<K>();
        block_scan(s, carry, wave_totals, args);
        if (t < tiles) summaries[t] = s;
    }
}

__global__ void __launch_bounds__(kBlock) window_ends_kernel(ScanBounds b, int64_t n, int32_t *__restrict__ part_end, int32_t *__restrict__ peer_end)
{
    const int64_t parts = b.part_ord[n - 1], peers = b.peer_ord[n - 1];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t po = b.part_ord[i], eo = b.peer_ord[i];   // the next head's number; >= 1
        int64_t pe = (po >= 0 && po < parts ? (int64_t)b.part_heads[po] : n) - 1, ee = (eo >= 0 && eo < peers ? (int64_t)b.peer_heads[eo] : n) - 1;
        // an end lies in [i, n - 1] and a peer group inside its partition; held to that here, so that no later kernel indexes with anything else
        pe = pe < i ? i : (pe > n - 1 ? n - 1 : pe);
        ee = ee < i ? i : (ee > pe ? pe : ee);
        part_end[i] = (int)pe;
        peer_end[i] = (int)ee;
    }
}

// ---- frames with offsets ----------------------------------------------------------------------------------------------------------------------
enum { kErrNullStart = 1, kErrNullEnd = 2, kErrNegative = 4, kErrNullCompare = 8 };      // error word 2
enum { kErrNthOffset = 1, kErrBuckets = 2 };                        // error word 3

struct FrameArgs {
    int type, start_type, end_type;      // tgpu_frame_type, tgpu_frame_bound
    TgColView start_offset, end_offset;  // BIGINT or INTEGER, in arrival order; read for PRECEDING / FOLLOWING only
    const int32_t *positions;
    const int32_t *part_start, *peer_start, *peer_ord, *peer_heads, *part_end, *peer_end;
    int32_t *frame_start, *frame_end;    // [n] indices of the sorted order; frame_start = -1: the frame is empty
    unsigned int *errors;
};

__device__ __forceinline__ bool bound_has_offset(int t) { return t == TGPU_BOUND_PRECEDING || t == TGPU_BOUND_FOLLOWING; }

// the offset of row r; false: null
__device__ __forceinline__ bool read_offset(const TgColView &c, long long r, long long &v)
{
    if (c.nulls && c.nulls[r]) return false;
    v = c.type == TGPU_BIGINT ? ((const long long *)c.values)[r] : (long long)((const int *)c.values)[r];
    return true;
}

__global__ void __launch_bounds__(kBlock) window_frame_bounds_kernel(FrameArgs f, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        int64_t ps = f.part_start[i];
        ps = ps < 0 ? 0 : (ps > i ? i : ps);
        int64_t pe = f.part_end[i];
        pe = pe < i ? i : (pe > n - 1 ? n - 1 : pe);
        const long long row = f.positions ? f.positions[i] : i;
        long long a = 0, b = 0;
        unsigned int bad = 0;
        if (bound_has_offset(f.start_type)) {
            if (!read_offset(f.start_offset, row, a)) bad |= kErrNullStart;
            else if (a < 0) bad |= kErrNegative;
        }
        if (bound_has_offset(f.end_type)) {
            if (!read_offset(f.end_offset, row, b)) bad |= kErrNullEnd;
            else if (b < 0) bad |= kErrNegative;
        }
        int64_t s = -1, e = -1;
        bool empty = bad != 0;
        if (bad) {
            atomicOr(&f.errors[2], bad);
        }
        else if (f.type == TGPU_FRAME_TYPE_ROWS) {
            // WindowPartition.java:281-323 with emptyFrame :541-573; every comparison is between an offset and a distance: nothing is added to an offset
            const long long r = i - ps, left = pe - i;   // rows before / behind the current one
            const int st = f.start_type, et = f.end_type;
            if (st == TGPU_BOUND_UNBOUNDED_PRECEDING && et == TGPU_BOUND_PRECEDING) empty = b > r;
            else if (st == TGPU_BOUND_FOLLOWING && et == TGPU_BOUND_UNBOUNDED_FOLLOWING) empty = a > left;
            else if (st == TGPU_BOUND_PRECEDING && et == TGPU_BOUND_PRECEDING) empty = a < b || (a > r && b > r);
            else if (st == TGPU_BOUND_FOLLOWING && et == TGPU_BOUND_FOLLOWING) empty = a > b || a > left;
            s = st == TGPU_BOUND_UNBOUNDED_PRECEDING ? ps : (st == TGPU_BOUND_PRECEDING ? (a > r ? ps : i - a) : (st == TGPU_BOUND_FOLLOWING ? (a > left ? pe : i + a) : i));
            e = et == TGPU_BOUND_UNBOUNDED_FOLLOWING ? pe : (et == TGPU_BOUND_PRECEDING ? (b > r ? ps : i - b) : (et == TGPU_BOUND_FOLLOWING ? (b > left ? pe : i + b) : i));
        }
        else {
            // GROUPS (:609-694), and RANGE by peers (:327-344) = GROUPS without offsets.  Peer groups are numbered through the whole input:
            // group g starts at peer_heads[g] and ends in front of peer_heads[g + 1] or at the partition's end
            const int64_t g = (int64_t)f.peer_ord[i] - 1, first = (int64_t)f.peer_ord[ps] - 1, last = (int64_t)f.peer_ord[pe] - 1;
            const long long before = g - first, behind = last - g;   // groups of the partition before / behind the current one
            const bool sane = first >= 0 && first <= g && g <= last && last < n;
            auto group_start = [&](int64_t x) { return (int64_t)f.peer_heads[x]; };
            auto group_end = [&](int64_t x) { return x < last ? (int64_t)f.peer_heads[x + 1] - 1 : pe; };
            if (!sane) {
                empty = true;   // (never: the scan numbers the heads)
            }
            else {
                switch (f.start_type) {
                case TGPU_BOUND_UNBOUNDED_PRECEDING: s = ps; break;
                case TGPU_BOUND_PRECEDING: s = a > before ? ps : group_start(g - a); break;
                case TGPU_BOUND_FOLLOWING: s = a > behind ? pe + 1 : group_start(g + a); break;   // behind the partition
                default: s = f.peer_start[i]; break;
                }
                switch (f.end_type) {
                case TGPU_BOUND_UNBOUNDED_FOLLOWING: e = pe; break;
                case TGPU_BOUND_PRECEDING: e = b > before ? ps - 1 : group_end(g - b); break;
                case TGPU_BOUND_FOLLOWING: e = b > behind ? pe : group_end(g + b); break;
                default: e = f.peer_end[i]; break;
                }
                empty = s > e || s > pe || e < ps;   // emptyFrame(Range), :523-528
            }
        }
        // a frame lies inside its partition; held to that here, so that no later kernel indexes with anything else
        if (!empty && (s < ps || e > pe || s > e)) empty = true;
        f.frame_start[i] = empty ? -1 : (int)s;
        f.frame_end[i] = empty ? -1 : (int)e;
    }
}

// ---- RANGE frames with PRECEDING / FOLLOWING bounds ------------------------------------------------------------------------------------------------
// the order code of a non-null BIGINT / INTEGER / DATE / DOUBLE cell in the direction of the sort: never decreasing along the sorted order
__device__ __forceinline__ unsigned long long range_code(const TgColView &c, long long r, int descending)
{
    const unsigned long long v = cell_order_bits(c, r);
    return descending ? ~v : v;
}

// codes[i] / key_null[i] of one comparison key channel `compare` (in arrival order, like `sort_key`), see the head of this file
__global__ void __launch_bounds__(kBlock) window_range_keys_kernel(TgColView sort_key, TgColView compare, int descending, const int32_t *__restrict__ positions, int64_t n,
                                                                   unsigned long long *__restrict__ codes, unsigned char *__restrict__ key_null,
                                                                   unsigned int *__restrict__ errors)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const long long r = positions ? positions[i] : i;
        const bool null_key = sort_key.nulls && sort_key.nulls[r];
        const bool null_compare = compare.nulls && compare.nulls[r];
        if (!null_key && null_compare) atomicOr(&errors[2], (unsigned int)kErrNullCompare);
        codes[i] = null_key || null_compare ? 0ULL : range_code(compare, r, descending);
        key_null[i] = null_key ? 1 : 0;
    }
}

struct RangeFrameArgs {
    int start_type, end_type, descending, nulls_first;
    TgColView start_bound, end_bound;                   // the bound VALUES in arrival order; read for PRECEDING / FOLLOWING in rows with a non-null sort key
    const unsigned long long *start_codes, *end_codes;  // [n] the comparison keys of the two bounds in sorted order
    const unsigned char *key_null;                      // [n]
    const int32_t *positions;
    const int32_t *part_start, *peer_start, *part_end, *peer_end;
    int32_t *frame_start, *frame_end;                   // as FrameArgs
    unsigned int *errors;
};

__global__ void __launch_bounds__(kBlock) window_range_bounds_kernel(RangeFrameArgs f, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        // every index is held to [0, n - 1], the partition to [ps, pe] around i and the peer group inside it, before anything is read through them
        int64_t ps = f.part_start[i];
        ps = ps < 0 ? 0 : (ps > i ? i : ps);
        int64_t pe = f.part_end[i];
        pe = pe < i ? i : (pe > n - 1 ? n - 1 : pe);
        int64_t peer_s = f.peer_start[i], peer_e = f.peer_end[i];
        peer_s = peer_s < ps ? ps : (peer_s > i ? i : peer_s);
        peer_e = peer_e < i ? i : (peer_e > pe ? pe : peer_e);
        const int row_null = f.key_null[i];
        long long lo = ps, hi = pe;
        unsigned long long start_bound = 0, end_bound = 0;
        unsigned int bad = 0;
        if (!row_null) {
            int64_t first_peer_e = f.peer_end[ps], last_peer_s = f.peer_start[pe];
            first_peer_e = first_peer_e < ps ? ps : (first_peer_e > pe ? pe : first_peer_e);
            last_peer_s = last_peer_s < ps ? ps : (last_peer_s > pe ? pe : last_peer_s);
            tg_range_run(f.nulls_first, ps, pe, f.key_null[ps], first_peer_e, f.key_null[pe], last_peer_s, &lo, &hi);
            const long long row = f.positions ? f.positions[i] : i;
            if (bound_has_offset(f.start_type)) {
                if (f.start_bound.nulls && f.start_bound.nulls[row]) bad |= kErrNullStart;
                else start_bound = range_code(f.start_bound, row, f.descending);
            }
            if (bound_has_offset(f.end_type)) {
                if (f.end_bound.nulls && f.end_bound.nulls[row]) bad |= kErrNullEnd;
                else end_bound = range_code(f.end_bound, row, f.descending);
            }
        }
        long long s = -1, e = -1;
        if (bad) atomicOr(&f.errors[2], bad);
        else tg_range_frame(f.start_type, f.end_type, i, ps, pe, peer_s, peer_e, row_null, lo, hi, f.start_codes, start_bound, f.end_codes, end_bound, &s, &e);
        f.frame_start[i] = (int)s;
        f.frame_end[i] = (int)e;
    }
}

// the range-maximum index over one function's per-row order codes (see the head of this file); all arrays [n] but top [levels][chunks]
struct ExtremeIndex {
    const unsigned long long *raw, *pre, *suf, *mask, *top;
    long long chunks;
};

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__global__ void __launch_bounds__(kBlock) window_extreme_chunks_kernel(const unsigned long long *__restrict__ raw, int64_t n, int64_t chunks, unsigned long long *__restrict__ pre,
                                                                       unsigned long long *__restrict__ suf, unsigned long long *__restrict__ mask,
                                                                       unsigned long long *__restrict__ top0)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t chunk = (int64_t)blockIdx.x * kWaves + wave; chunk < chunks; chunk += (int64_t)gridDim.x * kWaves) {   // the same for every lane of a wave
        const int64_t i = chunk * 64 + lane;
        const bool live = i < n;
        const unsigned long long v = live ? raw[i] : 0ULL;   // 0 = below or equal to every code
        unsigned long long p = v, q = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(p, d, 64), down = __shfl_down(q, d, 64);
            if (lane >= d) p = umax64(p, up);
            if (lane + d < 64) q = umax64(q, down);
        }
        // the candidates of [.., lane]: walking left from the lane, the rows that beat everything between them and the lane
        unsigned long long m = 1ULL << lane, running = v;
        for (int d = 1; d < 64; d++) {
            const unsigned long long o = __shfl_up(v, d, 64);
            if (lane >= d) {
                if (o > running) m |= 1ULL << (lane - d);
                running = umax64(running, o);
            }
        }
        if (live) {
            pre[i] = p;
            suf[i] = q;
            mask[i] = m;
        }
        const unsigned long long all = __shfl(p, 63, 64);
        if (lane == 0) top0[chunk] = all;
    }
}

// level[c] = the maximum of chunks c .. c + 2 * half - 1 (cut at the last chunk) from the level below
__global__ void __launch_bounds__(kBlock) window_extreme_level_kernel(const unsigned long long *__restrict__ below, unsigned long long *__restrict__ level, int64_t chunks,
                                                                      int64_t half)
{
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * kBlock)
        level[c] = c + half < chunks ? umax64(below[c], below[c + half]) : below[c];
}

// the maximum of raw[s .. e], 0 <= s <= e < n
__device__ __forceinline__ unsigned long long range_extreme(const ExtremeIndex &x, int64_t s, int64_t e)
{
    const int64_t cs = s >> 6, ce = e >> 6;
    if (cs == ce) {
        const unsigned long long bits = x.mask[e] & (~0ULL << (s & 63));   // bit (e & 63) is always set
        return bits ? x.raw[(cs << 6) + (__ffsll((unsigned long long)bits) - 1)] : x.raw[e];
    }
    unsigned long long r = umax64(x.suf[s], x.pre[e]);
    const long long between = ce - cs - 1;
    if (between > 0) {
        const int k = 63 - __clzll(between);
        const unsigned long long *level = x.top + (long long)k * x.chunks;
        r = umax64(r, umax64(level[cs + 1], level[ce - (1LL << k)]));
    }
    return r;
}

struct EvalArgs {
    int function, agg_function, frame;
    int general;                         // the frame is frame_start / frame_end
    const int32_t *frame_start, *frame_end;
    const unsigned long long *hi;        // general sum: the running sum's high word
    ExtremeIndex extremes;               // general min / max whose frame may start behind the partition's first row (raw == nullptr: it cannot)
    int has_offset, has_default;
    TgColView offset;                    // lag / lead: the BIGINT offset channel in arrival order
    const int32_t *positions;            // nullptr: the identity
    const int32_t *part_start, *peer_start, *peer_ord, *part_end, *peer_end;
    const long long *cnt;                // AGGREGATE: the running arrays
    const unsigned long long *val;
    long long *out;                      // 8-byte results (BIGINT, or DOUBLE bits)
    unsigned char *out_nulls;
    int32_t *out_row;                    // value functions: the source row per output row; -1 = null; source_rows + r = row r of the default column
    long long source_rows;
    unsigned int *errors;                // [0] sum overflow, [1] negative lag / lead offset, [2] kErrNullStart .., [3] kErrNthOffset ..
};

__global__ void __launch_bounds__(kBlock) window_evaluate_kernel(EvalArgs e, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        int64_t ps = e.part_start[i];
        ps = ps < 0 ? 0 : (ps > i ? i : ps);   // (never: the scan's maximum over head indices <= i)
        const int64_t pe = e.part_end[i];
        switch (e.function) {
        case TGPU_WINDOW_ROW_NUMBER: e.out[i] = i - ps + 1; break;
        case TGPU_WINDOW_RANK: e.out[i] = e.peer_start[i] - ps + 1; break;
        case TGPU_WINDOW_DENSE_RANK: e.out[i] = (int64_t)e.peer_ord[i] - e.peer_ord[ps] + 1; break;
        case TGPU_WINDOW_PERCENT_RANK: {   // PercentRankFunction.java: one IEEE division
            const int64_t total = pe - ps + 1, rank = e.peer_start[i] - ps + 1;
            const double v = total == 1 ? 0.0 : ((double)(rank - 1)) / (double)(total - 1);
            e.out[i] = __double_as_longlong(v);
            break;
        }
        case TGPU_WINDOW_CUME_DIST: {      // CumulativeDistributionFunction.java
            const int64_t total = pe - ps + 1, count = e.peer_end[i] - ps + 1;
            e.out[i] = __double_as_longlong(((double)count) / (double)total);
            break;
        }
        case TGPU_WINDOW_AGGREGATE: {
            if (e.general) {
                const bool counts = e.agg_function == TGPU_AGG_COUNT_ALL || e.agg_function == TGPU_AGG_COUNT_COLUMN;
                const int64_t s = e.frame_start[i], at = e.frame_end[i];
                if (s < 0) {   // empty: 0 / null
                    e.out[i] = 0;
                    if (!counts) e.out_nulls[i] = 1;
                    break;
                }
                // the running arrays restart at the partition's first row: nothing to take off there
                const long long c = e.cnt[at] - (s > ps ? e.cnt[s - 1] : 0);
                if (counts) {
                    e.out[i] = c;
                    break;
                }
                unsigned long long w;
                if (e.agg_function == TGPU_AGG_SUM_BIGINT) {
                    const unsigned long long lo1 = e.val[at], hi1 = e.hi[at], lo0 = s > ps ? e.val[s - 1] : 0ULL, hi0 = s > ps ? e.hi[s - 1] : 0ULL;
                    w = lo1 - lo0;
                    const unsigned long long high = hi1 - hi0 - (lo1 < lo0 ? 1ULL : 0ULL);
                    if (high != (unsigned long long)((long long)w >> 63)) atomicOr(&e.errors[0], 1u);   // this frame's sum does not fit an int64
                }
                else {
                    w = s <= ps || !e.extremes.raw ? e.val[at] : range_extreme(e.extremes, s, at);
                }
                e.out_nulls[i] = c == 0;
                e.out[i] = c == 0 ? 0 : (e.agg_function == TGPU_AGG_SUM_BIGINT ? (long long)w : (long long)tg_minmax_decode(e.agg_function, w));
                break;
            }
            const int64_t at = e.frame == TGPU_FRAME_PARTITION ? pe : (e.frame == TGPU_FRAME_RANGE_TO_CURRENT ? (int64_t)e.peer_end[i] : i);
            const long long c = e.cnt[at];
            if (e.agg_function == TGPU_AGG_COUNT_ALL || e.agg_function == TGPU_AGG_COUNT_COLUMN) {
                e.out[i] = c;
                break;
            }
            const unsigned long long w = e.val[at];
            e.out_nulls[i] = c == 0;
            e.out[i] = c == 0 ? 0 : (e.agg_function == TGPU_AGG_SUM_BIGINT ? (long long)w : (long long)tg_minmax_decode(e.agg_function, w));
            break;
        }
        case TGPU_WINDOW_FIRST_VALUE:
            if (e.general) {
                const int64_t s = e.frame_start[i];
                e.out_row[i] = s < 0 ? -1 : (e.positions ? e.positions[s] : (int)s);
                break;
            }
            e.out_row[i] = e.positions ? e.positions[ps] : (int)ps;   // all three frames start at the partition's first row
            break;
        case TGPU_WINDOW_NTH_VALUE: {   // NthValueFunction.java:41-77; always under frame_start / frame_end
            const int64_t s = e.frame_start[i], at = e.frame_end[i], r = e.positions ? e.positions[i] : i;
            int64_t row = -1;
            if (s >= 0 && !(e.offset.nulls && e.offset.nulls[r])) {
                const long long offset = ((const long long *)e.offset.values)[r];
                if (offset < 1) atomicOr(&e.errors[3], (unsigned int)kErrNthOffset);
                else if (offset - 1 <= at - s) row = e.positions ? e.positions[s + (offset - 1)] : s + (offset - 1);
            }
            e.out_row[i] = (int)row;
            break;
        }
        case TGPU_WINDOW_NTILE: {       // NTileFunction.java:45-74; ignores the frame
            const int64_t r = e.positions ? e.positions[i] : i;
            const bool null_buckets = e.offset.nulls && e.offset.nulls[r];
            const long long buckets = null_buckets ? 1 : ((const long long *)e.offset.values)[r];
            long long bucket = 0;
            if (buckets <= 0) {
                atomicOr(&e.errors[3], (unsigned int)kErrBuckets);
            }
            else {
                const long long current = i - ps, rows = pe - ps + 1;
                if (rows < buckets) {
                    bucket = current;
                }
                else {
                    const long long remainder = rows % buckets, per = rows / buckets;   // the remainder rows go to the first buckets, one each
                    bucket = current < (per + 1) * remainder ? current / (per + 1) : (current - remainder) / per;
                }
            }
            e.out_nulls[i] = null_buckets;
            e.out[i] = null_buckets ? 0 : bucket + 1;
            break;
        }
        case TGPU_WINDOW_LAST_VALUE: {
            if (e.general) {
                const int64_t at = e.frame_end[i];   // -1 with frame_start
                e.out_row[i] = at < 0 ? -1 : (e.positions ? e.positions[at] : (int)at);
                break;
            }
            const int64_t at = e.frame == TGPU_FRAME_PARTITION ? pe : (e.frame == TGPU_FRAME_RANGE_TO_CURRENT ? (int64_t)e.peer_end[i] : i);
            e.out_row[i] = e.positions ? e.positions[at] : (int)at;
            break;
        }
        case TGPU_WINDOW_LAG:
        case TGPU_WINDOW_LEAD: {
            const int64_t r = e.positions ? e.positions[i] : i;
            int64_t row = -1;
            long long offset = 1;
            bool null_offset = false;
            if (e.has_offset) {
                null_offset = e.offset.nulls && e.offset.nulls[r];
                offset = null_offset ? 0 : ((const long long *)e.offset.values)[r];
            }
            if (null_offset) {
                row = -1;
            }
            else if (offset < 0) {
                atomicOr(&e.errors[1], 1u);
            }
            else {
                // partition-relative, as the reference's long arithmetic has it: lag 0 <= current - offset, lead current + offset < size
                // (a sum that wraps is negative there: outside)
                const unsigned long long current = (unsigned long long)(i - ps), size = (unsigned long long)(pe - ps + 1), o = (unsigned long long)offset;
                int64_t at = -1;
                if (e.function == TGPU_WINDOW_LAG) {
                    if (o <= current) at = i - (int64_t)o;
                }
                else if (o < size - current) {
                    at = i + (int64_t)o;
                }
                if (at >= 0) row = e.positions ? e.positions[at] : at;
                else row = e.has_default ? e.source_rows + r : -1;
            }
            e.out_row[i] = (int)row;
            break;
        }
        default: break;
        }
    }
}

template <int K>
void run_scan(Context *ctx, const ScanAgg *aggs, int count, const unsigned char *heads, const int32_t *positions, int64_t n, int64_t tile_rows, const ScanBounds &bounds,
              unsigned int *errors)
{
    ScanArgs<K> args{};
    for (int k = 0; k < count; k++) args.a[k] = aggs[k];
    const int64_t tiles = ceil_div(n, tile_rows);
    TG_CHECK_ARG(tiles <= 0x7fffffffLL, "too many scan tiles");
    BufferPtr summaries = ctx->alloc((size_t)tiles * sizeof(State<K>));
    window_scan_tiles_kernel<K, false><<<(unsigned)tiles, kBlock, 0, ctx->stream()>>>(args, heads, positions, n, tile_rows, summaries->as<State<K>>(), bounds, errors);
    check_launch("window_scan_tiles");
    window_scan_carries_kernel<K><<<1, kBlock, 0, ctx->stream()>>>(args, summaries->as<State<K>>(), tiles);
    check_launch("window_scan_carries");
    window_scan_tiles_kernel<K, true><<<(unsigned)tiles, kBlock, 0, ctx->stream()>>>(args, heads, positions, n, tile_rows, summaries->as<State<K>>(), bounds, errors);
    check_launch("window_scan_final");
}

bool is_value_function(int32_t f)
{
    return f == TGPU_WINDOW_LAG || f == TGPU_WINDOW_LEAD || f == TGPU_WINDOW_FIRST_VALUE || f == TGPU_WINDOW_LAST_VALUE || f == TGPU_WINDOW_NTH_VALUE;
}
// the functions that read their frame
bool reads_frame(int32_t f) { return f == TGPU_WINDOW_AGGREGATE || f == TGPU_WINDOW_FIRST_VALUE || f == TGPU_WINDOW_LAST_VALUE || f == TGPU_WINDOW_NTH_VALUE; }
bool has_offset(int32_t bound) { return bound == TGPU_BOUND_PRECEDING || bound == TGPU_BOUND_FOLLOWING; }
// a RANGE frame whose bounds are values to search for
bool range_offsets(const WindowFunctionSpec &f)
{
    return f.general && f.ranged && f.frame_type == TGPU_FRAME_TYPE_RANGE && (has_offset(f.start_type) || has_offset(f.end_type));
}

// the tgpu_window_frame code of a general frame that is one of the three old frames, or -1
int old_frame_code(const WindowFunctionSpec &f)
{
    if (f.start_type != TGPU_BOUND_UNBOUNDED_PRECEDING) return -1;
    if (f.end_type == TGPU_BOUND_UNBOUNDED_FOLLOWING && f.frame_type != TGPU_FRAME_TYPE_GROUPS) return TGPU_FRAME_PARTITION;
    if (f.end_type != TGPU_BOUND_CURRENT_ROW) return -1;
    return f.frame_type == TGPU_FRAME_TYPE_RANGE ? TGPU_FRAME_RANGE_TO_CURRENT : (f.frame_type == TGPU_FRAME_TYPE_ROWS ? TGPU_FRAME_ROWS_TO_CURRENT : -1);
}

}  // namespace

void WindowGpu::validate(const std::vector<int32_t> &types, const std::vector<WindowFunctionSpec> &functions, const std::vector<int32_t> &partition_channels,
                         const std::vector<int32_t> &sort_channels, const std::vector<int32_t> &sort_orders)
{
    const int nt = (int)types.size();
    TG_CHECK_ARG(!types.empty(), "window needs at least one source channel");
    for (int32_t t : types) TG_CHECK_ARG(valid_type(t), "unknown type");
    TG_CHECK_ARG(sort_channels.size() == sort_orders.size(), "sort channels and sort orders differ in length");
    TG_CHECK_ARG((int)(partition_channels.size() + sort_channels.size()) <= kMaxKeyChannels, "at most 8 partition and sort channels together are supported");
    for (int32_t ch : partition_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "partition channel out of range");
    for (int32_t ch : sort_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "sort channel out of range");
    for (int32_t o : sort_orders) TG_CHECK_ARG(o >= TGPU_SORT_ASC_NULLS_FIRST && o <= TGPU_SORT_DESC_NULLS_LAST, "unknown sort order");
    TG_CHECK_ARG(!functions.empty(), "window needs at least one function");
    TG_CHECK_ARG((int)functions.size() <= TGPU_WINDOW_MAX_FUNCTIONS, "at most 16 window functions are supported");
    for (const WindowFunctionSpec &f : functions) {
        // nth_value and ntile come with the framed entry point only
        TG_CHECK_ARG(f.function >= TGPU_WINDOW_ROW_NUMBER && f.function <= (f.general ? TGPU_WINDOW_NTILE : TGPU_WINDOW_AGGREGATE), "unknown window function");
        if (!f.general) {
            TG_CHECK_ARG(f.frame >= TGPU_FRAME_PARTITION && f.frame <= TGPU_FRAME_ROWS_TO_CURRENT, "unknown window frame");
        }
        else {
            TG_CHECK_ARG(f.frame_type >= TGPU_FRAME_TYPE_RANGE && f.frame_type <= TGPU_FRAME_TYPE_GROUPS, "unknown window frame type");
            TG_CHECK_ARG(f.start_type >= TGPU_BOUND_UNBOUNDED_PRECEDING && f.start_type <= TGPU_BOUND_UNBOUNDED_FOLLOWING, "unknown window frame bound");
            TG_CHECK_ARG(f.end_type >= TGPU_BOUND_UNBOUNDED_PRECEDING && f.end_type <= TGPU_BOUND_UNBOUNDED_FOLLOWING, "unknown window frame bound");
            // the analyzer's rules (sql/analyzer/ExpressionAnalyzer: frame start / end)
            const bool combination = f.start_type != TGPU_BOUND_UNBOUNDED_FOLLOWING && f.end_type != TGPU_BOUND_UNBOUNDED_PRECEDING &&
                                     !(f.start_type == TGPU_BOUND_CURRENT_ROW && f.end_type == TGPU_BOUND_PRECEDING) &&
                                     !(f.start_type == TGPU_BOUND_FOLLOWING && f.end_type != TGPU_BOUND_FOLLOWING && f.end_type != TGPU_BOUND_UNBOUNDED_FOLLOWING);
            TG_CHECK_ARG(combination, "invalid window frame bounds");
            const bool by_value = f.ranged && f.frame_type == TGPU_FRAME_TYPE_RANGE && (has_offset(f.start_type) || has_offset(f.end_type));
            if (by_value) TG_CHECK_ARG(sort_channels.size() == 1, "a RANGE frame with an offset needs exactly one sort channel");
            for (int side = 0; side < 2; side++) {
                if (!has_offset(side == 0 ? f.start_type : f.end_type)) continue;
                const int32_t ch = side == 0 ? f.start_channel : f.end_channel;
                if (by_value) {   // the bound's value and the comparison key (FrameInfo.sortKeyChannelForStart/EndComparison)
                    const int32_t key = side == 0 ? f.start_sort_key_channel : f.end_sort_key_channel;
                    TG_CHECK_ARG(ch >= 0 && ch < nt, "frame bound channel out of range");
                    TG_CHECK_ARG(key >= 0 && key < nt, "frame comparison key channel out of range");
                    const int32_t t = types[(size_t)ch];
                    // the reference's offset over a timestamp sort key is an INTERVAL, a type the library does not have
                    if (t == TGPU_TIMESTAMP || types[(size_t)key] == TGPU_TIMESTAMP || types[(size_t)sort_channels[0]] == TGPU_TIMESTAMP)
                        fail(TGPU_ERR_NOT_SUPPORTED, "RANGE frames with an offset over a TIMESTAMP sort key are not supported");
                    TG_CHECK_ARG(t == types[(size_t)key], "a frame bound and its comparison key differ in type");
                    TG_CHECK_ARG(t == TGPU_BIGINT || t == TGPU_INTEGER || t == TGPU_DATE || t == TGPU_DOUBLE, "a RANGE frame bound must be BIGINT, INTEGER, DATE or DOUBLE");
                    continue;
                }
                TG_CHECK_ARG(ch >= 0 && ch < nt, "frame offset channel out of range");
                TG_CHECK_ARG(types[(size_t)ch] == TGPU_BIGINT || types[(size_t)ch] == TGPU_INTEGER, "a frame offset must be BIGINT or INTEGER");
            }
            // the reference compares the sort key with computed bound channels there: a value search, not a count of rows
            if (!f.ranged && f.frame_type == TGPU_FRAME_TYPE_RANGE && (has_offset(f.start_type) || has_offset(f.end_type)))
                fail(TGPU_ERR_NOT_SUPPORTED, "RANGE frames with an offset are not supported");
        }
        if (f.ignore_nulls != 0) fail(TGPU_ERR_NOT_SUPPORTED, "IGNORE NULLS is not supported");
        const int na = (int)f.argument_channels.size();
        for (int32_t ch : f.argument_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "argument channel out of range");
        auto type_of = [&](int a) { return types[(size_t)f.argument_channels[(size_t)a]]; };
        switch (f.function) {
        case TGPU_WINDOW_LAG:
        case TGPU_WINDOW_LEAD:
            TG_CHECK_ARG(na >= 1 && na <= 3, "lag / lead take 1 to 3 arguments");
            TG_CHECK_ARG(na < 2 || type_of(1) == TGPU_BIGINT, "the offset of lag / lead must be BIGINT");
            TG_CHECK_ARG(na < 3 || type_of(2) == type_of(0), "the default of lag / lead must have the value's type");
            break;
        case TGPU_WINDOW_FIRST_VALUE:
        case TGPU_WINDOW_LAST_VALUE: TG_CHECK_ARG(na == 1, "first_value / last_value take one argument"); break;
        case TGPU_WINDOW_NTH_VALUE: TG_CHECK_ARG(na == 2 && type_of(1) == TGPU_BIGINT, "nth_value takes a value and a BIGINT offset"); break;
        case TGPU_WINDOW_NTILE: TG_CHECK_ARG(na == 1 && type_of(0) == TGPU_BIGINT, "ntile takes one BIGINT argument"); break;
        case TGPU_WINDOW_AGGREGATE:
            // (ids above TGPU_AGG_MAX_DOUBLE, the TIMESTAMP extremes among them, stay unknown here: the switch below says so)
            if (f.agg_function >= TGPU_AGG_SUM_BIGINT && f.agg_function <= TGPU_AGG_MAX_DOUBLE && na == 1 && type_of(0) == TGPU_TIMESTAMP)
                fail(TGPU_ERR_NOT_SUPPORTED, "window aggregates over TIMESTAMP are not supported");
            switch (f.agg_function) {
            case TGPU_AGG_COUNT_ALL: TG_CHECK_ARG(na == 0, "count(*) takes no argument"); break;
            case TGPU_AGG_COUNT_COLUMN: TG_CHECK_ARG(na == 1, "count(x) takes one argument"); break;
            case TGPU_AGG_SUM_BIGINT:
            case TGPU_AGG_MIN_BIGINT:
            case TGPU_AGG_MAX_BIGINT: TG_CHECK_ARG(na == 1 && type_of(0) == TGPU_BIGINT, "the aggregate takes one BIGINT argument"); break;
            case TGPU_AGG_MIN_DOUBLE:
            case TGPU_AGG_MAX_DOUBLE: TG_CHECK_ARG(na == 1 && type_of(0) == TGPU_DOUBLE, "the aggregate takes one DOUBLE argument"); break;
            case TGPU_AGG_SUM_DOUBLE:
            case TGPU_AGG_AVG_BIGINT:
            case TGPU_AGG_AVG_DOUBLE:
                // the reference accumulates these in a double, left to right: a parallel scan cannot give its bits
                fail(TGPU_ERR_NOT_SUPPORTED, "sum(double) and avg are not supported as window aggregates");
            default: TG_CHECK_ARG(false, "unknown aggregate function");
            }
            break;
        default: TG_CHECK_ARG(na == 0, "the ranking functions take no argument"); break;
        }
    }
}

WindowGpu::WindowGpu(Context *ctx, std::vector<int32_t> types, std::vector<WindowFunctionSpec> functions, std::vector<int32_t> partition_channels,
                     std::vector<int32_t> sort_channels, std::vector<int32_t> sort_orders)
    : ctx_(ctx), types_(std::move(types)), functions_(std::move(functions)), partition_channels_(std::move(partition_channels)),
      sort_channels_(std::move(sort_channels)), sort_orders_(std::move(sort_orders))
{
    validate(types_, functions_, partition_channels_, sort_channels_, sort_orders_);
    for (WindowFunctionSpec &f : functions_) {
        if (!f.general) continue;
        const int code = old_frame_code(f);
        if (!reads_frame(f.function)) {   // the frame is ignored
            f.general = 0;
            f.frame = TGPU_FRAME_PARTITION;
        }
        else if (code >= 0 && f.function != TGPU_WINDOW_NTH_VALUE) {
            f.general = 0;
            f.frame = code;
        }
    }
}

std::vector<DeviceColumn> WindowGpu::evaluate(const DevicePage &all, BufferPtr *positions_out)
{
    const int64_t n = all.n;
    TG_CHECK_ARG(n > 0 && n <= 0x7fffffffLL, "1 to 2^31 - 1 rows: row numbers are int32");
    TG_CHECK_ARG(all.cols.size() == types_.size(), "page channel count does not match the operator's types");
    TG_CHECK_STATE(tile_rows_ > 0 && tile_rows_ % kBlock == 0, "the scan's tile must be a multiple of 256 rows");
    scratch_bytes_ = 0;
    auto scratch = [&](size_t bytes) {
        scratch_bytes_ += (int64_t)bytes;
        return ctx_->alloc(bytes);
    };
    // 1. the order
    BufferPtr positions;
    if (!partition_channels_.empty() || !sort_channels_.empty()) {
        // (no scope of its own: the profile shows the sort under TopNGpu's scopes, and the outermost of two nested scopes ends with the inner one)
        std::vector<int32_t> channels = partition_channels_, orders(partition_channels_.size(), TGPU_SORT_ASC_NULLS_LAST);   // WindowOperator.java:254
        channels.insert(channels.end(), sort_channels_.begin(), sort_channels_.end());
        orders.insert(orders.end(), sort_orders_.begin(), sort_orders_.end());
        int64_t count = 0;
        positions = TopNGpu::sorted_positions(ctx_, all, channels, orders, n, count);
        TG_CHECK_STATE(count == n, "the sort lost rows");
        scratch_bytes_ += n * 4;
    }
    const int32_t *pos = positions ? positions->as<int32_t>() : nullptr;
    *positions_out = positions;
    const int g = grid_for(ctx_, n);
    // 2. partition and peer heads
    BufferPtr heads = scratch((size_t)n);
    {
        ProfileScope ps(ctx_, "window_heads");
        WindowKeys host{};
        host.part.n = (int32_t)partition_channels_.size();
        for (size_t i = 0; i < partition_channels_.size(); i++) host.part.c[i] = view_of(all.cols[(size_t)partition_channels_[i]]);
        host.order.n = (int32_t)sort_channels_.size();
        for (size_t i = 0; i < sort_channels_.size(); i++) host.order.c[i] = view_of(all.cols[(size_t)sort_channels_[i]]);
        BufferPtr keys = ctx_->alloc(sizeof(WindowKeys));
        ctx_->upload(keys->ptr(), &host, sizeof(WindowKeys));
        window_heads_kernel<<<g, kBlock, 0, ctx_->stream()>>>(keys->as<WindowKeys>(), pos, n, heads->as<unsigned char>());
        check_launch("window_heads");
    }
    // 3. the scan
    BufferPtr errors = ctx_->alloc_zero(16);
    BufferPtr index_arrays = scratch((size_t)n * 4 * 8);
    int32_t *ia = index_arrays->as<int32_t>();
    const ScanBounds bounds{ia, ia + n, ia + 2 * n, ia + 3 * n, ia + 4 * n, ia + 5 * n};
    int32_t *part_end = ia + 6 * n, *peer_end = ia + 7 * n;
    std::vector<ScanAgg> aggs;
    std::vector<BufferPtr> cnt_bufs(functions_.size()), val_bufs(functions_.size()), hi_bufs(functions_.size()), raw_bufs(functions_.size());
    for (size_t f = 0; f < functions_.size(); f++) {
        const WindowFunctionSpec &spec = functions_[f];
        if (spec.function != TGPU_WINDOW_AGGREGATE) continue;
        ScanAgg a{};
        a.function = spec.agg_function;
        const bool count = spec.agg_function == TGPU_AGG_COUNT_ALL || spec.agg_function == TGPU_AGG_COUNT_COLUMN;
        a.op = count ? kOpCount : (spec.agg_function == TGPU_AGG_SUM_BIGINT ? kOpSum : kOpMax);
        if (!spec.argument_channels.empty()) a.arg = view_of(all.cols[(size_t)spec.argument_channels[0]]);
        cnt_bufs[f] = scratch((size_t)n * 8);
        a.cnt = cnt_bufs[f]->as<long long>();
        if (!count) {
            val_bufs[f] = scratch((size_t)n * 8);
            a.val = val_bufs[f]->as<unsigned long long>();
        }
        a.check_prefix = !spec.general;
        if (spec.general && a.op == kOpSum) {
            hi_bufs[f] = scratch((size_t)n * 8);
            a.hi = hi_bufs[f]->as<unsigned long long>();
        }
        if (spec.general && a.op == kOpMax && spec.start_type != TGPU_BOUND_UNBOUNDED_PRECEDING) {
            raw_bufs[f] = scratch((size_t)n * 8);
            a.raw = raw_bufs[f]->as<unsigned long long>();
        }
        aggs.push_back(a);
    }
    {
        ProfileScope ps(ctx_, "window_scan");
        size_t done = 0;
        do {   // at least once: the index arrays
            const int count = (int)std::min<size_t>(aggs.size() - done, (size_t)kMaxAggs);
            const ScanBounds b = done == 0 ? bounds : ScanBounds{};
            const ScanAgg *a = aggs.data() + done;
            unsigned int *err = errors->as<unsigned int>();
            if (count == 0) run_scan<0>(ctx_, a, count, heads->as<unsigned char>(), pos, n, tile_rows_, b, err);
            else if (count == 1) run_scan<1>(ctx_, a, count, heads->as<unsigned char>(), pos, n, tile_rows_, b, err);
            else if (count == 2) run_scan<2>(ctx_, a, count, heads->as<unsigned char>(), pos, n, tile_rows_, b, err);
            else run_scan<kMaxAggs>(ctx_, a, count, heads->as<unsigned char>(), pos, n, tile_rows_, b, err);
            done += (size_t)count;
        } while (done < aggs.size());
        ctx_->profile_note("window_scan_rows", n);
    }
    // 4a. + 4b. frames with offsets: the bounds per distinct frame, the range-extreme index per min / max that needs one
    bool any_general = false;
    for (const WindowFunctionSpec &spec : functions_) any_general = any_general || spec.general;
    std::vector<BufferPtr> frame_bufs(functions_.size());   // [2][n]: frame_start, frame_end; shared by the functions of one frame
    std::vector<BufferPtr> index_bufs(functions_.size());   // [3][n] pre, suf, mask, then [levels][chunks]
    const int64_t chunks = ceil_div(n, 64);
    BufferPtr range_null;                                          // [n] the sort key of the row at a sorted position is null
    std::vector<std::pair<int32_t, BufferPtr>> range_codes;        // comparison key channel -> [n] its codes in sorted order
    if (any_general) {
        {
            ProfileScope ps(ctx_, "window_frames");
            window_ends_kernel<<<g, kBlock, 0, ctx_->stream()>>>(bounds, n, part_end, peer_end);
            check_launch("window_ends");
            for (size_t f = 0; f < functions_.size(); f++) {
                const WindowFunctionSpec &spec = functions_[f];
                if (!spec.general) continue;
                for (size_t o = 0; o < f && !frame_bufs[f]; o++) {
                    const WindowFunctionSpec &other = functions_[o];
                    const bool same = other.general && other.frame_type == spec.frame_type && other.start_type == spec.start_type && other.end_type == spec.end_type &&
                                      (!has_offset(spec.start_type) || other.start_channel == spec.start_channel) &&
                                      (!has_offset(spec.end_type) || other.end_channel == spec.end_channel) &&
                                      (!range_offsets(spec) || (range_offsets(other) && (!has_offset(spec.start_type) || other.start_sort_key_channel == spec.start_sort_key_channel) &&
                                                                (!has_offset(spec.end_type) || other.end_sort_key_channel == spec.end_sort_key_channel)));
                    if (same) frame_bufs[f] = frame_bufs[o];
                }
                if (frame_bufs[f]) continue;
                frame_bufs[f] = scratch((size_t)n * 2 * 4);
                if (range_offsets(spec)) {
                    const bool descending = sort_orders_[0] == TGPU_SORT_DESC_NULLS_FIRST || sort_orders_[0] == TGPU_SORT_DESC_NULLS_LAST;
                    const DeviceColumn &sort_key = all.cols[(size_t)sort_channels_[0]];
                    if (!range_null) range_null = scratch((size_t)n);
                    // the comparison key of a bound in sorted order: gathered once per distinct channel
                    auto codes_of = [&](int32_t channel) {
                        for (const auto &made : range_codes)
                            if (made.first == channel) return made.second->as<unsigned long long>();
                        BufferPtr codes = scratch((size_t)n * 8);
                        window_range_keys_kernel<<<g, kBlock, 0, ctx_->stream()>>>(view_of(sort_key), view_of(all.cols[(size_t)channel]), descending ? 1 : 0, pos, n,
                                                                                   codes->as<unsigned long long>(), range_null->as<unsigned char>(), errors->as<unsigned int>());
                        check_launch("window_range_keys");
                        range_codes.emplace_back(channel, codes);
                        return codes->as<unsigned long long>();
                    };
                    RangeFrameArgs ra{};
                    ra.start_type = spec.start_type;
                    ra.end_type = spec.end_type;
                    ra.descending = descending ? 1 : 0;
                    ra.nulls_first = sort_orders_[0] == TGPU_SORT_ASC_NULLS_FIRST || sort_orders_[0] == TGPU_SORT_DESC_NULLS_FIRST;
                    if (has_offset(spec.start_type)) {
                        ra.start_bound = view_of(all.cols[(size_t)spec.start_channel]);
                        ra.start_codes = codes_of(spec.start_sort_key_channel);
                    }
                    if (has_offset(spec.end_type)) {
                        ra.end_bound = view_of(all.cols[(size_t)spec.end_channel]);
                        ra.end_codes = codes_of(spec.end_sort_key_channel);
                    }
                    ra.key_null = range_null->as<unsigned char>();
                    ra.positions = pos;
                    ra.part_start = bounds.part_start;
                    ra.peer_start = bounds.peer_start;
                    ra.part_end = part_end;
                    ra.peer_end = peer_end;
                    ra.frame_start = frame_bufs[f]->as<int32_t>();
                    ra.frame_end = ra.frame_start + n;
                    ra.errors = errors->as<unsigned int>();
                    window_range_bounds_kernel<<<g, kBlock, 0, ctx_->stream()>>>(ra, n);
                    check_launch("window_range_bounds");
                    continue;
                }
                FrameArgs fa{};
                fa.type = spec.frame_type;
                fa.start_type = spec.start_type;
                fa.end_type = spec.end_type;
                if (has_offset(spec.start_type)) fa.start_offset = view_of(all.cols[(size_t)spec.start_channel]);
                if (has_offset(spec.end_type)) fa.end_offset = view_of(all.cols[(size_t)spec.end_channel]);
                fa.positions = pos;
                fa.part_start = bounds.part_start;
                fa.peer_start = bounds.peer_start;
                fa.peer_ord = bounds.peer_ord;
                fa.peer_heads = bounds.peer_heads;
                fa.part_end = part_end;
                fa.peer_end = peer_end;
                fa.frame_start = frame_bufs[f]->as<int32_t>();
                fa.frame_end = fa.frame_start + n;
                fa.errors = errors->as<unsigned int>();
                window_frame_bounds_kernel<<<g, kBlock, 0, ctx_->stream()>>>(fa, n);
                check_launch("window_frame_bounds");
            }
        }
        ProfileScope ps(ctx_, "window_extremes");
        int levels = 1;
        while ((1LL << levels) <= chunks) levels++;   // level k spans 2^k chunks
        for (size_t f = 0; f < functions_.size(); f++) {
            if (!raw_bufs[f]) continue;
            index_bufs[f] = scratch(((size_t)n * 3 + (size_t)levels * (size_t)chunks) * 8);
            unsigned long long *x = index_bufs[f]->as<unsigned long long>(), *top = x + 3 * n;
            window_extreme_chunks_kernel<<<grid_for(ctx_, chunks, kWaves), kBlock, 0, ctx_->stream()>>>(raw_bufs[f]->as<unsigned long long>(), n, chunks, x, x + n, x + 2 * n, top);
            check_launch("window_extreme_chunks");
            for (int k = 1; k < levels; k++) {
                window_extreme_level_kernel<<<grid_for(ctx_, chunks), kBlock, 0, ctx_->stream()>>>(top + (size_t)(k - 1) * chunks, top + (size_t)k * chunks, chunks, 1LL << (k - 1));
                check_launch("window_extreme_level");
            }
        }
    }
    // 4. + 5. ends, then one launch per function
    std::vector<DeviceColumn> result(functions_.size());
    std::vector<BufferPtr> rows(functions_.size());
    {
        ProfileScope ps(ctx_, "window_evaluate");
        if (!any_general) {
            window_ends_kernel<<<g, kBlock, 0, ctx_->stream()>>>(bounds, n, part_end, peer_end);
            check_launch("window_ends");
        }
        for (size_t f = 0; f < functions_.size(); f++) {
            const WindowFunctionSpec &spec = functions_[f];
            EvalArgs e{};
            e.function = spec.function;
            e.agg_function = spec.agg_function;
            e.frame = spec.frame;
            e.positions = pos;
            e.part_start = bounds.part_start;
            e.peer_start = bounds.peer_start;
            e.peer_ord = bounds.peer_ord;
            e.part_end = part_end;
            e.peer_end = peer_end;
            e.source_rows = n;
            e.errors = errors->as<unsigned int>();
            e.general = spec.general;
            if (spec.general) {
                e.frame_start = frame_bufs[f]->as<int32_t>();
                e.frame_end = e.frame_start + n;
                if (hi_bufs[f]) e.hi = hi_bufs[f]->as<unsigned long long>();
                if (index_bufs[f]) {
                    const unsigned long long *x = index_bufs[f]->as<unsigned long long>();
                    e.extremes = ExtremeIndex{raw_bufs[f]->as<unsigned long long>(), x, x + n, x + 2 * n, x + 3 * n, (long long)chunks};
                }
            }
            if (is_value_function(spec.function)) {
                e.has_offset = spec.argument_channels.size() > 1;
                e.has_default = spec.argument_channels.size() > 2;
                TG_CHECK_ARG(!e.has_default || 2 * n <= 0x7fffffffLL, "lag / lead with a default: 2^30 rows or more");
                if (e.has_offset) e.offset = view_of(all.cols[(size_t)spec.argument_channels[1]]);
                rows[f] = scratch((size_t)n * 4);
                e.out_row = rows[f]->as<int32_t>();
            }
            else {
                DeviceColumn &c = result[f];
                c.type = spec.function == TGPU_WINDOW_PERCENT_RANK || spec.function == TGPU_WINDOW_CUME_DIST ? TGPU_DOUBLE : TGPU_BIGINT;
                c.n = n;
                c.values_buf = ctx_->alloc((size_t)n * 8);
                c.values = c.values_buf->ptr();
                e.out = c.values_buf->as<long long>();
                if (spec.function == TGPU_WINDOW_AGGREGATE) {
                    if (spec.agg_function == TGPU_AGG_MIN_DOUBLE || spec.agg_function == TGPU_AGG_MAX_DOUBLE) c.type = TGPU_DOUBLE;
                    e.cnt = cnt_bufs[f]->as<long long>();
                    if (val_bufs[f]) {
                        e.val = val_bufs[f]->as<unsigned long long>();
                        c.nulls_buf = ctx_->alloc((size_t)n);
                        c.nulls = c.nulls_buf->as<uint8_t>();
                        e.out_nulls = c.nulls_buf->as<uint8_t>();
                    }
                }
                else if (spec.function == TGPU_WINDOW_NTILE) {
                    e.offset = view_of(all.cols[(size_t)spec.argument_channels[0]]);
                    c.nulls_buf = ctx_->alloc((size_t)n);
                    c.nulls = c.nulls_buf->as<uint8_t>();
                    e.out_nulls = c.nulls_buf->as<uint8_t>();
                }
            }
            window_evaluate_kernel<<<g, kBlock, 0, ctx_->stream()>>>(e, n);
            check_launch("window_evaluate");
        }
    }
    // the error words, before anything is gathered for rows that must not be
    unsigned int err[4] = {0, 0, 0, 0};
    ctx_->download(err, errors->ptr(), sizeof(err));
    if (err[2] & kErrNullStart) fail(TGPU_ERR_INVALID_ARGUMENT, "Window frame starting offset must not be null");   // getFrameValue, WindowPartition.java:601-607
    if (err[2] & kErrNullEnd) fail(TGPU_ERR_INVALID_ARGUMENT, "Window frame ending offset must not be null");
    if (err[2] & kErrNegative) fail(TGPU_ERR_INVALID_ARGUMENT, "Window frame offset must not be negative");
    if (err[2] & kErrNullCompare) fail(TGPU_ERR_INVALID_ARGUMENT, "Window frame comparison key must not be null where the sort key is not null");
    if (err[3] & kErrNthOffset) fail(TGPU_ERR_INVALID_ARGUMENT, "Offset must be at least 1");                       // NthValueFunction.java:49
    if (err[3] & kErrBuckets) fail(TGPU_ERR_INVALID_ARGUMENT, "Buckets must be greater than 0");                   // NTileFunction.java:52
    if (err[0]) fail(TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE, "bigint addition overflow");   // BigintOperators.add under LongSumAggregation
    if (err[1]) fail(TGPU_ERR_INVALID_ARGUMENT, "Offset must be at least 0");            // LagFunction.java / LeadFunction.java checkCondition
    {
        for (size_t f = 0; f < functions_.size(); f++) {
            const WindowFunctionSpec &spec = functions_[f];
            if (!is_value_function(spec.function)) continue;
            const DeviceColumn &value = all.cols[(size_t)spec.argument_channels[0]];
            if (spec.argument_channels.size() > 2) {
                // the value column with the default column behind it: one gather serves both (and VARCHAR with them)
                PagesIndexGpu both(ctx_, {value.type});
                DevicePage one;
                one.n = n;
                one.cols.push_back(value);
                both.add_page(one);
                one.cols[0] = all.cols[(size_t)spec.argument_channels[2]];
                both.add_page(one);
                scratch_bytes_ += both.estimated_size();
                result[f] = k::gather_column(ctx_, both.column(0), rows[f]->as<int32_t>(), n, true);
            }
            else {
                result[f] = k::gather_column(ctx_, value, rows[f]->as<int32_t>(), n, true);
            }
        }
    }
    return result;
}

}  // namespace tgpu

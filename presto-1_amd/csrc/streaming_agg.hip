// streaming_agg.hip -- the group detection of StreamingAggregationOperator (streaming_agg.h) for gfx950.
//
// A page's groups are its runs of rows that are not distinct from their predecessor (row 0: from the carried key row).  The pass has the
// shape of the group-by's run route (groupby.hip gbh_run_heads_kernel / gbh_run_publish_kernel): tiles of kSaggTile rows, a thread's 8 rows
// one workgroup stride apart (coalesced), the loads of one channel in flight together, __ballot + popcount ranks inside a wave, one scan of
// the tile counts between two launches.  What differs: IS NOT DISTINCT FROM instead of an order (nulls legal and equal to each other, any
// NaN equal to any NaN, -0.0 equal to +0.0), VARCHAR channels (lengths first, then bytes), and no violation: any page is a valid input.
//
// Bytes per row (algorithmic, BIGINT key): each launch reads the key cell once from HBM (the predecessor's cell is the neighbouring
// lane's line: L2 / L1) = 2 x 8 B, the second writes the 4 B id -> 20 B; + 1 B per launch for a null byte, + 4 B per start for the list.
#include "streaming_agg.h"

#include "kernels.h"

namespace tgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kIters = kSaggTile / kBlock;
static_assert(kSaggTile % kBlock == 0 && kIters * kWaves <= 64, "one wave scans the tile's wave counts");

// One fixed-width channel's part of "row r is distinct from row r - 1" for this thread's kIters rows: channel-outer, rows-inner, no branch
// on what was loaded, so that the loads of a channel are in flight together.  KIND: 0 integers, 1 DOUBLE, 2 BOOLEAN (any non-zero byte is true)
template <typename T, int KIND>
__device__ __forceinline__ void sagg_fixed_channel(const T *__restrict__ p, const uint8_t *__restrict__ nulls, int64_t base, int64_t n, bool (&diff)[kIters])
{
    T u[kIters], v[kIters];
    uint8_t nu[kIters], nv[kIters];
#pragma unroll
    for (int it = 0; it < kIters; it++) {
        const int64_t r = base + (int64_t)it * kBlock;
        const bool live = r > 0 && r < n;
        u[it] = live ? p[r] : T(0);
        v[it] = live ? p[r - 1] : T(0);
        nu[it] = (live && nulls) ? nulls[r] : 0;
        nv[it] = (live && nulls) ? nulls[r - 1] : 0;
    }
#pragma unroll
    for (int it = 0; it < kIters; it++) {
        bool d;
        if constexpr (KIND == 1) d = !((u[it] != u[it] && v[it] != v[it]) || u[it] == v[it]);   // DoubleType.java:181-192
        else if constexpr (KIND == 2) d = (u[it] != 0) != (v[it] != 0);
        else d = u[it] != v[it];
        const bool a = nu[it] != 0, b = nv[it] != 0;
        if (a || b) d = a != b;   // null equals null, and nothing else
        diff[it] = diff[it] || d;
    }
}

// VARCHAR: the three offsets of (r - 1, r) together, lengths first; the bytes only where the lengths agree and no earlier channel decided
__device__ __forceinline__ void sagg_varchar_channel(const ColView &x, int64_t base, int64_t n, bool (&diff)[kIters])
{
    const int *__restrict__ off = x.offsets;
    const uint8_t *__restrict__ nulls = x.nulls;
    int o0[kIters], o1[kIters], o2[kIters];
    uint8_t nu[kIters], nv[kIters];
#pragma unroll
    for (int it = 0; it < kIters; it++) {
        const int64_t r = base + (int64_t)it * kBlock;
        const bool live = r > 0 && r < n;
        o0[it] = live ? off[r - 1] : 0;
        o1[it] = live ? off[r] : 0;
        o2[it] = live ? off[r + 1] : 0;
        nu[it] = (live && nulls) ? nulls[r] : 0;
        nv[it] = (live && nulls) ? nulls[r - 1] : 0;
    }
    const uint8_t *pool = (const uint8_t *)x.values;
#pragma unroll
    for (int it = 0; it < kIters; it++) {
        if (diff[it]) continue;
        const bool a = nu[it] != 0, b = nv[it] != 0;
        if (a || b) {
            diff[it] = a != b;
            continue;
        }
        const int len = o2[it] - o1[it];
        if (len != o1[it] - o0[it]) {
            diff[it] = true;
            continue;
        }
        const uint8_t *pa = pool + o1[it], *pb = pool + o0[it];
        bool d = false;
        for (int i = 0; i < len && !d; i++) d = pa[i] != pb[i];
        diff[it] = d;
    }
}

// start[it]: this thread's row base + it * kBlock begins a segment of the page (row 0 always does; rows past n never)
__device__ __forceinline__ void sagg_tile_starts(const KeyCols &batch, int64_t base, int64_t n, bool (&start)[kIters])
{
    bool diff[kIters];
#pragma unroll
    for (int it = 0; it < kIters; it++) diff[it] = false;
    for (int c = 0; c < batch.n; c++) {
        const ColView &x = batch.c[c];
        switch (x.type) {
        case TGPU_BIGINT: case TGPU_TIMESTAMP: sagg_fixed_channel<int64_t, 0>((const int64_t *)x.values, x.nulls, base, n, diff); break;
        case TGPU_INTEGER:
        case TGPU_DATE: sagg_fixed_channel<int32_t, 0>((const int32_t *)x.values, x.nulls, base, n, diff); break;
        case TGPU_DOUBLE: sagg_fixed_channel<double, 1>((const double *)x.values, x.nulls, base, n, diff); break;
        case TGPU_BOOLEAN: sagg_fixed_channel<uint8_t, 2>((const uint8_t *)x.values, x.nulls, base, n, diff); break;
        default: sagg_varchar_channel(x, base, n, diff); break;
        }
    }
#pragma unroll
    for (int it = 0; it < kIters; it++) {
        const int64_t r = base + (int64_t)it * kBlock;
        start[it] = r < n && (r == 0 || diff[it]);
    }
}

// keys_p[0]: the page's key columns, keys_p[1]: the carried one-row key columns (read only with has_carry).  info[1] <- shift
__global__ void __launch_bounds__(kBlock) sagg_heads_kernel(const KeyCols *keys_p, int64_t n, int has_carry, int32_t *__restrict__ tile_counts, long long *info)
{
    const KeyCols &batch = keys_p[0];
    __shared__ int s_count[kWaves];
    const int64_t tiles = (n + kSaggTile - 1) / kSaggTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        bool start[kIters];
        sagg_tile_starts(batch, t * kSaggTile + threadIdx.x, n, start);
        int c = 0;
#pragma unroll
        for (int it = 0; it < kIters; it++) c += start[it] ? 1 : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d, 64);
        if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) total += s_count[w];
            tile_counts[t] = total;
            if (t == 0) info[1] = (has_carry && !tg_rows_not_distinct(batch, 0, keys_p[1], 0)) ? 1 : 0;
        }
        __syncthreads();   // s_count is rewritten by the next tile
    }
}

__global__ void __launch_bounds__(kBlock) sagg_publish_kernel(const KeyCols *keys_p, int64_t n, const int32_t *__restrict__ tile_offsets, const long long *info,
                                                               int32_t *__restrict__ gids, int32_t *__restrict__ starts)
{
    const KeyCols &batch = keys_p[0];
    const int shift = (int)info[1];   // (uniform: written by the heads launch, which is complete)
    __shared__ int s_before[kIters * kWaves];   // starts of the tile before this wave's rows of iteration `it` (it-major = row order)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tiles = (n + kSaggTile - 1) / kSaggTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        bool start[kIters];
        sagg_tile_starts(batch, t * kSaggTile + threadIdx.x, n, start);
        unsigned long long ballots[kIters];
#pragma unroll
        for (int it = 0; it < kIters; it++) {
            ballots[it] = __ballot(start[it]);
            if (lane == 0) s_before[it * kWaves + wave] = __popcll(ballots[it]);
        }
        __syncthreads();
        if (wave == 0) {
            const int v = lane < kIters * kWaves ? s_before[lane] : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            if (lane < kIters * kWaves) s_before[lane] = incl - v;
        }
        __syncthreads();
        const int tile_base = tile_offsets[t];
        const int64_t base = t * kSaggTile + threadIdx.x;
#pragma unroll
        for (int it = 0; it < kIters; it++) {
            const int64_t r = base + (int64_t)it * kBlock;
            // the segment row r lies in: the starts at or before it, minus one (row 0 is a start, so this is never negative)
            const int seg = tile_base + s_before[it * kWaves + wave] + __popcll(ballots[it] & ((2ULL << lane) - 1ULL)) - 1;
            if (r < n) gids[r] = seg + shift;
            if (start[it]) starts[seg] = (int32_t)r;
        }
        __syncthreads();   // s_before is rewritten by the next tile
    }
}

}  // namespace

SaggGroups sagg_detect(Context *ctx, const std::vector<const DeviceColumn *> &keys, int64_t n, const std::vector<DeviceColumn> *carry)
{
    TG_CHECK_STATE(n > 0 && n <= 0x7fffffffLL, "group detection: a page has between 1 and 2^31 - 1 rows");
    TG_CHECK_ARG(!keys.empty(), "streaming aggregation needs at least one group-by channel");
    KeyCols both[2] = {key_cols_of(keys), KeyCols{}};
    if (carry) {
        TG_CHECK_STATE(carry->size() == keys.size(), "carried key row has a different number of channels");
        std::vector<const DeviceColumn *> cp;
        for (size_t i = 0; i < carry->size(); i++) {
            TG_CHECK_STATE((*carry)[i].type == keys[i]->type && (*carry)[i].n == 1, "carried key row does not match the group-by channels");
            cp.push_back(&(*carry)[i]);
        }
        both[1] = key_cols_of(cp);
    }
    SaggGroups out;
    const int64_t tiles = ceil_div(n, kSaggTile);
    BufferPtr dkeys = ctx->alloc(sizeof(both)), counts = ctx->alloc((size_t)tiles * 4), offsets = ctx->alloc((size_t)tiles * 4), info = ctx->alloc(16);
    out.gids = ctx->alloc((size_t)n * 4);
    out.starts = ctx->alloc((size_t)n * 4);   // at most every row starts a segment
    ctx->upload(dkeys->ptr(), both, sizeof(both));
    const int g = grid_for(ctx, n, kSaggTile);
    {
        ProfileScope ps(ctx, "sagg_heads");
        sagg_heads_kernel<<<g, kBlock, 0, ctx->stream()>>>(dkeys->as<KeyCols>(), n, carry ? 1 : 0, counts->as<int32_t>(), info->as<long long>());
        check_launch("sagg_heads");
    }
    k::exclusive_scan_i32(ctx, counts->as<int32_t>(), offsets->as<int32_t>(), tiles, info->as<int64_t>());
    {
        ProfileScope ps(ctx, "sagg_publish");
        sagg_publish_kernel<<<g, kBlock, 0, ctx->stream()>>>(dkeys->as<KeyCols>(), n, offsets->as<int32_t>(), info->as<long long>(), out.gids->as<int32_t>(),
                                                            out.starts->as<int32_t>());
        check_launch("sagg_publish");
    }
    long long host[2];
    ctx->download(host, info->ptr(), sizeof(host));   // the page's one read-back: segments, shift
    TG_CHECK_STATE(host[0] >= 1 && host[0] <= n && (host[1] == 0 || host[1] == 1), "group detection: bad segment count");
    out.segments = host[0];
    out.shift = host[1] != 0;
    return out;
}

}  // namespace tgpu

// minmax_varchar.hip -- min / max over VARCHAR: the round / select / install kernels and the value store (minmax_varchar.h).
#include "minmax_varchar.h"
#include "kernels.h"
#include "device_agg.h"

#include <algorithm>

namespace tgpu {

namespace {

constexpr int kBlock = 256;
enum { kNext = 0, kNeed = 1, kCursor = 2, kGarbage = 3, kCounters = 4 };   // the device counters (minmax_varchar.h counters_)

struct VxPage {
    const int32_t *gids;         // nullptr: group 0
    const uint8_t *bytes;
    const int32_t *offsets;
    const uint8_t *nulls, *mask, *mask_nulls;
    const long long *icounts;    // intermediate input: the count channel
    const int32_t *list;         // rounds > 0: the candidate rows; round 0: every row of the page
    int64_t m;                   // candidates
    int32_t round, is_min;
};

__device__ __forceinline__ bool vx_take(const VxPage &p, int64_t r)
{
    if (p.icounts) return p.icounts[r] > 0;
    if (p.mask && ((p.mask_nulls && p.mask_nulls[r]) || !p.mask[r])) return false;
    return !(p.nulls && p.nulls[r]);
}

// the round's code of the value [b, e): bytes [7k, 7k + 7) big-endian and zero-padded, then min(rest, 8); a candidate of round k has at
// least 7k bytes.  Byte loads inside the value's range only.  min: the complement, so that one unsigned max serves both.
__device__ __forceinline__ unsigned long long vx_code(const uint8_t *bytes, int32_t b, int32_t e, int round, bool is_min)
{
    const long long start = (long long)b + 7LL * round;
    const long long rest = (long long)e - start;
    unsigned long long w = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        w <<= 8;
        if (i < rest) w |= bytes[start + i];
    }
    const unsigned long long code = (w << 8) | (unsigned long long)(rest < 8 ? rest : 8);
    return is_min ? ~code : code;
}

// one atomicMax per candidate row into the round's word of its group; round 0 also counts the rows taken
__global__ void __launch_bounds__(kBlock) vx_round_kernel(VxPage p, unsigned long long *__restrict__ words, long long *__restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const int64_t rounded = (p.m + 63) / 64 * 64;   // whole waves go through the loop: the ballots below need every lane
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rounded; i += (int64_t)gridDim.x * kBlock) {
        bool active = false;
        int64_t r = 0, g = 0;
        if (i < p.m) {
            r = p.list ? p.list[i] : i;
            if (p.round > 0 || vx_take(p, r)) {
                g = p.gids ? p.gids[r] : 0;
                active = g >= 0;
            }
        }
        if (p.round == 0 && p.icounts) {
            if (active) atomicAdd((unsigned long long *)&counts[g], (unsigned long long)p.icounts[r]);
        }
        else if (p.round == 0) {
            // the rows of up to four groups are counted once per wave (a handful of groups: every lane of the chip would add 1 to the same
            // few words); whoever is left after that adds its own 1
            unsigned long long todo = __ballot(active);
            for (int it = 0; it < 4 && todo; it++) {
                const int leader = __ffsll((long long)todo) - 1;
                const long long g0 = __shfl((long long)g, leader, 64);
                const unsigned long long same = __ballot(active && g == g0);
                if (lane == leader) atomicAdd((unsigned long long *)&counts[g0], (unsigned long long)__popcll(same));
                todo &= ~same;
            }
            if (active && ((todo >> lane) & 1ULL)) atomicAdd((unsigned long long *)&counts[g], 1ULL);
        }
        if (!active) continue;
        const int32_t b = p.offsets[r], e = p.offsets[r + 1];
        tg_minmax_update(&words[g * 2 + (p.round & 1)], vx_code(p.bytes, b, e, p.round, p.is_min != 0));
    }
}

// the candidates whose code is their group's winner: where the winner ends in this round the first of them claims the group (they are
// byte-identical), else they go to the next round's list -- appended wave by wave -- and clear the word that round will use
__global__ void __launch_bounds__(kBlock) vx_select_kernel(VxPage p, unsigned long long *__restrict__ words, int *__restrict__ claim, int32_t *__restrict__ next,
                                                           unsigned long long *__restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t rounded = (p.m + 63) / 64 * 64;   // whole waves go through the loop: the ballot below needs every lane
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rounded; i += stride) {
        bool goes_on = false;
        int64_t r = 0;
        if (i < p.m) {
            r = p.list ? p.list[i] : i;
            const int64_t g = p.gids ? p.gids[r] : 0;
            if ((p.round > 0 || vx_take(p, r)) && g >= 0) {
                const int32_t b = p.offsets[r], e = p.offsets[r + 1];
                const unsigned long long code = vx_code(p.bytes, b, e, p.round, p.is_min != 0);
                if (code == words[g * 2 + (p.round & 1)]) {
                    const unsigned long long plain = p.is_min ? ~code : code;
                    if ((plain & 0xff) <= 7) {
                        if (atomicCAS(&claim[g], 0, (int)r + 1) == 0) atomicAdd(&counters[kNeed], (unsigned long long)(e - b));
                    }
                    else {
                        goes_on = true;
                        words[g * 2 + ((p.round + 1) & 1)] = 0ULL;   // (nobody reads or writes that word during this launch)
                    }
                }
            }
        }
        const unsigned long long going = __ballot(goes_on);
        if (going == 0) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&counters[kNext], (unsigned long long)__popcll(going));
        base = __shfl(base, 0, 64);
        if (goes_on) next[base + __popcll(going & ((1ULL << lane) - 1ULL))] = (int32_t)r;
    }
}

// The row that claimed its group compares its value with the group's stored one -- one comparison per group and page -- and, when it is
// better (or the first), takes room at the end of the arena; the wave then copies the values of its winning lanes together.  The group's
// two words and its claim are cleared for the next page.
__global__ void __launch_bounds__(kBlock) vx_install_kernel(VxPage p, unsigned long long *__restrict__ words, int *__restrict__ claim, long long *__restrict__ vpos,
                                                            int *__restrict__ vlen, uint8_t *__restrict__ arena, unsigned long long *__restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t rounded = (p.m + 63) / 64 * 64;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rounded; r += stride) {
        bool better = false;
        int32_t b = 0, len = 0;
        long long pos = 0;
        if (r < p.m && vx_take(p, r)) {
            const int64_t g = p.gids ? p.gids[r] : 0;
            if (g >= 0 && claim[g] == (int)r + 1) {
                words[g * 2] = words[g * 2 + 1] = 0ULL;
                claim[g] = 0;
                b = p.offsets[r];
                len = p.offsets[r + 1] - b;
                const long long at = vpos[g];
                better = at == 0;
                int old = 0;
                if (at != 0) {
                    old = vlen[g];
                    const uint8_t *mine = p.bytes + b, *kept = arena + (at - 1);
                    const int both = len < old ? len : old;
                    int i = 0;
                    while (i < both && mine[i] == kept[i]) i++;
                    const int c = i < both ? (mine[i] < kept[i] ? -1 : 1) : (len < old ? -1 : (len > old ? 1 : 0));   // Slice.compareTo
                    better = p.is_min ? c < 0 : c > 0;
                }
                if (better) {
                    pos = (long long)atomicAdd(&counters[kCursor], (unsigned long long)len);
                    if (old) atomicAdd(&counters[kGarbage], (unsigned long long)old);
                    vpos[g] = pos + 1;
                    vlen[g] = len;
                }
            }
        }
        unsigned long long todo = __ballot(better && len > 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int32_t sb = __shfl(b, src, 64), sl = __shfl(len, src, 64);
            const long long sp = __shfl(pos, src, 64);
            for (int j = lane; j < sl; j += 64) arena[sp + j] = p.bytes[(long long)sb + j];
        }
    }
}

// length of every group's output cell (0 where the count is 0), its null flag, and the sum of the lengths
__global__ void __launch_bounds__(kBlock) vx_lengths_kernel(const long long *__restrict__ counts, const long long *__restrict__ vpos, const int *__restrict__ vlen, int64_t groups,
                                                            int32_t *__restrict__ lens, uint8_t *__restrict__ nulls, unsigned long long *__restrict__ total)
{
    const int64_t rounded = (groups + 63) / 64 * 64;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < rounded; g += (int64_t)gridDim.x * kBlock) {
        long long len = 0;
        if (g < groups) {
            const bool has = (counts == nullptr || counts[g] > 0) && vpos[g] != 0;
            len = has ? vlen[g] : 0;
            lens[g] = (int32_t)len;
            if (nulls) nulls[g] = has ? 0 : 1;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d, 64);
        if ((threadIdx.x & 63) == 0 && len) atomicAdd(total, (unsigned long long)len);
    }
}

// one wave per group: its value from the arena to dst + offsets[g]; offsets[groups] is written behind the last group (close) and the
// group's position follows the copy (move: the arena's compaction)
__global__ void __launch_bounds__(kBlock) vx_gather_kernel(const uint8_t *__restrict__ arena, long long *__restrict__ vpos, const int32_t *__restrict__ lens,
                                                           int32_t *__restrict__ offsets, int64_t groups, uint8_t *__restrict__ dst, int close, int move)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t g = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); g < groups; g += waves) {
        const int32_t len = lens[g], off = offsets[g];
        const long long at = vpos[g];
        if (len > 0)
            for (int j = lane; j < len; j += 64) dst[(long long)off + j] = arena[at - 1 + j];
        if (lane == 0) {
            if (close && g == groups - 1) offsets[groups] = off + len;
            if (move && at != 0) vpos[g] = (long long)off + 1;
        }
    }
}

__global__ void vx_set_counters_kernel(unsigned long long *counters, unsigned long long cursor, unsigned long long garbage)
{
    counters[kCursor] = cursor;
    counters[kGarbage] = garbage;
}

// new array of new_elems elements: the old contents carried over, the tail zeroed
BufferPtr grown(Context *ctx, const BufferPtr &old, int64_t old_elems, int64_t new_elems, int elem_bytes)
{
    BufferPtr nb = ctx->alloc((size_t)new_elems * elem_bytes);
    const size_t keep = old ? (size_t)old_elems * elem_bytes : 0;
    if (keep) HIP_CHECK(hipMemcpyAsync(nb->ptr(), old->ptr(), keep, hipMemcpyDeviceToDevice, ctx->stream()));
    HIP_CHECK(hipMemsetAsync(nb->as<uint8_t>() + keep, 0, (size_t)new_elems * elem_bytes - keep, ctx->stream()));
    return nb;
}

constexpr int64_t kMaxPool = 0x7fffffffLL;   // a VariableWidthBlock's bytes

}  // namespace

void VarcharExtremes::ensure(int64_t groups)
{
    if (!counters_) counters_ = ctx_->alloc_zero(kCounters * 8);
    if (groups <= cap_) return;
    int64_t cap = cap_ ? cap_ : 256;
    while (cap < groups) cap <<= 1;
    counts_ = grown(ctx_, counts_, cap_, cap, 8);
    words_ = grown(ctx_, words_, cap_ * 2, cap * 2, 8);
    claim_ = grown(ctx_, claim_, cap_, cap, 4);
    vpos_ = grown(ctx_, vpos_, cap_, cap, 8);
    vlen_ = grown(ctx_, vlen_, cap_, cap, 4);
    cap_ = cap;
}

int64_t VarcharExtremes::estimated_size() const
{
    return cap_ * (8 + 16 + 4 + 8 + 4) + (arena_ ? (int64_t)arena_->bytes() : 0);
}

// Room for `need` more bytes behind `cursor`.  The arena is compacted -- into one sized 2 x (live + need) -- when its garbage exceeds its
// live bytes, and doubled to 2 x (cursor + need) when it is merely full: between pages cursor <= 2 x live + the last page's winners, so
// the arena never exceeds 4 x (live bytes + one page's winners), whatever the number of pages.
void VarcharExtremes::reserve_arena(int64_t cursor, int64_t garbage, int64_t need, int64_t groups)
{
    const int64_t live = cursor - garbage;
    groups = cap_;   // (every group that may hold a value, not only those the page at hand knows)
    if (garbage > live) {
        if (live > kMaxPool) fail(TGPU_ERR_INSUFFICIENT_RESOURCES, "variable width block cannot exceed 2GB");
        ProfileScope ps(ctx_, "agg_varchar_extreme_compact");
        BufferPtr fresh = ctx_->alloc((size_t)std::max<int64_t>(2 * (live + need), 4096));
        BufferPtr lens = ctx_->alloc((size_t)groups * 4), offsets = ctx_->alloc((size_t)(groups + 1) * 4), total = ctx_->alloc_zero(16);
        vx_lengths_kernel<<<grid_for(ctx_, groups), kBlock, 0, ctx_->stream()>>>(nullptr, vpos_->as<long long>(), vlen_->as<int>(), groups, lens->as<int32_t>(), nullptr,
                                                                                total->as<unsigned long long>());
        check_launch("agg_varchar_extreme_compact");
        k::exclusive_scan_i32(ctx_, lens->as<int32_t>(), offsets->as<int32_t>(), groups, (int64_t *)(total->as<unsigned long long>() + 1));
        vx_gather_kernel<<<grid_for(ctx_, groups, kBlock / 64), kBlock, 0, ctx_->stream()>>>(arena_->as<uint8_t>(), vpos_->as<long long>(), lens->as<int32_t>(),
                                                                                             offsets->as<int32_t>(), groups, fresh->as<uint8_t>(), 0, 1);
        check_launch("agg_varchar_extreme_compact");
        vx_set_counters_kernel<<<1, 1, 0, ctx_->stream()>>>(counters_->as<unsigned long long>(), (unsigned long long)live, 0ULL);
        check_launch("agg_varchar_extreme_compact");
        arena_ = fresh;
        return;
    }
    if (arena_ && cursor + need <= (int64_t)arena_->bytes()) return;
    BufferPtr fresh = ctx_->alloc((size_t)std::max<int64_t>(2 * (cursor + need), 4096));
    if (arena_ && cursor > 0) HIP_CHECK(hipMemcpyAsync(fresh->ptr(), arena_->ptr(), (size_t)cursor, hipMemcpyDeviceToDevice, ctx_->stream()));
    arena_ = fresh;
}

void VarcharExtremes::add(const int32_t *gids, int64_t n, const DeviceColumn &values, const uint8_t *mask, const uint8_t *mask_nulls, const long long *icounts, int64_t groups)
{
    if (n <= 0) return;
    TG_CHECK_ARG(values.type == TGPU_VARCHAR && values.offsets != nullptr, "aggregate input: unexpected channel type " + std::string(type_name(values.type)));
    TG_CHECK_ARG(n < 0x7fffffffLL, "min / max over VARCHAR: too many rows in a page");
    groups = groups > 0 ? groups : 1;
    ensure(groups);
    unsigned long long *counters = counters_->as<unsigned long long>();
    HIP_CHECK(hipMemsetAsync(counters, 0, 16, ctx_->stream()));   // next, need; the cursor and the garbage live on
    VxPage p{gids, (const uint8_t *)values.values, values.offsets, values.nulls, mask, mask_nulls, icounts, nullptr, n, 0, is_min_ ? 1 : 0};
    unsigned long long c[kCounters] = {0, 0, 0, 0};
    BufferPtr list, next;
    for (;;) {
        ProfileScope ps(ctx_, "agg_varchar_extreme_round");
        next = ctx_->alloc((size_t)p.m * 4);
        vx_round_kernel<<<grid_for(ctx_, p.m), kBlock, 0, ctx_->stream()>>>(p, words_->as<unsigned long long>(), counts_->as<long long>());
        check_launch("agg_varchar_extreme_round");
        HIP_CHECK(hipMemsetAsync(counters, 0, 8, ctx_->stream()));
        vx_select_kernel<<<grid_for(ctx_, p.m), kBlock, 0, ctx_->stream()>>>(p, words_->as<unsigned long long>(), claim_->as<int>(), next->as<int32_t>(), counters);
        check_launch("agg_varchar_extreme_round");
        ctx_->download(c, counters, sizeof(c));   // the round's one read-back
        rounds_++;
        if (p.round == 0) ctx_->profile_note("agg_varchar_extreme_survivors", (int64_t)c[kNext]);   // rows that go on to round 1
        if (c[kNext] == 0) break;
        TG_CHECK_STATE((int64_t)c[kNext] <= p.m, "min / max over VARCHAR: a round's survivors outnumber its candidates");
        list = next;
        p.list = list->as<int32_t>();
        p.m = (int64_t)c[kNext];
        p.round++;
    }
    reserve_arena((int64_t)c[kCursor], (int64_t)c[kGarbage], (int64_t)c[kNeed], groups);
    p.list = nullptr;
    p.m = n;
    p.round = 0;
    ProfileScope ps(ctx_, "agg_varchar_extreme_install");
    vx_install_kernel<<<grid_for(ctx_, n), kBlock, 0, ctx_->stream()>>>(p, words_->as<unsigned long long>(), claim_->as<int>(), vpos_->as<long long>(), vlen_->as<int>(),
                                                                        arena_->as<uint8_t>(), counters);
    check_launch("agg_varchar_extreme_install");
}

void VarcharExtremes::evaluate(int64_t groups, bool partial, std::vector<DeviceColumn> &out)
{
    const int64_t alloc_n = groups > 0 ? groups : 1;
    ensure(alloc_n);
    if (partial) {
        DeviceColumn c0;
        c0.n = groups;
        c0.type = TGPU_BIGINT;
        c0.values_buf = ctx_->alloc((size_t)alloc_n * 8);
        c0.values = c0.values_buf->ptr();
        if (groups > 0) HIP_CHECK(hipMemcpyAsync(c0.values_buf->ptr(), counts_->ptr(), (size_t)groups * 8, hipMemcpyDeviceToDevice, ctx_->stream()));
        out.push_back(c0);
    }
    DeviceColumn c;
    c.n = groups;
    c.type = TGPU_VARCHAR;
    c.nulls_buf = ctx_->alloc((size_t)alloc_n);
    c.nulls = c.nulls_buf->as<uint8_t>();
    c.offsets_buf = ctx_->alloc_zero((size_t)(alloc_n + 1) * 4);
    c.offsets = c.offsets_buf->as<int32_t>();
    int64_t total = 0;
    BufferPtr lens, sum;
    if (groups > 0) {
        lens = ctx_->alloc((size_t)groups * 4);
        sum = ctx_->alloc_zero(16);
        ProfileScope ps(ctx_, "agg_evaluate");
        vx_lengths_kernel<<<grid_for(ctx_, groups), kBlock, 0, ctx_->stream()>>>(counts_->as<long long>(), vpos_->as<long long>(), vlen_->as<int>(), groups, lens->as<int32_t>(),
                                                                                c.nulls_buf->as<uint8_t>(), sum->as<unsigned long long>());
        check_launch("agg_evaluate");
        total = (int64_t)ctx_->read_scalar(sum->as<unsigned long long>());
        if (total > kMaxPool) fail(TGPU_ERR_INSUFFICIENT_RESOURCES, "variable width block cannot exceed 2GB");
        k::exclusive_scan_i32(ctx_, lens->as<int32_t>(), c.offsets_buf->as<int32_t>(), groups, (int64_t *)(sum->as<unsigned long long>() + 1));
    }
    c.values_buf = ctx_->alloc((size_t)std::max<int64_t>(total, 1));
    c.values = c.values_buf->ptr();
    c.pool_bytes = total;
    c.pool_exact = true;
    c.pool_first = 0;
    if (groups > 0) {
        ProfileScope ps(ctx_, "agg_evaluate");
        vx_gather_kernel<<<grid_for(ctx_, groups, kBlock / 64), kBlock, 0, ctx_->stream()>>>(arena_ ? arena_->as<uint8_t>() : nullptr, vpos_->as<long long>(), lens->as<int32_t>(),
                                                                                             c.offsets_buf->as<int32_t>(), groups, c.values_buf->as<uint8_t>(), 1, 0);
        check_launch("agg_evaluate");
    }
    out.push_back(c);
}

}  // namespace tgpu

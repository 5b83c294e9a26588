// nested_loop.hip -- product materialisation of the nested loop join (nested_loop.h): pure HBM write.  Every kernel covers rows
// [r0, r0 + n) of the sequence of one (probe page, build page) pair; lanes write 16 bytes each, consecutive lanes consecutive chunks, and the
// division r / L is done once per chunk (the elements behind it step through (r / L, r % L) by increment and wrap).
#include "nested_loop.h"

namespace tgpu {
namespace {

struct alignas(16) Chunk16 { unsigned int w[4]; };

// out[i] = src[(r0 + i) % L] (tiled) or src[(r0 + i) / L] (repeated), i in [0, n).  Reads: tiled m < L = rows of src; repeated q <= (r0 + n - 1) / L
// < rows of the small side = rows of src.  Writes: [0, n) of out, whole 16-byte chunks while they fit, the last elements one by one.
template <typename T> __global__ void __launch_bounds__(256) nl_fixed_kernel(const T *__restrict__ src, T *__restrict__ out, int64_t n, int64_t r0, int64_t L, int tiled)
{
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t chunks = (n + E - 1) / E;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
        const int64_t i0 = c * E;
        int64_t q = (r0 + i0) / L, m = (r0 + i0) - q * L;
        union { Chunk16 chunk; T v[E]; } u;
#pragma unroll
        for (int k = 0; k < E; k++) {
            u.v[k] = (i0 + k < n) ? src[tiled ? m : q] : T(0);
            if (++m == L) { m = 0; q++; }
        }
        if (i0 + E <= n) *reinterpret_cast<Chunk16 *>(out + i0) = u.chunk;
        else
            for (int k = 0; i0 + k < n; k++) out[i0 + k] = u.v[k];
    }
}

// bytes of the channel before row r of the sequence, off = the source's offsets (absolute into its pool), rows = rows of the source
__host__ __device__ inline int64_t bytes_before(const int32_t *off, int64_t rows, bool tiled, int64_t L, int64_t r)
{
    const int64_t q = r / L, m = r - q * L;
    if (tiled) return q * (int64_t)(off[rows] - off[0]) + (off[m] - off[0]);   // rows == L, m < L
    if (q >= rows) return L * (int64_t)(off[rows] - off[0]);                    // r = the end of the sequence
    return L * (int64_t)(off[q] - off[0]) + m * (int64_t)(off[q + 1] - off[q]);
}

// out[i] = bytes before row r0 + i, less those before r0: i in [0, n] (n + 1 offsets)
__global__ void __launch_bounds__(256) nl_varchar_offsets_kernel(const int32_t *__restrict__ off, int64_t rows, int32_t *__restrict__ out, int64_t n, int64_t r0, int64_t L,
                                                                 int tiled, int64_t base)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (int64_t)gridDim.x * 256) out[i] = (int32_t)(bytes_before(off, rows, tiled != 0, L, r0 + i) - base);
}

// Lanes over 16-byte chunks of the output pool [0, bytes).  Byte x of it is byte X = base + x of the whole sequence's pool, and where that
// lies in the source is closed-form: tiled, the source pool (P bytes) over and over, X % P; repeated, small row s owns [L o[s], L o[s + 1])
// (o = offsets less off[0]; s by binary search over the source's offsets, once per chunk and again where a chunk crosses into the next
// row) and holds its len bytes L times, (X - L o[s]) % len.
__global__ void __launch_bounds__(256) nl_varchar_bytes_kernel(const uint8_t *__restrict__ pool, const int32_t *__restrict__ off, int64_t rows, uint8_t *__restrict__ out,
                                                               int64_t bytes, int64_t L, int tiled, int64_t base)
{
    const int64_t chunks = (bytes + 15) / 16;
    const int64_t off0 = off[0], P = off[rows] - off0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
        const int64_t x0 = c * 16;
        union { Chunk16 chunk; uint8_t v[16]; } u;
        int64_t X = base + x0;
        if (tiled) {
            int64_t p = X % P;   // bytes > 0, so P > 0
            for (int k = 0; k < 16; k++) {
                u.v[k] = (x0 + k < bytes) ? pool[off0 + p] : (uint8_t)0;
                if (++p == P) p = 0;
            }
        }
        else {
            int64_t s = 0, w = 0, len = 0, end = -1;   // X < end: s, len and w = (X - L o[s]) % len are valid
            for (int k = 0; k < 16 && x0 + k < bytes; k++, X++) {
                if (X >= end) {
                    // the first j in [1, rows] with L o[j] > X exists (X < L o[rows], the sequence's pool); s = j - 1
                    int64_t lo = 1, hi = rows;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (L * (int64_t)(off[mid] - off0) > X) hi = mid;
                        else lo = mid + 1;
                    }
                    s = lo - 1;
                    len = off[s + 1] - off[s];
                    end = L * (int64_t)(off[s + 1] - off0);
                    w = (X - L * (int64_t)(off[s] - off0)) % len;   // len > 0: the row's range holds X
                }
                u.v[k] = pool[off[s] + w];
                if (++w == len) w = 0;
            }
        }
        if (x0 + 16 <= bytes) *reinterpret_cast<Chunk16 *>(out + x0) = u.chunk;
        else
            for (int k = 0; x0 + k < bytes; k++) out[x0 + k] = u.v[k];
    }
}

template <typename T> void launch_fixed(Context *ctx, const void *src, void *out, int64_t n, int64_t r0, int64_t L, bool tiled)
{
    const int g = grid_for(ctx, ceil_div(n * (int64_t)sizeof(T), 16));
    nl_fixed_kernel<T><<<g, 256, 0, ctx->stream()>>>((const T *)src, (T *)out, n, r0, L, tiled ? 1 : 0);
}
}  // namespace

NlPage nl_keep(Context *ctx, DevicePage page)
{
    NlPage k;
    own_borrowed_columns(ctx, page);
    k.host_offsets.resize(page.cols.size());
    for (size_t i = 0; i < page.cols.size(); i++) {
        const DeviceColumn &c = page.cols[i];
        if (c.type != TGPU_VARCHAR || page.n == 0) continue;
        k.host_offsets[i].resize((size_t)page.n + 1);
        ctx->download(k.host_offsets[i].data(), c.offsets, ((size_t)page.n + 1) * 4);
    }
    k.page = std::move(page);
    return k;
}

int64_t nl_varchar_bytes_before(const NlPage &pg, int col, bool tiled, int64_t L, int64_t r)
{
    return bytes_before(pg.host_offsets[(size_t)col].data(), pg.page.n, tiled, L, r);
}

int64_t nl_cut_rows(const NlPage &pg, const std::vector<int32_t> &cols, bool tiled, int64_t L, int64_t r0, int64_t want)
{
    int64_t n = want;
    for (int32_t col : cols) {
        if (pg.page.cols[(size_t)col].type != TGPU_VARCHAR) continue;
        const int64_t base = nl_varchar_bytes_before(pg, col, tiled, L, r0);
        if (nl_varchar_bytes_before(pg, col, tiled, L, r0 + n) - base <= 0x7fffffffLL - 1) continue;
        int64_t lo = 1, hi = n;   // bytes are monotone in the row count; one row always fits (it is a row of the source)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (nl_varchar_bytes_before(pg, col, tiled, L, r0 + mid) - base <= 0x7fffffffLL - 1) lo = mid;
            else hi = mid - 1;
        }
        n = lo;
    }
    return n;
}

DeviceColumn nl_product_column(Context *ctx, const NlPage &pg, int col, bool tiled, int64_t L, int64_t r0, int64_t n)
{
    const DeviceColumn &src = pg.page.cols[(size_t)col];
    const int64_t rows = pg.page.n;
    TG_CHECK_ARG(n > 0 && r0 >= 0 && L > 0 && (tiled ? rows == L : (r0 + n - 1) / L < rows), "nested loop product: rows outside the sequence");
    DeviceColumn out;
    out.type = src.type;
    out.n = n;
    if (src.nulls) {
        out.nulls_buf = ctx->alloc((size_t)n);
        out.nulls = out.nulls_buf->as<uint8_t>();
        launch_fixed<uint8_t>(ctx, src.nulls, out.nulls_buf->ptr(), n, r0, L, tiled);
    }
    if (src.type == TGPU_VARCHAR) {
        const int64_t base = nl_varchar_bytes_before(pg, col, tiled, L, r0), bytes = nl_varchar_bytes_before(pg, col, tiled, L, r0 + n) - base;
        TG_CHECK_STATE(bytes <= 0x7fffffffLL - 1, "nested loop product: a piece's VARCHAR pool reached 2 GB");
        out.offsets_buf = ctx->alloc((size_t)(n + 1) * 4);
        out.offsets = out.offsets_buf->as<int32_t>();
        nl_varchar_offsets_kernel<<<grid_for(ctx, n + 1), 256, 0, ctx->stream()>>>(src.offsets, rows, out.offsets_buf->as<int32_t>(), n, r0, L, tiled ? 1 : 0, base);
        out.values_buf = ctx->alloc((size_t)(bytes > 0 ? bytes : 1));
        out.values = out.values_buf->ptr();
        out.pool_bytes = bytes;
        out.pool_exact = true;
        if (bytes > 0)
            nl_varchar_bytes_kernel<<<grid_for(ctx, ceil_div(bytes, 16)), 256, 0, ctx->stream()>>>((const uint8_t *)src.values, src.offsets, rows, out.values_buf->as<uint8_t>(), bytes,
                                                                                                  L, tiled ? 1 : 0, base);
    }
    else {
        const int w = type_width(src.type);
        out.values_buf = ctx->alloc((size_t)n * (size_t)w);
        out.values = out.values_buf->ptr();
        if (w == 8) launch_fixed<uint64_t>(ctx, src.values, out.values_buf->ptr(), n, r0, L, tiled);
        else if (w == 4) launch_fixed<uint32_t>(ctx, src.values, out.values_buf->ptr(), n, r0, L, tiled);
        else launch_fixed<uint8_t>(ctx, src.values, out.values_buf->ptr(), n, r0, L, tiled);
    }
    check_launch("nested_loop_product");
    return out;
}

}  // namespace tgpu

// device_order.h -- the row order of the sort channels on the device, shared by topn.hip, topn_ranking.hip and merge.hip: the 64-bit ORDER CODE of a
// row's first sort key and the full row comparator (SimplePageWithPositionComparator.java:58-79 + TypeOperators.java:578-596: nulls
// placed by the SortOrder, values by the type's COMPARISON operator, negated for DESC).  AOT kernels only (not embedded into JIT sources).
#pragma once

#include "common.h"

namespace tgpu {

// sort keys in device memory (read through a pointer: run-time column indices are then plain scalar loads)
struct TopNKeys {
    TgKeyCols cols;                       // the sort channels, in priority order
    int order[TG_MAX_KEY_CHANNELS];       // tgpu_sort_order per key
};

__device__ __forceinline__ bool asc(int order) { return order == TGPU_SORT_ASC_NULLS_FIRST || order == TGPU_SORT_ASC_NULLS_LAST; }
__device__ __forceinline__ bool nulls_first(int order) { return order == TGPU_SORT_ASC_NULLS_FIRST || order == TGPU_SORT_DESC_NULLS_FIRST; }

// Double.compare order as an unsigned key: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN (all NaNs equal)
__device__ __forceinline__ unsigned long long double_order_bits(unsigned long long bits)
{
    const double v = __longlong_as_double((long long)bits);
    if (v != v) bits = 0x7ff8000000000000ULL;
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
}

// order-preserving 64-bit pattern of a non-null cell (VARCHAR: a prefix)
__device__ __forceinline__ unsigned long long cell_order_bits(const TgColView &c, long long r)
{
    switch (c.type) {
    case TGPU_BIGINT: case TGPU_TIMESTAMP: return (unsigned long long)((const long long *)c.values)[r] ^ 0x8000000000000000ULL;
    case TGPU_INTEGER:
    case TGPU_DATE: return (unsigned long long)(long long)((const int *)c.values)[r] ^ 0x8000000000000000ULL;
    case TGPU_DOUBLE: return double_order_bits(((const unsigned long long *)c.values)[r]);
    case TGPU_BOOLEAN: return ((const unsigned char *)c.values)[r] ? 1ULL : 0ULL;
    case TGPU_VARCHAR: {
        const int a = c.offsets[r], l = c.offsets[r + 1] - a;
        const unsigned char *p = (const unsigned char *)c.values + a;
        unsigned long long v = 0;
        for (int i = 0; i < 8; i++) v = (v << 8) | (i < l ? (unsigned long long)p[i] : 0ULL);
        return v;
    }
    default: return 0;
    }
}

// the type's COMPARISON operator on two non-null cells, cell a of column x against cell b of column y (columns of one type): <0, 0, >0
// (Long.compare / Integer.compare / Double.compare / Boolean.compare / Slice.compareTo = unsigned bytes, then length)
__device__ __forceinline__ int compare_cells(const TgColView &x, long long a, const TgColView &y, long long b)
{
    if (x.type == TGPU_VARCHAR) {
        const int oa = x.offsets[a], la = x.offsets[a + 1] - oa, ob = y.offsets[b], lb = y.offsets[b + 1] - ob;
        const unsigned char *pa = (const unsigned char *)x.values + oa, *pb = (const unsigned char *)y.values + ob;
        const int m = la < lb ? la : lb;
        for (int i = 0; i < m; i++)
            if (pa[i] != pb[i]) return pa[i] < pb[i] ? -1 : 1;
        return la < lb ? -1 : (la > lb ? 1 : 0);
    }
    const unsigned long long p = cell_order_bits(x, a), q = cell_order_bits(y, b);
    return p < q ? -1 : (p > q ? 1 : 0);
}
__device__ __forceinline__ int compare_cells(const TgColView &c, long long a, long long b) { return compare_cells(c, a, c, b); }

// SimplePageWithPositionComparator.compareTo over the sort keys: row a of the columns x against row b of the columns y (the same
// channels of two pages; merge.hip compares rows of different streams)
__device__ __forceinline__ int compare_rows(const TgKeyCols &x, long long a, const TgKeyCols &y, long long b, const int *order)
{
    for (int i = 0; i < x.n; i++) {
        const TgColView &c = x.c[i], &d = y.c[i];
        const bool na = c.nulls && c.nulls[a], nb = d.nulls && d.nulls[b];
        if (na || nb) {   // TypeOperators.orderNulls
            if (na && nb) continue;
            if (na) return nulls_first(order[i]) ? -1 : 1;
            return nulls_first(order[i]) ? 1 : -1;
        }
        const int cmp = compare_cells(c, a, d, b);
        if (cmp) return asc(order[i]) ? cmp : -cmp;
    }
    return 0;
}
__device__ __forceinline__ int compare_rows(const TopNKeys &k, long long a, long long b) { return compare_rows(k.cols, a, k.cols, b, k.order); }

// The order code of row r: the first sort key's order-preserving bit pattern, complemented for DESC, shifted right by one and topped
// with a null bit placed by the SortOrder.  code(a) < code(b) implies a sorts before b; equal codes decide nothing.
__device__ __forceinline__ unsigned long long order_code(const TgColView &c, int order, long long r)
{
    const bool is_null = c.nulls && c.nulls[r];
    unsigned long long v = 0;
    if (!is_null) {
        v = cell_order_bits(c, r);
        if (!asc(order)) v = ~v;
    }
    // the null bit on top (nulls first: nulls get 0 and values 1), the value's upper 63 bits below it
    const unsigned long long top = (is_null == nulls_first(order)) ? 0ULL : 1ULL;
    return (top << 63) | (is_null ? 0ULL : (v >> 1));
}
__device__ __forceinline__ unsigned long long order_code(const TopNKeys &k, long long r) { return order_code(k.cols.c[0], k.order[0], r); }

}  // namespace tgpu

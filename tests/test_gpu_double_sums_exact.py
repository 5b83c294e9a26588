"""EXACT-mode DOUBLE sums bit for bit against an exact integer reference (tests/exact_sum.py), over adversarial value families x every path
a few-group aggregation takes: the global-atomics kernel, the lane-private LDS kernels (plain and fused, one launch per page), pages of
mixed size into one state, global aggregation, PARTIAL -> FINAL, spilled runs, and the Java order.  Per group: sum(double), avg(double)
(one IEEE division of the exact sum), avg(bigint) (the exact sum of the (double) values), the counts; one column with nulls and a mask."""
import numpy as np
import pytest

from agg_paths import (PATHS, assert_profile, drive, final_aggs, is_fused, late_group_first_row, max_lowcard_groups_fused, max_lowcard_groups_plain,
                       page_sizes, run_final, run_partials)
from exact_sum import FAMILIES, bits_equal, exact_double_sum, make_stream

pytestmark = pytest.mark.gpu

# the most groups that still decide EXACT on the lane-private path: 160 KiB of LDS / the bytes of one group's lane-private states --
# plain operator (agg.hip lowcard_bytes_per_group: 5 sums x 2 x 256 x 8 + 7 counts x 256 x 4), fused operator (jit.cpp: the sums over
# the same input and mask share a slot: 4 x 2 x 256 x 8 + (5 counts + the row count) x 256 x 4, 64 bytes of headroom)
MAX_EXACT_PLAIN = max_lowcard_groups_plain(5, 7)
MAX_EXACT_FUSED = max_lowcard_groups_fused(4, 5)
assert (MAX_EXACT_PLAIN, MAX_EXACT_FUSED) == ((160 * 1024) // (5 * 2 * 256 * 8 + 7 * 256 * 4), (160 * 1024 - 64) // (4 * 2 * 256 * 8 + 6 * 256 * 4))


def aggs_of(pkg):
    return [(pkg.SUM_DOUBLE, 1), (pkg.AVG_DOUBLE, 1), (pkg.SUM_DOUBLE, 2, 3), (pkg.AVG_DOUBLE, 2), (pkg.AVG_BIGINT, 4), (pkg.COUNT_ALL, -1),
            (pkg.COUNT_COLUMN, 2)]


def fused_spec(pkg):
    f = pkg.field
    B, D, BO = pkg.BIGINT, pkg.DOUBLE, pkg.BOOLEAN
    return [B, D, D, BO, B, D], f(5, D) < 0.9, [f(0, B), f(1, D), f(2, D), f(3, BO), f(4, B)]


def build(pkg, name, ngroups, path, seed):
    rng = np.random.default_rng(seed)
    sizes = page_sizes(path)
    n = sum(sizes)
    first_row = late_group_first_row(path, ngroups)
    gids, vals, nulls, mask, big, filt = make_stream(name, rng, ngroups, n, first_row=first_row, with_filter=path.startswith(("fused", "java_order_fused")))
    pages, at = [], 0
    B, D, BO = pkg.BIGINT, pkg.DOUBLE, pkg.BOOLEAN
    for m in sizes:
        s = slice(at, at + m)
        cols = [pkg.Block(B, gids[s]), pkg.Block(D, vals[s]), pkg.Block(D, vals[s], nulls[s]), pkg.Block(BO, mask[s]), pkg.Block(B, big[s])]
        if path.startswith(("fused", "java_order_fused")):
            cols.append(pkg.Block(D, filt[s]))
        pages.append(pkg.Page(*cols))
        at += m
    sel = filt < 0.9
    return pages, sizes, (gids[sel], vals[sel], nulls[sel], mask[sel], big[sel])


def expected(name_rows, ngroups, java=None):
    """{group: (sum, avg, masked sum, avg over the nullable column, avg(bigint), count(*), count(col))}"""
    gids, vals, nulls, mask, big = name_rows
    if java is None:
        cnt, s = exact_double_sum(vals, gids, ngroups)
        _, sm = exact_double_sum(vals, gids, ngroups, nulls=nulls, mask=mask)
        cn, sn = exact_double_sum(vals, gids, ngroups, nulls=nulls)
        _, sb = exact_double_sum(big.astype(np.float64), gids, ngroups)
    else:
        cnt, s = java.agg_double_sum(gids, vals, ngroups)
        _, sm = java.agg_double_sum(gids, vals, ngroups, nulls=nulls, mask=mask)
        cn, sn = java.agg_double_sum(gids, vals, ngroups, nulls=nulls)
        _, sb = java.agg_double_sum(gids, big.astype(np.float64), ngroups)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {g: (s[g], s[g] / cnt[g], sm[g], sn[g] / cn[g], sb[g] / cnt[g], int(cnt[g]), int(cn[g])) for g in range(ngroups)}


def check(rows, want, key_of=lambda r: r[0]):
    assert sorted(key_of(r) for r in rows) == sorted(want)
    bad = []
    for r in rows:
        w = want[key_of(r)]
        got = [np.nan if x is None else x for x in r[1:6]]
        if not bits_equal(got, list(w[:5])) or list(r[6:8]) != list(w[5:7]):
            bad.append((key_of(r), list(r[1:8]), list(w)))
    assert not bad, bad


CELLS = [(path, g) for path in PATHS for g in ([1] if path == "global" else [1, 3, "max"])]


@pytest.mark.parametrize("path,ngroups", CELLS)
@pytest.mark.parametrize("name", FAMILIES)
def test_double_sums_exact(pkg, oracle, monkeypatch, name, path, ngroups):
    if ngroups == "max":
        ngroups = MAX_EXACT_FUSED if is_fused(path) else MAX_EXACT_PLAIN
    seed = 3000 + 100 * FAMILIES.index(name) + ngroups
    pages, sizes, rows_in = build(pkg, name, ngroups, path, seed)
    want = expected(rows_in, ngroups, java=oracle if path.startswith("java_order") else None)
    got = drive(pkg, monkeypatch, path, ngroups, pages, aggs_of(pkg), fused_spec,
                partial_final=lambda ctx: partial_final(pkg, ctx, pages, sizes, rows_in, ngroups))
    if got.error is not None:
        raise got.error
    if path != "partial_final":                # (checked against its own partials in partial_final)
        check(got.rows, want)
    assert_profile(path, got.profile, ngroups)


def partial_final(pkg, ctx, pages, sizes, rows_in, ngroups):
    """each PARTIAL (one per page) equals the exact sums of its page; FINAL equals the exact sums of the rounded partials"""
    gids, vals, nulls, mask, big = rows_in
    partials, at = [], 0
    for out, m in zip(run_partials(pkg, ctx, [[pg] for pg in pages], ngroups, aggs_of(pkg)), sizes):
        s = slice(at, at + m)
        at += m
        cnt, sm = exact_double_sum(vals[s], gids[s], ngroups)
        cm, smm = exact_double_sum(vals[s], gids[s], ngroups, nulls=nulls[s], mask=mask[s])
        cn, sn = exact_double_sum(vals[s], gids[s], ngroups, nulls=nulls[s])
        _, sb = exact_double_sum(big[s].astype(np.float64), gids[s], ngroups)
        for r in [r for p in out for r in p.rows()]:
            g = r[0]
            # intermediate layout: key, (count, sum) x 5, count(*), count(col)
            assert list(r[1:12:2]) == [cnt[g], cnt[g], cm[g], cn[g], cnt[g], cnt[g]] and r[12] == cn[g], (g, r)
            assert bits_equal([r[2], r[4], r[8], r[10]], [sm[g], sm[g], sn[g], sb[g]]), (g, r, sm[g], sn[g], sb[g])
            if cm[g]:
                assert bits_equal(r[6], smm[g]), (g, r, smm[g])
        partials += out
    assert final_aggs(pkg, aggs_of(pkg)) == [(pkg.SUM_DOUBLE, 1), (pkg.AVG_DOUBLE, 3), (pkg.SUM_DOUBLE, 5), (pkg.AVG_DOUBLE, 7), (pkg.AVG_BIGINT, 9),
                                             (pkg.COUNT_ALL, 11), (pkg.COUNT_COLUMN, 12)]
    rows = run_final(pkg, ctx, partials, ngroups, aggs_of(pkg))
    inter = [r for p in partials for r in p.rows()]
    ig = np.array([r[0] for r in inter], dtype=np.int64)

    def col(i):
        return np.array([0.0 if r[i] is None else r[i] for r in inter], dtype=np.float64)

    def cnts(i):
        return np.array([r[i] for r in inter], dtype=np.int64)

    live_m = (cnts(5) > 0).astype(np.uint8)
    s, a1, sm2, a2, ab = (exact_double_sum(col(i), ig, ngroups, mask=live_m if i == 6 else None)[1] for i in (2, 4, 6, 8, 10))
    c1 = np.bincount(ig, weights=cnts(3), minlength=ngroups)
    c2 = np.bincount(ig, weights=cnts(7), minlength=ngroups)
    cb = np.bincount(ig, weights=cnts(9), minlength=ngroups)
    want = {g: (s[g], a1[g] / c1[g], sm2[g], a2[g] / c2[g], ab[g] / cb[g], int(np.bincount(ig, weights=cnts(11), minlength=ngroups)[g]),
                int(np.bincount(ig, weights=cnts(12), minlength=ngroups)[g])) for g in range(ngroups)}
    check(rows, want)
    return rows

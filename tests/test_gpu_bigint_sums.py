"""sum(bigint) at the int64 edges on every path that adds in 128 bits (tests/bigint_sum_cases.py x tests/agg_paths.py): only a group's
total decides -- the exact total, or NUMERIC_VALUE_OUT_OF_RANGE (-2) for the whole drive when a total leaves int64.  One operator holds
sum(big), avg(big) (same input: its 16-byte state is a DOUBLE sum, not the integer words), sum(big, mask), sum(big_nullable), min(big),
count(big_nullable), count(*).  Sums, min and counts are compared as ints with the Python-int reference; avg(bigint) bit for bit with
the exact sum of the (double) values / count -- in the row-order paths with the Java-order oracle, as test_gpu_double_sums_exact.py does."""
import numpy as np
import pytest

from agg_paths import (FUSED_GENERAL, ORDERED_GROUPS, ORDERED_PATHS, PARTIAL_FINAL_MANY, PATHS, assert_folded, assert_profile, drive, final_aggs, is_fused, late_group_first_row,
                       max_lowcard_groups_fused, max_lowcard_groups_plain, page_sizes, run_final, run_partials, run_plain)
from bigint_sum_cases import FAMILIES, FILTER_BELOW, RAISES, VARIANTS, heavy_group, make_stream, narrow, reference
from exact_sum import bits_equal, exact_double_sum

pytestmark = pytest.mark.gpu

# the most groups that still take the lane-private path with this aggregate list: 160 KiB of LDS / the bytes of one group's lane-private
# states.  Plain operator (agg.hip lowcard_bytes_per_group): 4 wide states (three sum(bigint), one avg(bigint); min and the counts have
# none) x 2 words x 256 lanes x 8 bytes + 7 counts x 256 x 4 = 23 552 bytes -> 6 groups.  Fused operator (jit.cpp): no two of the four
# share a pair -- sum(big) and avg(big) read the same input but are of different kinds --, the counts over (big), (big, mask),
# (big_nullable) and () are 4, plus the row count: 4 x 2 x 256 x 8 + 5 x 256 x 4 = 21 504 bytes, 64 bytes of headroom -> 7 groups.
MAX_LANE_PRIVATE_PLAIN = max_lowcard_groups_plain(4, 7)
MAX_LANE_PRIVATE_FUSED = max_lowcard_groups_fused(4, 4)
assert (MAX_LANE_PRIVATE_PLAIN, MAX_LANE_PRIVATE_FUSED) == (6, 7)


def aggs_of(pkg):
    return [(pkg.SUM_BIGINT, 1), (pkg.AVG_BIGINT, 1), (pkg.SUM_BIGINT, 1, 3), (pkg.SUM_BIGINT, 2), (pkg.MIN_BIGINT, 1), (pkg.COUNT_COLUMN, 2),
            (pkg.COUNT_ALL, -1)]


def fused_spec(pkg):
    """(the same for every family: one generated kernel set per path, compiled once)"""
    f = pkg.field
    B, D, BO = pkg.BIGINT, pkg.DOUBLE, pkg.BOOLEAN
    return [B, B, B, BO, D], f(4, D) < FILTER_BELOW, [f(0, B), f(1, B), f(2, B), f(3, BO)]


def build(pkg, name, variant, ngroups, path, seed):
    rng = np.random.default_rng(seed)
    sizes = page_sizes(path)
    cuts = np.cumsum(sizes)[:-1].tolist()
    fused = is_fused(path)
    heavy = heavy_group(name, ngroups, variant) if path.endswith("handoff") else None      # a tenth of the rows: more than kOrdHandoffRows in each page
    s = make_stream(name, rng, ngroups, sum(sizes), first_row=late_group_first_row(path, ngroups), with_filter=fused, variant=variant, cuts=cuts, heavy=heavy)
    pages, at = [], 0
    B = pkg.BIGINT
    for m in sizes:
        z = slice(at, at + m)
        cols = [pkg.Block(B, s.gids[z]), pkg.Block(B, s.big[z]), pkg.Block(B, s.big_nullable[z], s.big_nulls[z]), pkg.Block(pkg.BOOLEAN, s.mask_values[z], s.mask_nulls[z])]
        if fused:
            cols.append(pkg.Block(pkg.DOUBLE, s.filt[z]))
        pages.append(pkg.Page(*cols))
        if heavy is not None:
            # what gives the hand-off teeth (its launch alone proves nothing: it is made for every page of 4 096 rows): in this page the
            # heavy group has more selected rows than a lane walks (agg.h kOrdHandoffRows), with special rows before and after that point
            rows = at + np.nonzero((s.gids[z] == heavy) & (s.filt[z] < FILTER_BELOW))[0]
            assert len(rows) > 4096 + 256 and s.special[rows[:4096]].any() and s.special[rows[4096:]].any(), (name, len(rows))
        at += m
    return pages, sizes, s


def avg_of(s, ngroups, rows, java):
    """avg(bigint)'s sum per group over the selected rows: the exact sum of the (double) values, or the row-order sum"""
    keep = s.filt < FILTER_BELOW
    if rows is not None:
        only = np.zeros(len(keep), dtype=bool)
        only[rows] = True
        keep &= only
    vals = s.big[keep].astype(np.float64)
    if java is not None:
        return java.agg_double_sum(s.gids[keep], vals, ngroups)[1]
    return exact_double_sum(vals, s.gids[keep], ngroups)[1]


def expected_rows(s, ngroups, java=None):
    """{group: (sum, avg, masked sum, sum over the nullable column, min, count(col), count(*))} of the groups with a row, or RAISES"""
    ref = reference(s, ngroups)
    if ref.raises():
        return RAISES
    sb = avg_of(s, ngroups, None, java)
    out = {}
    for g in range(ngroups):
        if ref.count_all[g]:
            out[g] = (ref.sums[g], float(sb[g]) / ref.count_all[g], ref.sums_masked[g] if ref.count_masked[g] else None,
                      ref.sums_nullable[g] if ref.count_nullable[g] else None, ref.mins[g], ref.count_nullable[g], ref.count_all[g])
    return out


def check(rows, want):
    assert sorted(r[0] for r in rows) == sorted(want)
    bad = []
    for r in rows:
        w = want[r[0]]
        ints = [r[1], r[3], r[4], r[5], r[6], r[7]]
        if ints != [w[0], w[2], w[3], w[4], w[5], w[6]] or not bits_equal(r[2], w[1]) or any(isinstance(x, float) for x in ints):
            bad.append((r[0], list(r[1:8]), list(w)))
    assert not bad, bad[:4]


def cells():
    out = []
    for path in PATHS + (FUSED_GENERAL,):
        for g in ([1] if path == "global" else [1, 3, "max"]):
            out.append((path, g))
    for path in ORDERED_PATHS + (PARTIAL_FINAL_MANY,):
        out.append((path, ORDERED_GROUPS[path.rsplit("_", 1)[1]]))
    return out


def cases():
    """every family down every path; total_past_limit's position of the overflowing group runs over first / middle / last where a
    path has more than one group, and its no-raise variant everywhere"""
    out = []
    for name in FAMILIES:
        for path, g in cells():
            for variant in VARIANTS[name]:
                if g == 1 and variant in ("middle", "last") and path != "lowcard":    # (one group: the same case, kept once for the underflow)
                    continue
                out.append(pytest.param(name, variant, path, g, id="-".join(str(x) for x in (name, variant, path, g) if x is not None)))
    return out


@pytest.mark.parametrize("name,variant,path,ngroups", cases())
def test_bigint_sums(pkg, oracle, monkeypatch, name, variant, path, ngroups):
    if ngroups == "max":
        ngroups = MAX_LANE_PRIVATE_FUSED if is_fused(path) else MAX_LANE_PRIVATE_PLAIN
    seed = 5000 + 100 * FAMILIES.index(name) + 17 * VARIANTS[name].index(variant) + ngroups % 97
    pages, sizes, s = build(pkg, name, variant, ngroups, path, seed)
    row_order = path.startswith("java_order") or path in ORDERED_PATHS
    split = path in ("partial_final", PARTIAL_FINAL_MANY)
    want = None if split else expected_rows(s, ngroups, java=oracle if row_order else None)
    if path == "spilled" and name in ("extremes_cancel", "high_halves"):
        # the revokes fall at the page cuts: the first run's state of some group has a high word that is neither 0 nor ~0
        assert any((t >> 64) not in (0, -1) for t in reference(s, ngroups, rows=np.arange(0, sizes[0])).sums) and want != RAISES
    got = drive(pkg, monkeypatch, path, ngroups, pages, aggs_of(pkg), fused_spec,
                partial_final=lambda ctx: partial_final(pkg, ctx, pages, sizes, s, ngroups, name, variant, oracle if path == PARTIAL_FINAL_MANY else None))
    if split:                                  # (its expectation depends on the split: every raise is expected and caught in partial_final)
        if got.error is not None:
            raise got.error
    elif want == RAISES:
        assert got.rows is None and got.error is not None and got.error.code == -2, (got.error, got.rows and got.rows[:3])
    else:
        if got.error is not None:
            raise got.error
        check(got.rows, want)
    assert_profile(path, got.profile, ngroups)
    assert_folded(path, got.profile)


def partial_final(pkg, ctx, pages, sizes, s, ngroups, name, variant, java):
    """Two PARTIAL operators over disjoint page sets (the first page; the other two), then one FINAL; with many groups (java: the
    row-order oracle for avg's sums) one PARTIAL per page, eight of them, and FINAL in row order -- agg_ordered_kernel<INTERMEDIATE>, whose
    __int128 takes up to eight int64 partials per group.  A PARTIAL narrows its own total to int64 -- the reference behaves the same here: its intermediate state is a `long`
    -- so the expectation follows the actual split: a partial whose own group total leaves int64 raises -2 (even when the overall total
    is small; extremes_cancel, high_halves and high_word_only always end here: a page of theirs holds 2^63 or more of one sign -- FINAL
    meets their addends in test_final_over_edge_partials); otherwise each
    partial's intermediate row is exact, and FINAL returns the exact total of the partials or raises -2 (each partial in range, their
    sum not)."""
    aggs = aggs_of(pkg)
    cut = sizes[0]
    n = sum(sizes)
    if java is None:
        sets = [(pages[:1], np.arange(0, cut)), (pages[1:], np.arange(cut, n))]
    else:
        ends = np.cumsum(sizes)
        sets = [([pg], np.arange(e - m, e)) for pg, m, e in zip(pages, sizes, ends)]
    refs = [reference(s, ngroups, rows=rows) for _, rows in sets]
    whole = reference(s, ngroups)
    # both kinds of split occur in the streams of this file, whatever else does
    if name == "total_past_limit" and variant != "excluded":
        assert not any(ref.raises() for ref in refs) and whole.raises()             # every partial fits, their sum does not: FINAL raises
    if name == "extremes_cancel":
        assert any(ref.raises() for ref in refs) and not whole.raises()             # a partial does not fit, the total is small: it raises
    partials = []
    for (pgs, rows), ref in zip(sets, refs):
        if ref.raises():
            with pytest.raises(pkg.TgpuError) as e:
                run_partials(pkg, ctx, [pgs], ngroups, aggs)
            assert e.value.code == -2
            continue
        out = run_partials(pkg, ctx, [pgs], ngroups, aggs)[0]
        sb = avg_of(s, ngroups, rows, java)
        got = {r[0]: r for p in out for r in p.rows()}
        assert sorted(got) == [g for g in range(ngroups) if ref.count_all[g]]
        for g, r in got.items():
            # intermediate layout: key, (count, sum) of sum / avg / masked sum / nullable sum / min, count(col), count(*)
            assert list(r[1:11:2]) == [ref.count_all[g], ref.count_all[g], ref.count_masked[g], ref.count_nullable[g], ref.count_all[g]], (g, r)
            assert list(r[11:13]) == [ref.count_nullable[g], ref.count_all[g]], (g, r)
            assert [r[2], r[10]] == [ref.sums[g], ref.mins[g]] and bits_equal(r[4], sb[g]), (g, r, ref.sums[g], sb[g])
            assert (not ref.count_masked[g] or r[6] == ref.sums_masked[g]) and (not ref.count_nullable[g] or r[8] == ref.sums_nullable[g]), (g, r)
        partials += out
    if any(ref.raises() for ref in refs):
        return None
    assert final_aggs(pkg, aggs) == [(pkg.SUM_BIGINT, 1), (pkg.AVG_BIGINT, 3), (pkg.SUM_BIGINT, 5), (pkg.SUM_BIGINT, 7), (pkg.MIN_BIGINT, 9),
                                     (pkg.COUNT_COLUMN, 11), (pkg.COUNT_ALL, 12)]
    combine = "agg_combine" if java is None else "agg_combine_ordered"              # the FINAL step's kernel: per-row atomics | row order
    if whole.raises():
        with pytest.raises(pkg.TgpuError) as e:
            run_final(pkg, ctx, partials, ngroups, aggs)
        assert e.value.code == -2
        assert combine in ctx.profile(), sorted(ctx.profile())
        return None
    rows = run_final(pkg, ctx, partials, ngroups, aggs)
    assert combine in ctx.profile(), sorted(ctx.profile())
    inter = [r for p in partials for r in p.rows()]
    ig = np.array([r[0] for r in inter], dtype=np.int64)
    iv = np.array([r[4] for r in inter], dtype=np.float64)
    # avg: the exact sum of the rounded partials, or their sum in the order FINAL receives them
    sb = exact_double_sum(iv, ig, ngroups)[1] if java is None else java.agg_double_sum(ig, iv, ngroups)[1]
    want = {}
    for g in range(ngroups):
        if whole.count_all[g]:
            want[g] = (whole.sums[g], float(sb[g]) / whole.count_all[g], whole.sums_masked[g] if whole.count_masked[g] else None,
                       whole.sums_nullable[g] if whole.count_nullable[g] else None, whole.mins[g], whole.count_nullable[g], whole.count_all[g])
    check(rows, want)
    return rows


FINAL_CASES = [(name, variant) for name in FAMILIES for variant in VARIANTS[name] if variant in (None, "middle", "excluded")]


@pytest.mark.parametrize("ngroups", [3, ORDERED_GROUPS["many"]])
@pytest.mark.parametrize("name,variant", FINAL_CASES)
def test_final_over_edge_partials(pkg, name, variant, ngroups):
    """The FINAL step alone, fed intermediate pages that no PARTIAL of this product could have narrowed: every selected row of a family
    is a partial state (count 1, sum = the addend), a null row is an EMPTY partial state (count 0) whose sum column holds extreme bytes
    and must be skipped.  Few groups: agg_combine (tg_i128_add per partial); many: agg_combine_ordered (agg_ordered_kernel<INTERMEDIATE>,
    `__int128 big += input2`), hundreds or thousands of partials per special group, totals of 2^64 and beyond included."""
    many = ngroups > 8
    sizes = page_sizes("ordered_many" if many else "lowcard_multi")
    rng = np.random.default_rng(7000 + 100 * FAMILIES.index(name) + 17 * VARIANTS[name].index(variant) + ngroups % 97)
    s = make_stream(name, rng, ngroups, sum(sizes), variant=variant, cuts=np.cumsum(sizes)[:-1].tolist())
    ref = reference(s, ngroups)
    ones = np.ones(len(s.gids), dtype=np.int64)
    live = (s.big_nulls == 0).astype(np.int64)
    B = pkg.BIGINT
    pages, at = [], 0
    for m in sizes:
        z = slice(at, at + m)
        pages.append(pkg.Page(pkg.Block(B, s.gids[z]), pkg.Block(B, ones[z]), pkg.Block(B, s.big[z]), pkg.Block(B, live[z]), pkg.Block(B, s.big_nullable[z]),
                              pkg.Block(B, ones[z])))
        at += m
    aggs = [(pkg.SUM_BIGINT, 1), (pkg.SUM_BIGINT, 3), (pkg.COUNT_ALL, 5)]
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    rows = error = None
    try:
        try:
            rows = run_plain(pkg, ctx, pages, ngroups, aggs, step=pkg.FINAL)
        except pkg.TgpuError as e:
            error = e
        prof = ctx.profile()
    finally:
        ctx.close()
    assert ("agg_combine_ordered" if many else "agg_combine") in prof and ("agg_combine" if many else "agg_combine_ordered") not in prof, sorted(prof)
    if any(narrow(t) == RAISES for t in ref.sums + ref.sums_nullable):
        assert rows is None and error is not None and error.code == -2, (error, rows and rows[:3])
        return
    if error is not None:
        raise error
    want = {g: (ref.sums[g], ref.sums_nullable[g] if ref.count_nullable[g] else None, ref.count_all[g]) for g in range(ngroups) if ref.count_all[g]}
    assert {r[0]: tuple(r[1:]) for r in rows} == want

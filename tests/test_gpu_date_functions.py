"""The DATE functions on the device (jit.cpp gen_date, csrc/device_date.h) against tests/date_fn_expected.py: every cell is compared, on the
flat, dictionary, run-length, fused-aggregation and fused-probe paths.  About a dozen projections share a program, so the file compiles a
few dozen kernels."""
import json
import os

import numpy as np
import pytest

import date_fn_cases as C
import date_fn_expected as X
import expr_harness as H

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "date_function_vectors.json")))
RANGE = -2


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


def project(pkg, ctx, types, filt, exprs, page):
    """-> one list per projection over all output pages"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs)
    op = fac.createOperator()
    outs = pkg.to_pages(op, [page])
    op.close()
    fac.close()
    return [[v for o in outs for v in o.getBlock(k).to_list()] for k in range(len(exprs))]


def failure(pkg, ctx, types, filt, exprs, page):
    """-> (code, position) of the error the page raises, or None"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs)
    op = fac.createOperator()
    outs, err = H.drive_pages(pkg, op, [page])
    op.close()
    fac.close()
    return None if err is None else (err[0].code, err[2])


def unary_exprs(pkg, d, last):
    return [pkg.year(d), pkg.quarter(d), pkg.month(d), pkg.week(d), pkg.day(d), pkg.day_of_week(d), pkg.day_of_year(d), pkg.year_of_week(d), pkg.last_day_of_month(last)]


def unary_want(days, last_days):
    rows = [None if d is None else X.unary_row(d) for d in days]
    return [[None if r is None else r[k] for r in rows] for k in range(8)] + [[X.last_day_of_month(d) for d in last_days]]


def no_last_day(days):
    """the days whose month ends past the last int32 day become NULL"""
    return [None if d is not None and X.unary_row(d)[8] is None else d for d in days]


def unit_exprs(pkg, d, k, e):
    """date_trunc, date_add, date_diff for each of the five units: 15 projections"""
    return [g(u, *a) for u in X.UNITS for g, a in ((pkg.date_trunc, (d,)), (pkg.date_add, (k, d)), (pkg.date_diff, (d, e)))]


# ---- (1) the reference's pinned cases -----------------------------------------------------------------------------------------------
def golden_exprs(pkg):
    """every golden case as an expression over constants -> [(expression, expected)]"""
    D = pkg.DATE
    c = lambda day: pkg.constant(day, D)
    fn = {n: getattr(pkg, n) for n in X.UNARY_NAMES}
    out, seen = [], set()
    for g in GOLD["extract"]:
        if (g["function"], g["day"]) not in seen:          # EXTRACT(f FROM d) and f(d) are one expression here
            seen.add((g["function"], g["day"]))
            out.append((fn[g["function"]](c(g["day"])), g["expected"]))
    out += [(pkg.last_day_of_month(c(g["day"])), g["expected"]) for g in GOLD["last_day_of_month"]]
    out += [(pkg.date_trunc(g["unit"], c(g["day"])), g["expected"]) for g in GOLD["date_trunc"]]
    out += [(pkg.date_add(g["unit"], g["value"], c(g["day"])), g["expected"]) for g in GOLD["date_add"]]
    out += [(pkg.date_diff(g["unit"], c(g["day1"]), c(g["day2"])), g["expected"]) for g in GOLD["date_diff"]]
    return out


def test_golden_cases_as_constants(pkg, ctx):
    cases = golden_exprs(pkg)
    assert len(cases) > 40
    page = pkg.Page(pkg.Block(pkg.BIGINT, [0]))
    for at in range(0, len(cases), 16):
        part = cases[at:at + 16]
        got = project(pkg, ctx, [pkg.BIGINT], None, [e for e, _ in part], page)
        assert got == [[w] for _, w in part], at


def test_golden_cases_as_column_values(pkg, ctx):
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    cases = GOLD["extract"] + GOLD["last_day_of_month"]
    days = [g["day"] for g in cases]
    got = project(pkg, ctx, [D], None, unary_exprs(pkg, f(0, D), f(0, D)), pkg.Page(pkg.Block(D, days)))
    assert got == unary_want(days, days)
    for r, g in enumerate(cases):
        assert got[X.UNARY_NAMES.index(g.get("function", "last_day_of_month"))][r] == g["expected"], g
    # date_trunc / date_add / date_diff: one row per case, the case's unit picks the projection
    rows = [(g["day"], 0, 0, 3 * X.UNITS.index(g["unit"]), g) for g in GOLD["date_trunc"]]
    rows += [(g["day"], g["value"], 0, 3 * X.UNITS.index(g["unit"]) + 1, g) for g in GOLD["date_add"]]
    rows += [(g["day1"], 0, g["day2"], 3 * X.UNITS.index(g["unit"]) + 2, g) for g in GOLD["date_diff"]]
    page = pkg.Page(pkg.Block(D, [r[0] for r in rows]), pkg.Block(B, [r[1] for r in rows]), pkg.Block(D, [r[2] for r in rows]))
    got = project(pkg, ctx, [D, B, D], None, unit_exprs(pkg, f(0, D), f(1, B), f(2, D)), page)
    for r, (_, _, _, ch, g) in enumerate(rows):
        assert got[ch][r] == g["expected"], g


# ---- (2) the edge page at each row count ----------------------------------------------------------------------------------------------
def edge_pages():
    """(n, days): the edge rows from a different start for each row count, and the whole list"""
    rows = C.edge_rows()
    return [(n, C.cycle(rows[::-1] if n == 1 else rows, n, start=0 if n == 1 else 5 * n)) for n in C.ROW_COUNTS] + [(len(rows), rows)]


def test_edge_page_unary_ops_every_row_count(pkg, ctx):
    f, D = pkg.field, pkg.DATE
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D, D], None, unary_exprs(pkg, f(0, D), f(1, D)))
    for n, days in edge_pages():
        last = no_last_day(days)
        outs = pkg.to_pages(fac.createOperator(), [pkg.Page(pkg.Block(D, days), pkg.Block(D, last))])
        got = [[v for o in outs for v in o.getBlock(k).to_list()] for k in range(9)]
        assert got == unary_want(days, last), n
    assert edge_pages()[0][1] == [X.INT32_MAX] and len(edge_pages()[-1][1]) > 300


FILTERS = {
    "year_is_1995": (lambda pkg, d: pkg.year(d).eq(1995), lambda d: X.year(d) == 1995),
    "weekend": (lambda pkg, d: pkg.in_(pkg.day_of_week(d), [6, 7]), lambda d: X.day_of_week(d) in (6, 7)),
    "week_52_or_53": (lambda pkg, d: pkg.between(pkg.week(d), 52, 53), lambda d: 52 <= X.week(d) <= 53),
}


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_edge_page_filters_every_row_count(pkg, ctx, name):
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    build, keeps = FILTERS[name]
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D, B], build(pkg, f(0, D)), [f(1, B), f(0, D)])
    in_1995 = [X.to_days(1995, 1, 1), X.to_days(1995, 12, 31), X.to_days(1994, 12, 31), None, X.to_days(1996, 1, 1), X.to_days(1995, 6, 15)]
    total = 0
    for n, days in edge_pages():
        days = (in_1995 + days)[:n] if n > 1 else [in_1995[0]]
        outs = pkg.to_pages(fac.createOperator(), [pkg.Page(pkg.Block(D, days), pkg.Block(B, np.arange(len(days), dtype=np.int64)))])
        got = [[v for o in outs for v in o.getBlock(k).to_list()] for k in range(2)]
        sel = [r for r, d in enumerate(days) if d is not None and keeps(d)]
        assert got == [sel, [days[r] for r in sel]], n
        total += len(sel)
    assert total > 5


# ---- (3) date_trunc, date_add, date_diff: the amount from a BIGINT column, the dates from two columns ------------------------------------
def checked(call):
    try:
        return call()
    except X.OutOfRange:
        return X.OutOfRange


@pytest.mark.parametrize("unit", X.UNITS)
def test_trunc_add_diff_over_columns(pkg, ctx, unit):
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    days = C.edge_days()
    rows = []
    for i, d in enumerate(days):
        for j, v in enumerate(C.AMOUNTS):
            e = days[(i * 31 + j * 7) % len(days)]
            rows.append((d, v, e))
            if (i + j) % 5 == 0:
                rows.append((None if j % 3 == 0 else d, None if j % 3 == 1 else v, None if j % 3 == 2 else e))
    want = [[checked(lambda: X.date_trunc(unit, d)) for d, v, e in rows], [checked(lambda: X.date_add(unit, v, d)) for d, v, e in rows],
            [X.date_diff(unit, d, e) for d, v, e in rows]]
    # a page raises when one cell overflows: the value pages hold the rows that do not, the others are counted here and raised in (4)
    clean = [r for r in range(len(rows)) if want[0][r] is not X.OutOfRange and want[1][r] is not X.OutOfRange]
    assert len(rows) > 4000 and len(rows) // 2 < len(clean) < len(rows)
    d, k, e = f(0, D), f(1, B), f(2, D)
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D, B, D], None, [pkg.date_trunc(unit, d), pkg.date_add(unit, k, d), pkg.date_diff(unit, d, e)])
    for n in C.ROW_COUNTS + [len(clean)]:
        part = clean[:n] if n == len(clean) else clean[3 * n:4 * n]
        page = pkg.Page(pkg.Block(D, [rows[r][0] for r in part]), pkg.Block(B, [rows[r][1] for r in part]), pkg.Block(D, [rows[r][2] for r in part]))
        outs = pkg.to_pages(fac.createOperator(), [page])
        got = [[v for o in outs for v in o.getBlock(ch).to_list()] for ch in range(3)]
        assert got == [[w[r] for r in part] for w in want], (unit, n)


# ---- (4) errors --------------------------------------------------------------------------------------------------------------------------
def test_overflow_errors(pkg, ctx):
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    d, k = f(0, D), f(1, B)
    n = 300
    days = [X.to_days(1995, 1, 1) + r for r in range(n)]
    page = lambda ds, ks: pkg.Page(pkg.Block(D, ds), pkg.Block(B, ks))
    one = lambda at, v: [v if r == at else 1 for r in range(n)]
    # a page whose only failing cell is one date_add, for each way of overflowing
    for unit, at, v, day in (("day", 257, 1, X.INT32_MAX), ("day", 3, 2**31, 0), ("week", 64, -(2**31 - 1), 0), ("month", 299, 2**31 - 1, 0), ("year", 0, -2**31 - 1, 0),
                             ("quarter", 130, 3, X.INT32_MAX - 40), ("month", 200, -1, X.INT32_MIN + 3), ("year", 63, 2**62, 0)):
        ds = [day if r == at else x for r, x in enumerate(days)]
        assert checked(lambda: X.date_add(unit, v, day)) is X.OutOfRange
        assert failure(pkg, ctx, [D, B], None, [d, pkg.date_add(unit, k, d)], page(ds, one(at, v))) == (RANGE, at), (unit, v)
        # a NULL amount or a NULL date on the otherwise overflowing row gives NULL, not an error
        for nd, nk in ((ds, one(at, None)), ([None if r == at else x for r, x in enumerate(ds)], one(at, v))):
            got = project(pkg, ctx, [D, B], None, [pkg.date_add(unit, k, d)], page(nd, nk))
            assert got == [[X.date_add(unit, b, a) for a, b in zip(nd, nk)]] and got[0][at] is None
    # date_trunc and last_day_of_month at the ends of the range
    ds = [X.INT32_MIN + 2 if r == 77 else x for r, x in enumerate(days)]
    assert failure(pkg, ctx, [D, B], None, [pkg.date_trunc("week", d), pkg.date_trunc("month", d)], page(ds, one(0, 1))) == (RANGE, 77)
    ds[77] = X.INT32_MIN + 8                                     # a Wednesday; the first Monday of the range is day -2^31 + 6
    assert project(pkg, ctx, [D, B], None, [pkg.date_trunc("week", d)], page(ds, one(0, 1)))[0][77] == X.INT32_MIN + 6
    ds = [X.INT32_MAX - 10 if r == 5 else x for r, x in enumerate(days)]
    assert failure(pkg, ctx, [D, B], None, [pkg.year(d), pkg.last_day_of_month(d)], page(ds, one(0, 1))) == (RANGE, 5)
    # two failing projections and rows: the lowest projection index, then its first row
    ds = list(days)
    ds[9], ds[12], ds[2] = X.INT32_MAX, X.INT32_MAX - 1, X.INT32_MIN
    ks = [5] * n
    exprs = [pkg.year(d), pkg.date_add("day", k, d), pkg.date_add("month", -1, d)]
    assert failure(pkg, ctx, [D, B], None, exprs, page(ds, ks)) == (RANGE, 9)                # projection 1 fails on rows 9 and 12, projection 2 on row 2
    assert failure(pkg, ctx, [D, B], None, [exprs[0], exprs[2], exprs[1]], page(ds, ks)) == (RANGE, 2)
    # the filter rejects the failing rows: nothing is raised
    got = project(pkg, ctx, [D, B], pkg.between(pkg.year(d), 1995, 1996), exprs, page(ds, ks))
    keep = [r for r in range(n) if r not in (9, 12, 2)]
    assert got == [[X.year(ds[r]) for r in keep], [ds[r] + 5 for r in keep], [X.date_add("month", -1, ds[r]) for r in keep]]


# ---- (5) DICTIONARY and RLE input blocks ---------------------------------------------------------------------------------------------------
def test_dictionary_and_rle_inputs(pkg, ctx):
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    entries = [X.to_days(2000, 2, 29), X.to_days(1999, 12, 31), None, X.INT32_MIN + 400, X.to_days(2004, 12, 31), X.to_days(0, 1, 1), X.INT32_MAX - 400]
    rng = np.random.default_rng(4)
    n = 1000
    ids = rng.integers(0, len(entries), n).astype(np.int32)
    days = [entries[i] for i in ids]
    ks = [None if r % 17 == 0 else r % 25 - 12 for r in range(n)]
    d, k = f(0, D), f(1, B)
    exprs = unary_exprs(pkg, d, d) + [pkg.date_add("month", k, d), pkg.date_trunc("quarter", pkg.date_add("day", 40, d)), pkg.date_diff("week", d, pkg.constant(0, D))]
    want = unary_want(days, days) + [[X.date_add("month", b, a) for a, b in zip(days, ks)], [X.date_trunc("quarter", X.date_add("day", 40, a)) for a in days],
                                     [X.date_diff("week", a, 0) for a in days]]
    amounts = pkg.Block(B, ks)
    got = project(pkg, ctx, [D, B], None, exprs, pkg.Page(pkg.DictionaryBlock(pkg.Block(D, entries), ids), amounts))
    assert got == want
    assert got == project(pkg, ctx, [D, B], None, exprs, pkg.Page(pkg.Block(D, days), amounts))
    # one column: the dictionary-aware path evaluates once per entry.  Then with an entry that no row refers to and whose month ends past
    # the range: it raises nothing
    single = unary_exprs(pkg, d, d) + [pkg.date_trunc("year", d)]
    ids = np.array([0, 3, 2, 0, 3, 3, 2, 0] * 40, dtype=np.int32)
    for unused in (X.to_days(1997, 7, 7), X.INT32_MAX):
        small = [X.to_days(1995, 3, 1), unused, None, X.to_days(1996, 2, 29)]
        op = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D], pkg.year(d) > 1994, single).createOperator()
        outs = pkg.to_pages(op, [pkg.Page(pkg.DictionaryBlock(pkg.Block(D, small), ids))])
        if unused != X.INT32_MAX:
            assert pkg._lib.lib().tgpu_debug_dictionary_pages(op.handle) == 1
        kept = [small[i] for i in ids if small[i] is not None]
        assert [[v for o in outs for v in o.getBlock(ch).to_list()] for ch in range(10)] == unary_want(kept, kept) + [[X.date_trunc("year", a) for a in kept]]
    for value in (X.to_days(2020, 12, 31), None):
        page = pkg.Page(pkg.RunLengthEncodedBlock(pkg.Block(D, [value]), 257), pkg.Block(B, ks[:257]))
        assert project(pkg, ctx, [D, B], None, exprs, page) == unary_want([value] * 257, [value] * 257) + [
            [X.date_add("month", b, value) for b in ks[:257]], [X.date_trunc("quarter", X.date_add("day", 40, value))] * 257, [X.date_diff("week", value, 0)] * 257]


# ---- (6) compositions ----------------------------------------------------------------------------------------------------------------------
def test_compositions(pkg, ctx):
    f, c, D, B, V = pkg.field, pkg.constant, pkg.DATE, pkg.BIGINT, pkg.VARCHAR
    days = [d for d in C.edge_rows() if d is None or -3 * 146097 <= d <= 3 * 146097]
    n = len(days)
    ks = [None if r % 11 == 5 else (r * 37) % 61 - 30 for r in range(n)]
    d, k = f(0, D), f(1, B)
    year_start = pkg.date_trunc("year", d)
    exprs = [pkg.year(pkg.date_add("month", k, d)),
             pkg.date_diff("day", year_start, d) + 1, pkg.day_of_year(d),
             pkg.if_(pkg.day_of_week(d) > 5, pkg.date_trunc("week", d), pkg.last_day_of_month(d)),
             pkg.coalesce(pkg.date_add("day", k, d), pkg.date_trunc("month", d), c(0, D)),
             pkg.date_trunc(c(None, V), d), pkg.date_add(None, k, d), pkg.date_diff(None, d, d),
             pkg.is_null(pkg.date_add(None, k, d)),
             pkg.date_diff("month", pkg.date_add("month", k, d), d),
             pkg.month(pkg.coalesce(d, c(X.to_days(1970, 7, 4), D))),
             pkg.date_add("year", pkg.year(d) - pkg.year_of_week(d), pkg.date_trunc("QUARTER", d))]
    got = project(pkg, ctx, [D, B], None, exprs, pkg.Page(pkg.Block(D, days), pkg.Block(B, ks)))

    def row(a, b):
        plus = X.date_add("day", b, a)
        moved = X.date_add("month", b, a)
        return (X.year(moved), None if a is None else X.date_diff("day", X.date_trunc("year", a), a) + 1, X.day_of_year(a),
                None if a is None else (X.date_trunc("week", a) if X.day_of_week(a) > 5 else X.last_day_of_month(a)),
                plus if plus is not None else X.date_trunc("month", a) if a is not None else 0,
                None, None, None, True,
                X.date_diff("month", moved, a),
                X.month(a if a is not None else X.to_days(1970, 7, 4)),
                None if a is None else X.date_add("year", X.year(a) - X.year_of_week(a), X.date_trunc("quarter", a)))
    want = [list(col) for col in zip(*[row(a, b) for a, b in zip(days, ks)])]
    for ch, w in enumerate(want):
        assert got[ch] == w, ch
    assert got[1] == got[2] and sum(v is not None for v in got[1]) > 150           # date_diff('day', date_trunc('year', d), d) + 1 = day_of_year(d)
    assert {-1, 0, 1} <= {X.year(a) - X.year_of_week(a) for a in days if a is not None}


# ---- (7) the fused paths --------------------------------------------------------------------------------------------------------------------
def tpch_rows(n=1000):
    rng = np.random.default_rng(12)
    first, last = X.to_days(1992, 1, 1), X.to_days(1998, 12, 31)
    days = [None if r % 43 == 7 else int(v) for r, v in enumerate(rng.integers(first, last, n, endpoint=True))]
    return days, rng.integers(-1000, 1000, n).astype(np.int64)


def pages_of(pkg, days, vals, size=257):
    return [pkg.Page(pkg.Block(pkg.DATE, days[a:a + size]), pkg.Block(pkg.BIGINT, vals[a:a + size])) for a in range(0, len(days), size)]


def in_order(rows):
    return sorted(rows, key=lambda r: tuple((v is None, 0 if v is None else v) for v in r))


@pytest.mark.parametrize("key", ["year", "month_start"])
def test_fused_aggregation_groups_by_a_date_function(pkg, ctx, key):
    """GROUP BY extract(year FROM d) with count(*), GROUP BY date_trunc('month', d) with sum(bigint): a computed group key keeps the unfused
    composition inside the fused factory; the same functions as the filter and an aggregate's input run in the fused kernels"""
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    days, vals = tpch_rows()
    expr, fn, kt = {"year": (pkg.year(f(0, D)), X.year, B), "month_start": (pkg.date_trunc("month", f(0, D)), lambda a: X.date_trunc("month", a), D)}[key]
    aggs = [(pkg.COUNT_ALL, -1)] if key == "year" else [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)]
    filt = pkg.year(f(0, D)) < 1998
    projs = [expr, f(1, B)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [D, B], filt, projs, [kt], [0], aggs)
    got = in_order(tuple(r) for pg in pkg.to_pages(fused.createOperator(), pages_of(pkg, days, vals)) for r in pg.rows())
    mid = pkg.to_pages(pkg.FilterAndProjectOperatorFactory(ctx, 1, [D, B], filt, projs).createOperator(), pages_of(pkg, days, vals))
    two = in_order(tuple(r) for pg in pkg.to_pages(pkg.HashAggregationOperatorFactory(ctx, 2, [kt], [0], aggs).createOperator(), mid) for r in pg.rows())
    want = {}
    for a, v in zip(days, vals):
        if a is not None and X.year(a) < 1998:
            cnt, s = want.get(fn(a), (0, 0))
            want[fn(a)] = (cnt + 1, s + int(v))
    assert got == two == in_order((g, cnt) + ((s,) if key != "year" else ()) for g, (cnt, s) in want.items())
    assert len(want) == (6 if key == "year" else 72)
    # ... and as an aggregate's input under a raw group key: the fused kernels evaluate month(d) and year(d)
    grp = (np.arange(len(days)) % 3).astype(np.int64)
    pages = [pkg.Page(pkg.Block(D, days[a:a + 257]), pkg.Block(B, grp[a:a + 257])) for a in range(0, len(days), 257)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 3, [D, B], filt, [f(1, B), pkg.month(f(0, D)), pkg.year(f(0, D))], [B], [0],
                                                            [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1), (pkg.SUM_BIGINT, 2)])
    ctx.profile_enable(True)
    ctx.profile_reset()
    rows = in_order(tuple(r) for pg in pkg.to_pages(fused.createOperator(), pages) for r in pg.rows())
    prof = ctx.profile()
    ctx.profile_enable(False)
    prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
    assert any(name.startswith("fused_") for name in prof), sorted(prof)
    keep = [r for r, a in enumerate(days) if a is not None and X.year(a) < 1998]
    assert rows == [(g, sum(1 for r in keep if grp[r] == g), sum(X.month(days[r]) for r in keep if grp[r] == g), sum(X.year(days[r]) for r in keep if grp[r] == g)) for g in range(3)]


def test_fused_probe_keyed_by_date_trunc(pkg, ctx):
    f, D, B = pkg.field, pkg.DATE, pkg.BIGINT
    days, vals = tpch_rows()
    build = [X.to_days(y, m, 1) for y in range(1992, 1999) for m in (1, 2, 6, 11)]
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [D], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(D, build)))
    b.finish()
    filt = pkg.day_of_week(f(0, D)) < 6
    projs = [pkg.date_trunc("month", f(0, D)), f(1, B), pkg.week(f(0, D))]
    fj = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [D, B], filt, projs, [0])
    before = sum(pkg.fused_probe_launch_counts())
    got = [tuple(r) for pg in pkg.to_pages(fj.createOperator(), pages_of(pkg, days, vals)) for r in pg.rows()]
    assert sum(pkg.fused_probe_launch_counts()) > before      # the fused probe kernel ran
    mid = pkg.to_pages(pkg.FilterAndProjectOperatorFactory(ctx, 3, [D, B], filt, projs).createOperator(), pages_of(pkg, days, vals))
    two = [tuple(r) for pg in pkg.to_pages(pkg.LookupJoinOperatorFactory(ctx, 4, bf.lookup_source_factory, [D, B, B], [0]).createOperator(), mid) for r in pg.rows()]
    want = [(X.date_trunc("month", a), int(v), X.week(a), X.date_trunc("month", a)) for a, v in zip(days, vals)
            if a is not None and X.day_of_week(a) < 6 and X.date_trunc("month", a) in build]
    assert got == two == want and 100 < len(want) < 500

"""The TIMESTAMP functions on the device (jit.cpp gen_timestamp, csrc/device_timestamp.h over csrc/device_date.h) against
tests/timestamp_fn_expected.py: every cell of the seeded corpus (tests/timestamp_fn_cases.py) is compared bit for bit -- to_unixtime as bits --
on the flat route at 1, 63, 64, 65 and 4097 rows, with nulls -- every function, unit and precision -- and the unary functions, the casts and a
sample of date_trunc / date_diff on the dictionary-aware, fused-aggregation and fused-join-filter routes (the generated expression text is the
same on every route); then the errors and which of them wins."""
import json
import os
import struct

import numpy as np
import pytest

import timestamp_fn_cases as C
import timestamp_fn_expected as X
import expr_harness as H

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "timestamp_function_vectors.json")))
RANGE = -2


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


def columns(outs, n):
    return [[v for o in outs for v in o.getBlock(k).to_list()] for k in range(n)]


def run(pkg, fac, pages):
    """one operator of `fac` over `pages`, closed afterwards -> host pages"""
    op = fac.createOperator()
    try:
        return pkg.to_pages(op, pages)
    finally:
        op.close()


def project(pkg, ctx, types, filt, exprs, page):
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs)
    op = fac.createOperator()
    outs = pkg.to_pages(op, [page])
    op.close()
    fac.close()
    return columns(outs, len(exprs))


def failure(pkg, ctx, types, filt, exprs, page):
    """-> (code, position) of the error the page raises, or None"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs)
    op = fac.createOperator()
    outs, err = H.drive_pages(pkg, op, [page])
    op.close()
    fac.close()
    return None if err is None else (err[0].code, err[2])


def bits(values):
    return [None if v is None else struct.unpack("<q", struct.pack("<d", v))[0] for v in values]


def unary_exprs(pkg, t):
    return [pkg.year(t), pkg.quarter(t), pkg.month(t), pkg.week(t), pkg.day(t), pkg.day_of_week(t), pkg.day_of_year(t), pkg.year_of_week(t), pkg.last_day_of_month(t),
            pkg.hour(t), pkg.minute(t), pkg.second(t), pkg.millisecond(t), pkg.to_unixtime(t), pkg.cast(t, pkg.DATE)]


def unary_want(xs):
    rows = [None if t is None else X.unary_row(t) for t in xs]
    return [[None if r is None else r[k] for r in rows] for k in range(13)] + [[X.double_bits(X.to_unixtime(t)) for t in xs], [X.to_date(t) for t in xs]]


def unary_got(cols):
    return cols[:13] + [bits(cols[13]), cols[14]]


def checked(call):
    try:
        return call()
    except X.OutOfRange:
        return X.OutOfRange


# ---- (1) the reference's pinned literals ----------------------------------------------------------------------------------------------------
def test_golden_cases_as_column_values(pkg, ctx):
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    cases = GOLD["extract"] + GOLD["last_day_of_month"] + GOLD["to_unixtime"] + GOLD["to_date"]
    xs = [g["us"] for g in cases]
    got = unary_got(project(pkg, ctx, [T], None, unary_exprs(pkg, f(0, T)), pkg.Page(pkg.Block(T, xs))))
    assert got == unary_want(xs)
    for r, g in enumerate(GOLD["extract"]):
        assert got[X.UNARY_NAMES.index(g["function"])][r] == g["expected"], g
    for name in ("date_trunc", "date_add", "date_diff", "cast_precision", "from_date", "compare"):
        for g in GOLD[name]:
            t = pkg.constant(g.get("us", g.get("us1", 0)), T)
            expr = {"date_trunc": lambda: pkg.date_trunc(g["unit"], t), "date_add": lambda: pkg.date_add(g["unit"], g["value"], t, g["precision"]),
                    "date_diff": lambda: pkg.date_diff(g["unit"], t, pkg.constant(g["us2"], T)), "cast_precision": lambda: pkg.cast(t, T, g["target"]),
                    "from_date": lambda: pkg.cast(pkg.constant(g["day"], pkg.DATE), T),
                    "compare": lambda: pkg.between(t, g["us2"], g["us3"]) if g["op"] == "BETWEEN" else pkg.call(g["op"], pkg.BOOLEAN, t, pkg.constant(g["us2"], T))}[name]()
            g["_expr"] = expr
    flat = [g for name in ("date_trunc", "date_add", "date_diff", "cast_precision", "from_date", "compare") for g in GOLD[name]]
    page = pkg.Page(pkg.Block(B, [0]))
    for at in range(0, len(flat), 16):
        part = flat[at:at + 16]
        assert project(pkg, ctx, [B], None, [g["_expr"] for g in part], page) == [[g["expected"]] for g in part], part[0]["sql"]


# ---- (2) every cell of the corpus, flat, at each row count --------------------------------------------------------------------------------
def corpus_rows():
    return C.with_nulls(C.instants())


def test_corpus_unary_ops_every_row_count(pkg, ctx):
    f, T = pkg.field, pkg.TIMESTAMP
    rows = corpus_rows()
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [T], None, unary_exprs(pkg, f(0, T)))
    for n in C.ROW_COUNTS + [len(rows)]:
        xs = rows if n == len(rows) else C.cycle(rows[::-1] if n == 1 else rows, n, start=0 if n == 1 else 5 * n)
        outs = run(pkg, fac, [pkg.Page(pkg.Block(T, xs))])
        assert unary_got(columns(outs, 15)) == unary_want(xs), n
    fac.close()
    assert len(rows) > 2500 and rows[3] is None and C.cycle(rows[::-1], 1)[0] is not None


def test_corpus_casts_and_comparisons(pkg, ctx):
    f, T, D_ = pkg.field, pkg.TIMESTAMP, pkg.DATE
    xs = corpus_rows()
    ys = C.cycle(xs, len(xs), start=7)
    t, u = f(0, T), f(1, T)
    exprs = [pkg.cast(t, T, q) for q in C.PRECISIONS] + [t < u, t.eq(u), t >= u, pkg.between(t, u, 10**15), pkg.in_(t, [0, -1, None, X.INT64_MIN, 999]), pkg.is_null(t),
                                                         pkg.if_(t < u, t, u), pkg.coalesce(t, u, pkg.constant(5, T))]
    got = project(pkg, ctx, [T, T], None, exprs, pkg.Page(pkg.Block(T, xs), pkg.Block(T, ys)))
    both = lambda fn: [None if a is None or b is None else fn(a, b) for a, b in zip(xs, ys)]
    items = {0, -1, X.INT64_MIN, 999}
    want = [[X.cast_precision(a, q) for a in xs] for q in C.PRECISIONS] + [
        both(lambda a, b: a < b), both(lambda a, b: a == b), both(lambda a, b: a >= b),
        [None if a is None else (False if b is not None and a < b else (None if b is None and a <= 10**15 else (False if a > 10**15 else True))) for a, b in zip(xs, ys)],
        [None if a is None else (True if a in items else None) for a in xs], [a is None for a in xs],
        [(a if (a is not None and b is not None and a < b) else b) for a, b in zip(xs, ys)], [a if a is not None else b if b is not None else 5 for a, b in zip(xs, ys)]]
    for ch, w in enumerate(want):
        assert got[ch] == w, ch
    days = C.with_nulls(C.DATE_CAST_DAYS)
    assert project(pkg, ctx, [D_], None, [pkg.cast(f(0, D_), T)], pkg.Page(pkg.Block(D_, days))) == [[X.from_date(d) for d in days]]


@pytest.mark.parametrize("unit", X.UNITS)
def test_trunc_add_diff_over_columns(pkg, ctx, unit):
    """date_trunc, date_add at every precision, date_diff: the amount from a BIGINT column, the instants from two columns"""
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    xs = C.edge_instants()[::2] + C.random_instants(100, seed=32)
    rows = []
    for i, t in enumerate(xs):
        for j, v in enumerate(C.AMOUNTS[:: 2 if i % 2 else 1]):
            e = xs[(i * 31 + j * 7) % len(xs)]
            rows.append((t, v, e))
            if (i + j) % 5 == 0:
                rows.append((None if j % 3 == 0 else t, None if j % 3 == 1 else v, None if j % 3 == 2 else e))
    t_, k_, e_ = f(0, T), f(1, B), f(2, T)
    exprs = [pkg.date_trunc(unit, t_), pkg.date_diff(unit, t_, e_)] + [pkg.date_add(unit, k_, t_, p) for p in C.PRECISIONS]
    want = [[checked(lambda: X.date_trunc(unit, t)) for t, v, e in rows], [X.date_diff(unit, t, e) for t, v, e in rows]]
    want += [[checked(lambda: X.date_add(unit, v, t, p)) for t, v, e in rows] for p in C.PRECISIONS]
    # a page raises when one cell overflows: the value pages hold the rows where nothing does, the others are raised in the error test
    clean = [r for r in range(len(rows)) if all(w[r] is not X.OutOfRange for w in want)]
    assert len(rows) > 2000 and len(rows) // 3 < len(clean) < len(rows)
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [T, B, T], None, exprs)
    for n in C.ROW_COUNTS[:4] + [len(clean)]:
        part = clean if n == len(clean) else clean[3 * n:4 * n]
        page = pkg.Page(pkg.Block(T, [rows[r][0] for r in part]), pkg.Block(B, [rows[r][1] for r in part]), pkg.Block(T, [rows[r][2] for r in part]))
        outs = run(pkg, fac, [page])
        assert columns(outs, len(exprs)) == [[w[r] for r in part] for w in want], (unit, n)
    # every overflowing cell raises, alone on an otherwise clean page of more than one wave: a sample of them per projection
    dirty = [r for r in range(len(rows)) if r not in set(clean)]
    for ch in (0, 2, 5, 8):
        bad = [r for r in dirty if want[ch][r] is X.OutOfRange][:3]
        for at, r in zip((0, 64, 99), bad):
            part = clean[:100]
            part[at] = r
            page = pkg.Page(pkg.Block(T, [rows[q][0] for q in part]), pkg.Block(B, [rows[q][1] for q in part]), pkg.Block(T, [rows[q][2] for q in part]))
            assert failure(pkg, ctx, [T, B, T], None, [exprs[1], exprs[ch]], page) == (RANGE, at), (unit, ch, rows[r])


# ---- (3) errors and which of them wins ------------------------------------------------------------------------------------------------------
def test_overflow_errors(pkg, ctx):
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    t, k = f(0, T), f(1, B)
    n = 300
    xs = [C.at(1995, 1, 1, 12) + r * 3_600_000_001 for r in range(n)]
    page = lambda ts, ks: pkg.Page(pkg.Block(T, ts), pkg.Block(B, ks))
    one = lambda at, v: [v if r == at else 1 for r in range(n)]
    for unit, at, v, us in (("millisecond", 257, 1, X.INT64_MAX), ("day", 3, 2**31, 0), ("week", 64, -2**31 - 1, 0), ("month", 299, 2**31 - 1, 0), ("year", 0, -2**31, 0),
                            ("second", 130, -1, X.INT64_MIN + 500), ("hour", 63, 2**62, 0), ("quarter", 65, 4, X.INT64_MAX - 10**9)):
        ts = [us if r == at else x for r, x in enumerate(xs)]
        assert checked(lambda: X.date_add(unit, v, us)) is X.OutOfRange
        assert failure(pkg, ctx, [T, B], None, [t, pkg.date_add(unit, k, t)], page(ts, one(at, v))) == (RANGE, at), (unit, v)
        # a NULL amount or a NULL timestamp on the otherwise overflowing row gives NULL, not an error
        for nt, nk in ((ts, one(at, None)), ([None if r == at else x for r, x in enumerate(ts)], one(at, v))):
            got = project(pkg, ctx, [T, B], None, [pkg.date_add(unit, k, t)], page(nt, nk))
            assert got == [[X.date_add(unit, b, a) for a, b in zip(nt, nk)]] and got[0][at] is None
    ts = [X.INT64_MIN + 5 if r == 77 else x for r, x in enumerate(xs)]
    assert failure(pkg, ctx, [T, B], None, [pkg.date_trunc("second", t), pkg.date_trunc("year", t)], page(ts, one(0, 1))) == (RANGE, 77)
    assert failure(pkg, ctx, [T, B], None, [pkg.year(t), pkg.last_day_of_month(t), pkg.cast(t, T, 0), pkg.hour(t)], page(ts, one(0, 1))) is None      # none of these raises
    # two failing projections and rows: the lowest projection index, then its first row
    ts = list(xs)
    ts[9], ts[12], ts[2] = X.INT64_MAX, X.INT64_MAX - 1, X.INT64_MIN
    ks = [5] * n
    exprs = [pkg.year(t), pkg.date_add("day", k, t), pkg.date_add("month", -1, t)]
    assert failure(pkg, ctx, [T, B], None, exprs, page(ts, ks)) == (RANGE, 9)                # projection 1 fails on rows 9 and 12, projection 2 on row 2
    assert failure(pkg, ctx, [T, B], None, [exprs[0], exprs[2], exprs[1]], page(ts, ks)) == (RANGE, 2)
    # the filter rejects the failing rows: nothing is raised
    got = project(pkg, ctx, [T, B], pkg.between(pkg.year(t), 1995, 1996), exprs, page(ts, ks))
    keep = [r for r in range(n) if r not in (9, 12, 2)]
    assert got == [[X.year(ts[r]) for r in keep], [X.date_add("day", 5, ts[r]) for r in keep], [X.date_add("month", -1, ts[r]) for r in keep]]


# ---- (4) DICTIONARY and RLE input blocks: the dictionary-aware route -----------------------------------------------------------------------
def test_dictionary_and_rle_inputs(pkg, ctx):
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    entries = C.with_nulls(C.edge_instants())
    t = f(0, T)
    single = unary_exprs(pkg, t) + [pkg.cast(t, T, 3)]
    # ... and date_trunc / date_diff of a precise and of a calendar unit (date_add raises on some entries: the flat route's test has its cells)
    binary = [pkg.date_trunc("minute", t), pkg.date_trunc("quarter", t), pkg.date_diff("hour", t, pkg.constant(0, T)), pkg.date_diff("month", pkg.constant(0, T), t)]
    safe = [a for a in entries if a is None or checked(lambda: X.date_trunc("quarter", a)) is not X.OutOfRange]
    for n in C.ROW_COUNTS:
        ids = ((np.arange(n, dtype=np.int64) * 7919 + n) % len(entries)).astype(np.int32)
        xs = [entries[i] for i in ids]
        op = pkg.FilterAndProjectOperatorFactory(ctx, 0, [T], None, single).createOperator()
        outs = pkg.to_pages(op, [pkg.Page(pkg.DictionaryBlock(pkg.Block(T, entries), ids))])
        if n == 4097:
            assert pkg._lib.lib().tgpu_debug_dictionary_pages(op.handle) == 1           # evaluated once per dictionary entry
        cols = columns(outs, 16)
        assert unary_got(cols[:15]) == unary_want(xs) and cols[15] == [X.cast_precision(a, 3) for a in xs], n
        op.close()
        ys = [safe[i % len(safe)] for i in ids]
        got = project(pkg, ctx, [T], None, binary, pkg.Page(pkg.DictionaryBlock(pkg.Block(T, safe), (ids % len(safe)).astype(np.int32))))
        assert got == [[X.date_trunc("minute", a) for a in ys], [X.date_trunc("quarter", a) for a in ys], [X.date_diff("hour", a, 0) for a in ys], [X.date_diff("month", 0, a) for a in ys]], n
    # an entry that no row refers to and whose date_add overflows raises nothing
    small = [C.at(1995, 3, 1, 5), X.INT64_MAX, None, C.at(1996, 2, 29, 23, 59, 59, 999_999)]
    ids = np.array([0, 3, 2, 0, 3, 3, 2, 0] * 40, dtype=np.int32)
    op = pkg.FilterAndProjectOperatorFactory(ctx, 0, [T], pkg.year(t) > 1994, [pkg.date_add("day", 1, t), pkg.date_trunc("hour", t)]).createOperator()
    outs = pkg.to_pages(op, [pkg.Page(pkg.DictionaryBlock(pkg.Block(T, small), ids))])
    kept = [small[i] for i in ids if small[i] is not None]
    assert columns(outs, 2) == [[X.date_add("day", 1, a) for a in kept], [X.date_trunc("hour", a) for a in kept]]
    ks = [None if r % 17 == 0 else r % 25 - 12 for r in range(257)]
    for value in (C.at(2020, 12, 31, 23, 59, 59, 999_999), None):
        page = pkg.Page(pkg.RunLengthEncodedBlock(pkg.Block(T, [value]), 257), pkg.Block(B, ks))
        got = project(pkg, ctx, [T, B], None, [pkg.date_add("month", f(1, B), t, 2), pkg.second(t), pkg.to_unixtime(t)], page)
        assert got[:2] == [[X.date_add("month", b, value, 2) for b in ks], [X.second(value)] * 257] and bits(got[2]) == [X.double_bits(X.to_unixtime(value))] * 257


# ---- (5) the fused routes: every corpus cell through the aggregation's and the join filter's generated kernels -------------------------------
def in_order(rows):
    return sorted(rows, key=lambda r: tuple((v is None, 0 if v is None else v) for v in r))


def test_fused_aggregation_evaluates_the_corpus(pkg, ctx):
    """min / max of each function's value per group: with groups of a few rows every cell decides an output cell.  The functions run as the
    aggregates' inputs and in the filter of the fused kernels (proven by the profile's scope)."""
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    xs = corpus_rows()
    n = len(xs)
    grp = (np.arange(n) // 2).astype(np.int64)                     # two rows per group
    t = f(0, T)
    projs = [f(1, B), pkg.year(t), pkg.day_of_year(t), pkg.week(t), pkg.hour(t), pkg.minute(t), pkg.second(t), pkg.millisecond(t), pkg.cast(t, T, 2), pkg.date_diff("month", t, 0)]
    fns = [X.year, X.day_of_year, X.week, X.hour, X.minute, X.second, X.millisecond, lambda a: X.cast_precision(a, 2), lambda a: X.date_diff("month", a, 0)]
    aggs = [(pkg.COUNT_ALL, -1)] + [(pkg.MIN_TIMESTAMP if k == 8 else pkg.MIN_BIGINT, k) for k in range(1, 10)] + [(pkg.MAX_TIMESTAMP, 8)]
    filt = pkg.or_(pkg.is_null(t), pkg.millisecond(t) >= 0)        # keeps every row, and runs a TIMESTAMP function in the fused filter
    size = 4097
    pages = [pkg.Page(pkg.Block(T, xs[a:a + size]), pkg.Block(B, grp[a:a + size])) for a in range(0, n, size)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 3, [T, B], filt, projs, [B], [0], aggs)
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = run(pkg, fused, pages)
    fused.close()
    prof = ctx.profile()
    ctx.profile_enable(False)
    prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
    assert any(name.startswith("fused_") for name in prof), sorted(prof)
    assert out[0].getBlock(9).type == T and out[0].getBlock(11).type == T and out[0].getBlock(10).type == B
    rows = in_order(tuple(r) for pg in out for r in pg.rows())
    want = []
    for g in range((n + 1) // 2):
        cell = [a for a in xs[2 * g:2 * g + 2] if a is not None]
        vals = [[fn(a) for a in cell] for fn in fns]
        want.append((g, len(xs[2 * g:2 * g + 2])) + tuple(min(v) if v else None for v in vals) + ((max(vals[7]) if cell else None),))
    assert rows == want


def test_fused_join_filter_evaluates_the_corpus(pkg, ctx):
    """the filter / project fused into the probe: the filter compares two TIMESTAMP functions, the probe key is date_trunc('day', t), and the
    carried projections hold the function values"""
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    xs = corpus_rows()
    vals = np.arange(len(xs), dtype=np.int64)
    keys = sorted({X.date_trunc("day", a) for a in xs if a is not None and checked(lambda: X.date_trunc("day", a)) is not X.OutOfRange and X.millisecond(a) % 2 == 0})
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [T], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(T, keys)))
    b.finish()
    t = f(0, T)
    safe = t > X.INT64_MIN + 86_400_000_000                          # (date_trunc('day') of the first day of the range overflows: the filter keeps it out)
    filt = pkg.and_(safe, pkg.and_(pkg.hour(t) < 23, pkg.year(t) > -290300))
    projs = [pkg.date_trunc("day", pkg.if_(safe, t, pkg.constant(0, T))), f(1, B), pkg.minute(t), pkg.cast(t, pkg.DATE)]
    size = 4097
    pages = [pkg.Page(pkg.Block(T, xs[a:a + size]), pkg.Block(B, vals[a:a + size])) for a in range(0, len(xs), size)]
    fj = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [T, B], filt, projs, [0])
    before = sum(pkg.fused_probe_launch_counts())
    out = run(pkg, fj, pages)
    assert sum(pkg.fused_probe_launch_counts()) > before      # the fused probe kernel ran
    got = [tuple(r) for pg in out for r in pg.rows()]
    assert out[0].getBlock(0).type == T and out[0].getBlock(4).type == T
    keyset = set(keys)
    want = [(X.date_trunc("day", a), int(v), X.minute(a), X.to_date(a), X.date_trunc("day", a)) for a, v in zip(xs, vals)
            if a is not None and a > X.INT64_MIN + 86_400_000_000 and X.hour(a) < 23 and X.year(a) > -290300 and X.date_trunc("day", a) in keyset]
    assert got == want and len(want) > 500

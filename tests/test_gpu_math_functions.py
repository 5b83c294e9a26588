"""The math functions on the device (jit.cpp gen_math, csrc/device_math.h) against tests/math_fn_expected.py.  Exact group: every cell bit for
bit (any NaN for a NaN), on the flat, dictionary, run-length, fused-aggregation, fused-probe and nested-loop paths.  Bounded group: every
corpus argument within the corpus' per-function bound of the correctly rounded result, the `exact` entries at 0 ulp.  About a dozen
projections share a program."""
import json
import os

import numpy as np
import pytest

import expr_harness as H
import math_fn_cases as C
import math_fn_expected as X
import nested_loop_gpu as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
CORPUS = json.load(open(os.path.join(HERE, "golden", "math_function_ulp_corpus.json")))
GOLD = json.load(open(os.path.join(HERE, "golden", "math_function_vectors.json")))
RANGE = -2
ABS_BIGINT = "Value -9223372036854775808 is out of range for abs(bigint)"
ABS_INTEGER = "Value -2147483648 is out of range for abs(integer)"


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


def run(pkg, fac, page, n_out):
    op = fac.createOperator()
    outs = pkg.to_pages(op, [page])
    op.close()
    return [[v for o in outs for v in o.getBlock(k).to_list()] for k in range(n_out)]


def project(pkg, ctx, types, filt, exprs, page):
    """-> one list per projection over all output pages"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs)
    got = run(pkg, fac, page, len(exprs))
    fac.close()
    return got


def failure(pkg, ctx, types, filt, exprs, page):
    """-> (code, message without its position, position) of the error the page raises, or None"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs)
    op = fac.createOperator()
    outs, err = H.drive_pages(pkg, op, [page])
    op.close()
    fac.close()
    if err is None:
        return None
    text = str(err[0])
    at = text.find(" (position ")
    start = max(text.find("Value "), text.find("numerical overflow"), 0)
    return err[0].code, text[start:at], err[2]


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for ch, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, ch)
        for r, (a, b) in enumerate(zip(g, w)):
            assert X.same(a, b), (what, ch, r, a, b)


# ---- (1) the reference's pinned cases as constant expressions --------------------------------------------------------------------------------
def golden_value(v):
    return None if v is None else X.from_bits(int(v["bits"], 16)) if isinstance(v, dict) else v


def golden_constant(pkg, a):
    t = {"bigint": pkg.BIGINT, "integer": pkg.INTEGER, "double": pkg.DOUBLE}[a["type"]]
    return pkg.constant(golden_value(a["value"]), t)


def golden_call(pkg, g):
    fn = {"abs": pkg.abs_, "sign": pkg.sign, "floor": pkg.floor, "ceiling": pkg.ceiling, "ceil": pkg.ceil, "truncate": pkg.truncate, "round": pkg.round_, "sqrt": pkg.sqrt,
          "cbrt": pkg.cbrt, "exp": pkg.exp, "ln": pkg.ln, "log2": pkg.log2, "log10": pkg.log10, "log": pkg.log, "power": pkg.power, "pow": pkg.pow_, "is_nan": pkg.is_nan,
          "is_finite": pkg.is_finite, "is_infinite": pkg.is_infinite, "degrees": pkg.degrees, "radians": pkg.radians}[g["function"]]
    args = [golden_constant(pkg, a) for a in g["arguments"]]
    if g["function"] == "round" and len(args) == 2:
        return fn(args[0], args[1])
    return fn(*args)


def test_golden_cases_as_constants(pkg, ctx):
    cases = [g for g in GOLD["cases"] if "expected" in g]
    assert len(cases) > 150
    page = pkg.Page(pkg.Block(pkg.BIGINT, [0]))
    worst = {}
    for at in range(0, len(cases), 16):
        part = cases[at:at + 16]
        got = project(pkg, ctx, [pkg.BIGINT], None, [golden_call(pkg, g) for g in part], page)
        for g, (v,) in zip(part, got):
            want = golden_value(g["expected"])
            if want is not None and (g["function"] in X.BOUNDED or g["function"] == "pow"):
                bound = CORPUS["bounds"]["power" if g["function"] == "pow" else g["function"]]
                d = X.ulp_distance(v, want)
                worst[g["function"]] = max(worst.get(g["function"], 0), d)
                assert d <= bound, (g, v)
            else:
                assert X.same(v, float(want) if isinstance(v, float) else want), (g, v)
    print("golden bounded cases, worst distance from the reference's literal in doubles:", worst)
    failing = [g for g in GOLD["cases"] if "error" in g]
    assert len(failing) >= 8
    for g in failing:
        v, kind = g["arguments"][0]["value"], g["arguments"][0]["type"]
        want = checked(lambda: X.abs_(v, kind) if g["function"] == "abs" else X.round_(v, g["arguments"][1]["value"], kind))
        assert isinstance(want, X.OutOfRange) and g["error"] == "NUMERIC_VALUE_OUT_OF_RANGE"
        assert failure(pkg, ctx, [pkg.BIGINT], None, [golden_call(pkg, g)], page) == (RANGE, str(want), 0), g


# ---- (2) the exact group over DOUBLE columns ----------------------------------------------------------------------------------------------------
def double_rows():
    return C.with_nulls(C.edge_doubles() + C.random_doubles(720, 7))


def pages_by_count(rows):
    """(n, rows): the rows from a different start for each row count, and the whole list"""
    return [(n, C.cycle(rows[::-1] if n == 1 else rows, n, start=0 if n == 1 else 5 * n)) for n in C.ROW_COUNTS] + [(len(rows), rows)]


def test_exact_group_over_double_columns_every_row_count(pkg, ctx):
    f, D = pkg.field, pkg.DOUBLE
    x = f(0, D)
    exprs = [pkg.abs_(x), pkg.sign(x), pkg.floor(x), pkg.ceiling(x), pkg.truncate(x), pkg.round_(x), pkg.sqrt(x), pkg.is_nan(x), pkg.is_finite(x), pkg.is_infinite(x),
             pkg.degrees(x), pkg.radians(x), pkg.round_(x, 2)]
    model = [X.abs_, X.sign, X.floor, X.ceiling, X.truncate, X.round_, X.sqrt, X.is_nan, X.is_finite, X.is_infinite, X.degrees, X.radians, lambda v: X.round_(v, 2)]
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D], None, exprs)
    for n, rows in pages_by_count(double_rows()):
        got = run(pkg, fac, pkg.Page(pkg.Block(D, rows)), len(exprs))
        assert_same(got, [[m(v) for v in rows] for m in model], n)
    fac.close()
    assert len(double_rows()) > 1025


def test_round_over_double_columns_every_decimals(pkg, ctx):
    f, D = pkg.field, pkg.DOUBLE
    rows = double_rows()
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D], None, [pkg.round_(f(0, D), d) for d in C.DECIMALS])
    for n, part in pages_by_count(rows)[3:]:
        got = run(pkg, fac, pkg.Page(pkg.Block(D, part)), len(C.DECIMALS))
        assert_same(got, [[X.round_(v, d) for v in part] for d in C.DECIMALS], n)
    fac.close()
    # what the rule gives beyond the double range: factor +inf -> a zero with the argument's sign, factor 0 -> NaN
    assert X.same(X.round_(-3.5, 309), -0.0) and X.same(X.round_(3.5, 309), 0.0) and X.round_(3.5, -324) != X.round_(3.5, -324)
    assert X.round_(2.5) == 3.0 and X.round_(-2.5) == -3.0 and X.same(X.round_(-0.3), -0.0) and X.same(X.round_(-0.0), 0.0) and X.round_(0.49999999999999994) == 0.0


# ---- (3) the exact group over integer columns ---------------------------------------------------------------------------------------------------
def checked(call):
    try:
        return call()
    except X.OutOfRange as e:
        return e


@pytest.mark.parametrize("kind", ["bigint", "integer"])
def test_exact_group_over_integer_columns(pkg, ctx, kind):
    f = pkg.field
    T = pkg.BIGINT if kind == "bigint" else pkg.INTEGER
    values = C.edge_bigints() if kind == "bigint" else C.edge_integers()
    x = f(0, T)
    exprs = [pkg.abs_(x), pkg.sign(x), pkg.floor(x), pkg.ceiling(x), pkg.round_(x)] + [pkg.round_(x, d) for d in C.INTEGER_DECIMALS if d > -19]
    model = [lambda v: X.abs_(v, kind), X.sign, X.floor, X.ceiling, X.round_] + [(lambda v, d=d: X.round_(v, d, kind)) for d in C.INTEGER_DECIMALS if d > -19]
    # a page raises when one cell fails: the value pages hold the rows that do not; the others are raised in (6)
    clean = [v for v in values if not any(isinstance(checked(lambda: m(v)), X.OutOfRange) for m in model)]
    assert len(values) // 2 < len(clean) < len(values)
    rows = C.with_nulls(clean)
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [T], None, exprs)
    for n, part in pages_by_count(rows):
        got = run(pkg, fac, pkg.Page(pkg.Block(T, part)), len(exprs))
        assert_same(got, [[m(v) for v in part] for m in model], (kind, n))
    fac.close()


# ---- (4) routes: DICTIONARY and RLE inputs, a filter that uses a math function, the fused kernels ---------------------------------------------------
def test_dictionary_and_rle_inputs_with_and_without_a_math_filter(pkg, ctx):
    f, D, B = pkg.field, pkg.DOUBLE, pkg.BIGINT
    entries = [2.5, -2.5, None, 0.49999999999999994, -0.0, C.NAN, 1e300, -7.45, 5e-324, C.INF, 1234.5678]
    rng = np.random.default_rng(4)
    n = 1000
    ids = rng.integers(0, len(entries), n).astype(np.int32)
    xs = [entries[i] for i in ids]
    ks = [None if r % 17 == 0 else (r % 25 - 12 if r % 5 else -2**63 + r) for r in range(n)]
    x, k = f(0, D), f(1, B)
    exprs = [pkg.round_(x), pkg.round_(x, 1), pkg.floor(x), pkg.ceiling(x), pkg.truncate(x), pkg.abs_(x), pkg.sign(x), pkg.sqrt(pkg.abs_(x)), pkg.sign(k), pkg.is_nan(x),
             pkg.round_(pkg.abs_(x) * 100.0, -1)]
    want = [[m(v) for v in xs] for m in (X.round_, lambda v: X.round_(v, 1), X.floor, X.ceiling, X.truncate, X.abs_, X.sign, lambda v: X.sqrt(X.abs_(v)))]
    want += [[X.sign(v) for v in ks], [X.is_nan(v) for v in xs], [None if v is None else X.round_(X.abs_(v) * 100.0, -1) for v in xs]]
    amounts = pkg.Block(B, ks)
    got = project(pkg, ctx, [D, B], None, exprs, pkg.Page(pkg.DictionaryBlock(pkg.Block(D, entries), ids), amounts))
    assert_same(got, want, "dictionary")
    assert_same(project(pkg, ctx, [D, B], None, exprs, pkg.Page(pkg.Block(D, xs), amounts)), want, "flat")
    # a filter that is itself a math function, over the dictionary and over the flat column
    filt = pkg.and_(pkg.is_finite(x), pkg.abs_(pkg.round_(x)) >= 1.0)
    keep = [r for r, v in enumerate(xs) if v is not None and X.is_finite(v) and X.abs_(X.round_(v)) >= 1.0]
    for page in (pkg.Page(pkg.DictionaryBlock(pkg.Block(D, entries), ids), amounts), pkg.Page(pkg.Block(D, xs), amounts)):
        assert_same(project(pkg, ctx, [D, B], filt, exprs, page), [[w[r] for r in keep] for w in want], "filtered")
    assert 100 < len(keep) < n - 100
    # one column: the dictionary-aware path evaluates once per entry
    single = [pkg.round_(x, 2), pkg.ceiling(x), pkg.radians(x)]
    op = pkg.FilterAndProjectOperatorFactory(ctx, 0, [D], pkg.floor(x) > -100.0, single).createOperator()
    outs = pkg.to_pages(op, [pkg.Page(pkg.DictionaryBlock(pkg.Block(D, entries), ids))])
    assert pkg._lib.lib().tgpu_debug_dictionary_pages(op.handle) == 1
    kept = [v for v in xs if v is not None and X.floor(v) > -100.0]
    assert_same([[v for o in outs for v in o.getBlock(ch).to_list()] for ch in range(3)], [[X.round_(v, 2) for v in kept], [X.ceiling(v) for v in kept], [X.radians(v) for v in kept]], "dictionary-aware")
    for value in (-2.5, None, C.NAN):
        page = pkg.Page(pkg.RunLengthEncodedBlock(pkg.Block(D, [value]), 257), pkg.Block(B, ks[:257]))
        assert_same(project(pkg, ctx, [D, B], None, exprs, page), [[w_for(value, kv) for kv in ks[:257]] for w_for in rle_model()], ("rle", value))


def rle_model():
    x_only = [X.round_, lambda v: X.round_(v, 1), X.floor, X.ceiling, X.truncate, X.abs_, X.sign, lambda v: X.sqrt(X.abs_(v))]
    fns = [(lambda v, k, m=m: m(v)) for m in x_only]
    return fns + [lambda v, k: X.sign(k), lambda v, k: X.is_nan(v), lambda v, k: None if v is None else X.round_(X.abs_(v) * 100.0, -1)]


def in_order(rows):
    return sorted(rows, key=lambda r: tuple((v is None, 0 if v is None else v) for v in r))


def fused_rows(n=1000):
    rng = np.random.default_rng(12)
    xs = [None if r % 43 == 7 else float(int(v)) / 4.0 for r, v in enumerate(rng.integers(-4000, 4000, n))]
    return xs, rng.integers(-1000, 1000, n).astype(np.int64)


def test_fused_aggregation_with_math_inputs_and_filter(pkg, ctx):
    """sum / count over round(x), abs(k) and floor(x) under a raw group key with a filter that uses abs: the fused kernels evaluate them; a group
    key that is itself round(x) keeps the unfused composition inside the fused factory and gives the same groups"""
    f, D, B = pkg.field, pkg.DOUBLE, pkg.BIGINT
    xs, ks = fused_rows()
    grp = (np.arange(len(xs)) % 3).astype(np.int64)
    pages = [pkg.Page(pkg.Block(D, xs[a:a + 257]), pkg.Block(B, ks[a:a + 257]), pkg.Block(B, grp[a:a + 257])) for a in range(0, len(xs), 257)]
    filt = pkg.abs_(f(0, D)) < 900.0
    projs = [f(2, B), pkg.round_(f(0, D)), pkg.abs_(f(1, B)), pkg.floor(f(0, D) * 0.5)]
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_DOUBLE, 1), (pkg.SUM_BIGINT, 2), (pkg.MIN_DOUBLE, 3), (pkg.MAX_DOUBLE, 3)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 3, [D, B, B], filt, projs, [B], [0], aggs)
    ctx.profile_enable(True)
    ctx.profile_reset()
    rows = in_order(tuple(r) for pg in pkg.to_pages(fused.createOperator(), pages) for r in pg.rows())
    prof = ctx.profile()
    ctx.profile_enable(False)
    prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
    assert any(name.startswith("fused_") for name in prof), sorted(prof)
    keep = [r for r, v in enumerate(xs) if v is not None and abs(v) < 900.0]
    want = []
    for g in range(3):
        mine = [r for r in keep if grp[r] == g]
        halves = [X.floor(xs[r] * 0.5) for r in mine]
        want.append((g, len(mine), sum(X.round_(xs[r]) for r in mine), sum(abs(int(ks[r])) for r in mine), min(halves), max(halves)))   # (sums of small integers: exact in any order)
    assert rows == want
    # a computed key, sign(k): the factory keeps the unfused composition for it and gives the same groups
    projs = [pkg.sign(f(1, B)), pkg.ceiling(f(0, D))]
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_DOUBLE, 1)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 4, [D, B, B], filt, projs, [B], [0], aggs)
    got = in_order(tuple(r) for pg in pkg.to_pages(fused.createOperator(), pages) for r in pg.rows())
    want = [(g, sum(1 for r in keep if X.sign(int(ks[r])) == g), sum(X.ceiling(xs[r]) for r in keep if X.sign(int(ks[r])) == g)) for g in (-1, 0, 1)]
    assert got == [w for w in want if w[1]] and len(got) >= 2        # (sums of small integers again)


def test_fused_probe_keyed_by_a_math_function(pkg, ctx):
    f, D, B = pkg.field, pkg.DOUBLE, pkg.BIGINT
    xs, ks = fused_rows()
    build = [0, 1] + list(range(7, 1000, 7))
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(B, build)))
    b.finish()
    pages = [pkg.Page(pkg.Block(D, xs[a:a + 257]), pkg.Block(B, ks[a:a + 257])) for a in range(0, len(xs), 257)]
    filt = pkg.is_finite(pkg.sqrt(f(0, D)))                                  # x >= 0: the square root of a negative is NaN
    # abs(k) as the key can raise (the minimum), which the fused probe takes for its key; sign(k) cannot raise
    for key, fn, must_fuse in ((pkg.abs_(f(1, B)), lambda k: abs(k), False), (pkg.sign(f(1, B)), X.sign, True)):
        projs = [key, pkg.ceiling(f(0, D)), pkg.round_(f(0, D), 1)]
        fj = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [D, B], filt, projs, [0])
        before = sum(pkg.fused_probe_launch_counts())
        got = [tuple(r) for pg in pkg.to_pages(fj.createOperator(), pages) for r in pg.rows()]
        assert sum(pkg.fused_probe_launch_counts()) > before or not must_fuse      # the fused probe kernel ran
        mid = pkg.to_pages(pkg.FilterAndProjectOperatorFactory(ctx, 3, [D, B], filt, projs).createOperator(), pages)
        two = [tuple(r) for pg in pkg.to_pages(pkg.LookupJoinOperatorFactory(ctx, 4, bf.lookup_source_factory, [B, D, D], [0]).createOperator(), mid) for r in pg.rows()]
        want = [(fn(int(k)), X.ceiling(v), X.round_(v, 1), fn(int(k))) for v, k in zip(xs, ks) if v is not None and v >= 0 and fn(int(k)) in build]
        assert got == two == want and 20 < len(want) < 500


# ---- (5) the bounded group over the corpus ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CORPUS["functions"]))
def test_bounded_group_over_the_corpus(pkg, ctx, name):
    f, D = pkg.field, pkg.DOUBLE
    rows = CORPUS["functions"][name]
    arity = len(rows[0]) - 2
    cols = [[X.from_bits(int(r[k], 16)) for r in rows] for k in range(arity)]
    want = [X.from_bits(int(r[arity], 16)) for r in rows]
    assert len(rows) <= 512
    # NaN arguments travel as they are; a NULL row in between shows the null path
    cols = [c + [None] for c in cols]
    expr = getattr(pkg, name)(*[f(k, D) for k in range(arity)])
    (got,) = project(pkg, ctx, [D] * arity, None, [expr], pkg.Page(*[pkg.Block(D, c) for c in cols]))
    assert got[-1] is None
    bound, worst, bad = CORPUS["bounds"][name], 0, []
    for r, (row, g, w) in enumerate(zip(rows, got, want)):
        d = X.ulp_distance(g, w)
        if d != X.INF:
            worst = max(worst, d)
        if d > (0 if row[-1] else bound):
            bad.append((row, g, w, d))
    print("%s: maximum distance from the correctly rounded result over %d arguments: %s doubles (bound %d)" % (name, len(rows), worst, bound))
    assert not bad, bad[:10]


# ---- (6) raising cases ------------------------------------------------------------------------------------------------------------------------------
def test_abs_and_round_failures(pkg, ctx):
    f, B, I, D = pkg.field, pkg.BIGINT, pkg.INTEGER, pkg.DOUBLE
    b, i = f(0, B), f(1, I)
    n = 300
    page = lambda bs, is_: pkg.Page(pkg.Block(B, bs), pkg.Block(I, is_))
    plain_b, plain_i = [r - 150 for r in range(n)], [r * 7 - 1000 for r in range(n)]
    put = lambda base, at, v: [v if r == at else x for r, x in enumerate(base)]
    BMIN, IMIN = -2**63, -2**31
    # one failing cell, for each way of failing: (expression, column, value, row, message)
    cases = [(pkg.abs_(b), 0, BMIN, 257, ABS_BIGINT), (pkg.abs_(i), 1, IMIN, 64, ABS_INTEGER),
             (pkg.round_(b, -1), 0, 2**63 - 1, 3, "numerical overflow: 9223372036854775807"), (pkg.round_(b, -14), 0, -(2**63 - 1), 299, "numerical overflow: -9223372036854775807"),
             (pkg.round_(b, -1), 0, BMIN, 0, "numerical overflow: -9223372036854775808"), (pkg.round_(i, -1), 1, 2**31 - 1, 63, "numerical overflow: 2147483647"),
             (pkg.round_(i, -5), 1, 2147450000, 130, "numerical overflow: 2147450000"), (pkg.round_(i, -3), 1, -2**31, 255, "numerical overflow: -2147483648"),
             (pkg.round_(b, -19), 0, 12, 12, "numerical overflow: 12")]
    for expr, col, v, at, message in cases:
        bs, is_ = (put(plain_b, at, v), plain_i) if col == 0 else (plain_b, put(plain_i, at, v))
        kind = "bigint" if col == 0 else "integer"
        want = checked(lambda: X.abs_(v, kind) if message.startswith("Value") else X.round_(v, int(expr.arguments[1].value), kind))
        assert isinstance(want, X.OutOfRange) and str(want) == message
        if message != "numerical overflow: 12":
            assert failure(pkg, ctx, [B, I], None, [f(0, B), expr], page(bs, is_)) == (RANGE, message, at), message
            # a NULL on the failing row gives NULL, not an error
            nb, ni = (put(bs, at, None), is_) if col == 0 else (bs, put(is_, at, None))
            got = project(pkg, ctx, [B, I], None, [expr], page(nb, ni))
            assert got[0][at] is None and sum(v is None for v in got[0]) == 1
        else:   # decimals <= -19: the first non-null row fails whatever it holds
            assert failure(pkg, ctx, [B, I], None, [expr], page(put(put(bs, 0, None), 1, None), is_)) == (RANGE, "numerical overflow: -148", 2)
    # the values next to the failing ones do not fail
    near_b, near_i = [BMIN + 1, 2**63 - 1], [IMIN + 1, 2**31 - 1]
    assert project(pkg, ctx, [B, I], None, [pkg.abs_(b), pkg.abs_(i)], page(near_b, near_i)) == [[2**63 - 1, 2**63 - 1], [2**31 - 1, 2**31 - 1]]
    near_b, near_i = [-9223372036854775804, 9223372036854775804], [1499999999, -1499999999]
    assert project(pkg, ctx, [B, I], None, [pkg.round_(b, -1), pkg.round_(i, -9), pkg.round_(i, -10)], page(near_b, near_i)) == [
        [X.round_(v, -1) for v in near_b], [X.round_(v, -9, "integer") for v in near_i], [X.round_(v, -10, "integer") for v in near_i]] == [
        [-9223372036854775800, 9223372036854775800], [1000000000, -1000000000], [0, 0]]
    # several failing projections and rows: the lowest projection index, then its first row
    bs = put(put(put(plain_b, 9, BMIN), 12, BMIN), 2, 2**63 - 1)
    exprs = [pkg.sign(b), pkg.abs_(b), pkg.round_(b, -1)]
    assert failure(pkg, ctx, [B, I], None, exprs, page(bs, plain_i)) == (RANGE, ABS_BIGINT, 9)          # projection 1 fails on rows 9 and 12, projection 2 on 2, 9 and 12
    assert failure(pkg, ctx, [B, I], None, [exprs[0], exprs[2], exprs[1]], page(bs, plain_i)) == (RANGE, "numerical overflow: 9223372036854775807", 2)
    # a filter failure comes before any projection's, with its operand
    assert failure(pkg, ctx, [B, I], pkg.round_(b, -3) > -10**18, exprs, page(bs, plain_i)) == (RANGE, "numerical overflow: 9223372036854775807", 2)
    # the filter rejects the failing rows: nothing is raised
    got = project(pkg, ctx, [B, I], pkg.between(b, -10**6, 10**6), exprs, page(bs, plain_i))
    keep = [r for r in range(n) if r not in (9, 12, 2)]
    assert got == [[X.sign(bs[r]) for r in keep], [abs(bs[r]) for r in keep], [X.round_(bs[r], -1) for r in keep]]
    # IF and COALESCE guard a failing branch
    guarded = [pkg.if_(b.eq(BMIN), pkg.constant(0, B), pkg.abs_(b)), pkg.coalesce(pkg.if_(pkg.or_(b > 10**18, b < -10**18), pkg.constant(None, B), pkg.round_(b, -1)), pkg.constant(-1, B))]
    got = project(pkg, ctx, [B, I], None, guarded, page(bs, plain_i))
    assert got == [[0 if v == BMIN else abs(v) for v in bs], [-1 if abs(v) > 10**18 else X.round_(v, -1) for v in bs]]
    # a failing row among 8,192 selected ones, in the last tile
    big = [r % 1000 for r in range(8192)]
    big[8000], big[8100] = BMIN, BMIN
    assert failure(pkg, ctx, [B], None, [pkg.abs_(f(0, B))], pkg.Page(pkg.Block(B, big))) == (RANGE, ABS_BIGINT, 8000)
    assert failure(pkg, ctx, [B], f(0, B) < 5, [pkg.round_(f(0, B), -1)], pkg.Page(pkg.Block(B, big))) == (RANGE, "numerical overflow: -9223372036854775808", 8000)
    # the same failure through the fused aggregation's factory
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 3, [B], None, [f(0, B) % 3, pkg.abs_(f(0, B))], [B], [0], [(pkg.SUM_BIGINT, 1)])
    op = fused.createOperator()
    outs, err = H.drive_pages(pkg, op, [pkg.Page(pkg.Block(B, big))])
    assert err is not None and err[0].code == RANGE and ABS_BIGINT in str(err[0])
    op.close()
    # ... and a round whose message names its operand: such a program is left to the page processor inside the fused factories
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 4, [B], None, [pkg.sign(f(0, B)), pkg.round_(f(0, B), -1)], [B], [0], [(pkg.SUM_BIGINT, 1)])
    op = fused.createOperator()
    outs, err = H.drive_pages(pkg, op, [pkg.Page(pkg.Block(B, big))])
    assert err is not None and err[0].code == RANGE and "numerical overflow: -9223372036854775808 (position 8000)" in str(err[0])
    op.close()


# ---- (7) the nested loop join's filter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["double", "bigint"])
def test_nested_loop_join_filter_with_abs(pkg, ctx, kind):
    """abs(l.x - r.y) <= k.  Over DOUBLE nothing in it can raise: the predicate is fused into the pair kernels.  Over BIGINT the subtraction and
    abs can raise: the product pieces go through the page processor.  Either way the rows are the model's."""
    f = pkg.field
    T = pkg.DOUBLE if kind == "double" else pkg.BIGINT
    conv = float if kind == "double" else int
    left = [None if r % 13 == 5 else conv((r * 37) % 101 - 50) for r in range(257)]
    right = [None if r % 7 == 3 else conv((r * 11) % 61 - 30) for r in range(65)]
    if kind == "double":
        left[1], left[2], right[0] = C.NAN, C.INF, -C.INF
    bf, bop = G.build(pkg, ctx, [T], [pkg.Page(pkg.Block(T, right))])
    filt = pkg.abs_(f(0, T) - f(1, T)) <= conv(2)
    jf = pkg.FilterProjectNestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, [T], filt, [f(0, T), f(1, T), pkg.abs_(f(0, T) - f(1, T))])
    jop = jf.createOperator()
    ctx.profile_enable(True)
    ctx.profile_reset()
    outs = pkg.to_pages(jop, [pkg.Page(pkg.Block(T, left))])
    prof = ctx.profile()
    ctx.profile_enable(False)
    prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
    jop.close()
    G.end(bf, bop, jf)
    got = sorted((tuple(r) for o in outs for r in o.rows()), key=repr)
    want = sorted(((a, b, abs(a - b)) for a in left for b in right if a is not None and b is not None and abs(a - b) <= 2), key=repr)
    assert got == want and len(want) > 100
    assert any(name.startswith("nlj_pair") for name in prof) == (kind == "double"), sorted(prof)
    assert any(name.startswith("nlj_product") for name in prof) == (kind == "bigint"), sorted(prof)

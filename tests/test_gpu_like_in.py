"""LIKE and IN in the generated kernels (jit.cpp gen_like / gen_in) against tests/like_in_expected.py: every cell is compared, as a filter
and as a BOOLEAN projection, and on the dictionary, fused-aggregation and fused-probe paths."""
import json

import numpy as np
import pytest

import like_in_cases as C
import like_in_expected as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


def project_all(pkg, ctx, page, types, exprs):
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, None, exprs)
    out = pkg.to_pages(fac.createOperator(), [page])
    return [[v for p in out for v in p.getBlock(ch).to_list()] for ch in range(len(exprs))]


def filter_positions(pkg, ctx, page, types, filt):
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, [pkg.field(len(types) - 1, pkg.BIGINT)])
    out = pkg.to_pages(fac.createOperator(), [page])
    return [int(v) for p in out for v in p.getBlock(0).values]


def like_expr(pkg, pattern, escape):
    return pkg.like(pkg.field(0, pkg.VARCHAR), pattern, escape)


def check_like(pkg, ctx, page, values, patterns, filters):
    """every pattern as a projection (12 per program); `filters` of them as the filter too"""
    V, B = pkg.VARCHAR, pkg.BIGINT
    for part in C.chunks(patterns, 12):
        got = project_all(pkg, ctx, page, [V, B], [like_expr(pkg, p, e) for p, e in part])
        for (p, e), g in zip(part, got):
            assert g == X.like_column(values, p, e), (p, e)
    for p, e in filters:
        want = X.like_column(values, p, e)
        assert filter_positions(pkg, ctx, page, [V, B], like_expr(pkg, p, e)) == [i for i, w in enumerate(want) if w], (p, e)


def test_like_boundary_page(pkg, ctx):
    """device blocks sized to the byte: the first string begins the tensor and the last one ends it.  (An allocator may round the tensor up, so
    a small over-read need not fault here: the page pins the answers at every length and anchor, not the absence of such a load.)"""
    import torch

    values = C.boundary_values()
    patterns = C.boundary_patterns()
    data = [v.encode() for v in values if v is not None]
    pool = b"".join(data)
    offs = np.zeros(len(values) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([0 if v is None else len(v.encode()) for v in values])
    d_pool = torch.tensor(list(pool), dtype=torch.uint8, device="cuda:0")
    assert d_pool.untyped_storage().nbytes() == len(pool)
    d_offs = torch.tensor(offs, dtype=torch.int32, device="cuda:0")
    d_nulls = torch.tensor([v is None for v in values], dtype=torch.uint8, device="cuda:0")
    d_rows = torch.arange(len(values), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    page = pkg.Page(pkg.DeviceBlock(pkg.VARCHAR, len(values), d_pool, d_nulls.data_ptr(), d_offs.data_ptr()), pkg.DeviceBlock(pkg.BIGINT, len(values), d_rows.data_ptr()))
    check_like(pkg, ctx, page, values, patterns, [("%ab%c%", None), ("ab%ba", None), ("%_b", None), ("a\\%c", "\\")])
    ctx.synchronize()
    # the traps, spelled out
    assert X.like("aba", "ab%ba") is False and X.like("aab", "%ab") and X.like("abab", "%ab") and X.like("ab01c0", "%ab%c%")
    for p, e in patterns[:-7]:
        if p not in ("ab%ba",):
            assert any(X.like_column(values, p, e)), p   # every pattern matches some row


RANDOM_PATTERNS = C.chunks(C.random_patterns(), 48)


@pytest.fixture(scope="module")
def random_page(pkg):
    values = C.random_values()
    return values, pkg.Page(pkg.Block(pkg.VARCHAR, values), pkg.Block(pkg.BIGINT, np.arange(len(values), dtype=np.int64)))


@pytest.mark.parametrize("part", range(len(RANDOM_PATTERNS)))
def test_like_randomised_differential(pkg, ctx, random_page, part):
    values, page = random_page
    good, raised = [], 0
    for p, e in RANDOM_PATTERNS[part]:
        try:
            X.like_regex(p, e)
            good.append((p, e))
        except X.LikeError as ex:       # a pattern the reference refuses must be refused when the factory is created, with its message
            with pytest.raises(pkg.TgpuError) as err:
                pkg.FilterAndProjectOperatorFactory(ctx, 0, [pkg.VARCHAR, pkg.BIGINT], like_expr(pkg, p, e), [])
            assert err.value.code == -1 and str(ex) in str(err.value)
            raised += 1
    assert len(good) + raised == len(RANDOM_PATTERNS[part])
    check_like(pkg, ctx, page, values, good, good[:2])


def test_like_null_pattern_and_escape(pkg, ctx, random_page):
    values, page = random_page
    V, f = pkg.VARCHAR, pkg.field
    got = project_all(pkg, ctx, page, [V, pkg.BIGINT], [pkg.like(f(0, V), pkg.constant(None, V)), pkg.like(f(0, V), "a%", pkg.constant(None, V)),
                                                       pkg.like(pkg.constant("foobar", V), "f%b__"), pkg.like(pkg.constant("foob", V), "f%b__")])
    n = len(values)
    assert got == [[None] * n, [None] * n, [True] * n, [False] * n]


@pytest.mark.parametrize("case", range(6))
def test_in_lists(pkg, ctx, case):
    name, values, lists = C.in_cases()[case]
    t = getattr(pkg, name.upper())
    B = pkg.BIGINT
    pages = {n: pkg.Page(pkg.Block(t, values[:n]), pkg.Block(B, np.arange(n, dtype=np.int64))) for n in C.ROW_COUNTS}
    for part in C.chunks(lists, 12):
        exprs = [pkg.in_(pkg.field(0, t), items) for items in part]
        fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [t, B], None, exprs)
        for n, page in pages.items():
            out = pkg.to_pages(fac.createOperator(), [page])
            for ch, items in enumerate(part):
                got = [v for p in out for v in p.getBlock(ch).to_list()]
                assert got == X.in_column(values[:n], items), (name, n, len(items), items[:8])
    for items in (lists[1], lists[6] if len(lists) > 8 else lists[-1], lists[-4]):
        want = X.in_column(values, items)
        assert filter_positions(pkg, ctx, pages[1000], [t, B], pkg.in_(pkg.field(0, t), items)) == [i for i, w in enumerate(want) if w], (name, items[:8])


def test_dictionary_and_rle_blocks(pkg, ctx):
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    entries = ["PROMO BRASS", "PROMO TIN", "STANDARD BRASS", "ab", "", "promo", "名 PROMO", None]
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 8, 1000).astype(np.int32)
    values = [entries[i] for i in ids]
    exprs = [pkg.like(f(0, V), "PROMO%"), pkg.like(f(0, V), "%BRASS"), pkg.like(f(0, V), "%O_B%"), pkg.in_(f(0, V), ["ab", "", "PROMO TIN"]),
             pkg.in_(f(0, V), ["s%d" % i for i in range(20)] + ["promo", None])]
    want = [X.like_column(values, "PROMO%"), X.like_column(values, "%BRASS"), X.like_column(values, "%O_B%"), X.in_column(values, ["ab", "", "PROMO TIN"]),
            X.in_column(values, ["s%d" % i for i in range(20)] + ["promo", None])]
    page = pkg.Page(pkg.DictionaryBlock(pkg.Block(V, entries), ids), pkg.Block(B, np.arange(1000, dtype=np.int64)))
    ctx.profile_enable(True)
    ctx.profile_reset()
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [V, B], None, exprs)
    out = pkg.to_pages(fac.createOperator(), [page])
    prof = ctx.profile()
    ctx.profile_enable(False)
    prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
    assert prof.get("dictionary_entries", {}).get("count", 0) >= 1, sorted(prof)   # the expressions ran over the 8 entries, not the 1,000 rows
    assert [[v for p in out for v in p.getBlock(ch).to_list()] for ch in range(len(exprs))] == want
    for value in ("PROMO TIN", "x", None):
        rle = pkg.Page(pkg.RunLengthEncodedBlock(pkg.Block(V, [value]), 1000), pkg.Block(B, np.arange(1000, dtype=np.int64)))
        got = project_all(pkg, ctx, rle, [V, B], exprs[:4])
        assert got == [[X.like(value, "PROMO%")] * 1000, [X.like(value, "%BRASS")] * 1000, [X.like(value, "%O_B%")] * 1000, [X.in_list(value, ["ab", "", "PROMO TIN"])] * 1000]


def test_fused_aggregation_q14_shape(pkg, ctx):
    """sum(if(type LIKE 'PROMO%', price, 0)), sum(price) under a filter with IN: FilterProjectHashAggregationOperator against the same
    rows summed on the host (the prices are small integers: every order of addition gives the same double)"""
    V, D, B, f = pkg.VARCHAR, pkg.DOUBLE, pkg.BIGINT, pkg.field
    rng = np.random.default_rng(4)
    kinds = ["PROMO BRASS", "PROMO TIN", "STANDARD BRASS", "ECONOMY PROMO", "PROM", None]
    types_ = [kinds[i] for i in rng.integers(0, 6, 1000)]
    price = rng.integers(1, 1000, 1000).astype(np.float64)
    mode = rng.integers(0, 12, 1000).astype(np.int64)
    keep = [3, 5, 7, 2**40] + list(range(100, 110))          # 14 items: the hash table in the fused module
    group = rng.integers(0, 3, 1000).astype(np.int64)         # a grouped aggregation: the global one is not fused
    projs = [pkg.if_(pkg.like(f(0, V), "PROMO%"), f(1, D), pkg.constant(0.0, D)), f(1, D),
             pkg.if_(pkg.like(f(0, V), "%O_B%S%"), f(1, D), pkg.constant(0.0, D)), f(3, B)]   # a general shape: the helpers in the fused module
    fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [V, D, B, B], pkg.in_(f(2, B), keep), projs, [B], [3],
                                                          [(pkg.SUM_DOUBLE, 0), (pkg.SUM_DOUBLE, 1), (pkg.COUNT_ALL, -1), (pkg.SUM_DOUBLE, 2)])
    page = pkg.Page(pkg.Block(V, types_), pkg.Block(D, price), pkg.Block(B, mode), pkg.Block(B, group))
    ctx.profile_enable(True)
    ctx.profile_reset()
    rows = [list(r) for pg in pkg.to_pages(fac.createOperator(), [page]) for r in pg.rows()]
    prof = ctx.profile()
    ctx.profile_enable(False)
    assert any(k.startswith("fused_") for k in prof), sorted(prof)   # the fused kernels ran, not filter/project + aggregation
    want = []
    for g in range(3):
        sel = [i for i in range(1000) if group[i] == g and X.in_list(int(mode[i]), keep)]
        want.append([g, sum(price[i] for i in sel if X.like(types_[i], "PROMO%")), sum(price[i] for i in sel), len(sel),
                     sum(price[i] for i in sel if X.like(types_[i], "%O_B%S%"))])
    assert sorted(rows) == want and all(w[1] > 0 and w[4] > 0 for w in want)


def test_fused_probe_filter(pkg, ctx):
    """FilterProjectLookupJoinOperator: LIKE over a VARCHAR column and IN over the key in the probe's filter"""
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    rng = np.random.default_rng(5)
    names = ["special requests", "no special thing", "requests special", "a special set of requests", None, ""]
    comment = [names[i] for i in rng.integers(0, 6, 1000)]
    key = rng.integers(0, 50, 1000).astype(np.int64)
    allowed = list(range(0, 50, 3))
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(B, np.arange(0, 50, 2, dtype=np.int64))))
    b.finish()
    filt = pkg.and_(pkg.like(f(1, V), "%special%requests%"), pkg.in_(f(0, B), allowed))
    fj = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [B, V], filt, [f(0, B)], [0])
    before = sum(pkg.fused_probe_launch_counts())
    out = pkg.to_pages(fj.createOperator(), [pkg.Page(pkg.Block(B, key), pkg.Block(V, comment))])
    assert sum(pkg.fused_probe_launch_counts()) > before      # the fused probe kernel ran
    got = [int(v) for p in out for v in p.getBlock(0).values]
    want = [int(k) for k, c in zip(key, comment) if X.like(c, "%special%requests%") and k in allowed and k % 2 == 0]
    assert got == want and len(want) > 10


def drain(op):
    pages = []
    for _ in range(100_000):
        if op.isFinished():
            break
        o = op.getOutput()
        if o is not None:
            pages.append(o.to_host())
            o.release()
    assert op.isFinished()
    return pages


def scan_rows():
    rng = np.random.default_rng(6)
    words = ["special requests", "PROMO BRASS", "no special thing", "a special set of requests", "", "名 requests", None]
    return [(words[int(rng.integers(0, 7))], None if i % 31 == 0 else int(rng.integers(0, 40)) * (2**33 if i % 5 == 0 else 1)) for i in range(1000)]


def scan_program(pkg):
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    items = [3, 5, None, 7 * 2**33] + list(range(10, 20))
    filt = pkg.or_(pkg.like(f(0, V), "%special%requests%"), pkg.in_(f(1, B), items))
    projs = [f(1, B), pkg.like(f(0, V), "_ req%"), pkg.in_(f(0, V), ["", "PROMO BRASS", None])]

    def want(rows):
        out = []
        for c, k in rows:
            a, b = X.like(c, "%special%requests%"), X.in_list(k, items)
            if a is True or b is True:
                out.append([k, X.like(c, "_ req%"), X.in_list(c, ["", "PROMO BRASS", None])])
        return out
    return filt, projs, want


def test_scan_with_a_page_source(pkg, ctx):
    V, B = pkg.VARCHAR, pkg.BIGINT
    rows = scan_rows()
    filt, projs, want = scan_program(pkg)
    op = pkg.ScanFilterAndProjectOperatorFactory(ctx, 0, [V, B], filt, projs).createOperator()
    pages = [pkg.Page(pkg.Block(V, [r[0] for r in part]), pkg.Block(B, [r[1] for r in part])) for part in (rows[:300], rows[300:])]
    op.addSplit(pkg.PageSource(pages))
    op.noMoreSplits()
    got = [list(r) for pg in drain(op) for r in pg.rows()]
    assert got == want(rows) and 50 < len(got) < 950


def test_scan_with_a_record_cursor(pkg, ctx):
    V, B = pkg.VARCHAR, pkg.BIGINT
    rows = scan_rows()
    filt, projs, want = scan_program(pkg)
    op = pkg.ScanFilterAndProjectOperatorFactory(ctx, 0, [V, B], filt, projs).createOperator()
    op.addSplit(pkg.RecordCursor([V, B], rows))
    op.noMoreSplits()
    got = [list(r) for pg in drain(op) for r in pg.rows()]
    assert got == want(rows)


def test_join_filter_function(pkg, ctx):
    """the join filter copies the node array, remaps its channels and appends nodes: the IN list, named by node index, must survive that.
    build (key, name), probe (key, tag): build.name LIKE '%an%' AND probe.tag IN (14 items) over the key-equal pairs"""
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    rng = np.random.default_rng(8)
    names = ["banana", "apple", "mango", "cranberry", "", None, "an"]
    bkey = [int(k) for k in rng.integers(0, 30, 200)]
    bname = [names[int(i)] for i in rng.integers(0, 7, 200)]
    pkey = [int(k) for k in rng.integers(0, 40, 500)]
    ptag = [None if i % 17 == 0 else int(t) for i, t in enumerate(rng.integers(0, 30, 500))]
    tags = list(range(0, 28, 2))
    filt = pkg.and_(pkg.like(f(1, V), "%an%"), pkg.in_(f(3, B), tags))
    bf = pkg.HashBuilderOperatorFactory(ctx, 0, [B, V], [0, 1], [0])
    bf.lookup_source_factory.setJoinFilter([B, B], filt)
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(B, bkey), pkg.Block(V, bname)))
    b.finish()
    jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, [B, B], [0])
    got = sorted(tuple(r) for pg in pkg.to_pages(jf.createOperator(), [pkg.Page(pkg.Block(B, pkey), pkg.Block(B, ptag))]) for r in pg.rows())
    want = sorted((pk, pt, bk, bn) for pk, pt in zip(pkey, ptag) for bk, bn in zip(bkey, bname)
                  if pk == bk and X.like(bn, "%an%") is True and X.in_list(pt, tags) is True)
    assert got == want and len(want) > 50


def test_pages_of_empty_strings(pkg, ctx):
    """every string empty: the pool has no bytes and a value's address may be 0; '' LIKE '_' is false all the same"""
    V, B = pkg.VARCHAR, pkg.BIGINT
    values = ["", "", None, ""] * 20
    pats = [("_", None), ("___", None), ("%", None), ("", None), ("_%", None), ("%_", None), ("a", None), ("a%", None), ("%a", None), ("%a%", None), ("a_", None), ("%_a%", None)]
    page = pkg.Page(pkg.Block(V, values), pkg.Block(B, np.arange(len(values), dtype=np.int64)))
    check_like(pkg, ctx, page, values, pats, [("_", None), ("%", None)])
    got = project_all(pkg, ctx, page, [V, B], [pkg.in_(pkg.field(0, V), ["", "a"]), pkg.in_(pkg.field(0, V), ["s%d" % i for i in range(20)] + [""])])
    assert got == [X.in_column(values, ["", "a"])] * 2


def test_device_block_over_an_empty_tensor(pkg, ctx):
    """the same with a device block whose byte tensor is empty: its data_ptr() is 0"""
    import torch

    V, B = pkg.VARCHAR, pkg.BIGINT
    n = 70
    d_pool = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    d_rows = torch.arange(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    page = pkg.Page(pkg.DeviceBlock(V, n, d_pool, None, d_offs), pkg.DeviceBlock(B, n, d_rows))
    check_like(pkg, ctx, page, [""] * n, [("_", None), ("___", None), ("%", None), ("", None), ("_%", None), ("a_", None)], [("_", None), ("", None)])
    ctx.synchronize()


# ---- the reference's pinned cases (tests/golden/like_in_vectors.json) through FilterAndProjectOperator --------------------------------
import os

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "like_in_vectors.json")))
TABLES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "expression_vectors.json")))["expression_compiler"]["value_tables"]


def test_golden_like_cases(pkg, ctx):
    """every pinned (value, pattern, escape) -> result: all values in one column, one projection per distinct pattern (each also checked
    against the restatement on every other value), a sample as the filter; then the stringLefts x stringLefts loop with escape backslash"""
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    cases = GOLD["interpreter_like"] + GOLD["like_functions"]["like"]
    raw = lambda c: bytes(c["value_bytes"]) if "value_bytes" in c else c["value"]
    values = []
    for c in cases:
        if raw(c) not in values:
            values.append(raw(c))
    as_text = [v.decode("utf-8", "surrogateescape") if isinstance(v, bytes) else v for v in values]   # the invalid byte: any byte-wise search agrees
    page = pkg.Page(pkg.Block(V, [v if isinstance(v, (bytes, type(None))) else v.encode() for v in values]), pkg.Block(B, np.arange(len(values), dtype=np.int64)))
    keys = []
    for c in cases:
        k = (c["pattern"], c["escape"], c["has_escape"])
        if k not in keys:
            keys.append(k)

    def expr(k):
        p, e, has = k
        pat = pkg.constant(None, V) if p is None else p
        return pkg.like(f(0, V), pat, pkg.constant(None, V) if (has and e is None) else e)

    checked = 0
    for part in C.chunks(keys, 12):
        got = project_all(pkg, ctx, page, [V, B], [expr(k) for k in part])
        for k, g in zip(part, got):
            assert g == [X.like(v, k[0], k[1], k[2]) for v in as_text], k
            for c in cases:
                if (c["pattern"], c["escape"], c["has_escape"]) == k:
                    assert g[values.index(raw(c))] is c["expected"], c
                    checked += 1
    assert checked == len(cases)
    for k in keys[::5]:
        want = [X.like(v, k[0], k[1], k[2]) for v in as_text]
        assert filter_positions(pkg, ctx, page, [V, B], expr(k)) == [i for i, w in enumerate(want) if w], k
    loop = GOLD["compiler_like_loop"]
    lpage = pkg.Page(pkg.Block(V, loop["values"]), pkg.Block(B, np.arange(len(loop["values"]), dtype=np.int64)))
    got = project_all(pkg, ctx, lpage, [V, B], [pkg.like(f(0, V), pkg.constant(None, V) if p is None else p, loop["escape"]) for p in loop["patterns"]])
    assert got == [[X.like(v, p, loop["escape"]) for v in loop["values"]] for p in loop["patterns"]]
    for c in GOLD["like_functions"]["errors"]:
        with pytest.raises(pkg.TgpuError) as err:
            pkg.FilterAndProjectOperatorFactory(ctx, 0, [V, B], pkg.like(f(0, V), c["pattern"], c["escape"]), [])
        assert err.value.code == -1 and c["message"] in str(err.value)


def test_golden_in_lists(pkg, ctx):
    tables = dict(TABLES, **{"smallInts+extremeInts": TABLES["smallInts"] + TABLES["extremeInts"]})
    B = pkg.BIGINT
    by_table = {}
    for c in GOLD["compiler_in"]:
        by_table.setdefault((c["type"], c["values_table"]), []).append(c)
    for (tname, table), cs in by_table.items():
        t = getattr(pkg, tname.upper())
        values = tables[table]
        page = pkg.Page(pkg.Block(t, values), pkg.Block(B, np.arange(len(values), dtype=np.int64)))
        for part in C.chunks(cs, 12):
            got = project_all(pkg, ctx, page, [t, B], [pkg.in_(pkg.field(0, t), c["items"]) for c in part])
            for c, g in zip(part, got):
                contains = [i for i in c["items"] if i is not None]
                want = [None if v is None else (True if v in contains else (None if None in c["items"] else False)) for v in values]   # the test's own expression
                assert g == want, c
        want = X.in_column(values, cs[0]["items"])
        assert filter_positions(pkg, ctx, page, [t, B], pkg.in_(pkg.field(0, t), cs[0]["items"])) == [i for i, w in enumerate(want) if w]
    for c in GOLD["compiler_huge_in"]:    # testHugeIn: the bound symbol's value against 5,000 items, with and without itself
        t = getattr(pkg, c["type"].upper())
        conv = {"integer": int, "bigint": int, "double": float, "varchar": str}[c["type"]]
        items = [conv(i) for i in range(*c["range"])]
        page = pkg.Page(pkg.Block(t, [c["value"], None, items[17]]), pkg.Block(B, np.arange(3, dtype=np.int64)))
        got = project_all(pkg, ctx, page, [t, B], [pkg.in_(pkg.field(0, t), [c["extra"]] + items), pkg.in_(pkg.field(0, t), items)])
        assert got == [[c["expected_with_extra"], None, True], [c["expected_without"], None, True]], c["type"]

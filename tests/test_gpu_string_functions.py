"""The string functions and computed VARCHAR projections on the device (jit.cpp gen_string, fp_vwrite) against tests/string_fn_expected.py:
every cell is compared, the VARCHAR blocks byte for byte with their offsets, on the flat, dictionary, scan, fused-aggregation and fused-probe
paths.  The concat-too-large and 2 GB errors cannot be reached at test sizes; they were checked by reading."""
import functools
import json
import os

import numpy as np
import pytest

import string_fn_cases as C
import string_fn_expected as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


# the restatement walks bytes in Python: each distinct (function, arguments) is computed once
substring = functools.lru_cache(maxsize=None)(X.substring)
length = functools.lru_cache(maxsize=None)(X.length)
strpos = functools.lru_cache(maxsize=None)(X.strpos)


def concat(*parts):
    out = parts[0]
    for p in parts[1:]:
        out = X.concat(out, p)
    return out


def column(block, info_bytes=None):
    """a host block as a Python list (VARCHAR: bytes); a VARCHAR block's structure is checked on the way"""
    n = block.position_count
    nulls = [block.isNull(i) for i in range(n)]
    if block.offsets is None:
        return block.to_list()
    o = block.offsets
    assert len(o) == n + 1 and o[0] == 0 and bool(np.all(np.diff(o) >= 0)), "offsets"
    if info_bytes is not None:
        assert int(o[n]) == info_bytes, "offsets[n] is the pool's byte count"
    assert all(o[i + 1] == o[i] for i in range(n) if nulls[i]), "a NULL row has no bytes"
    data = block.values.tobytes()
    return [None if nulls[i] else data[o[i]:o[i + 1]] for i in range(n)]


def run(pkg, op, pages, n_channels):
    """-> one list per output channel over all output pages"""
    outs = pkg.to_pages(op, pages, to_host=False)
    cols = [[] for _ in range(n_channels)]
    L = pkg._lib.lib()
    import ctypes
    for o in outs:
        host = o.to_host()
        for ch in range(n_channels):
            t, vb, mn = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
            pkg._lib.check(L.tgpu_output_page_block_info(o.handle, ch, ctypes.byref(t), ctypes.byref(vb), ctypes.byref(mn)))
            cols[ch] += column(host.getBlock(ch), vb.value if t.value == pkg.VARCHAR else None)
        o.release()
    return cols


def project(pkg, ctx, types, filt, exprs, page):
    return run(pkg, pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, exprs).createOperator(), [page], len(exprs))


def device_varchar(pkg, values):
    """a VARCHAR device block whose pool tensor is exactly as long as its bytes"""
    import torch

    pool = b"".join(v for v in values if v is not None)
    offs = np.zeros(len(values) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([0 if v is None else len(v) for v in values])
    d_pool = torch.tensor(list(pool), dtype=torch.uint8, device="cuda:0")
    assert d_pool.untyped_storage().nbytes() == len(pool)
    d_offs = torch.tensor(offs, dtype=torch.int32, device="cuda:0")
    d_nulls = torch.tensor([v is None for v in values], dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return pkg.DeviceBlock(pkg.VARCHAR, len(values), d_pool, d_nulls.data_ptr(), d_offs.data_ptr()), (d_pool, d_offs, d_nulls)


# ---- the operations program: every op once or more, 8 VARCHAR results -----------------------------------------------------------------------
def ops_program(pkg):
    f, V, B = pkg.field, pkg.VARCHAR, pkg.BIGINT
    x, k = f(0, V), f(1, B)
    exprs = [pkg.length(x), pkg.substr(x, 1), pkg.substr(x, 2, 3), pkg.substr(x, -3), pkg.substr(x, -9, 8), pkg.concat(x, "|"), pkg.concat(x, x),
             pkg.strpos(x, "ab"), pkg.starts_with(x, "ab"), pkg.cast(k, V), pkg.concat(pkg.substr(x, 1, 2), pkg.cast(k, V)), pkg.strpos(x, pkg.substr(x, -2))]

    def want(values, rows):
        i = lambda v: None if v is None else str(v).encode()
        return [[length(v) for v in values], [substring(v, 1) for v in values], [substring(v, 2, 3, True) for v in values], [substring(v, -3) for v in values],
                [substring(v, -9, 8, True) for v in values], [concat(v, b"|") for v in values], [concat(v, v) for v in values], [strpos(v, b"ab") for v in values],
                [X.starts_with(v, b"ab") for v in values], [i(r) for r in rows], [concat(substring(v, 1, 2, True), i(r)) for v, r in zip(values, rows)],
                [strpos(v, substring(v, -2)) for v in values]]
    return [V, B], exprs, want


FILTERS = ["none", "every_other", "keeps_none", "keeps_all"]


def filter_of(pkg, name):
    k = pkg.field(1, pkg.BIGINT)
    return {"none": None, "every_other": (k % 2).eq(0), "keeps_none": k < 0, "keeps_all": k >= 0}[name]


def kept(name, n):
    return [r for r in range(n) if name != "keeps_none" and (name != "every_other" or r % 2 == 0)]


@pytest.mark.parametrize("filt", FILTERS)
def test_boundary_page_every_op_every_row_count(pkg, ctx, filt):
    """device blocks sized to the byte (the first value begins the tensor, the last one ends it), at every row count, under each filter"""
    import torch

    types, exprs, want = ops_program(pkg)
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filter_of(pkg, filt), exprs)
    for n in C.ROW_COUNTS:
        values = C.cycle(C.boundary_values()[::-1] if n == 1 else C.boundary_values(), n)   # one row: the last value; else from the empty one on
        block, keep = device_varchar(pkg, values)
        rows = torch.arange(n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        got = run(pkg, fac.createOperator(), [pkg.Page(block, pkg.DeviceBlock(pkg.BIGINT, n, rows.data_ptr()))], len(exprs))
        ctx.synchronize()
        sel = kept(filt, n)
        expected = want(values, list(range(n)))
        for ch in range(len(exprs)):
            assert got[ch] == [expected[ch][r] for r in sel], (filt, n, ch)


@pytest.mark.parametrize("filt", ["none", "every_other"])
def test_substr_argument_pairs(pkg, ctx, filt):
    """every (start, length) pair of substring's branches on every boundary value, the arguments as columns; then the row-count edges"""
    f, V, B = pkg.field, pkg.VARCHAR, pkg.BIGINT
    values, pairs = C.boundary_values(), C.substr_pairs()
    rows = [(v, s, l) for s, l in pairs for v in values]
    x, s, l = f(0, V), f(2, B), f(3, B)
    exprs = [pkg.substr(x, s), pkg.substr(x, s, l), pkg.length(pkg.substr(x, s, l)), pkg.substr(pkg.substr(x, s), 2, l)]
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [V, B, B, B], filter_of(pkg, filt), exprs)
    for n in [len(rows)] + C.ROW_COUNTS:
        part = rows[:n] if n == len(rows) else rows[7 * n:8 * n]
        page = pkg.Page(pkg.Block(V, [r[0] for r in part]), pkg.Block(B, np.arange(n, dtype=np.int64)), pkg.Block(B, [r[1] for r in part]), pkg.Block(B, [r[2] for r in part]))
        got = run(pkg, fac.createOperator(), [page], len(exprs))
        sel = [part[r] for r in kept(filt, n)]
        assert got[0] == [substring(v, a) for v, a, b in sel], n
        assert got[1] == [substring(v, a, b, True) for v, a, b in sel], n
        assert got[2] == [length(substring(v, a, b, True)) for v, a, b in sel], n
        assert got[3] == [substring(substring(v, a), 2, b, True) for v, a, b in sel], n


def test_both_copy_paths_are_byte_identical(pkg, ctx, monkeypatch):
    """TGPU_VW_COOP_MIN is read when the kernel is generated: 0 copies every non-empty row with the whole wave, a huge value none"""
    types, exprs, want = ops_program(pkg)
    n = 1025
    values = C.cycle(C.boundary_values(), n)
    page = pkg.Page(pkg.Block(pkg.VARCHAR, values), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64)))
    results = []
    for setting in ("0", str(2**40), None):
        if setting is None:
            monkeypatch.delenv("TGPU_VW_COOP_MIN", raising=False)
        else:
            monkeypatch.setenv("TGPU_VW_COOP_MIN", setting)
        ctx.profile_enable(True)
        ctx.profile_reset()
        outs = pkg.to_pages(pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filter_of(pkg, "every_other"), exprs).createOperator(), [page])
        prof = ctx.profile()
        ctx.profile_enable(False)
        prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
        assert prof.get("project_varchar_write", {}).get("count", 0) >= 1, sorted(prof)
        assert len(outs) == 1
        blocks = [outs[0].getBlock(ch) for ch in range(len(exprs))]
        results.append([(b.values.tobytes(), None if b.offsets is None else b.offsets.tobytes(), None if b.nulls is None else b.nulls.tobytes()) for b in blocks])
        expected = want(values, list(range(n)))
        for ch, b in enumerate(blocks):
            assert column(b) == [expected[ch][r] for r in kept("every_other", n)], (setting, ch)
    assert results[0] == results[1] == results[2]


def test_edge_pages(pkg, ctx):
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    x = f(0, V)
    exprs = [pkg.substr(x, 1), pkg.concat(x, x), pkg.substr(x, 2), pkg.concat(x, "")]
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, [V, B], None, exprs)
    long_a, long_b = C.ascii_value(1025, 1), C.ascii_value(1024, 2)
    for values in ([None] * 70, [b""] * 70, [b"", None] * 35, [C.ascii_value(5000, 3)], [long_a, long_b, b"a", b"bc", b"", None, b"def", b"ghijklm", long_b, b"z"]):
        page = pkg.Page(pkg.Block(V, values, nulls=np.array([v is None for v in values], dtype=np.uint8)), pkg.Block(B, np.arange(len(values), dtype=np.int64)))
        got = run(pkg, fac.createOperator(), [page], len(exprs))
        assert got == [[substring(v, 1) for v in values], [concat(v, v) for v in values], [substring(v, 2) for v in values], [concat(v, b"") for v in values]]


def test_seeded_random_differential(pkg, ctx):
    V, B, f, c = pkg.VARCHAR, pkg.BIGINT, pkg.field, pkg.constant
    values, ints = C.random_values(), C.random_ints()
    n = len(values)
    small = [None if i % 53 == 0 else (i * 7919) % 23 - 11 for i in range(n)]
    page = pkg.Page(pkg.Block(V, values), pkg.Block(B, np.arange(n, dtype=np.int64)), pkg.Block(B, ints), pkg.Block(B, small))
    x, k, s = f(0, V), f(2, B), f(3, B)
    i = lambda v: None if v is None else str(v).encode()
    e = "é".encode()
    programs = [
        ([pkg.length(x), pkg.substr(x, s), pkg.substr(x, s, 4), pkg.strpos(x, "ab"), pkg.strpos(x, "é"), pkg.starts_with(x, "a"), pkg.concat(x, "-", pkg.cast(k, V)),
          pkg.substr(x, -5, 3), pkg.if_(pkg.starts_with(x, "a"), x, c("no", V)), pkg.coalesce(x, "n/a"), pkg.cast(k, V), pkg.length(pkg.concat(x, pkg.cast(k, V)))],
         lambda: [[length(v) for v in values], [substring(v, a) for v, a in zip(values, small)], [substring(v, a, 4, True) for v, a in zip(values, small)],
                  [strpos(v, b"ab") for v in values], [strpos(v, e) for v in values], [X.starts_with(v, b"a") for v in values],
                  [concat(v, b"-", i(a)) for v, a in zip(values, ints)], [substring(v, -5, 3, True) for v in values],
                  [v if X.starts_with(v, b"a") else b"no" for v in values], [b"n/a" if v is None else v for v in values], [i(a) for a in ints],
                  [length(concat(v, i(a))) for v, a in zip(values, ints)]]),
        ([pkg.substr(x, 2, s), pkg.strpos(pkg.substr(x, 3), "b"), pkg.length(pkg.substr(x, s, 2)) > 1, pkg.starts_with(x, pkg.substr(x, 1, 1)), pkg.concat(pkg.substr(x, -1), x),
          pkg.is_null(pkg.concat(x, pkg.cast(s, V))), pkg.substr(x, k), pkg.substr(x, 1, k), pkg.concat(pkg.cast(s, V), pkg.cast(k, V)), pkg.length(pkg.cast(k, V)),
          pkg.coalesce(pkg.substr(x, 40), "short"), pkg.in_(pkg.substr(x, 1, 1), ["a", "é", "1"])],
         lambda: [[substring(v, 2, a, True) for v, a in zip(values, small)], [strpos(substring(v, 3), b"b") for v in values],
                  [None if v is None or a is None else length(substring(v, a, 2, True)) > 1 for v, a in zip(values, small)],
                  [X.starts_with(v, substring(v, 1, 1, True)) for v in values], [concat(substring(v, -1), v) for v in values],
                  [v is None or a is None for v, a in zip(values, small)], [substring(v, a) for v, a in zip(values, ints)],
                  [substring(v, 1, a, True) for v, a in zip(values, ints)], [concat(i(a), i(b)) for a, b in zip(small, ints)], [length(i(a)) for a in ints],
                  [b"short" if v is None else substring(v, 40) for v in values],
                  [None if v is None else substring(v, 1, 1, True) in (b"a", e, b"1") for v in values]]),
    ]
    for exprs, want in programs:
        got = project(pkg, ctx, [V, B, B, B], None, exprs, page)
        for ch, w in enumerate(want()):
            assert got[ch] == w, ch
    # as a filter: views feed the existing consumers
    filt = pkg.and_(pkg.in_(pkg.substr(x, 1, 1), ["a", "b"]), pkg.length(pkg.substr(x, 2)) > 3)
    got = project(pkg, ctx, [V, B, B, B], filt, [f(1, B), pkg.substr(x, 1, 1)], page)
    rows = [r for r, v in enumerate(values) if v is not None and substring(v, 1, 1, True) in (b"a", b"b") and length(substring(v, 2)) > 3]
    assert got[0] == rows and got[1] == [substring(values[r], 1, 1, True) for r in rows] and 20 < len(rows) < n


def test_built_values(pkg, ctx):
    V, B, I, BO, f, c = pkg.VARCHAR, pkg.BIGINT, pkg.INTEGER, pkg.BOOLEAN, pkg.field, pkg.constant
    ks = C.INT64_EDGES + [None]
    n = len(ks)
    i32 = [None if k is None else max(-2**31, min(2**31 - 1, k)) for k in ks]
    flags = [None if r % 7 == 3 else r % 2 == 0 for r in range(n)]
    names = [None if r % 5 == 1 else C.ascii_value(r % 19, r) for r in range(n)]
    page = pkg.Page(pkg.Block(B, ks), pkg.Block(I, i32), pkg.Block(BO, flags), pkg.Block(V, names))
    k, j, b, x = f(0, B), f(1, I), f(2, BO), f(3, V)
    i = lambda v: None if v is None else str(v).encode()
    exprs = [pkg.concat("Customer#", pkg.cast(k, V)), pkg.cast(k, V), pkg.cast(j, V), pkg.cast(b, V),
             pkg.if_(b, pkg.concat(x, "-", pkg.cast(k, V), "-", x), pkg.cast(j, V)),              # built values of 5 and 1 pieces
             pkg.if_(b, x, pkg.concat("#", pkg.cast(k, V))),                                     # a view and a built value
             pkg.coalesce(pkg.concat(x, "z"), pkg.cast(b, V)),                                    # a null-producing concat, then a view
             pkg.coalesce(pkg.concat(x, pkg.cast(k, V)), pkg.concat("none:", pkg.cast(j, V), "!")),
             pkg.length(pkg.concat("Customer#", pkg.cast(k, V))), pkg.is_null(pkg.concat(x, pkg.cast(k, V)))]
    got = project(pkg, ctx, [B, I, BO, V], None, exprs, page)
    want = [[concat(b"Customer#", i(a)) for a in ks], [i(a) for a in ks], [i(a) for a in i32], [X.cast_boolean(a) for a in flags],
            [concat(v, b"-", i(a), b"-", v) if fl else i(a32) for v, a, a32, fl in zip(names, ks, i32, flags)],
            [v if fl else concat(b"#", i(a)) for v, a, fl in zip(names, ks, flags)],
            [concat(v, b"z") if v is not None else X.cast_boolean(fl) for v, fl in zip(names, flags)],
            [concat(v, i(a)) if concat(v, i(a)) is not None else concat(b"none:", i(a32), b"!") for v, a, a32 in zip(names, ks, i32)],
            [None if a is None else len(b"Customer#") + len(i(a)) for a in ks], [v is None or a is None for v, a in zip(names, ks)]]
    for ch, w in enumerate(want):
        assert got[ch] == w, ch
    assert {len(i(a)) - (a < 0) for a in ks if a is not None} == set(range(1, 20))   # every digit count


def test_dictionary_input(pkg, ctx):
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    entries = [b"13-555-0100", "名古屋 PROMO".encode(), b"", None, C.ascii_value(300, 5), b"31-999"]
    rng = np.random.default_rng(3)
    ids = rng.integers(0, len(entries), 1000).astype(np.int32)
    values = [entries[i] for i in ids]
    x = f(0, V)
    exprs = [pkg.substr(x, 1, 2), pkg.concat(x, "#", x), pkg.length(x), f(1, B)]
    want = [[substring(v, 1, 2, True) for v in values], [concat(v, b"#", v) for v in values], [length(v) for v in values], list(range(1000))]
    rows = pkg.Block(B, np.arange(1000, dtype=np.int64))
    for filt, sel in ((None, list(range(1000))), (pkg.starts_with(x, "1"), [r for r, v in enumerate(values) if v is not None and v[:1] == b"1"])):
        op = pkg.FilterAndProjectOperatorFactory(ctx, 0, [V, B], filt, exprs).createOperator()
        got = run(pkg, op, [pkg.Page(pkg.DictionaryBlock(pkg.Block(V, entries), ids), rows)], len(exprs))
        assert pkg._lib.lib().tgpu_debug_dictionary_pages(op.handle) == 1      # evaluated once per entry, gathered by id
        assert got == [[w[r] for r in sel] for w in want]
        flat = project(pkg, ctx, [V, B], filt, exprs, pkg.Page(pkg.Block(V, values), rows))
        assert flat == got


def profile_of(ctx, fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = fn()
    prof = ctx.profile()
    ctx.profile_enable(False)
    return out, (json.loads(prof) if isinstance(prof, (str, bytes)) else prof)


def phone_rows(n=1000):
    rng = np.random.default_rng(9)
    phones = [None if i % 41 == 0 else ("%02d-%03d-555" % (int(rng.integers(10, 35)), i)).encode() for i in range(n)]
    bal = rng.integers(-1000, 1000, n).astype(np.int64)
    return phones, bal


def test_group_by_a_computed_varchar_key(pkg, ctx):
    """the Q22 shape: GROUP BY substr(c_phone, 1, 2) with count(*) and sum(bigint); the fused factory runs the unfused composition"""
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    phones, bal = phone_rows()
    page = lambda: pkg.Page(pkg.Block(V, phones), pkg.Block(B, bal))
    filt = pkg.in_(pkg.substr(f(0, V), 1, 2), ["13", "31", "23", "29", "30", "18", "17"])
    projs = [pkg.substr(f(0, V), 1, 2), f(1, B)]
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [V, B], filt, projs, [V], [0], aggs)
    got = sorted((r[0].encode(), r[1], r[2]) for pg in pkg.to_pages(fused.createOperator(), [page()]) for r in pg.rows())
    mid = pkg.to_pages(pkg.FilterAndProjectOperatorFactory(ctx, 1, [V, B], filt, projs).createOperator(), [page()])
    two = sorted((r[0].encode(), r[1], r[2]) for pg in pkg.to_pages(pkg.HashAggregationOperatorFactory(ctx, 2, [V], [0], aggs).createOperator(), mid) for r in pg.rows())
    want = {}
    for p, b in zip(phones, bal):
        key = substring(p, 1, 2, True)
        if key in (b"13", b"31", b"23", b"29", b"30", b"18", b"17"):
            c, s = want.get(key, (0, 0))
            want[key] = (c + 1, s + int(b))
    assert got == two == sorted((k, c, s) for k, (c, s) in want.items()) and len(want) == 7


def test_fused_paths_take_string_functions_in_their_filters(pkg, ctx):
    """a string function over a view inside the filter keeps the fused kernels (their profile scopes); the results equal the unfused operators"""
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    phones, bal = phone_rows()
    grp = (np.arange(1000) % 3).astype(np.int64)
    filt = pkg.and_(pkg.starts_with(f(0, V), "1"), pkg.strpos(pkg.substr(f(0, V), 4), "5") > 0)
    keep = [r for r, p in enumerate(phones) if p is not None and p[:1] == b"1" and strpos(substring(p, 4), b"5") > 0]
    # aggregation
    page = pkg.Page(pkg.Block(V, phones), pkg.Block(B, bal), pkg.Block(B, grp))
    projs = [f(2, B), f(1, B), pkg.length(f(0, V))]
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1), (pkg.SUM_BIGINT, 2)]
    fused = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [V, B, B], filt, projs, [B], [0], aggs)
    rows, prof = profile_of(ctx, lambda: sorted(tuple(r) for pg in pkg.to_pages(fused.createOperator(), [page]) for r in pg.rows()))
    assert any(k.startswith("fused_") for k in prof), sorted(prof)
    want = sorted((g, sum(1 for r in keep if grp[r] == g), sum(int(bal[r]) for r in keep if grp[r] == g), sum(length(phones[r]) for r in keep if grp[r] == g)) for g in range(3))
    assert rows == want and 100 < len(keep) < 900
    # join: build keys 0, 2, 4, ...; probe key = row % 50
    key = (np.arange(1000) % 50).astype(np.int64)
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(B, np.arange(0, 50, 2, dtype=np.int64))))
    b.finish()
    ppage = pkg.Page(pkg.Block(V, phones), pkg.Block(B, key))
    fj = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [V, B], filt, [f(1, B), pkg.length(f(0, V))], [0])
    before = sum(pkg.fused_probe_launch_counts())
    got = [tuple(r) for pg in pkg.to_pages(fj.createOperator(), [ppage]) for r in pg.rows()]
    assert sum(pkg.fused_probe_launch_counts()) > before      # the fused probe kernel ran
    assert got == [(int(key[r]), length(phones[r]), int(key[r])) for r in keep if key[r] % 2 == 0] and len(got) > 50


def test_fused_join_with_a_computed_varchar_output(pkg, ctx):
    """a computed VARCHAR among the probe output channels keeps the unfused composition: the factory constructs, runs and equals the pair"""
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    phones, _ = phone_rows()
    key = (np.arange(1000) % 50).astype(np.int64)
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(B, np.arange(0, 50, 2, dtype=np.int64))))
    b.finish()
    page = lambda: pkg.Page(pkg.Block(V, phones), pkg.Block(B, key))
    filt = f(1, B) > 3
    projs = [f(1, B), pkg.substr(f(0, V), 1, 2), pkg.concat("Customer#", pkg.cast(f(1, B), V))]
    fj = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [V, B], filt, projs, [0])
    got = [tuple(r) for pg in pkg.to_pages(fj.createOperator(), [page()]) for r in pg.rows()]
    mid = pkg.to_pages(pkg.FilterAndProjectOperatorFactory(ctx, 3, [V, B], filt, projs).createOperator(), [page()])
    two = [tuple(r) for pg in pkg.to_pages(pkg.LookupJoinOperatorFactory(ctx, 4, bf.lookup_source_factory, [B, V, V], [0]).createOperator(), mid) for r in pg.rows()]
    dec = lambda v: None if v is None else v.decode()
    want = [(int(k), dec(substring(p, 1, 2, True)), "Customer#%d" % k, int(k)) for p, k in zip(phones, key) if k > 3 and k % 2 == 0]
    assert got == two == want and len(want) > 100


def test_scan_filter_and_project(pkg, ctx):
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    phones, bal = phone_rows()
    filt = pkg.starts_with(f(0, V), "2")
    exprs = [pkg.substr(f(0, V), 4), pkg.concat(pkg.substr(f(0, V), 1, 2), ":", pkg.cast(f(1, B), V)), pkg.length(f(0, V))]
    op = pkg.ScanFilterAndProjectOperatorFactory(ctx, 0, [V, B], filt, exprs).createOperator()
    op.addSplit(pkg.PageSource([pkg.Page(pkg.Block(V, phones[a:b]), pkg.Block(B, bal[a:b])) for a, b in ((0, 300), (300, 1000))]))
    op.noMoreSplits()
    pages = []
    for _ in range(100_000):
        if op.isFinished():
            break
        o = op.getOutput()
        if o is not None:
            pages.append(o.to_host())
            o.release()
    assert op.isFinished()
    got = [[v for pg in pages for v in column(pg.getBlock(ch))] for ch in range(3)]
    sel = [r for r, p in enumerate(phones) if p is not None and p[:1] == b"2"]
    assert got == [[substring(phones[r], 4) for r in sel], [concat(substring(phones[r], 1, 2, True), b":", str(int(bal[r])).encode()) for r in sel],
                   [length(phones[r]) for r in sel]] and len(sel) > 100


def test_golden_cases_on_the_device(pkg, ctx):
    """the reference's pinned literals (tests/golden/string_function_vectors.json) through FilterAndProjectOperator, as column values"""
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "string_function_vectors.json")))
    V, B, f = pkg.VARCHAR, pkg.BIGINT, pkg.field
    enc = lambda s: None if s is None else s.encode()
    cases = gold["substr"]
    page = pkg.Page(pkg.Block(V, [enc(c["value"]) for c in cases]), pkg.Block(B, [c["start"] for c in cases]), pkg.Block(B, [c["length"] for c in cases]))
    got = project(pkg, ctx, [V, B, B], None, [pkg.substr(f(0, V), f(1, B)), pkg.substr(f(0, V), f(1, B), f(2, B))], page)
    for r, c in enumerate(cases):
        assert got[0 if c["length"] is None else 1][r] == enc(c["expected"]), c
    cases = gold["strpos"] + [dict(c, substring=c["prefix"]) for c in gold["starts_with"]]
    page = pkg.Page(pkg.Block(V, [enc(c["value"]) for c in cases]), pkg.Block(V, [enc(c["substring"]) for c in cases]))
    got = project(pkg, ctx, [V, V], None, [pkg.strpos(f(0, V), f(1, V)), pkg.starts_with(f(0, V), f(1, V)), pkg.concat(f(0, V), f(1, V)), pkg.length(f(0, V))], page)
    for r, c in enumerate(cases):
        if "prefix" in c:
            assert got[1][r] is c["expected"], c
        else:
            assert got[0][r] == c["expected"], c
        assert got[2][r] == X.concat(enc(c["value"]), enc(c["substring"])) and got[3][r] == X.length(enc(c["value"]))
    for c in gold["length"]:
        one = project(pkg, ctx, [V, V], None, [pkg.length(f(0, V))], pkg.Page(pkg.Block(V, [enc(c["value"])]), pkg.Block(V, [b""])))
        assert one == [[c["expected"]]], c

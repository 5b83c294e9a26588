"""StreamingAggregationOperator on the GPU through the C ABI against the plain Python model (tests/streaming_aggregation_expected.py): the
reference's six test cases, one stream under many page cuts, the edges of the detection kernel's tile and of a wave, long runs, every key
type alone and combined, every aggregate function with and without a mask, PARTIAL -> FINAL, block encodings, the route by profile scopes,
memory, output cuts, errors and lifecycle.  Keys are compared bit for bit (key_cases.same_bits), DOUBLE results by their bits."""
import json
import os

import numpy as np
import pytest

import key_cases as K
import streaming_aggregation_expected as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_aggregation_vectors.json")
T = 2048                      # rows of one tile of the detection kernels: csrc/streaming_agg.h kSaggTile
ORD_HANDOFF_ROWS = 4096       # csrc/agg.h kOrdHandoffRows
INVALID_ARGUMENT, OUT_OF_RANGE, INTERNAL = -1, -2, -5
B, I, DT, D, BO, V = K.BIGINT, K.INTEGER, K.DATE, K.DOUBLE, K.BOOLEAN, K.VARCHAR


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


def to_page(pkg, cols):
    return pkg.Page(*[K.to_block(pkg, c) for c in cols], position_count=cols[0].n)


def types_of(page):
    return [c.type for c in page]


def output_types(key_types, aggs, step):
    out = list(key_types)
    for a in aggs:
        f = a[0]
        value = B if f in (S.SUM_BIGINT, S.MIN_BIGINT, S.MAX_BIGINT) else D
        if f in (S.COUNT_ALL, S.COUNT_COLUMN):
            out.append(B)
        elif step == S.PARTIAL:
            out += [B, value]
        else:
            out.append(value)
    return out


def drive(pkg, ctx, types, channels, aggs, pages, step=S.SINGLE, convert=None):
    """the reference's driver loop (OperatorAssertion.toPages); the output pages are coalesced on the device (MergePagesOperator, flushed at
    finish only) and come to the host as ONE page.  -> the output columns as KeyCols (None: no output row)"""
    convert = convert or (lambda p: to_page(pkg, p))
    out_types = output_types([types[c] for c in channels], aggs, step)
    fac = pkg.StreamingAggregationOperatorFactory(ctx, 7, types, channels, step, aggs)
    cfac = pkg.MergePagesOperatorFactory(ctx, 8, out_types, 1 << 40, 0x7FFFFFFF, 1 << 41)
    op, collect = fac.createOperator(), cfac.createOperator()

    def pull():
        o = op.getOutput()
        if o is not None:
            assert o.position_count > 0
            collect.addInput(o)
            o.release()
            return True
        return False

    for p in pages:
        assert op.needsInput() and not op.isFinished()
        op.addInput(convert(p))
        while pull():
            pass
    op.finish()
    while not op.isFinished():
        assert not op.needsInput()
        assert pull()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    collect.finish()
    o = collect.getOutput()
    cols = None
    if o is not None:
        host = o.to_host()
        cols = [K.from_block(host.getBlock(c)) for c in range(len(out_types))]
        assert [c.type for c in cols] == out_types
        o.release()
    assert collect.isFinished()
    for h in (op, collect, fac, cfac):
        h.close()
    return cols


def value_tokens(col, nan_is_one=False):
    toks = K.cells(col)
    if nan_is_one and col.type == D:
        return [v if v is None or not K.is_nan_bits(v) else "nan" for v in toks]
    return toks


def want_token(v, nan_is_one=False):
    if v is None:
        return None
    if isinstance(v, float):
        return "nan" if nan_is_one and v != v else S.double_bits(v)
    return int(v) % 2**64   # key_cases.cells gives a BIGINT's raw bits


def assert_matches(cols, pages, channels, aggs, step=S.SINGLE, want=None):
    """the operator's output columns against the model's rows: key cells bit for bit, values bit for bit (the NaN of a min / max: any NaN)"""
    want = S.aggregate(pages, channels, aggs, step) if want is None else want
    if not want:
        assert cols is None
        return want
    assert cols is not None and cols[0].n == len(want), (None if cols is None else cols[0].n, len(want))
    keys = S.key_cells(pages, channels, want)
    nk = len(channels)
    for k in range(nk):
        want_col = K.col_from_tokens(cols[k].type, [cell[k] for cell in keys])
        assert K.same_bits(cols[k], want_col), "key channel %d" % k
    ch = nk
    for a in aggs:
        width = 1 if (a[0] in (S.COUNT_ALL, S.COUNT_COLUMN) or step != S.PARTIAL) else 2
        loose = a[0] in (S.MIN_DOUBLE, S.MAX_DOUBLE)
        for j in range(width):
            got = value_tokens(cols[ch], loose)
            exp = [want_token(r.values[ch - nk], loose) for r in want]
            bad = [i for i in range(len(exp)) if got[i] != exp[i]]
            assert not bad, ("aggregate %r channel %d" % (a, ch), bad[:5], [got[i] for i in bad[:5]], [exp[i] for i in bad[:5]])
            ch += 1
    return want


def cut(cols, edges):
    """the stream's columns cut into pages at `edges` (ascending row numbers; equal neighbours give an empty page)"""
    n = cols[0].n
    edges = [0] + list(edges) + [n]
    return [[K.take(c, np.arange(a, b)) for c in cols] for a, b in zip(edges, edges[1:])]


# ---- golden cases -------------------------------------------------------------------------------------------------------------------------
def golden_cases():
    return json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_golden_cases(pkg, ctx, case):
    types, pages = S.golden_pages(case)
    channels, aggs, step = case["group_by_channels"], S.golden_aggs(case), S.STEP_CODES[case["step"]]
    cols = drive(pkg, ctx, types, channels, aggs, pages, step)
    expected = S.golden_expected(case)
    if not expected:
        assert cols is None
        return
    key_type = types[channels[0]]
    if key_type == V:
        assert cols[0].values == [r[0] for r in expected]
    else:
        got = [None if v is None else ("NaN" if K.is_nan_bits(v) else K.bits_to_doubles([v])[0].item()) for v in K.cells(cols[0])]
        assert got == [r[0] for r in expected]
    assert cols[1].nulls is None and cols[1].values.tolist() == [r[1] for r in expected]
    assert cols[2].values.tolist() == [r[2] for r in expected] and (cols[2].nulls is None or not cols[2].nulls.any())
    if case["name"] != "testLargeInputPage":   # (the model agrees as well; the million rows are covered by the literal expectation)
        assert_matches(cols, pages, channels, aggs, step)


# ---- one stream, many page cuts -----------------------------------------------------------------------------------------------------------
def clustered_double_stream(seed, rows):
    """~rows rows of runs of 1..7 rows over a DOUBLE key: run i is a zero run (both signs inside), a NaN run (several payloads inside), a NULL
    run (over other bytes) or the number i; neighbours always differ.  Values: a BIGINT and an order-sensitive DOUBLE, both with nulls."""
    rng = np.random.default_rng(seed)
    lengths = []
    while sum(lengths) < rows:
        lengths.append(int(rng.integers(1, 8)))
    run = np.repeat(np.arange(len(lengths)), lengths)
    n = len(run)
    kind = run % 7
    bits = run.astype(np.float64).view(np.uint64).copy()
    zero, nan, null = kind == 0, kind == 2, kind == 5
    bits[zero] = np.where(rng.integers(0, 2, int(zero.sum())) == 0, np.uint64(K.NEG_ZERO), np.uint64(K.POS_ZERO))
    bits[nan] = np.array(K.NAN_BITS, dtype=np.uint64)[rng.integers(0, 4, int(nan.sum()))]
    bits[null] = rng.integers(0, 2**63, int(null.sum())).astype(np.uint64)
    key = K.KeyCol(D, bits.view(np.float64), null.astype(np.uint8))
    big = K.KeyCol(B, rng.integers(-10**12, 10**12, n), (rng.random(n) < 0.1).astype(np.uint8))
    dbl = K.KeyCol(D, rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n), (rng.random(n) < 0.1).astype(np.uint8))
    ends = np.cumsum(lengths)[:-1]
    return [key, big, dbl], ends


CUT_AGGS = [(S.COUNT_ALL, -1), (S.SUM_DOUBLE, 2), (S.COUNT_COLUMN, 1), (S.AVG_BIGINT, 1)]


@pytest.fixture(scope="module")
def cut_stream():
    cols, ends = clustered_double_stream(5, 20_000)
    return cols, ends


def values_of(rows):
    return [tuple(S.value_token(v) for v in r.values) for r in rows]


@pytest.mark.parametrize("cuts", ["one_page", "one_row_pages", "at_run_ends", "before_run_ends", "after_run_ends"])
def test_page_cuts_do_not_change_the_rows(pkg, ctx, cut_stream, cuts):
    cols, ends = cut_stream
    n = cols[0].n
    edges = {"one_page": [], "one_row_pages": list(range(1, n)), "at_run_ends": ends.tolist(), "before_run_ends": sorted(set((ends - 1)[ends - 1 > 0].tolist())),
             "after_run_ends": sorted(set((ends + 1)[ends + 1 < n].tolist()))}[cuts]
    pages = cut(cols, edges)
    got = drive(pkg, ctx, types_of(cols), [0], CUT_AGGS, pages)
    want = assert_matches(got, pages, [0], CUT_AGGS)
    # the values are those of the uncut stream; the key cells follow the row rule, which the cuts move
    whole = S.aggregate([cols], [0], CUT_AGGS)
    assert values_of(want) == values_of(whole)
    if cuts == "at_run_ends":   # every group is flushed by the next page's first row: it takes its LAST row
        at = np.concatenate([[0], ends])
        assert [(r.page, r.row) for r in want] == [(i, int(e - s) - 1) for i, (s, e) in enumerate(zip(at, np.concatenate([ends, [n]])))]
    if cuts == "one_page":
        assert [r.row for r in want[:-1]] == np.concatenate([[0], ends])[:-1].tolist() and want[-1].row == n - 1


def test_the_cut_stream_makes_the_chosen_row_visible(cut_stream):
    """(no GPU work) inside one run the key's bits differ, so first row and last row are told apart"""
    cols, ends = cut_stream
    bits = cols[0].values.view(np.uint64)
    at = np.concatenate([[0], ends, [cols[0].n]])
    differing = sum(1 for s, e in zip(at, at[1:]) if e - s > 1 and cols[0].nulls[s] == 0 and bits[s] != bits[e - 1])
    assert differing > 200


# ---- tile and wave edges ------------------------------------------------------------------------------------------------------------------
def stream_with_heads(sizes, heads_in_page, rng):
    """pages of the given sizes; a row is a head where heads_in_page(page index, size) says so (row 0 of a page: only if listed)"""
    keys, cur = [], 0
    for p, size in enumerate(sizes):
        h = set(heads_in_page(p, size))
        for r in range(size):
            if r in h or (p == 0 and r == 0):
                cur += 1
            keys.append(cur)
    keys = np.array(keys, dtype=np.int64)
    n = len(keys)
    cols = [K.KeyCol(B, keys), K.KeyCol(B, rng.integers(-1000, 1000, n)), K.KeyCol(D, rng.standard_normal(n))]
    return cut(cols, np.cumsum(sizes)[:-1].tolist())


EDGE_AGGS = [(S.COUNT_ALL, -1), (S.SUM_BIGINT, 1), (S.SUM_DOUBLE, 2)]


@pytest.mark.parametrize("first_row_heads", [True, False])
def test_tile_and_wave_edges(pkg, ctx, first_row_heads):
    rng = np.random.default_rng(8)
    sizes = [T - 1, T, T + 1, 2 * T + 1, 63, 64, 65, 2 * T + 1, T + 1]
    edges = (62, 63, 64, 65, 127, 128, T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T)

    def heads(p, size):
        if p == 7:
            return range(size)                          # a page of all heads
        if p == 8:
            return [0] if first_row_heads else []       # a page that is one single run
        h = [r for r in edges if r < size] + [size - 1]  # a head on the first / last row of a tile and of a wave, and on the page's last row
        return h + ([0] if first_row_heads or p % 2 == 0 else [])

    pages = stream_with_heads(sizes, heads, rng)
    got = drive(pkg, ctx, [B, B, D], [0], EDGE_AGGS, pages)
    want = assert_matches(got, pages, [0], EDGE_AGGS)
    assert len(want) > 2 * T


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_one_page_of_every_edge_size(pkg, ctx, n):
    rng = np.random.default_rng(n)
    for keys in (np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64) // 2):
        cols = [K.KeyCol(B, keys), K.KeyCol(B, rng.integers(-1000, 1000, n)), K.KeyCol(D, rng.standard_normal(n))]
        assert_matches(drive(pkg, ctx, [B, B, D], [0], EDGE_AGGS, [cols]), [cols], [0], EDGE_AGGS)


# ---- long runs ----------------------------------------------------------------------------------------------------------------------------
def sorted_order_sum(values):
    s = 0.0
    for v in sorted(values):
        s += v
    return s


def test_a_long_group_over_three_pages_sums_in_row_order(pkg, ctx):
    """one group of 3 x kOrdHandoffRows + 5 rows (beyond the lane-per-group kernel's hand-off and the 2048-row accumulate tile) between small
    groups, over three pages; first with pages that are almost one group (the chained kernel), then inside pages of many small groups (the hand-off)"""
    rng = np.random.default_rng(3)
    long_rows = 3 * ORD_HANDOFF_ROWS + 5
    for small_before, small_after, edges in ((3, 3, [5000, 5000 + ORD_HANDOFF_ROWS]), (3000, 3000, [3000 + 4200, 3000 + 4200 + 4100])):
        keys = np.concatenate([np.arange(small_before) // 3, np.full(long_rows, 10**6), 10**7 + np.arange(small_after) // 2]).astype(np.int64)
        n = len(keys)
        dbl = rng.standard_normal(n) * 10.0 ** rng.integers(-10, 11, n)
        cols = [K.KeyCol(B, keys), K.KeyCol(D, dbl), K.KeyCol(B, rng.integers(-10**15, 10**15, n))]
        pages = cut(cols, edges)
        aggs = [(S.SUM_DOUBLE, 1), (S.AVG_DOUBLE, 1), (S.SUM_BIGINT, 2), (S.COUNT_ALL, -1)]
        want = assert_matches(drive(pkg, ctx, [B, D, B], [0], aggs, pages), pages, [0], aggs)
        long_row = [r for r in want if r.values[3] == long_rows][0]
        addends = dbl[keys == 10**6].tolist()
        assert long_row.values[0] != sorted_order_sum(addends)   # the order matters for these addends


def test_single_grouping_value_with_an_empty_page_between(pkg, ctx):
    """testSingleGroupingValue's shape: one group over pages of 5, 3, 0 and 2 rows; DOUBLE addends whose sum depends on the order"""
    vals = np.array([1e308, 1e308, -1e308, 1.0, 1e-300, -1e308, 3.5, 1e16, 1.0, -1e16])
    cols = [K.KeyCol(BO, (np.arange(10) % 2 == 0).astype(np.uint8)), K.KeyCol(V, ["a"] * 10), K.KeyCol(D, vals)]
    pages = cut(cols, [5, 8, 8])
    assert [p[0].n for p in pages] == [5, 3, 0, 2]
    aggs = [(S.COUNT_COLUMN, 0), (S.SUM_DOUBLE, 2)]
    want = assert_matches(drive(pkg, ctx, [BO, V, D], [1], aggs, pages), pages, [1], aggs)
    assert len(want) == 1 and want[0].values[0] == 10 and want[0].values[1] == float("inf") and want[0].values[1] != sorted_order_sum(vals.tolist())
    assert (want[0].page, want[0].row) == (3, 1)


# ---- every key type, alone and combined ---------------------------------------------------------------------------------------------------
KEY_CASES = {"BIGINT": ([B], [(-5, 5)]), "INTEGER": ([I], [(-5, 5)]), "DATE": ([DT], [(9000, 9008)]), "DOUBLE": ([D], [(-3, 4)]), "BOOLEAN": ([BO], [None]),
             "VARCHAR": ([V], [(0, 8)]), "DOUBLE_BIGINT": (K.KEY_SCHEMAS["DOUBLE_BIGINT"], K.SCHEMA_DOMAINS["DOUBLE_BIGINT"]),
             "BOOLEAN_VARCHAR_VARCHAR": (K.KEY_SCHEMAS["BOOLEAN_VARCHAR_VARCHAR"], K.SCHEMA_DOMAINS["BOOLEAN_VARCHAR_VARCHAR"]),
             "VARCHAR_DOUBLE_BOOLEAN_DATE": (K.KEY_SCHEMAS["VARCHAR_DOUBLE_BOOLEAN_DATE"], K.SCHEMA_DOMAINS["VARCHAR_DOUBLE_BOOLEAN_DATE"])}


def clustered_keys(rng, types, domains, runs, null_frac):
    """run keys drawn from small domains (so keys repeat and come back: A, B, A), each run 1..6 rows; inside a run a DOUBLE cell varies in
    its NaN payload / the sign of its zero and a NULL cell lies over varying bytes"""
    heads = K.key_page(rng, types, runs, domains, null_frac, extremes=False)
    if types == [V]:   # values that differ only in length or in the last byte, and the empty string next to NULL
        lead = ["", None, "", "a", "ab", "ac", "a", None, None, ""]
        heads = [K.KeyCol(V, lead + heads[0].values[len(lead):])]
    lengths = rng.integers(1, 7, runs)
    idx = np.repeat(np.arange(runs), lengths)
    cols = [K.take(c, idx) for c in heads]
    n = len(idx)
    for c in cols:
        if c.type != D:
            continue
        bits = c.values.view(np.uint64).copy()
        nan = np.array([K.is_nan_bits(int(b)) for b in bits])
        zero = (bits == K.NEG_ZERO) | (bits == K.POS_ZERO)
        bits[nan] = np.array(K.NAN_BITS, dtype=np.uint64)[rng.integers(0, 4, int(nan.sum()))]
        bits[zero] = np.where(rng.integers(0, 2, int(zero.sum())) == 0, np.uint64(K.NEG_ZERO), np.uint64(K.POS_ZERO))
        if c.nulls is not None:
            under = c.nulls != 0
            bits[under] = rng.integers(0, 2**63, int(under.sum())).astype(np.uint64)
        c.values = bits.view(np.float64)
    return cols, n


@pytest.mark.parametrize("null_frac", [0.05, 0.3])
@pytest.mark.parametrize("name", sorted(KEY_CASES))
def test_every_key_type(pkg, ctx, name, null_frac):
    types, domains = KEY_CASES[name]
    rng = np.random.default_rng(K._seed(name, 31) + int(null_frac * 100))
    keys, n = clustered_keys(rng, types, domains, 1500, null_frac)
    nk = len(types)
    vals = [K.KeyCol(B, rng.integers(-10**9, 10**9, n), (rng.random(n) < 0.1).astype(np.uint8)), K.KeyCol(D, rng.standard_normal(n) * 10.0 ** rng.integers(-5, 6, n))]
    cols = keys + vals
    edges = sorted(rng.choice(np.arange(1, n), 6, replace=False).tolist())
    edges = edges[:3] + [edges[2], edges[2] + 1] + edges[3:]   # an empty page and a page of one row
    pages = cut(cols, sorted(edges))
    aggs = [(S.COUNT_ALL, -1), (S.SUM_BIGINT, nk), (S.SUM_DOUBLE, nk + 1)]
    channels = list(range(nk))
    want = assert_matches(drive(pkg, ctx, types_of(cols), channels, aggs, pages), pages, channels, aggs)
    ids = S.run_groups(pages, channels)
    assert len(want) == ids[-1] + 1
    if name != "BOOLEAN":
        toks = [t for p in pages if p[0].n for t in S.key_tokens(p, channels)]
        firsts = [toks[i] for i in range(n) if i == 0 or ids[i] != ids[i - 1]]
        assert len(set(firsts)) < len(firsts)   # some key comes back later and is a new group


def test_key_channels_need_not_lead_the_page(pkg, ctx):
    rng = np.random.default_rng(12)
    keys, n = clustered_keys(rng, [V, I], [(0, 6), (0, 3)], 800, 0.1)
    cols = [K.KeyCol(D, rng.standard_normal(n)), keys[0], K.KeyCol(B, rng.integers(0, 100, n)), keys[1]]
    aggs = [(S.SUM_DOUBLE, 0), (S.MAX_BIGINT, 2)]
    pages = cut(cols, [100, 101, 700])
    assert_matches(drive(pkg, ctx, types_of(cols), [3, 1], aggs, pages), pages, [3, 1], aggs)


# ---- every aggregate function -------------------------------------------------------------------------------------------------------------
ALL_FUNCTIONS = [(S.COUNT_ALL, -1), (S.COUNT_COLUMN, 2), (S.SUM_BIGINT, 1), (S.SUM_DOUBLE, 2), (S.AVG_BIGINT, 1), (S.AVG_DOUBLE, 2), (S.MIN_BIGINT, 1), (S.MAX_BIGINT, 1),
                 (S.MIN_DOUBLE, 3), (S.MAX_DOUBLE, 3)]


@pytest.fixture(scope="module")
def function_stream():
    """[key BIGINT, BIGINT with nulls, finite DOUBLE with nulls (sums), DOUBLE with NaN / zeros of both signs / infinities and nulls (min, max),
    mask BOOLEAN with nulls]; one group whose mask is false throughout, one whose inputs are all null, one whose doubles are all NaN"""
    rng = np.random.default_rng(17)
    lengths = rng.integers(1, 40, 600)
    key = np.repeat(rng.permutation(600), lengths).astype(np.int64)
    n = len(key)
    run = np.repeat(np.arange(600), lengths)
    big_nulls, dbl_nulls, mm_nulls = ((rng.random(n) < 0.15).astype(np.uint8) for _ in range(3))
    mm = rng.integers(-5, 6, n).astype(np.float64)
    for special in (np.inf, -np.inf, np.nan, -0.0, 0.0):
        mm[rng.integers(0, n, n // 12)] = special
    mask_values, mask_nulls = rng.integers(0, 2, n).astype(np.uint8), (rng.random(n) < 0.1).astype(np.uint8)
    mask_values[mask_nulls != 0] = 1   # ("true" under a null mask)
    mask_values[run == 7] = 0
    mask_nulls[run == 7] = 0
    for c in (big_nulls, dbl_nulls, mm_nulls):
        c[run == 11] = 1
    mm[run == 13] = np.nan
    return [K.KeyCol(B, key), K.KeyCol(B, rng.integers(-10**14, 10**14, n), big_nulls), K.KeyCol(D, rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n), dbl_nulls),
            K.KeyCol(D, mm, mm_nulls), K.KeyCol(BO, mask_values, mask_nulls)], run


@pytest.mark.parametrize("masked", [False, True])
def test_every_aggregate_function(pkg, ctx, function_stream, masked):
    cols, run = function_stream
    aggs = [(f, ch, 4) for f, ch in ALL_FUNCTIONS] if masked else ALL_FUNCTIONS
    n = cols[0].n
    pages = cut(cols, [n // 3, n // 3 + 1, 2 * n // 3])
    want = assert_matches(drive(pkg, ctx, types_of(cols), [0], aggs, pages), pages, [0], aggs)
    assert len(want) == 600
    if masked:
        assert want[7].values == (0, 0) + (None,) * 8            # the masked-out group: counts 0, everything else NULL
    assert want[11].values[1] == 0 and want[11].values[2] is None and (masked or want[11].values[0] > 0)    # count over all-null inputs
    assert want[13].values[8] != want[13].values[8] or want[13].values[8] is None


# ---- PARTIAL -> FINAL ---------------------------------------------------------------------------------------------------------------------
def test_partial_then_final_gives_the_single_result(pkg, ctx, function_stream):
    cols, _ = function_stream
    aggs = [(S.COUNT_ALL, -1), (S.SUM_BIGINT, 1), (S.SUM_DOUBLE, 2), (S.AVG_DOUBLE, 2), (S.MIN_BIGINT, 1), (S.MAX_DOUBLE, 3), (S.COUNT_COLUMN, 3, 4)]
    n = cols[0].n
    in_pages = cut(cols, [n // 4, n // 2])
    partial = drive(pkg, ctx, types_of(cols), [0], aggs, in_pages, S.PARTIAL)
    assert len(partial) == 1 + 1 + 2 + 2 + 2 + 2 + 2 + 1 and partial[0].n == 600
    final_aggs, ch = [], 1
    for a in aggs:
        final_aggs.append((a[0], ch))
        ch += 1 if a[0] in (S.COUNT_ALL, S.COUNT_COLUMN) else 2
    mid_pages = cut(partial, [1, 77, 77, 300])   # cut differently from the input
    final = drive(pkg, ctx, types_of(partial), [0], final_aggs, mid_pages, S.FINAL)
    single = S.aggregate(in_pages, [0], aggs)
    assert final[0].n == len(single) == 600 and K.same_bits(final[0], partial[0])
    for j, a in enumerate(aggs):
        loose = a[0] in (S.MIN_DOUBLE, S.MAX_DOUBLE)
        assert value_tokens(final[1 + j], loose) == [want_token(r.values[j], loose) for r in single], a


# ---- block encodings ----------------------------------------------------------------------------------------------------------------------
def test_dictionary_rle_and_device_blocks_give_the_flat_result(pkg, ctx):
    import torch
    rng = np.random.default_rng(23)
    # a dictionary whose entries hold NaNs of two payloads and both zeros: the emitted key cell is the dictionary value of the chosen row
    dict_bits = np.array([K.NEG_ZERO, K.POS_ZERO, K.NAN_BITS[1], K.NAN_BITS[3], S.double_bits(1.5), S.double_bits(2.5)], dtype=np.uint64)
    runs = rng.integers(0, 3, 700)                      # classes: zero, NaN, numbers
    lengths = rng.integers(1, 6, 700)
    cls = np.repeat(runs, lengths)
    n = len(cls)
    ids = (cls * 2 + rng.integers(0, 2, n)).astype(np.int32)
    vals = rng.integers(-100, 100, n).astype(np.int64)
    flat = [K.KeyCol(D, dict_bits[ids].view(np.float64)), K.KeyCol(B, vals)]
    aggs = [(S.COUNT_ALL, -1), (S.SUM_BIGINT, 1)]
    edges = [n // 3, 2 * n // 3]
    flat_pages = cut(flat, edges)
    bounds = [0] + edges + [n]

    def dictionary_page(p):
        a, b = bounds[flat_pages.index(p)], bounds[flat_pages.index(p) + 1]
        return pkg.Page(pkg.DictionaryBlock(pkg.Block(D, dict_bits.view(np.float64)), ids[a:b]), pkg.Block(B, vals[a:b]))

    assert_matches(drive(pkg, ctx, [D, B], [0], aggs, flat_pages, convert=dictionary_page), flat_pages, [0], aggs)
    # RLE key blocks: every page is one run; neighbours with the same value continue the group
    rle_values = [7, 7, 8, 7, 7, 7]
    rle_sizes = [5, 1, 300, 2, T + 1, 3]
    rle_flat, at = [], 0
    for v, size in zip(rle_values, rle_sizes):
        rle_flat.append([K.KeyCol(I, np.full(size, v, dtype=np.int32)), K.KeyCol(B, np.arange(at, at + size))])
        at += size

    def rle_page(p):
        return pkg.Page(pkg.RunLengthEncodedBlock(pkg.Block(I, p[0].values[:1]), p[0].n), pkg.Block(B, p[1].values))

    want = assert_matches(drive(pkg, ctx, [I, B], [0], aggs, rle_flat, convert=rle_page), rle_flat, [0], aggs)
    assert [r.values[0] for r in want] == [6, 300, T + 6]
    # device-resident input pages (borrowed blocks: the tensors stay alive until the operator is done)
    cols, _ = clustered_double_stream(29, 6000)
    pages = cut(cols, [1000, 1001, 1000 + T])
    alive = []

    def device_page(p):
        blocks = []
        for c in p:
            raw = c.values.view(np.uint8 if c.type == BO else (np.int64 if c.type in (B, D) else np.int32))
            vals_t = torch.from_numpy(raw.copy()).to("cuda:0")
            nulls_t = None if c.nulls is None else torch.from_numpy(c.nulls.copy()).to("cuda:0")
            alive.append((vals_t, nulls_t))
            blocks.append(pkg.DeviceBlock(c.type, c.n, vals_t, nulls_t))
        torch.cuda.synchronize()
        return pkg.Page(*blocks, position_count=p[0].n)

    assert_matches(drive(pkg, ctx, types_of(cols), [0], CUT_AGGS, pages, convert=device_page), pages, [0], CUT_AGGS)


# ---- route, memory, output cuts -----------------------------------------------------------------------------------------------------------
def test_route_by_profile_scopes(pkg):
    c = pkg.Context(0)
    c.profile_enable(True)
    try:
        cols, _ = clustered_double_stream(41, 5000)
        pages = cut(cols, [2000, 2001])
        assert_matches(drive(pkg, c, types_of(cols), [0], CUT_AGGS, pages), pages, [0], CUT_AGGS)
        c.synchronize()
        prof = c.profile()
        count = lambda name: prof.get(name, {}).get("count", 0)
        assert count("sagg_heads") == 3 and count("sagg_publish") == 3 and count("sagg_carry") >= 2
        assert count("gbh_insert") == 0 and count("gbh_probe") == 0 and count("gbh_runs") == 0 and count("gbh_finalize") == 0
        assert count("agg_accumulate_ordered") + count("agg_accumulate_ordered_chain") == 3
    finally:
        c.close()


def test_memory_does_not_grow_with_the_stream(pkg, ctx):
    rng = np.random.default_rng(2)
    n = 5000
    page = [K.KeyCol(V, ["k%d" % (i // 3) for i in range(n)]), K.KeyCol(B, rng.integers(0, 100, n)), K.KeyCol(D, rng.standard_normal(n))]
    product_page = to_page(pkg, page)
    fac = pkg.StreamingAggregationOperatorFactory(ctx, 7, [V, B, D], [0], S.SINGLE, [(S.SUM_BIGINT, 1), (S.SUM_DOUBLE, 2), (S.MIN_DOUBLE, 2)])
    op = fac.createOperator()
    seen, rows = {}, 0
    for i in range(1, 201):
        op.addInput(product_page)
        if i in (10, 150):
            seen[i] = op.memoryBytes()
        o = op.getOutput()
        rows += o.position_count
        o.release()
    assert 0 < seen[150] <= seen[10]
    op.finish()
    o = op.getOutput()
    rows += o.position_count
    o.release()
    # equal pages: "k0" of the next page is a new group after "k1666"
    assert rows == 200 * ((n + 2) // 3) and op.isFinished()
    op.close()
    fac.close()


def test_output_pages_respect_the_row_limit(pkg):
    c = pkg.Context(0)
    try:
        cols, _ = clustered_double_stream(43, 6000)
        pages = cut(cols, [2500, 4000])
        want = S.aggregate(pages, [0], CUT_AGGS)
        c.set_max_output_page(0, 100)
        fac = pkg.StreamingAggregationOperatorFactory(c, 7, types_of(cols), [0], S.SINGLE, CUT_AGGS)
        outs = pkg.to_pages(fac.createOperator(), [to_page(pkg, p) for p in pages])
        assert len(outs) > 10 and all(0 < o.position_count <= 100 for o in outs)
        got = [K.concat([K.from_block(o.getBlock(ch)) for o in outs]) for ch in range(5)]
        assert_matches(got, pages, [0], CUT_AGGS, want=want)
        fac.close()
    finally:
        c.close()


# ---- errors and protocol ------------------------------------------------------------------------------------------------------------------
def test_a_bigint_overflow_fails_the_call_that_completes_the_group(pkg, ctx):
    big = 2**62
    pages = [[K.KeyCol(B, np.array([1, 1, 2, 3])), K.KeyCol(B, np.array([5, 6, big, 9]))],
             [K.KeyCol(B, np.array([3, 4, 4, 5, 5, 5, 6, 7])), K.KeyCol(B, np.array([1, 2, 3, big, big - 1, 1, 0, 0]))]]
    model = S.stream(pages, [0], [(S.SUM_BIGINT, 1), (S.COUNT_ALL, -1)])
    first = next(model)
    with pytest.raises(S.NumericValueOutOfRange):   # the third group of the second page: 2^63
        next(model)
    fac = pkg.StreamingAggregationOperatorFactory(ctx, 7, [B, B], [0], S.SINGLE, [(S.SUM_BIGINT, 1), (S.COUNT_ALL, -1)])
    op = fac.createOperator()
    op.addInput(to_page(pkg, pages[0]))
    out = op.getOutput()
    with pytest.raises(pkg.TgpuError) as e:
        op.addInput(to_page(pkg, pages[1]))
    assert e.value.code == OUT_OF_RANGE
    assert op.getOutput() is None                                  # no row of that page is emitted
    assert out.to_host().rows() == [(1, 11, 2), (2, big, 1)] == [(k,) + r.values for k, r in zip((1, 2), first)]   # page 1's output is intact
    out.release()
    op.close()
    # the last group overflows: finish raises
    op = fac.createOperator()
    op.addInput(to_page(pkg, [K.KeyCol(B, np.array([1, 2, 2])), K.KeyCol(B, np.array([1, big, big]))]))
    assert op.getOutput().to_host().rows() == [(1, 1, 1)]
    with pytest.raises(pkg.TgpuError) as e:
        op.finish()
    assert e.value.code == OUT_OF_RANGE
    op.close()
    # at the limit nothing raises
    op = fac.createOperator()
    rows = pkg.to_pages(op, [to_page(pkg, [K.KeyCol(B, np.array([2, 2, 2])), K.KeyCol(B, np.array([big, big - 1, 0]))])])[0].rows()
    assert rows == [(2, 2**63 - 1, 3)]
    op.close()
    fac.close()


def test_protocol_and_page_checks(pkg, ctx):
    fac = pkg.StreamingAggregationOperatorFactory(ctx, 7, [B, D], [0], S.SINGLE, [(S.SUM_DOUBLE, 1)])
    op = fac.createOperator()
    assert op.needsInput() and not op.isFinished() and op.getOutput() is None
    op.addInput(pkg.Page(pkg.Block(B, np.zeros(0, dtype=np.int64)), pkg.Block(D, np.zeros(0)), position_count=0))   # a no-op
    assert op.needsInput() and op.getOutput() is None
    with pytest.raises(pkg.TgpuError) as e:
        op.addInput(pkg.Page(pkg.Block(B, np.arange(3))))                       # wrong channel count
    assert e.value.code == INVALID_ARGUMENT
    with pytest.raises(pkg.TgpuError) as e:
        op.addInput(pkg.Page(pkg.Block(D, np.zeros(3)), pkg.Block(D, np.zeros(3))))   # wrong type
    assert e.value.code == INVALID_ARGUMENT
    op.addInput(pkg.Page(pkg.Block(B, np.array([1, 2])), pkg.Block(D, np.array([0.5, 0.25]))))
    assert not op.needsInput()                                                  # an output page waits
    with pytest.raises(pkg.TgpuError):
        op.addInput(pkg.Page(pkg.Block(B, np.array([3])), pkg.Block(D, np.array([1.0]))))
    assert op.getOutput().to_host().rows() == [(1, 0.5)] and op.needsInput()
    op.finish()
    assert not op.needsInput() and not op.isFinished()
    with pytest.raises(pkg.TgpuError):
        op.addInput(pkg.Page(pkg.Block(B, np.array([3])), pkg.Block(D, np.array([1.0]))))   # after finish
    assert op.getOutput().to_host().rows() == [(2, 0.25)] and op.isFinished() and op.getOutput() is None
    op.close()
    # no input, no output
    op = fac.createOperator()
    op.finish()
    assert op.isFinished() and op.getOutput() is None
    op.close()
    fac.close()


def test_factory_arguments_and_lifecycle(pkg, ctx):
    make = lambda types, channels, aggs, step=S.SINGLE: pkg.StreamingAggregationOperatorFactory(ctx, 7, types, channels, step, aggs)
    import ctypes as C
    h = C.c_void_p()
    no_channels = (C.c_int32 * 1)()
    types = (C.c_int32 * 1)(B)
    rc = pkg._lib.lib().tgpu_streaming_aggregation_factory_create(ctx.handle, 7, 1, types, 0, no_channels, S.SINGLE, 0, None, C.byref(h))
    assert rc == INVALID_ARGUMENT and not h.value                                   # group_by_count == 0, said by the library itself
    for bad in (lambda: make([B], [1], []), lambda: make([B], [-1], []), lambda: make([B, 99], [0], []), lambda: make([B], [0], [(11, 0)]),
                lambda: make([B], [0], [(0, 0)]), lambda: make([B], [0], [(S.SUM_BIGINT, 3)]), lambda: make([B, D], [0], [(S.SUM_DOUBLE, 1, 1)]),
                lambda: make([B], [0], [(S.COUNT_ALL, -1)] * 17), lambda: make([B], [0], [], 3), lambda: make([B] * 9, list(range(9)), [])):
        with pytest.raises(pkg.TgpuError) as e:
            bad()
        assert e.value.code == INVALID_ARGUMENT
    fac = make([B, B], [0], [(S.SUM_BIGINT, 1)])
    dup = fac.duplicate()
    page = pkg.Page(pkg.Block(B, np.array([1, 1, 2])), pkg.Block(B, np.array([1, 2, 3])))
    fac.noMoreOperators()
    with pytest.raises(pkg.TgpuError):
        fac.createOperator()                                                       # Factory is already closed
    op = dup.createOperator()                                                      # the duplicate is independent
    assert [r for p in pkg.to_pages(op, [page]) for r in p.rows()] == [(1, 3), (2, 3)]
    op2 = dup.createOperator()
    dup.noMoreOperators()
    dup.close()                                                                    # an operator outlives its factory
    assert [r for p in pkg.to_pages(op2, [page, page]) for r in p.rows()] == [(1, 3), (2, 3), (1, 3), (2, 3)]
    op.close()
    op2.close()
    fac.close()

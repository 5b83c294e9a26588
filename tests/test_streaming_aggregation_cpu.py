"""The streaming aggregation model (tests/streaming_aggregation_expected.py) against the six cases of the reference's
TestStreamingAggregationOperator (tests/golden/streaming_aggregation_vectors.json), against key_cases' restatement of IS NOT DISTINCT FROM,
its own key-cell and flush rules, and the binding of the new entry point.  No GPU."""
import json
import os

import numpy as np
import pytest

import key_cases as K
import streaming_aggregation_expected as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_aggregation_vectors.json")


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def cell_token(type_id, cell):
    """an expected key cell of the fixture as the token key_cases.cells gives"""
    if cell is None:
        return None
    if type_id == K.VARCHAR:
        return cell.encode()
    if type_id == K.DOUBLE:
        return "nan" if cell == "NaN" else S.double_bits(float(cell))
    return int(cell)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_the_model_reproduces_every_golden_case(case):
    types, pages = S.golden_pages(case)
    channels = case["group_by_channels"]
    rows = S.aggregate(pages, channels, S.golden_aggs(case), S.STEP_CODES[case["step"]])
    want = S.golden_expected(case)
    assert len(rows) == len(want)
    keys = S.key_cells(pages, channels, rows)
    key_type = types[channels[0]]
    for got_key, got, exp in zip(keys, rows, want):
        tok = got_key[0]
        if key_type == K.DOUBLE and tok is not None and K.is_nan_bits(tok):
            tok = "nan"
        assert tok == cell_token(key_type, exp[0]) and got.values == tuple(exp[1:])


def test_the_fixture_holds_the_six_cases():
    cases = golden_cases()
    assert [c["name"] for c in cases] == ["test", "testLargeInputPage", "testEmptyInput", "testSinglePage", "testUniqueGroupingValues", "testSingleGroupingValue"]
    assert os.path.getsize(GOLDEN) < 8192
    test = S.golden_expected(cases[0])
    assert test[-2][0] == "NaN" and test[-1][0] is None   # the NaN group and the null group


@pytest.mark.parametrize("schema", sorted(K.KEY_SCHEMAS))
def test_the_models_groups_are_the_runs_of_not_distinct_keys(schema):
    """on random special-value keys (NaN payloads, both zeros, nulls over other bytes): a new group starts exactly where
    key_cases.group_ids_not_distinct changes from one row to the next, whatever the page cuts"""
    rng = np.random.default_rng(K._seed(schema, 11))
    types = K.KEY_SCHEMAS[schema]
    n = 3000
    cols = K.key_page(rng, types, n, K.SCHEMA_DOMAINS[schema], null_frac=0.2)
    ids = K.group_ids_not_distinct(cols)
    want, g = [], -1
    for i in range(n):
        if i == 0 or ids[i] != ids[i - 1]:
            g += 1
        want.append(g)
    channels = list(range(len(types)))
    for cuts in ([], [1, 2, 1500], sorted(rng.choice(np.arange(1, n), 40, replace=False).tolist())):
        edges = [0] + cuts + [n]
        pages = [[K.take(c, np.arange(a, b)) for c in cols] for a, b in zip(edges, edges[1:])]
        assert S.run_groups(pages, channels) == want
        rows = S.aggregate(pages, channels, [(S.COUNT_ALL, -1)])
        assert [r.values[0] for r in rows] == np.bincount(want).tolist()
    # the wrong groupings differ on this input, or the check above could not fail
    if K.DOUBLE in types:
        assert list(K.group_ids_bitwise(cols)) != list(ids) and list(K.group_ids_ieee(cols)) != list(ids)


def page_of(double_bits, bigints):
    return [K.KeyCol(K.DOUBLE, K.bits_to_doubles(double_bits)), K.KeyCol(K.BIGINT, np.array(bigints, dtype=np.int64))]


def test_the_key_cell_rule_names_the_row_the_reference_reads():
    nz, pz, n1, n2 = K.NEG_ZERO, K.POS_ZERO, K.NAN_BITS[1], K.NAN_BITS[3]
    one = S.double_bits(1.0)
    # page 0: zeros (-0.0 first), then a NaN run that runs on into page 1 and ends inside it; page 1 ends with a run of 1.0 that finish flushes
    pages = [page_of([nz, pz, n1, n2], [1, 2, 3, 4]), page_of([n2, n1, one, one], [5, 6, 7, 8])]
    out = list(S.stream(pages, [0], [(S.SUM_BIGINT, 1)]))
    assert out == [[S.Row(0, 0, (3,))], [S.Row(1, 0, (18,))], [S.Row(1, 3, (15,))]]
    assert S.key_cells(pages, [0], [r for rows in out for r in rows]) == [(nz,), (n2,), (one,)]
    # the same stream cut at the run end: the NaN group is flushed by the next page's first row and takes the LAST row of its page
    pages = [page_of([nz, pz, n1, n2, n2, n1], [1, 2, 3, 4, 5, 6]), page_of([one, one], [7, 8])]
    out = list(S.stream(pages, [0], [(S.SUM_BIGINT, 1)]))
    assert out == [[S.Row(0, 0, (3,))], [S.Row(0, 5, (18,))], [S.Row(1, 1, (15,))]]
    # a key that comes back is a new group; an empty page is a no-op
    pages = [page_of([one, nz, one], [1, 2, 3]), page_of([], []), page_of([one], [4])]
    assert [r.values for r in S.aggregate(pages, [0], [(S.COUNT_ALL, -1), (S.SUM_BIGINT, 1)])] == [(1, 1), (1, 2), (2, 7)]


def test_sums_masks_and_the_overflow_call():
    B, D, BO = K.BIGINT, K.DOUBLE, K.BOOLEAN
    key = K.KeyCol(B, np.array([1, 1, 1, 2, 2]))
    dbl = K.KeyCol(D, np.array([1e308, 1e308, -1e308, 0.5, -0.0]), np.array([0, 0, 0, 1, 0], dtype=np.uint8))
    mask = K.KeyCol(BO, np.array([1, 0, 1, 1, 1], dtype=np.uint8), np.array([0, 0, 1, 0, 0], dtype=np.uint8))
    rows = S.aggregate([[key, dbl, mask]], [0], [(S.SUM_DOUBLE, 1), (S.SUM_DOUBLE, 1, 2), (S.COUNT_ALL, -1, 2), (S.AVG_DOUBLE, 1), (S.MIN_DOUBLE, 1), (S.MAX_DOUBLE, 1)])
    assert rows[0].values[:3] == (float("inf"), 1e308, 1) and rows[0].values[3] == float("inf")     # row order: (1e308 + 1e308) - 1e308
    assert rows[1].values[:3] == (0.0, 0.0, 2) and S.double_bits(rows[1].values[4]) == K.NEG_ZERO   # 0.0 + -0.0 = +0.0; min keeps -0.0
    # PARTIAL -> FINAL gives SINGLE
    aggs = [(S.COUNT_ALL, -1), (S.SUM_DOUBLE, 1), (S.AVG_DOUBLE, 1)]
    partial = S.aggregate([[key, dbl, mask]], [0], aggs, S.PARTIAL)
    assert [len(r.values) for r in partial] == [5, 5]
    inter = [K.KeyCol(B, np.array([1, 2]))] + [K.KeyCol(B if j in (0, 1, 3) else D, np.array([r.values[j] for r in partial])) for j in range(5)]
    final = S.aggregate([inter], [0], [(S.COUNT_ALL, 1), (S.SUM_DOUBLE, 2), (S.AVG_DOUBLE, 4)], S.FINAL)
    assert [tuple(map(S.value_token, r.values)) for r in final] == [tuple(map(S.value_token, r.values)) for r in S.aggregate([[key, dbl, mask]], [0], aggs)]
    # sum(bigint): the total decides, and the call that completes the group raises
    big = 2**62
    pages = [[K.KeyCol(B, np.array([1, 2])), K.KeyCol(B, np.array([5, big]))], [K.KeyCol(B, np.array([2, 2, 3])), K.KeyCol(B, np.array([big, -1, 7]))],
             [K.KeyCol(B, np.array([3, 4, 4, 5])), K.KeyCol(B, np.array([1, big, big, 0]))]]
    it = S.stream(pages, [0], [(S.SUM_BIGINT, 1)])
    assert next(it) == [S.Row(0, 0, (5,))]
    assert next(it) == [S.Row(1, 0, (2**63 - 1,))]   # 2^62 + 2^62 - 1: at the limit
    with pytest.raises(S.NumericValueOutOfRange):
        next(it)


def test_the_library_binds_the_streaming_aggregation(pkg):
    assert "tgpu_streaming_aggregation_factory_create" in pkg._lib.SYMBOLS
    assert issubclass(pkg.StreamingAggregationOperatorFactory, pkg.OperatorFactory)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tgpu.h")).read()
    assert "tgpu_streaming_aggregation_factory_create(" in header
    so = pkg.SO_PATH
    if os.path.exists(so):   # (built: the symbol is exported)
        import ctypes
        assert hasattr(ctypes.CDLL(so), "tgpu_streaming_aggregation_factory_create")
    with pytest.raises(pkg.TgpuError) as e:   # rejected before the library or a device is needed
        pkg.StreamingAggregationOperatorFactory(None, 0, [pkg.BIGINT], [], pkg.SINGLE, [(pkg.COUNT_ALL, -1)])
    assert e.value.code == -1

"""The merge model (tests/merge_expected.py) against the literals of the reference's TestMergeSortedPages and TestMergeOperator
(tests/golden/merge_vectors.json), the model's own rules, and the binding of the three merge symbols.  No GPU."""
import json
import os

import numpy as np
import pytest

import merge_expected as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_vectors.json")


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def decode(case):
    types = [M.TYPE_CODES[t] for t in case["types"]]
    orders = [M.ORDER_CODES[o] for o in case["sort_orders"]]
    streams = [[[tuple(r) for r in page] for page in stream] for stream in case["streams"]]
    return types, case["sort_channels"], orders, case["output_channels"], streams, [tuple(r) for r in case["expected"]]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_the_model_reproduces_every_golden_case(case):
    types, sort_channels, orders, out, streams, expected = decode(case)
    assert M.merge(types, sort_channels, orders, out, streams) == expected


def test_the_fixture_holds_the_eight_cases_and_records_the_unsorted_literal():
    doc = json.load(open(GOLDEN))
    assert [c["source"] for c in doc["cases"]] == [
        "TestMergeSortedPages.testSingleStream", "TestMergeSortedPages.testSimpleTwoStreams", "TestMergeSortedPages.testMultipleStreams", "TestMergeSortedPages.testEmptyStreams",
        "TestMergeSortedPages.testDifferentTypes", "TestMergeOperator.testSingleStream", "TestMergeOperator.testMergeDifferentTypes",
        "TestMergeOperator.testMultipleStreamsSameOutputColumns"]
    assert "(99,1,1) before (99,2,2)" in doc["note"]
    # as the reference lists them the two rows are not sorted under the declared order, and the model says so
    case = [c for c in doc["cases"] if c["source"] == "TestMergeSortedPages.testMultipleStreams"][0]
    types, sort_channels, orders, out, streams, _ = decode(case)
    page = streams[1][2]
    assert page[-1] == (99, 2, 2) and streams[1][3][0] == (99, 1, 1)
    streams[1][2], streams[1][3] = page[:-1] + [(99, 1, 1)], [(99, 2, 2)] + streams[1][3][1:]
    with pytest.raises(ValueError):
        M.merge(types, sort_channels, orders, out, streams)


def test_the_model_refuses_unsorted_streams():
    with pytest.raises(ValueError):
        M.merge([M.BIGINT], [0], [M.ASC_NULLS_FIRST], [0], [[[(1,), (3,)], [(2,)]]])
    with pytest.raises(ValueError):   # nulls last, but a null leads
        M.merge([M.BIGINT], [0], [M.ASC_NULLS_LAST], [0], [[[(None,), (3,)]]])
    assert M.merge([M.BIGINT], [0], [M.DESC_NULLS_LAST], [0], [[[(3,), (1,), (None,)]], [[(2,)]]]) == [(3,), (2,), (1,), (None,)]


def test_comparator_special_values():
    nan1, nan2 = float("nan"), np.frombuffer(np.array([0x7FF0000000000123], dtype=np.uint64).tobytes(), dtype=np.float64)[0].item()
    assert M.compare_cells(M.DOUBLE, nan1, nan2) == 0 and M.compare_cells(M.DOUBLE, float("inf"), nan1) < 0
    assert M.compare_cells(M.DOUBLE, -0.0, 0.0) < 0 and M.compare_cells(M.DOUBLE, float("-inf"), -1e308) < 0
    assert M.compare_cells(M.VARCHAR, "abcdefgh", "abcdefghi") < 0 and M.compare_cells(M.VARCHAR, "abcdefghA", "abcdefghB") < 0 and M.compare_cells(M.VARCHAR, "", "a") < 0
    assert M.compare_cells(M.VARCHAR, b"\xff", b"a") > 0   # bytes compare unsigned
    assert M.compare_rows([M.VARCHAR], [0], [M.ASC_NULLS_FIRST], (None,), ("",)) < 0 and M.compare_rows([M.VARCHAR], [0], [M.DESC_NULLS_LAST], (None,), ("",)) > 0


def test_the_settled_set_rule():
    T, S, O = [M.BIGINT], [0], [M.ASC_NULLS_FIRST]
    rows = lambda *v: [(x,) for x in v]
    # B = (5, stream 0): stream 0 settles rows <= 5, stream 1 (after t_B) only rows < 5
    assert M.settled_counts(T, S, O, [rows(1, 5), rows(2, 5, 5, 7)], [False, False]) == [2, 1]
    # B = (5, stream 1): stream 0 (before t_B) settles its 5 as well
    assert M.settled_counts(T, S, O, [rows(1, 5, 9), rows(2, 5)], [False, False]) == [2, 2]
    # a finished stream sets no bound but is bounded by the others
    assert M.settled_counts(T, S, O, [rows(1, 5, 9), rows(2, 3)], [True, False]) == [1, 2]
    assert M.settled_counts(T, S, O, [rows(1, 5, 9), rows(2, 3)], [True, True]) == [3, 2]
    assert M.settled_counts(T, S, O, [rows(1), []], [False, False]) is None
    assert M.settled_counts(T, S, O, [rows(1), []], [False, True]) == [1, 0]
    m = M.StreamingModel(T, S, O, 2)
    m.arrive(0, rows(1, 4))
    assert m.round() is None
    m.arrive(1, rows(2, 3, 8))
    assert m.round() == rows(1, 2, 3, 4) and m.buffered == [[], rows(8)]
    m.end(0)
    m.end(1)
    assert m.round() == rows(8) and m.done()


def test_the_stream_generator_gives_sorted_streams_with_empty_pages_and_streams():
    rng = np.random.default_rng(1)
    T, S, O = [M.BIGINT, M.BIGINT], [0], [M.DESC_NULLS_FIRST]
    streams = M.sorted_streams(rng, T, S, O, lambda rng, s, i: (None if rng.random() < 0.1 else int(rng.integers(0, 50)), s * 1000 + i), [0, 1, 40, 200, 0], 16)
    assert len(streams) == 5 and M.flatten(streams[0]) == [] and len(M.flatten(streams[3])) == 200
    assert any(page == [] for stream in streams for page in stream)
    merged = M.merge_rows(T, S, O, streams)   # (checks every stream)
    assert len(merged) == 241
    ties = [r for r in merged if r[0] == merged[100][0]]
    assert [r[1] // 1000 for r in ties] == sorted(r[1] // 1000 for r in ties)   # equal keys: lower stream first


def test_the_array_specialisation_agrees_with_the_model():
    rng = np.random.default_rng(2)
    keys = [np.sort(rng.integers(0, 20, n)) for n in (50, 0, 31, 7)]
    payloads = [s * 1000 + np.arange(len(k)) for s, k in enumerate(keys)]
    streams = [[[(int(a), int(b)) for a, b in zip(k, p)]] for k, p in zip(keys, payloads)]
    want = M.merge_rows([M.BIGINT, M.BIGINT], [0], [M.ASC_NULLS_FIRST], streams)
    got_k, got_p = M.merge_ascending_bigint(keys, payloads)
    assert [(int(a), int(b)) for a, b in zip(got_k, got_p)] == want
    with pytest.raises(ValueError):
        M.merge_ascending_bigint([np.array([2, 1])], [np.array([0, 1])])


def test_the_library_binds_the_merge_operator(pkg):
    for name in ("tgpu_merge_factory_create", "tgpu_merge_operator_add_page_source", "tgpu_merge_operator_no_more_splits"):
        assert name in pkg._lib.SYMBOLS
    assert issubclass(pkg.MergeOperatorFactory, pkg.OperatorFactory) and issubclass(pkg.MergeOperator, pkg.Operator)
    assert hasattr(pkg.MergeOperator, "addSplit") and hasattr(pkg.MergeOperator, "noMoreSplits")

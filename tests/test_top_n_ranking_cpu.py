"""TopNRankingOperator without a GPU: the expected-value helper (tests/top_n_ranking_expected.py) reproduces every case transcribed from the reference's
tests (tests/golden/top_n_ranking_vectors.json), so the yardstick of the GPU tests is itself checked; hand-written ties show the arrival-order rule and
the RANK boundary; tgpu.h declares the factory, libtgpu.so exports it, _lib.py binds it and the package exports the Python factory and constants; the
JNI shim rejects bad ranking types, channels, counts and limits with a pending NativeError before the library is called (a call with the null context
handle would reach it otherwise)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from jni_harness import FakeJvm, build_fake_jni, header_symbols
from top_n_ranking_expected import (ASC_NULLS_FIRST, ASC_NULLS_LAST, BIGINT, DESC_NULLS_FIRST, DESC_NULLS_LAST, DOUBLE, RANK, ROW_NUMBER, VARCHAR, compare_rows,
                                    compare_values, expected_output, golden_case_inputs, oracle_col, tokens)

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "top_n_ranking_vectors.json")))
ORDERS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}
RANKINGS = {"ROW_NUMBER": 0, "RANK": 1}


def run_helper(oracle, types, pages, outputs, partitions, sorts, orders, ranking, n, partial=False, expected_positions=10):
    keys = [[oracle_col(oracle, types[c], [r[c] for r in page]) for c in partitions] for page in pages]
    return expected_output(oracle, types, pages, keys, outputs, partitions, sorts, orders, ranking, n, partial, expected_positions)


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_helper_reproduces_reference_case(oracle, case):
    types, pages, expected = golden_case_inputs(case)
    got = run_helper(oracle, types, pages, case["output_channels"], case["partition_channels"], case["sort_channels"], [ORDERS[o] for o in case["sort_orders"]],
                     RANKINGS[case["ranking_type"]], case["max_rank_per_partition"], case["partial"], case["expected_positions"])
    assert tokens(got) == tokens(expected)


def test_golden_file_covers_what_it_should():
    names = {c["name"] for c in GOLD["cases"]}
    assert {"partitioned", "unpartitioned_final", "unpartitioned_partial", "rank_null_and_nan", "row_number_builder_multi_group", "rank_builder_multi_group"} <= names
    assert any(c["hash_parametrised"] for c in GOLD["cases"])


def test_ties_rank_in_arrival_order_and_rank_keeps_the_boundary(oracle):
    """sort keys [1, 1, 1, 2, 2] with n = 2; channel 1 tells the rows apart"""
    types = [BIGINT, BIGINT]
    pages = [[(1, 10), (2, 11), (1, 12)], [(2, 13), (1, 14)]]
    assert run_helper(oracle, types, pages, [0, 1], [], [0], [ASC_NULLS_LAST], ROW_NUMBER, 2) == [(1, 10, 1), (1, 12, 2)]
    assert run_helper(oracle, types, pages, [0, 1], [], [0], [ASC_NULLS_LAST], RANK, 2) == [(1, 10, 1), (1, 12, 1), (1, 14, 1)]   # the 2s have rank 4
    assert run_helper(oracle, types, pages, [0, 1], [], [0], [ASC_NULLS_LAST], RANK, 4) == [(1, 10, 1), (1, 12, 1), (1, 14, 1), (2, 11, 4), (2, 13, 4)]
    assert run_helper(oracle, types, pages, [1], [], [0], [DESC_NULLS_LAST], ROW_NUMBER, 3, partial=True) == [(11,), (13,), (10,)]
    # the boundary tie: the second and third row share rank 2, both are kept, a partition returns more than n rows
    pages = [[(5, 0), (7, 1)], [(7, 2), (9, 3)]]
    assert run_helper(oracle, types, pages, [1], [], [0], [ASC_NULLS_LAST], RANK, 2) == [(0, 1), (1, 2), (2, 2)]
    assert run_helper(oracle, types, pages, [1], [], [0], [ASC_NULLS_LAST], ROW_NUMBER, 2) == [(0, 1), (1, 2)]


def test_partitions_come_out_in_first_arrival_order_and_null_is_a_key(oracle):
    types = [VARCHAR, BIGINT]
    pages = [[("b", 3), (None, 1), ("a", 2)], [(None, 0), ("b", 1), ("a", 9)]]
    assert run_helper(oracle, types, pages, [0, 1], [0], [1], [ASC_NULLS_LAST], ROW_NUMBER, 1) == [("b", 1, 1), (None, 0, 1), ("a", 2, 1)]
    assert run_helper(oracle, types, [], [0, 1], [0], [1], [ASC_NULLS_LAST], ROW_NUMBER, 1) == []


def test_comparator_restates_the_reference():
    nan, inf = float("nan"), float("inf")
    assert compare_values(DOUBLE, -0.0, 0.0) < 0 and compare_values(DOUBLE, nan, nan) == 0 and compare_values(DOUBLE, inf, nan) < 0 and compare_values(DOUBLE, nan, -inf) > 0
    assert compare_values(VARCHAR, "abcdefgh1", "abcdefgh2") < 0 and compare_values(VARCHAR, "ab", "abc") < 0 and compare_values(VARCHAR, "z", "é") < 0   # 0x7a < 0xc3
    types = [DOUBLE, BIGINT]
    for order, null_first, ascending in ((ASC_NULLS_FIRST, True, True), (ASC_NULLS_LAST, False, True), (DESC_NULLS_FIRST, True, False), (DESC_NULLS_LAST, False, False)):
        assert (compare_rows(types, [0], [order], (None, 0), (1.0, 0)) < 0) == null_first
        assert (compare_rows(types, [0], [order], (1.0, 0), (2.0, 0)) < 0) == ascending
        assert compare_rows(types, [0], [order], (None, 0), (None, 1)) == 0
        assert compare_rows(types, [0, 1], [order, ASC_NULLS_LAST], (nan, 1), (nan, 2)) < 0   # the leading keys tie


def test_header_library_and_binding_have_the_top_n_ranking_operator(pkg):
    name = "tgpu_top_n_ranking_factory_create"
    assert name in set(header_symbols())
    assert hasattr(pkg._lib.lib(), name)
    assert name in pkg._lib.SYMBOLS
    assert hasattr(pkg, "TopNRankingOperatorFactory")
    assert (pkg.ROW_NUMBER, pkg.RANK, pkg.DENSE_RANK) == (0, 1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tgpu.h")).read()
    assert "TGPU_RANKING_ROW_NUMBER = 0, TGPU_RANKING_RANK = 1, TGPU_RANKING_DENSE_RANK = 2" in header
    assert " *   - tgpu_top_n_ranking_*" in header   # the list of replaced interfaces at the top


@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


# (rankingType, types, output channels, partition channels, sort channels, sort orders, maxRankPerPartition, hashChannel, expectedPositions, message)
BAD = [
    (2, (1, 4), (0,), (0,), (1,), (1,), 3, -1, 10, "dense_rank is not supported"),
    (3, (1, 4), (0,), (0,), (1,), (1,), 3, -1, 10, "unknown ranking type"),
    (-1, (1, 4), (0,), (0,), (1,), (1,), 3, -1, 10, "unknown ranking type"),
    (0, (), (), (), (0,), (1,), 3, -1, 10, "empty type array"),
    (0, (1, 4), (0, 2), (0,), (1,), (1,), 3, -1, 10, "output channel out of range"),
    (0, (1, 4), (-1,), (0,), (1,), (1,), 3, -1, 10, "output channel out of range"),
    (0, (1, 4), (0,), (2,), (1,), (1,), 3, -1, 10, "partition channel out of range"),
    (0, (1, 4), (0,), (0,) * 9, (1,), (1,), 3, -1, 10, "more than 8 partition channels"),
    (0, (1, 4), (0,), (0,), (), (), 3, -1, 10, "1 to 8 sort channels"),
    (0, (1, 4), (0,), (0,), (1,) * 9, (1,) * 9, 3, -1, 10, "1 to 8 sort channels"),
    (0, (1, 4), (0,), (0,), (1, 0), (1,), 3, -1, 10, "sort channels and sort orders differ in length"),
    (0, (1, 4), (0,), (0,), (2,), (1,), 3, -1, 10, "sort channel out of range"),
    (0, (1, 4), (0,), (0,), (1,), (4,), 3, -1, 10, "sort order out of range"),
    (0, (1, 4), (0,), (0,), (1,), (-1,), 3, -1, 10, "sort order out of range"),
    (0, (1, 1), (0,), (), (0,), (1,), 3, 1, 10, "hash channel without partition channels"),
    (0, (1, 1), (0,), (0,), (0,), (1,), 3, 2, 10, "hash channel out of range"),
    (0, (1, 4), (0,), (0,), (1,), (1,), 3, 1, 10, "hash channel is not BIGINT"),
    (1, (1, 4), (0,), (0,), (1,), (1,), 0, -1, 10, "max rank per partition must be a positive int"),
    (1, (1, 4), (0,), (0,), (1,), (1,), -5, -1, 10, "max rank per partition must be a positive int"),
    (1, (1, 4), (0,), (0,), (1,), (1,), 2**31, -1, 10, "max rank per partition must be a positive int"),
    (0, (1, 4), (0,), (0,), (1,), (1,), 3, -1, 0, "expected positions must be positive"),
]


@pytest.mark.parametrize("ranking, types, outputs, partitions, sorts, orders, max_rank, hash_channel, expected_positions, why", BAD)
def test_arguments_are_checked_in_front_of_the_library(jvm, ranking, types, outputs, partitions, sorts, orders, max_rank, hash_channel, expected_positions, why):
    r = jvm.call("createTopNRankingFactory", C.c_int64, C.c_int64(0), C.c_int32(1), C.c_int32(ranking), ints(jvm, *types), ints(jvm, *outputs), ints(jvm, *partitions),
                 ints(jvm, *sorts), ints(jvm, *orders), C.c_int64(max_rank), C.c_uint8(0), C.c_int32(hash_channel), C.c_int32(expected_positions))
    assert r == 0
    assert jvm.pending_code() == -1 and jvm.pending_message() == "top n ranking: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0

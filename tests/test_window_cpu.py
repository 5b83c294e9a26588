"""WindowOperator without a GPU: the expected-value helper (tests/window_expected.py) reproduces every case transcribed from the reference's tests
(tests/golden/window_vectors.json), so the yardstick of the GPU tests is itself checked; hand-written cases pin arrival order among equal rows, -0.0 /
+0.0 and NaN as peers and as one partition, the no-keys case, the bounds of lag and lead and the sum's overflow rule; tgpu.h declares the factory and
the enums, libtgpu.so exports it, _lib.py binds it and the package exports the names; the JNI shim rejects every bad argument with a pending
NativeError before the library is called (a call with the null context handle would reach it otherwise); the Java sources declare the native and
the factory method."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from jni_harness import FakeJvm, build_fake_jni, header_symbols
from window_expected import (AGGREGATE, ASC_NULLS_LAST, BIGINT, COUNT_ALL, CUME_DIST, DENSE_RANK, DOUBLE, FIRST_VALUE, FRAME_PARTITION, FRAME_RANGE_TO_CURRENT,
                             FRAME_ROWS_TO_CURRENT, LAG, LAST_VALUE, LEAD, MAX_DOUBLE, MIN_DOUBLE, PERCENT_RANK, RANK, ROW_NUMBER, SUM_BIGINT, VARCHAR, Fn, InvalidArgument,
                             NumericValueOutOfRange, expected_output, golden_case, not_distinct, tokens)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "window_vectors.json")))
ORDERS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_helper_reproduces_reference_case(case):
    types, pages, functions, expected = golden_case(case)
    got = tokens(expected_output(types, pages, case["output_channels"], functions, case["partition_channels"], case["sort_channels"],
                                 [ORDERS[o] for o in case["sort_orders"]]))
    if case["ordered"]:
        assert got == tokens(expected)
    else:   # the reference compares these ignoring order
        assert sorted(map(repr, got)) == sorted(map(repr, tokens(expected)))


def test_golden_file_covers_what_it_should():
    sources = {c["source"].split("#")[0] for c in GOLD["cases"]}
    for method in ("testRowNumber", "testRowNumberPartition", "testRowNumberArbitrary", "testDistinctPartitionAndPeers", "testFirstValuePartition", "testLastValuePartition",
                   "testLagPartition", "testLeadPartition"):
        assert "TestWindowOperator." + method in sources
    assert all(c["ordered"] for c in GOLD["cases"] if c["source"].startswith("TestWindowOperator."))
    for cls in ("Rank", "DenseRank", "PercentRank", "CumulativeDistribution", "RowNumber", "Lag", "Lead", "FirstValue", "LastValue", "AggregateWindow"):
        assert any(s.startswith("Test%sFunction." % cls) for s in sources), cls
    assert GOLD["skipped"] and all(s["reason"] and s["source"] and s["sql"] for s in GOLD["skipped"])
    used = {f["function"] for c in GOLD["cases"] for f in c["functions"]}
    assert used == {"ROW_NUMBER", "RANK", "DENSE_RANK", "PERCENT_RANK", "CUME_DIST", "LAG", "LEAD", "FIRST_VALUE", "LAST_VALUE", "AGGREGATE"}
    assert {f["frame"] for c in GOLD["cases"] for f in c["functions"]} == {"PARTITION", "RANGE_TO_CURRENT", "ROWS_TO_CURRENT"}


def test_fully_equal_rows_keep_arrival_order_across_pages():
    types = [BIGINT, BIGINT, BIGINT]   # partition key, sort key, row id
    pages = [[(1, 5, 0), (0, 5, 1), (1, 5, 2)], [(1, 5, 3), (0, 5, 4)], [(1, 4, 5)]]
    got = expected_output(types, pages, [2], [Fn(ROW_NUMBER), Fn(RANK), Fn(AGGREGATE, (), FRAME_ROWS_TO_CURRENT, COUNT_ALL)], [0], [1], [ASC_NULLS_LAST])
    assert got == [(1, 1, 1, 1), (4, 2, 1, 2), (5, 1, 1, 1), (0, 2, 2, 2), (2, 3, 2, 3), (3, 4, 2, 4)]


def test_both_zeros_and_nans_are_peers_and_one_partition():
    nan = float("nan")
    assert not_distinct(DOUBLE, -0.0, 0.0) and not_distinct(DOUBLE, nan, nan) and not_distinct(DOUBLE, None, None)
    assert not not_distinct(DOUBLE, nan, 1.0) and not not_distinct(DOUBLE, None, 0.0) and not not_distinct(DOUBLE, 1.0, 2.0)
    types = [DOUBLE, BIGINT]
    rows = [(0.0, 0), (nan, 1), (-0.0, 2), (nan, 3), (0.0, 4), (1.0, 5)]
    fns = [Fn(RANK), Fn(DENSE_RANK), Fn(AGGREGATE, (), FRAME_RANGE_TO_CURRENT, COUNT_ALL), Fn(CUME_DIST)]
    # as the sort key: -0.0 sorts first (Double.compare) but is a peer of the +0.0s; the NaNs are peers of each other
    assert expected_output(types, [rows], [1], fns, [], [0], [ASC_NULLS_LAST]) == [(2, 1, 1, 3, 0.5), (0, 1, 1, 3, 0.5), (4, 1, 1, 3, 0.5), (5, 4, 2, 4, 4 / 6),
                                                                                 (1, 5, 3, 6, 1.0), (3, 5, 3, 6, 1.0)]
    # as the partition key: the zeros are ONE partition of three rows
    got = expected_output(types, [rows], [1], [Fn(ROW_NUMBER), Fn(AGGREGATE, (), FRAME_PARTITION, COUNT_ALL)], [0], [], [])
    assert got == [(2, 1, 3), (0, 2, 3), (4, 3, 3), (5, 1, 1), (1, 1, 2), (3, 2, 2)]
    # min / max over both zeros and NaN, as the tgpu_agg_function comments have it
    vals = expected_output(types, [rows], [], [Fn(AGGREGATE, (0,), FRAME_PARTITION, MIN_DOUBLE), Fn(AGGREGATE, (0,), FRAME_PARTITION, MAX_DOUBLE)], [0], [], [])
    assert tokens(vals) == tokens([(-0.0, 0.0)] * 3 + [(1.0, 1.0)] + [(nan, nan)] * 2)


def test_without_keys_the_input_is_one_partition_of_peers_in_arrival_order():
    types = [BIGINT]
    pages = [[(3,), (1,)], [(2,), (None,)]]
    fns = [Fn(ROW_NUMBER), Fn(RANK), Fn(DENSE_RANK), Fn(PERCENT_RANK), Fn(CUME_DIST), Fn(AGGREGATE, (0,), FRAME_RANGE_TO_CURRENT, SUM_BIGINT),
           Fn(AGGREGATE, (0,), FRAME_ROWS_TO_CURRENT, SUM_BIGINT), Fn(LAST_VALUE, (0,), FRAME_RANGE_TO_CURRENT), Fn(FIRST_VALUE, (0,), FRAME_ROWS_TO_CURRENT)]
    assert expected_output(types, pages, [0], fns, [], [], []) == [(3, 1, 1, 1, 0.0, 1.0, 6, 3, None, 3), (1, 2, 1, 1, 0.0, 1.0, 6, 4, None, 3),
                                                                   (2, 3, 1, 1, 0.0, 1.0, 6, 6, None, 3), (None, 4, 1, 1, 0.0, 1.0, 6, 6, None, 3)]
    assert expected_output(types, [], [0], fns, [], [], []) == []


def test_the_bounds_of_lag_and_lead():
    types = [BIGINT, BIGINT, BIGINT, BIGINT]   # partition, value (also the sort key), offset, default
    rows = [(0, 10, None, -1), (0, 11, 0, -2), (0, 12, 2, -3), (0, 13, 3, -4), (0, 14, 2**63 - 1, -5), (1, 20, 1, -6)]
    got = expected_output(types, [rows], [1], [Fn(LAG, (1, 2, 3)), Fn(LEAD, (1, 2, 3)), Fn(LAG, (1,)), Fn(LEAD, (1,))], [0], [1], [ASC_NULLS_LAST])
    assert got == [(10, None, None, None, 11),      # a null offset: null, not the default
                   (11, 11, 11, 10, 12),            # offset 0: the row itself
                   (12, 10, 14, 11, 13),            # 0 <= 2 - 2; 2 + 2 < 5
                   (13, 10, -4, 12, 14),            # 0 <= 3 - 3; 3 + 3 >= 5: the current row's default
                   (14, -5, -5, 13, None),          # the largest long: current - offset < 0, current + offset wraps below 0
                   (20, -6, -6, None, None)]        # the neighbouring partition is out of reach
    for f in (LAG, LEAD):
        with pytest.raises(InvalidArgument, match="Offset must be at least 0"):
            expected_output(types, [[(0, 1, -1, 0)]], [1], [Fn(f, (1, 2))], [0], [1], [ASC_NULLS_LAST])


def test_sum_raises_where_add_exact_would():
    big = 2**63 - 1
    run = lambda values, frame: [r[0] for r in expected_output([BIGINT], [[(v,) for v in values]], [], [Fn(AGGREGATE, (0,), frame, SUM_BIGINT)], [], [], [])]
    assert run([big, -1, 1], FRAME_ROWS_TO_CURRENT) == [big, big - 1, big] and run([big, -1, 1], FRAME_PARTITION) == [big] * 3
    assert run([-2**62, -2**62, None, 2**62, 2**62, 2**62], FRAME_ROWS_TO_CURRENT) == [-2**62, -2**63, -2**63, -2**62, 0, 2**62]
    for frame in (FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT):
        with pytest.raises(NumericValueOutOfRange, match="bigint addition overflow"):
            run([big, 1, -1], frame)
    assert run([None, None], FRAME_PARTITION) == [None, None]


def test_header_library_and_binding_have_the_window_operator(pkg):
    name = "tgpu_window_factory_create"
    assert name in set(header_symbols())
    assert hasattr(pkg._lib.lib(), name)
    assert name in pkg._lib.SYMBOLS
    assert hasattr(pkg, "WindowOperatorFactory") and hasattr(pkg, "WindowFunction")
    assert (pkg.WINDOW_ROW_NUMBER, pkg.WINDOW_RANK, pkg.WINDOW_DENSE_RANK, pkg.WINDOW_PERCENT_RANK, pkg.WINDOW_CUME_DIST, pkg.WINDOW_LAG, pkg.WINDOW_LEAD,
            pkg.WINDOW_FIRST_VALUE, pkg.WINDOW_LAST_VALUE, pkg.WINDOW_AGGREGATE) == tuple(range(10))
    assert (pkg.FRAME_PARTITION, pkg.FRAME_RANGE_TO_CURRENT, pkg.FRAME_ROWS_TO_CURRENT) == (0, 1, 2)
    assert (ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST, LAG, LEAD, FIRST_VALUE, LAST_VALUE, AGGREGATE) == tuple(range(10))   # the helper's codes
    header = open(os.path.join(ROOT, "include", "tgpu.h")).read()
    assert "TGPU_WINDOW_LAG = 5, TGPU_WINDOW_LEAD = 6, TGPU_WINDOW_FIRST_VALUE = 7, TGPU_WINDOW_LAST_VALUE = 8, TGPU_WINDOW_AGGREGATE = 9" in header
    assert "TGPU_FRAME_PARTITION = 0, TGPU_FRAME_RANGE_TO_CURRENT = 1, TGPU_FRAME_ROWS_TO_CURRENT = 2" in header
    assert " *   - tgpu_window_*" in header   # the list of replaced interfaces at the top
    spec = pkg.WindowFunction(pkg.WINDOW_LAG, (4, 2, 1), pkg.FRAME_PARTITION).spec()
    assert C.sizeof(spec) == 32 and (spec.function, spec.frame, spec.argument_count, list(spec.argument_channels), spec.ignore_nulls) == (5, 0, 3, [4, 2, 1], 0)


def test_java_sources_declare_the_native_and_the_factory_method():
    strip = lambda t: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    native = strip(open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuNative.java")).read())
    m = re.search(r"public static native long createWindowFactory\((.*?)\);", native, flags=re.S)
    assert m and [p.strip().rsplit(" ", 1)[0] for p in m.group(1).split(",")] == ["long", "int", "int[]", "int[]", "int[]", "int[]", "int[]", "int[]", "int"]
    glue = strip(open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuOperatorFactories.java")).read())
    assert re.search(r"public Optional<OperatorFactory> window\(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels", glue)
    assert "GpuNative.createWindowFactory(context, operatorId, codes," in glue and '"GpuWindowOperator"' in glue
    assert re.search(r"public static int\[\] windowFunction\(int function, int aggFunction, int frame, boolean ignoreNulls, List<Integer> argumentChannels\)", glue)
    for name, code in (("WINDOW_ROW_NUMBER", 0), ("WINDOW_AGGREGATE", 9), ("FRAME_PARTITION", 0), ("FRAME_ROWS_TO_CURRENT", 2)):
        assert re.search(r"public static final int %s = %d;" % (name, code), glue)
    shim = open(os.path.join(ROOT, "jni", "tgpu_jni.c")).read()
    assert "JFN(jlong, createWindowFactory)" in shim and "tgpu_window_factory_create(" in shim


@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


def fn(function, agg=0, frame=1, args=(), ignore_nulls=0):
    return (function, agg, frame, len(args)) + tuple(args) + (0,) * (3 - len(args)) + (ignore_nulls,)


T = (1, 4, 6, 6)   # BIGINT, DOUBLE, VARCHAR, VARCHAR
# (types, output channels, functions flattened, partition channels, sort channels, sort orders, expectedPositions, code, message)
BAD = [
    ((), (), fn(0), (), (), (), 10, -1, "empty type array"),
    ((1, 7), (0,), fn(0), (), (), (), 10, -1, "unknown type"),
    (T, (4,), fn(0), (), (), (), 10, -1, "output channel out of range"),
    (T, (-1,), fn(0), (), (), (), 10, -1, "output channel out of range"),
    (T, (0,), fn(0), (0,), (1, 0), (1,), 10, -1, "sort channels and sort orders differ in length"),
    (T, (0,), fn(0), (0,) * 5, (1,) * 4, (1,) * 4, 10, -1, "more than 8 partition and sort channels"),
    (T, (0,), fn(0), (4,), (), (), 10, -1, "partition channel out of range"),
    (T, (0,), fn(0), (0,), (-1,), (1,), 10, -1, "sort channel out of range"),
    (T, (0,), fn(0), (0,), (1,), (4,), 10, -1, "sort order out of range"),
    (T, (0,), fn(0), (0,), (1,), (-1,), 10, -1, "sort order out of range"),
    (T, (0,), fn(0)[:7], (0,), (1,), (1,), 10, -1, "malformed function array"),
    (T, (0,), (), (0,), (1,), (1,), 10, -1, "no window function"),
    (T, (0,), fn(0) * 17, (0,), (1,), (1,), 10, -1, "more than 16 window functions"),
    (T, (0,), fn(10), (0,), (1,), (1,), 10, -1, "unknown window function"),
    (T, (0,), fn(-1), (0,), (1,), (1,), 10, -1, "unknown window function"),
    (T, (0,), fn(0, frame=3), (0,), (1,), (1,), 10, -1, "unknown window frame"),
    (T, (0,), fn(0, frame=-1), (0,), (1,), (1,), 10, -1, "unknown window frame"),
    (T, (0,), fn(5, args=(0,), ignore_nulls=1), (0,), (1,), (1,), 10, -8, "IGNORE NULLS is not supported"),
    (T, (0,), (5, 0, 1, 4, 0, 0, 0, 0), (0,), (1,), (1,), 10, -1, "a window function takes 0 to 3 arguments"),
    (T, (0,), fn(7, args=(4,)), (0,), (1,), (1,), 10, -1, "argument channel out of range"),
    (T, (0,), fn(1, args=(0,)), (0,), (1,), (1,), 10, -1, "the ranking functions take no argument"),
    (T, (0,), fn(5), (0,), (1,), (1,), 10, -1, "lag / lead take 1 to 3 arguments"),
    (T, (0,), fn(6, args=(2, 1)), (0,), (1,), (1,), 10, -1, "the offset of lag / lead must be BIGINT"),
    (T, (0,), fn(5, args=(2, 0, 1)), (0,), (1,), (1,), 10, -1, "the default of lag / lead must have the value's type"),
    (T, (0,), fn(7), (0,), (1,), (1,), 10, -1, "first_value / last_value take one argument"),
    (T, (0,), fn(8, args=(0, 0)), (0,), (1,), (1,), 10, -1, "first_value / last_value take one argument"),
    (T, (0,), fn(9, agg=1, args=(0,)), (0,), (1,), (1,), 10, -1, "count(*) takes no argument"),
    (T, (0,), fn(9, agg=2), (0,), (1,), (1,), 10, -1, "count(x) takes one argument"),
    (T, (0,), fn(9, agg=3, args=(1,)), (0,), (1,), (1,), 10, -1, "the aggregate takes one BIGINT argument"),
    (T, (0,), fn(9, agg=8), (0,), (1,), (1,), 10, -1, "the aggregate takes one BIGINT argument"),
    (T, (0,), fn(9, agg=9, args=(0,)), (0,), (1,), (1,), 10, -1, "the aggregate takes one DOUBLE argument"),
    (T, (0,), fn(9, agg=4, args=(1,)), (0,), (1,), (1,), 10, -8, "sum(double) and avg are not supported as window aggregates"),
    (T, (0,), fn(9, agg=5, args=(0,)), (0,), (1,), (1,), 10, -8, "sum(double) and avg are not supported as window aggregates"),
    (T, (0,), fn(9, agg=6, args=(1,)), (0,), (1,), (1,), 10, -8, "sum(double) and avg are not supported as window aggregates"),
    (T, (0,), fn(9, agg=0), (0,), (1,), (1,), 10, -1, "unknown aggregate function"),
    (T, (0,), fn(9, agg=11, args=(0,)), (0,), (1,), (1,), 10, -1, "unknown aggregate function"),
    (T, (0,), fn(0) + fn(9, agg=11), (0,), (1,), (1,), 10, -1, "unknown aggregate function"),   # the second function
    (T, (0,), fn(0), (0,), (1,), (1,), 0, -1, "expected positions must be positive"),
    (T, (0,), fn(0), (0,), (1,), (1,), -3, -1, "expected positions must be positive"),
]


@pytest.mark.parametrize("types, outputs, functions, partitions, sorts, orders, expected_positions, code, why", BAD)
def test_arguments_are_checked_in_front_of_the_library(jvm, types, outputs, functions, partitions, sorts, orders, expected_positions, code, why):
    r = jvm.call("createWindowFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), ints(jvm, *outputs), ints(jvm, *functions), ints(jvm, *partitions),
                 ints(jvm, *sorts), ints(jvm, *orders), C.c_int32(expected_positions))
    assert r == 0
    assert jvm.pending_code() == code and jvm.pending_message() == "window: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0

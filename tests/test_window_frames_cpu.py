"""Window frames with bounds without a GPU: the expected-value helper (tests/window_frames_expected.py) reproduces every case transcribed from the
reference's tests (tests/golden/window_frame_vectors.json), so the yardstick of the GPU tests is itself checked; the golden file covers the five
empty-frame rules of ROWS, a GROUPS case with every bound type, nth_value and ntile; hand-written cases pin offsets beyond the partition, the
per-row offset, the errors and the frame-local sum overflow; tgpu.h declares the framed entry point and the enums, libtgpu.so exports it, _lib.py
binds it and the package exports the names; the JNI shim's createFramedWindowFactory rejects every bad argument with a pending NativeError before
the library is called and accepts what createWindowFactory refuses; the Java sources declare the native, the helper and the factory method."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from jni_harness import FakeJvm, build_fake_jni, header_symbols
from window_expected import AGGREGATE, ASC_NULLS_LAST, BIGINT, COUNT_ALL, FIRST_VALUE, FRAME_ROWS_TO_CURRENT, LAST_VALUE, SUM_BIGINT, Fn, InvalidArgument, NumericValueOutOfRange, tokens
from window_frames_expected import (CURRENT_ROW, FOLLOWING, GROUPS, NTH_VALUE, NTILE, PRECEDING, RANGE, ROWS, UNBOUNDED_FOLLOWING, UNBOUNDED_PRECEDING, Frame, expected_output,
                                    golden_case, golden_group_case, valid_bounds)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "window_frame_vectors.json")))
ORDERS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}


def multiset(rows):
    return sorted(map(repr, tokens(rows)))


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_helper_reproduces_reference_case(case):
    types, pages, functions, expected = golden_case(case)
    got = expected_output(types, pages, case["output_channels"], functions, case["partition_channels"], case["sort_channels"], [ORDERS[o] for o in case["sort_orders"]])
    assert multiset(got) == multiset(expected)   # the reference compares these ignoring order


@pytest.mark.parametrize("case", GOLD["groups"], ids=lambda c: c["name"])
def test_helper_reproduces_reference_groups_case(case):
    types, pages, functions, expected = golden_group_case(case)
    got = expected_output(types, pages, case["output_channels"], functions, case["partition_channels"], case["sort_channels"], [ORDERS[o] for o in case["sort_orders"]])
    assert multiset(got) == multiset(expected)


def test_golden_file_covers_what_it_should():
    sources = {c["source"].split("#")[0] for c in GOLD["cases"]}
    for method in ("testCountRowsRolling", "testSumRolling", "testSumRollingUnboundedPrecedingNPreceding", "testSumRollingNFollowingUnboundedFollowing", "testSumCurrentRow",
                   "testSumEmptyWindow"):
        assert "TestAggregateWindowFunction." + method in sources
    for cls in ("FirstValue", "LastValue", "NthValue", "NTile"):
        assert any(s.startswith("Test%sFunction." % cls) for s in sources), cls
    assert GOLD["skipped"] and all(s["reason"] and s["source"] and s["sql"] for s in GOLD["skipped"])
    assert not any("avg(" in c["sql"] for c in GOLD["cases"])
    assert {f["function"] for c in GOLD["cases"] for f in c["functions"]} == {"AGGREGATE", "FIRST_VALUE", "LAST_VALUE", "NTH_VALUE", "NTILE"}
    # ROWS: a case where each of the five empty-frame rules empties at least one row's frame (the expected value is null / 0 there)
    rows = {(c["functions"][0]["frame"]["start"], c["functions"][0]["frame"]["end"], c["sql"]) for c in GOLD["cases"] if c["functions"][0]["frame"]["type"] == "ROWS"}
    has = lambda start, end, text: any(s == start and e == end and text in sql for s, e, sql in rows)
    assert has("UNBOUNDED_PRECEDING", "PRECEDING", "AND 2 PRECEDING")          # b > r
    assert has("FOLLOWING", "UNBOUNDED_FOLLOWING", "3 FOLLOWING AND")          # a > E - r
    assert has("PRECEDING", "PRECEDING", "2 PRECEDING AND 3 PRECEDING")        # a < b
    assert has("PRECEDING", "PRECEDING", "4 PRECEDING AND 2 PRECEDING")        # a > r and b > r in the first rows
    assert has("FOLLOWING", "FOLLOWING", "4 FOLLOWING AND 3 FOLLOWING")        # a > b
    assert has("FOLLOWING", "FOLLOWING", "2 FOLLOWING AND 4 FOLLOWING")        # a > E - r in the last rows
    # GROUPS: every bound type on each side it can stand on
    starts = {c["frame"]["start"] for c in GOLD["groups"]}
    ends = {c["frame"]["end"] for c in GOLD["groups"]}
    assert starts == {"UNBOUNDED_PRECEDING", "PRECEDING", "CURRENT_ROW", "FOLLOWING"} and ends == {"PRECEDING", "CURRENT_ROW", "FOLLOWING", "UNBOUNDED_FOLLOWING"}
    assert any("INTEGER" in c["types"] for c in GOLD["groups"])                # a per-row INTEGER offset column
    assert any(c["partition_channels"] for c in GOLD["groups"]) and any(f is None for c in GOLD["groups"] for f in c["frames"])
    for c in GOLD["cases"] + GOLD["groups"]:
        frame = c["functions"][0]["frame"] if "functions" in c else c["frame"]
        assert ("start_channel" in frame) == (frame["start"] in ("PRECEDING", "FOLLOWING")) and ("end_channel" in frame) == (frame["end"] in ("PRECEDING", "FOLLOWING"))


# ---- hand-written cases of the helper -------------------------------------------------------------------------------------------------------------
def one_partition(values, offsets, frame, functions):
    """rows (value, start offset, end offset) in one partition ordered by arrival"""
    rows = [(v, a, b) for v, (a, b) in zip(values, offsets)]
    fns = [Fn(f, args, Frame(frame[0], frame[1], frame[2], 1, 2), agg) for f, args, agg in functions]
    return [r[1:] for r in expected_output([BIGINT] * 3, [rows], [0], fns, [], [], [])]


def test_rows_offsets_are_read_per_row_and_may_exceed_any_partition():
    big = 2**63 - 1
    got = one_partition([1, 2, 3, 4], [(0, 0), (1, big), (big, 1), (2, 0)], (ROWS, PRECEDING, FOLLOWING), [(AGGREGATE, (0,), SUM_BIGINT), (AGGREGATE, (), COUNT_ALL)])
    assert got == [(1, 1), (1 + 2 + 3 + 4, 4), (1 + 2 + 3 + 4, 4), (2 + 3 + 4, 3)]
    got = one_partition([1, 2, 3], [(big, big)] * 3, (ROWS, FOLLOWING, FOLLOWING), [(FIRST_VALUE, (0,), 0), (AGGREGATE, (), COUNT_ALL)])
    assert got == [(None, 0)] * 3                                              # a > E - r everywhere: even in the last row, where E - r = 0 < a
    got = one_partition([1, 2, 3], [(big, big)] * 3, (ROWS, PRECEDING, PRECEDING), [(LAST_VALUE, (0,), 0)])
    assert got == [(None,)] * 3                                                # a > r and b > r
    got = one_partition([1, 2, 3], [(big, 0)] * 3, (ROWS, PRECEDING, PRECEDING), [(LAST_VALUE, (0,), 0), (FIRST_VALUE, (0,), 0)])
    assert got == [(1, 1), (2, 1), (3, 1)]                                     # max(r - a, 0) .. r


def test_groups_count_peer_groups_not_rows():
    types = [BIGINT, BIGINT]   # sort key with ties, row id
    rows = [(1, 0), (1, 1), (2, 2), (3, 3), (3, 4), (3, 5), (4, 6)]
    frame = lambda s, e: Frame(GROUPS, s, e, 2, 2)
    rows = [r + (1,) for r in rows]
    fns = [Fn(FIRST_VALUE, (1,), frame(PRECEDING, FOLLOWING)), Fn(LAST_VALUE, (1,), frame(PRECEDING, FOLLOWING)), Fn(AGGREGATE, (), frame(FOLLOWING, UNBOUNDED_FOLLOWING), COUNT_ALL),
           Fn(AGGREGATE, (), frame(UNBOUNDED_PRECEDING, PRECEDING), COUNT_ALL), Fn(AGGREGATE, (), Frame(RANGE, CURRENT_ROW, CURRENT_ROW), COUNT_ALL)]
    got = expected_output(types + [BIGINT], [rows], [1], fns, [], [0], [ASC_NULLS_LAST])
    assert got == [(0, 0, 2, 5, 0, 2), (1, 0, 2, 5, 0, 2), (2, 0, 5, 4, 2, 1), (3, 2, 6, 1, 3, 3), (4, 2, 6, 1, 3, 3), (5, 2, 6, 1, 3, 3), (6, 3, 6, 0, 6, 1)]


def test_offset_errors_and_function_argument_errors():
    for offsets, text in (([(None, 0)], "Window frame starting offset must not be null"), ([(0, None)], "Window frame ending offset must not be null"),
                          ([(-1, 0)], "Window frame offset must not be negative"), ([(0, -5)], "Window frame offset must not be negative")):
        for kind in (ROWS, GROUPS):
            with pytest.raises(InvalidArgument, match=text):
                one_partition([1], offsets, (kind, PRECEDING, FOLLOWING), [(AGGREGATE, (), COUNT_ALL)])
    nth = lambda value, offset: expected_output([BIGINT, BIGINT], [[(value, offset), (value + 1, offset)]], [], [Fn(NTH_VALUE, (0, 1), Frame(ROWS, UNBOUNDED_PRECEDING, CURRENT_ROW))],
                                                [], [], [])
    assert nth(5, 1) == [(5,), (5,)] and nth(5, 2) == [(None,), (6,)] and nth(5, None) == [(None,), (None,)] and nth(5, 2**63 - 1) == [(None,), (None,)]
    with pytest.raises(InvalidArgument, match="Offset must be at least 1"):
        nth(5, 0)
    tile = lambda n, buckets: [r[0] for r in expected_output([BIGINT], [[(buckets,)] * n], [], [Fn(NTILE, (0,), 0)], [], [], [])]
    assert tile(5, 1) == [1] * 5 and tile(5, 5) == [1, 2, 3, 4, 5] and tile(5, 9) == [1, 2, 3, 4, 5] and tile(5, 2) == [1, 1, 1, 2, 2] and tile(7, 3) == [1, 1, 1, 2, 2, 3, 3]
    assert tile(3, None) == [None] * 3
    for bad in (0, -1):
        with pytest.raises(InvalidArgument, match="Buckets must be greater than 0"):
            tile(2, bad)


def test_only_a_frames_own_sum_has_to_fit():
    big = 2**62
    values = [big, big, -big, big, big, None, -big]
    two = lambda vals: [r[0] for r in one_partition(vals, [(1, 0)] * len(vals), (ROWS, PRECEDING, FOLLOWING), [(AGGREGATE, (0,), SUM_BIGINT)])]
    with pytest.raises(NumericValueOutOfRange, match="bigint addition overflow"):
        two(values)                                                            # rows 0 + 1 = 2^63
    values = [big, big - 1, 5, big - 1, 3, None, big - 1]
    assert two(values) == [big, 2 * big - 1, big + 4, big + 4, big + 2, 3, big - 1]   # the prefix 2^62 + 2^62 - 1 + 5 leaves int64, no frame of two rows does
    with pytest.raises(NumericValueOutOfRange):                                # the same values under an old frame: the prefix counts
        expected_output([BIGINT], [[(v,) for v in values]], [], [Fn(AGGREGATE, (0,), FRAME_ROWS_TO_CURRENT, SUM_BIGINT)], [], [], [])


def test_the_numpy_reduction_of_wide_frames_agrees_with_the_accumulator(monkeypatch):
    """every aggregate over frames of 16 to 400 rows: one numpy reduction (WideColumns) against the Accumulator fed the frame's rows one by one"""
    import window_frames_expected as w
    rng = np.random.default_rng(11)
    n = 400
    d = rng.integers(-3, 4, n).astype(np.float64)
    d[rng.random(n) < 0.2] = np.nan
    d[rng.random(n) < 0.2] = -0.0
    d[40:80] = np.nan   # frames of NaN only, and below of nulls only
    big = [int(v) for v in rng.integers(-2**62, 2**62, n)]
    nulls = rng.random(n) < 0.2
    nulls[100:140] = True
    rows = [(None if nulls[i] else int(rng.integers(-9, 10)), None if nulls[i] else float(d[i]), None if nulls[i] else big[i] // 512, i % 21, 17) for i in range(n)]
    frame = Frame(ROWS, PRECEDING, FOLLOWING, 3, 4)
    fns = [Fn(AGGREGATE, args, frame, agg) for agg, args in ((1, ()), (2, (0,)), (3, (0,)), (3, (2,)), (7, (0,)), (8, (0,)), (7, (2,)), (9, (1,)), (10, (1,)))]
    types = [BIGINT, 4, BIGINT, BIGINT, BIGINT]
    fast = tokens(expected_output(types, [rows], [], fns, [], [], []))
    monkeypatch.setattr(w, "WIDE", 10**9)
    slow = tokens(expected_output(types, [rows], [], fns, [], [], []))
    assert fast == slow and any(r[7] != r[7] or repr(r[7]) == "nan" or r[7] is None for r in slow)


def test_valid_bound_combinations_are_the_analyzers():
    ok = {(s, e) for s in range(5) for e in range(5) if valid_bounds(s, e)}
    assert ok == {(UNBOUNDED_PRECEDING, e) for e in (PRECEDING, CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING)} | {(PRECEDING, e) for e in (PRECEDING, CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING)} | \
        {(CURRENT_ROW, e) for e in (CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING)} | {(FOLLOWING, FOLLOWING), (FOLLOWING, UNBOUNDED_FOLLOWING)}


# ---- header, library, binding, package -----------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_framed_entry_point(pkg):
    name = "tgpu_window_factory_create_framed"
    assert name in set(header_symbols())
    assert hasattr(pkg._lib.lib(), name)
    assert name in pkg._lib.SYMBOLS
    assert (pkg.WINDOW_NTH_VALUE, pkg.WINDOW_NTILE) == (10, 11) == (NTH_VALUE, NTILE)
    assert (pkg.FRAME_TYPE_RANGE, pkg.FRAME_TYPE_ROWS, pkg.FRAME_TYPE_GROUPS) == (0, 1, 2) == (RANGE, ROWS, GROUPS)
    assert (pkg.BOUND_UNBOUNDED_PRECEDING, pkg.BOUND_PRECEDING, pkg.BOUND_CURRENT_ROW, pkg.BOUND_FOLLOWING, pkg.BOUND_UNBOUNDED_FOLLOWING) == (0, 1, 2, 3, 4)
    assert (UNBOUNDED_PRECEDING, PRECEDING, CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING) == (0, 1, 2, 3, 4)
    header = open(os.path.join(ROOT, "include", "tgpu.h")).read()
    assert "TGPU_WINDOW_AGGREGATE = 9,\n    TGPU_WINDOW_NTH_VALUE = 10, TGPU_WINDOW_NTILE = 11" in header
    assert "TGPU_FRAME_TYPE_RANGE = 0, TGPU_FRAME_TYPE_ROWS = 1, TGPU_FRAME_TYPE_GROUPS = 2" in header
    assert "TGPU_BOUND_UNBOUNDED_PRECEDING = 0, TGPU_BOUND_PRECEDING = 1, TGPU_BOUND_CURRENT_ROW = 2, TGPU_BOUND_FOLLOWING = 3, TGPU_BOUND_UNBOUNDED_FOLLOWING = 4" in header
    assert "typedef struct tgpu_window_frame_spec { int32_t type, start_type, start_channel, end_type, end_channel; } tgpu_window_frame_spec;" in header
    frame = pkg.WindowFrame(pkg.FRAME_TYPE_ROWS, pkg.BOUND_PRECEDING, pkg.BOUND_FOLLOWING, 3, 4)
    spec = frame.spec()
    assert isinstance(spec, pkg._lib.WindowFrameSpec) and C.sizeof(pkg._lib.WindowFrameSpec) == 20
    assert (spec.type, spec.start_type, spec.start_channel, spec.end_type, spec.end_channel) == (1, 1, 3, 3, 4)
    assert pkg.WindowFrame(0, 0, 4).spec().start_channel == -1 and pkg.WindowFrame(0, 0, 4).spec().end_channel == -1
    # which entry point a function needs, and the old codes as frames
    assert not pkg.WindowFunction(pkg.WINDOW_LAG, (0,), pkg.FRAME_PARTITION).framed()
    assert pkg.WindowFunction(pkg.WINDOW_NTILE, (0,)).framed() and pkg.WindowFunction(pkg.WINDOW_FIRST_VALUE, (0,), frame).framed()
    as_frames = [pkg.WindowFunction(pkg.WINDOW_ROW_NUMBER, (), code).frame_spec() for code in (pkg.FRAME_PARTITION, pkg.FRAME_RANGE_TO_CURRENT, pkg.FRAME_ROWS_TO_CURRENT)]
    assert [(s.type, s.start_type, s.end_type) for s in as_frames] == [(0, 0, 4), (0, 0, 2), (1, 0, 2)]
    assert pkg.WindowFunction(pkg.WINDOW_FIRST_VALUE, (0,), frame).spec().frame == 0 and C.sizeof(pkg.WindowFunction(pkg.WINDOW_RANK).spec()) == 32


def test_java_sources_declare_the_native_the_helper_and_the_factory_method():
    strip = lambda t: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    native = strip(open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuNative.java")).read())
    m = re.search(r"public static native long createFramedWindowFactory\((.*?)\);", native, flags=re.S)
    assert m and [p.strip().rsplit(" ", 1)[0] for p in m.group(1).split(",")] == ["long", "int", "int[]", "int[]", "int[]", "int[]", "int[]", "int[]", "int[]", "int"]
    assert [p.strip().rsplit(" ", 1)[1] for p in m.group(1).split(",")][4:6] == ["functions", "frames"]
    glue = strip(open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuOperatorFactories.java")).read())
    assert re.search(r"public Optional<OperatorFactory> framedWindow\(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels, "
                     r"List<int\[\]> functions,\s*List<int\[\]> frames,", glue)
    assert "GpuNative.createFramedWindowFactory(context, operatorId, codes," in glue and "import io.trino.operator.window.FrameInfo;" in glue
    assert re.search(r"public static int\[\] windowFrame\(FrameInfo frame\)", glue)
    assert "frame.getType().ordinal(), frame.getStartType().ordinal(), frame.getStartChannel(), frame.getEndType().ordinal(), frame.getEndChannel()" in glue
    for name, code in (("WINDOW_NTH_VALUE", 10), ("WINDOW_NTILE", 11), ("FRAME_TYPE_RANGE", 0), ("FRAME_TYPE_ROWS", 1), ("FRAME_TYPE_GROUPS", 2), ("BOUND_UNBOUNDED_PRECEDING", 0),
                       ("BOUND_PRECEDING", 1), ("BOUND_CURRENT_ROW", 2), ("BOUND_FOLLOWING", 3), ("BOUND_UNBOUNDED_FOLLOWING", 4)):
        assert re.search(r"public static final int %s = %d;" % (name, code), glue)
    shim = open(os.path.join(ROOT, "jni", "tgpu_jni.c")).read()
    assert "JFN(jlong, createFramedWindowFactory)" in shim and "tgpu_window_factory_create_framed(" in shim


# ---- the JNI shim ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


def fn(function, agg=0, frame=1, args=(), ignore_nulls=0):
    return (function, agg, frame, len(args)) + tuple(args) + (0,) * (3 - len(args)) + (ignore_nulls,)


def fr(kind=1, start=0, end=2, start_channel=-1, end_channel=-1):
    return (kind, start, start_channel, end, end_channel)


T = (1, 4, 6, 2)   # BIGINT, DOUBLE, VARCHAR, INTEGER
# (types, output channels, functions flattened, frames flattened, partition channels, sort channels, sort orders, expectedPositions, code, message)
BAD = [
    ((), (), fn(0), fr(), (), (), (), 10, -1, "empty type array"),
    ((1, 7), (0,), fn(0), fr(), (), (), (), 10, -1, "unknown type"),
    (T, (4,), fn(0), fr(), (), (), (), 10, -1, "output channel out of range"),
    (T, (0,), fn(0), fr(), (0,), (1, 0), (1,), 10, -1, "sort channels and sort orders differ in length"),
    (T, (0,), fn(0), fr(), (0,) * 5, (1,) * 4, (1,) * 4, 10, -1, "more than 8 partition and sort channels"),
    (T, (0,), fn(0), fr(), (4,), (), (), 10, -1, "partition channel out of range"),
    (T, (0,), fn(0), fr(), (0,), (-1,), (1,), 10, -1, "sort channel out of range"),
    (T, (0,), fn(0), fr(), (0,), (1,), (4,), 10, -1, "sort order out of range"),
    (T, (0,), fn(0)[:7], fr(), (0,), (1,), (1,), 10, -1, "malformed function array"),
    (T, (0,), (), (), (0,), (1,), (1,), 10, -1, "no window function"),
    (T, (0,), fn(0) * 17, fr() * 17, (0,), (1,), (1,), 10, -1, "more than 16 window functions"),
    (T, (0,), fn(0), fr()[:4], (0,), (1,), (1,), 10, -1, "malformed frame array"),
    (T, (0,), fn(0), fr() + (0,), (0,), (1,), (1,), 10, -1, "malformed frame array"),
    (T, (0,), fn(0), fr() * 2, (0,), (1,), (1,), 10, -1, "frame array and function array differ in length"),
    (T, (0,), fn(0) * 2, fr(), (0,), (1,), (1,), 10, -1, "frame array and function array differ in length"),
    (T, (0,), fn(0), (), (0,), (1,), (1,), 10, -1, "frame array and function array differ in length"),
    (T, (0,), fn(12), fr(), (0,), (1,), (1,), 10, -1, "unknown window function"),
    (T, (0,), fn(-1), fr(), (0,), (1,), (1,), 10, -1, "unknown window function"),
    (T, (0,), fn(0), fr(kind=3), (0,), (1,), (1,), 10, -1, "unknown window frame type"),
    (T, (0,), fn(0), fr(kind=-1), (0,), (1,), (1,), 10, -1, "unknown window frame type"),
    (T, (0,), fn(0), fr(start=5), (0,), (1,), (1,), 10, -1, "unknown window frame bound"),
    (T, (0,), fn(0), fr(end=-1), (0,), (1,), (1,), 10, -1, "unknown window frame bound"),
    (T, (0,), fn(0), fr(start=4, end=4), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),                       # UNBOUNDED FOLLOWING start
    (T, (0,), fn(0), fr(start=0, end=0), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),                       # UNBOUNDED PRECEDING end
    (T, (0,), fn(0), fr(start=2, end=1, end_channel=0), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),        # CURRENT ROW .. PRECEDING
    (T, (0,), fn(0), fr(start=3, end=2, start_channel=0), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),      # FOLLOWING .. CURRENT ROW
    (T, (0,), fn(0), fr(start=3, end=1, start_channel=0, end_channel=0), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),   # FOLLOWING .. PRECEDING
    (T, (0,), fn(0), fr(start=1, start_channel=4), (0,), (1,), (1,), 10, -1, "frame offset channel out of range"),
    (T, (0,), fn(0), fr(start=1, start_channel=-1), (0,), (1,), (1,), 10, -1, "frame offset channel out of range"),
    (T, (0,), fn(0), fr(end=3, end_channel=9), (0,), (1,), (1,), 10, -1, "frame offset channel out of range"),
    (T, (0,), fn(0), fr(start=1, start_channel=1), (0,), (1,), (1,), 10, -1, "a frame offset must be BIGINT or INTEGER"),
    (T, (0,), fn(0), fr(kind=2, end=3, end_channel=2), (0,), (1,), (1,), 10, -1, "a frame offset must be BIGINT or INTEGER"),
    (T, (0,), fn(0), fr(kind=0, start=1, start_channel=0), (0,), (1,), (1,), 10, -8, "RANGE frames with an offset are not supported"),
    (T, (0,), fn(0), fr(kind=0, end=3, end_channel=3), (0,), (1,), (1,), 10, -8, "RANGE frames with an offset are not supported"),
    (T, (0,), fn(0) + fn(0), fr() + fr(kind=0, end=3, end_channel=3), (0,), (1,), (1,), 10, -8, "RANGE frames with an offset are not supported"),   # the second frame
    (T, (0,), fn(10, args=(2,)), fr(), (0,), (1,), (1,), 10, -1, "nth_value takes a value and a BIGINT offset"),
    (T, (0,), fn(10, args=(2, 1)), fr(), (0,), (1,), (1,), 10, -1, "nth_value takes a value and a BIGINT offset"),
    (T, (0,), fn(10, args=(2, 3)), fr(), (0,), (1,), (1,), 10, -1, "nth_value takes a value and a BIGINT offset"),     # INTEGER is not BIGINT
    (T, (0,), fn(10, args=(2, 0), ignore_nulls=1), fr(), (0,), (1,), (1,), 10, -8, "IGNORE NULLS is not supported"),
    (T, (0,), fn(11), fr(), (0,), (1,), (1,), 10, -1, "ntile takes one BIGINT argument"),
    (T, (0,), fn(11, args=(1,)), fr(), (0,), (1,), (1,), 10, -1, "ntile takes one BIGINT argument"),
    (T, (0,), fn(7, args=(4,)), fr(), (0,), (1,), (1,), 10, -1, "argument channel out of range"),
    (T, (0,), fn(9, agg=4, args=(1,)), fr(), (0,), (1,), (1,), 10, -8, "sum(double) and avg are not supported as window aggregates"),
    (T, (0,), fn(9, agg=3, args=(1,)), fr(start=1, start_channel=0), (0,), (1,), (1,), 10, -1, "the aggregate takes one BIGINT argument"),
    (T, (0,), fn(0), fr(), (0,), (1,), (1,), 0, -1, "expected positions must be positive"),
]


def call(jvm, types, outputs, functions, frames, partitions, sorts, orders, expected_positions):
    return jvm.call("createFramedWindowFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), ints(jvm, *outputs), ints(jvm, *functions), ints(jvm, *frames),
                    ints(jvm, *partitions), ints(jvm, *sorts), ints(jvm, *orders), C.c_int32(expected_positions))


@pytest.mark.parametrize("types, outputs, functions, frames, partitions, sorts, orders, expected_positions, code, why", BAD)
def test_arguments_are_checked_in_front_of_the_library(jvm, types, outputs, functions, frames, partitions, sorts, orders, expected_positions, code, why):
    assert call(jvm, types, outputs, functions, frames, partitions, sorts, orders, expected_positions) == 0
    assert jvm.pending_code() == code and jvm.pending_message() == "window: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


def test_the_framed_native_accepts_what_the_old_one_refuses(jvm):
    """function = 10 passes the shim's checks and reaches the library, which refuses the null context handle: not one of the shim's own "window: .." messages"""
    old = jvm.call("createWindowFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *T), ints(jvm, 0), ints(jvm, *fn(10, args=(2, 0))), ints(jvm, 0), ints(jvm, 1),
                   ints(jvm, 1), C.c_int32(10))
    assert old == 0 and jvm.pending_message() == "window: unknown window function"
    jvm.clear()
    for functions, frames in ((fn(10, args=(2, 0)), fr(start=1, end=3, start_channel=0, end_channel=3)), (fn(11, args=(0,)), fr()),
                              (fn(9, agg=8, args=(0,)), fr(kind=2, start=3, end=4, start_channel=3)), (fn(8, args=(2,), frame=99), fr(kind=0, start=2, end=4))):
        assert call(jvm, T, (0,), functions, frames, (0,), (1,), (1,), 10) == 0   # the null context
        assert jvm.pending_code() != 0 and not (jvm.pending_message() or "").startswith("window: ")
        jvm.clear()
        assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0

"""RANGE frames with k PRECEDING / k FOLLOWING bounds, on the CPU: the reference's stateful walk restated (tests/window_range_expected.py walk_frames), the
closed form include/tgpu.h states (closed_frames) and the kernels' decision logic compiled for the host under the sanitizers
(presto-1_amd/csrc/device_range_frame.h through tests/range_frame/range_main.cpp) give the same frames on the reference's cases
(tests/golden/window_range_vectors.json) and on a seeded corpus of planner-conforming tables; closed form and host program agree on arbitrary bounds
too; the golden file skips only what it may; tgpu.h declares the ranged entry point, libtgpu.so exports it, _lib.py binds it, the Java sources declare the
native and the two methods; the JNI shim's createRangeWindowFactory rejects every bad argument with a pending NativeError before the library sees it; and
the framed entry point still refuses RANGE offsets."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import window_range_cases as W
import window_range_expected as X
from jni_harness import FakeJvm, build_fake_jni, header_symbols
from window_expected import InvalidArgument, tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "window_range_vectors.json")))
LIVE = [c for c in GOLD["cases"] if "skip" not in c]
SRC = os.path.join(ROOT, "tests", "range_frame", "range_main.cpp")
OUT = os.path.join(ROOT, "tests", "range_frame", "build")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MASK = 2**64 - 1


# ---- the golden file -------------------------------------------------------------------------------------------------------------------------------
def test_golden_file_skips_only_what_it_may():
    assert len(GOLD["cases"]) == 84 and len(LIVE) == 63
    skipped = [c for c in GOLD["cases"] if "skip" in c]
    assert {c["test"] for c in skipped} == {"testInvalidOffset"} and all("planner" in c["skip"] and c["message"] == "Window frame offset value must not be negative or null" for c in skipped)
    inner = [(c["test"], o["function"], o["argument"]) for c in LIVE for o in c["outputs"] if "skip" in o]
    assert inner == [("testMultipleWindowFunctions", "avg", "number")]
    assert {c["test"] for c in LIVE} == {"testNullsSortKey", "testNoValueFrameBounds", "testMixedTypeFrameBoundsAscendingNullsFirst", "testMixedTypeFrameBoundsAscendingNullsLast",
                                         "testMixedTypeFrameBoundsDescendingNullsFirst", "testMixedTypeFrameBoundsDescendingNullsLast", "testEmptyFrame", "testOnlyNulls",
                                         "testAllPartitionSameValues", "testZeroOffset", "testNonConstantOffset", "testWindowPartitioning", "testTypes", "testMultipleWindowFunctions"}
    assert {c["key_type"] for c in LIVE} == {"INTEGER", "DOUBLE", "DATE", "BIGINT"}


def multiset(rows):
    return sorted(map(repr, tokens(rows)))


@pytest.mark.parametrize("how", ["walk", "closed"])
@pytest.mark.parametrize("case", LIVE, ids=lambda c: c["sql"][7:90])
def test_walk_and_closed_form_give_the_reference_arrays(case, how):
    """matches() ignores row order: multisets"""
    types, rows, outputs, functions, partitions, order, expected = W.golden_table(case)
    got = X.expected_output(types, [rows], outputs, functions, partitions, [0], [order], how)
    assert multiset(got) == multiset(expected)


# ---- the host program ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def range_main():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "range_main")
    deps = [SRC, os.path.join(ROOT, "presto-1_amd", "csrc", "device_range_frame.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-std=c++17"] + SANITIZE + ["-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def partition_lines(part, order):
    """one partition in range_main's format; codes complemented under a descending sort, as window.hip's gather leaves them"""
    flip = (lambda c: 0 if c is None else c) if part.asc else (lambda c: 0 if c is None else ~c & MASK)
    lines = ["P %d %d %d %d" % (part.n, part.frame.start, part.frame.end, 1 if X.nulls_first(order) else 0)]
    for p in range(part.n):
        lines.append("%d %d %d %d %d %d %d" % (part.key_null[p], flip(part.start_key[p]), flip(part.end_key[p]), flip(part.start_bound[p]), flip(part.end_bound[p]),
                                               part.peer_s[p], part.peer_e[p]))
    return lines


def host_frames(exe, parts_with_orders, tmp_path, name):
    path = str(tmp_path / (name + ".cases"))
    with open(path, "w") as f:
        for part, order in parts_with_orders:
            f.write("\n".join(partition_lines(part, order)) + "\n")
    # (the time limit only catches a program that does not end: the cases take a second or two)
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, "sanitizer report or crash (exit %d):\n%s" % (p.returncode, p.stderr.decode()[-3000:])
    frames = [tuple(int(x) for x in line.split()) for line in p.stdout.decode().splitlines()]
    assert len(frames) == sum(part.n for part, _ in parts_with_orders)
    out, at = [], 0
    for part, _ in parts_with_orders:
        out.append([None if f == (-1, -1) else f for f in frames[at:at + part.n]])
        at += part.n
    return out


def corpus_partitions(cases):
    out = []
    for c in cases:
        for part in X.sorted_partitions(c["types"], [c["rows"]], [0], [1], [c["order"]]):
            out.append((X.Partition(c["types"], 1, c["order"], c["frame"], part), c["order"], c["name"]))
    return out


def test_corpus_covers_what_it_should():
    cases = W.corpus(20260101, per_combination=4)
    assert len(cases) == 4 * 4 * 13 * 4
    assert {(c["types"][1], c["order"], c["frame"].start, c["frame"].end) for c in cases} == {(t, o, s, e) for t in W.KEY_TYPES for o in W.ORDERS for s, e in W.COMBINATIONS}
    keys = [r[1] for c in cases for r in c["rows"]]
    assert W.I64_MIN in keys and W.I64_MAX in keys and any(k != k for k in keys if isinstance(k, float)) and W.INF in keys and -W.INF in keys
    assert any(isinstance(k, float) and k == 0 and np.signbit(k) for k in keys) and any(isinstance(k, float) and k == 0 and not np.signbit(k) for k in keys)
    assert any(all(r[1] is None for r in c["rows"]) for c in cases) and any(all(r[1] is not None for r in c["rows"]) for c in cases)
    assert any(len({r[1] for r in c["rows"]}) == 1 and c["rows"][0][1] is not None and len(c["rows"]) > 3 for c in cases)
    # offsets 0, constant, per row, beyond the domain: |bound - key| over the non-null rows
    gaps = {abs(r[4] - r[1]) for c in cases if c["types"][1] == W.BIGINT for r in c["rows"] if r[1] is not None and r[4] is not None}
    assert 0 in gaps and 1000 in gaps and 7 in gaps
    # the bounds at both int64 edges
    bounds = {r[4] for c in cases for r in c["rows"]} | {r[5] for c in cases for r in c["rows"]}
    assert W.I64_MIN in bounds and W.I64_MAX in bounds


def test_walk_closed_form_and_host_program_agree_on_conforming_inputs(range_main, tmp_path):
    """if the walk and the closed form disagreed here, the walk would be the reference"""
    parts = corpus_partitions(W.corpus(20260101, per_combination=4))
    for case in LIVE:
        types, rows, _, functions, partitions, order, _ = W.golden_table(case)
        for frame in {f.frame for f in functions}:
            for part in X.sorted_partitions(types, [rows], partitions, [0], [order]):
                parts.append((X.Partition(types, 0, order, frame, part), order, case["sql"]))
    host = host_frames(range_main, [(p, o) for p, o, _ in parts], tmp_path, "conforming")
    for (part, _, name), from_host in zip(parts, host):
        walk, closed = X.walk_frames(part), X.closed_frames(part)
        assert walk == closed, name
        assert from_host == closed, name


def test_closed_form_and_host_program_agree_on_arbitrary_bounds(range_main, tmp_path):
    """bounds that have nothing to do with the keys: the reference's walk may leave the partition there, the library's frame is the closed form and the
    sanitizers see no read outside the partition's arrays"""
    parts = corpus_partitions(W.corpus(77, per_combination=4, conforming=False))
    host = host_frames(range_main, [(p, o) for p, o, _ in parts], tmp_path, "arbitrary")
    left = 0
    for (part, _, name), from_host in zip(parts, host):
        assert from_host == X.closed_frames(part), name
        try:
            X.walk_frames(part)
        except X.WalkLeftPartition:
            left += 1
    assert left > 0   # what the contract's "no parity" is about


def test_null_errors_of_the_helper():
    types, frame = [W.BIGINT, W.BIGINT, W.BIGINT, W.BIGINT, W.BIGINT], X.RangeFrame(X.PRECEDING, X.FOLLOWING, 1, 2, 3, 4)
    good = [(5, 4, 6, 5, 5), (None, None, None, None, None)]   # a bound in a null-key row is never read
    fn = [X.Fn(X.AGGREGATE, (), frame, 1)]
    assert X.expected_output(types, [good], [0], fn, [], [0], [1]) == [(5, 1), (None, 1)]
    for row, message in (((5, None, 6, 5, 5), "Window frame starting offset must not be null"), ((5, 4, None, 5, 5), "Window frame ending offset must not be null"),
                         ((5, 4, 6, None, 5), "Window frame comparison key must not be null where the sort key is not null"),
                         ((5, None, None, None, None), "Window frame starting offset must not be null")):
        with pytest.raises(InvalidArgument, match=message):
            X.expected_output(types, [good + [row]], [0], fn, [], [0], [1])


# ---- header, library, binding, package -----------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_ranged_entry_point(pkg):
    name = "tgpu_window_factory_create_ranged"
    assert name in set(header_symbols())
    assert hasattr(pkg._lib.lib(), name)
    assert name in pkg._lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "tgpu.h")).read()
    assert re.search(r"typedef struct tgpu_window_range_frame_spec \{\s*int32_t type, start_type, start_channel, end_type, end_channel;\s*"
                     r"int32_t start_sort_key_channel, end_sort_key_channel;", header)
    assert "NOT monotone in the sort key gives an unspecified frame inside the" in header
    assert C.sizeof(pkg._lib.WindowRangeFrameSpec) == 28 and C.sizeof(pkg._lib.WindowFrameSpec) == 20
    frame = pkg.WindowRangeFrame(pkg.BOUND_PRECEDING, pkg.BOUND_FOLLOWING, 3, 4, 5, 6)
    s = frame.range_spec()
    assert (s.type, s.start_type, s.start_channel, s.end_type, s.end_channel, s.start_sort_key_channel, s.end_sort_key_channel) == (0, 1, 3, 3, 4, 5, 6)
    d = pkg.WindowRangeFrame(pkg.BOUND_UNBOUNDED_PRECEDING, pkg.BOUND_CURRENT_ROW).range_spec()
    assert (d.start_channel, d.end_channel, d.start_sort_key_channel, d.end_sort_key_channel) == (-1, -1, -1, -1)
    # the other frames beside a ranged one keep their five ints
    rows = pkg.WindowFunction(pkg.WINDOW_FIRST_VALUE, (0,), pkg.WindowFrame(pkg.FRAME_TYPE_ROWS, pkg.BOUND_PRECEDING, pkg.BOUND_FOLLOWING, 3, 4)).range_frame_spec()
    assert (rows.type, rows.start_type, rows.start_channel, rows.end_type, rows.end_channel, rows.start_sort_key_channel, rows.end_sort_key_channel) == (1, 1, 3, 3, 4, -1, -1)
    old = pkg.WindowFunction(pkg.WINDOW_RANK, (), pkg.FRAME_ROWS_TO_CURRENT).range_frame_spec()
    assert (old.type, old.start_type, old.end_type) == (1, 0, 2)
    # a plain WindowFrame with a RANGE offset is not a WindowRangeFrame: it keeps going to the framed entry point
    assert not isinstance(pkg.WindowFrame(pkg.FRAME_TYPE_RANGE, pkg.BOUND_PRECEDING, pkg.BOUND_CURRENT_ROW, 1), pkg.WindowRangeFrame)


def test_bound_helper_projects_what_a_planner_would(pkg):
    key, off = pkg.field(1, pkg.BIGINT), pkg.field(2, pkg.BIGINT)

    def repr_tree(e):
        if isinstance(e, pkg.expressions.CallExpression):
            return [e.name] + [repr_tree(a) for a in e.arguments]
        if isinstance(e, pkg.expressions.ConstantExpression):
            return ["const", e.value]
        return ["field", e.field]
    for order, bound, name in ((pkg.ASC_NULLS_LAST, pkg.BOUND_PRECEDING, "SUBTRACT"), (pkg.ASC_NULLS_FIRST, pkg.BOUND_FOLLOWING, "ADD"),
                               (pkg.DESC_NULLS_LAST, pkg.BOUND_PRECEDING, "ADD"), (pkg.DESC_NULLS_FIRST, pkg.BOUND_FOLLOWING, "SUBTRACT")):
        assert repr_tree(pkg.window_range_bound(key, off, bound, order)) == [name, ["field", 1], ["field", 2]]
    date = pkg.field(0, pkg.DATE)
    assert repr_tree(pkg.window_range_bound(date, 1, pkg.BOUND_PRECEDING, pkg.ASC_NULLS_LAST, unit="month")) == ["DATE_ADD", ["const", "month"], ["const", -1], ["field", 0]]
    assert repr_tree(pkg.window_range_bound(date, off, pkg.BOUND_PRECEDING, pkg.DESC_NULLS_LAST, unit="day")) == ["DATE_ADD", ["const", "day"], ["field", 2], ["field", 0]]
    assert repr_tree(pkg.window_range_bound(date, off, pkg.BOUND_FOLLOWING, pkg.DESC_NULLS_LAST, unit="day")) == ["DATE_ADD", ["const", "day"], ["NEGATE", ["field", 2]], ["field", 0]]
    with pytest.raises(ValueError):
        pkg.window_range_bound(key, off, pkg.BOUND_CURRENT_ROW, pkg.ASC_NULLS_LAST)


def test_java_sources_declare_the_native_and_the_two_methods():
    strip = lambda t: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    native = strip(open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuNative.java")).read())
    m = re.search(r"public static native long createRangeWindowFactory\((.*?)\);", native, flags=re.S)
    assert m and [p.strip().rsplit(" ", 1)[0] for p in m.group(1).split(",")] == ["long", "int", "int[]", "int[]", "int[]", "int[]", "int[]", "int[]", "int[]", "int"]
    glue = strip(open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuOperatorFactories.java")).read())
    assert re.search(r"public static int\[\] windowRangeFrame\(FrameInfo frame\)", glue)
    assert "frame.getSortKeyChannelForStartComparison(), frame.getSortKeyChannelForEndComparison()" in glue
    assert re.search(r"public Optional<OperatorFactory> rangeWindow\(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels, "
                     r"List<int\[\]> functions,\s*List<FrameInfo> frames,", glue)
    assert "info.getSortKeyChannel() != sortChannels.get(0)" in glue and "info.getOrdering()" in glue
    assert "GpuNative.createRangeWindowFactory(context, operatorId, codes," in glue
    shim = open(os.path.join(ROOT, "jni", "tgpu_jni.c")).read()
    assert "JFN(jlong, createRangeWindowFactory)" in shim and "tgpu_window_factory_create_ranged(" in shim
    assert "createRangeWindowFactory" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- the JNI shim ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


def fn(function, agg=0, frame=1, args=(), ignore_nulls=0):
    return (function, agg, frame, len(args)) + tuple(args) + (0,) * (3 - len(args)) + (ignore_nulls,)


def fr(kind=0, start=1, end=3, start_channel=0, end_channel=0, start_key=0, end_key=0):
    return (kind, start, start_channel, end, end_channel, start_key, end_key)


T = (1, 4, 6, 2, 3)   # BIGINT, DOUBLE, VARCHAR, INTEGER, DATE
# (types, output channels, functions flattened, frames flattened, partition channels, sort channels, sort orders, expectedPositions, code, message)
BAD = [
    ((), (), fn(0), fr(), (), (), (), 10, -1, "empty type array"),
    ((1, 7), (0,), fn(0), fr(), (), (), (), 10, -1, "unknown type"),
    (T, (5,), fn(0), fr(), (), (0,), (1,), 10, -1, "output channel out of range"),
    (T, (0,), fn(0), fr(), (0,), (1, 0), (1,), 10, -1, "sort channels and sort orders differ in length"),
    (T, (0,), fn(0), fr(), (0,) * 5, (1,) * 4, (1,) * 4, 10, -1, "more than 8 partition and sort channels"),
    (T, (0,), fn(0), fr(), (5,), (0,), (1,), 10, -1, "partition channel out of range"),
    (T, (0,), fn(0), fr(), (0,), (-1,), (1,), 10, -1, "sort channel out of range"),
    (T, (0,), fn(0), fr(), (0,), (1,), (4,), 10, -1, "sort order out of range"),
    (T, (0,), fn(0)[:7], fr(), (0,), (1,), (1,), 10, -1, "malformed function array"),
    (T, (0,), (), (), (0,), (1,), (1,), 10, -1, "no window function"),
    (T, (0,), fn(0) * 17, fr() * 17, (0,), (1,), (1,), 10, -1, "more than 16 window functions"),
    (T, (0,), fn(0), fr()[:5], (0,), (1,), (1,), 10, -1, "malformed frame array"),            # the framed native's five ints
    (T, (0,), fn(0), fr() * 2, (0,), (1,), (1,), 10, -1, "frame array and function array differ in length"),
    (T, (0,), fn(12), fr(), (0,), (1,), (1,), 10, -1, "unknown window function"),
    (T, (0,), fn(0), fr(kind=3), (0,), (1,), (1,), 10, -1, "unknown window frame type"),
    (T, (0,), fn(0), fr(start=5), (0,), (1,), (1,), 10, -1, "unknown window frame bound"),
    (T, (0,), fn(0), fr(end=9), (0,), (1,), (1,), 10, -1, "unknown window frame bound"),
    (T, (0,), fn(0), fr(start=3, end=1), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),
    (T, (0,), fn(0), fr(start=2, end=1), (0,), (1,), (1,), 10, -1, "invalid window frame bounds"),
    (T, (0,), fn(0), fr(), (0,), (), (), 10, -1, "a RANGE frame with an offset needs exactly one sort channel"),
    (T, (0,), fn(0), fr(), (), (0, 1), (1, 1), 10, -1, "a RANGE frame with an offset needs exactly one sort channel"),
    (T, (0,), fn(0), fr(start_channel=5), (0,), (0,), (1,), 10, -1, "frame bound channel out of range"),
    (T, (0,), fn(0), fr(end_channel=-1), (0,), (0,), (1,), 10, -1, "frame bound channel out of range"),
    (T, (0,), fn(0), fr(start_key=-1), (0,), (0,), (1,), 10, -1, "frame comparison key channel out of range"),
    (T, (0,), fn(0), fr(start=0, end_key=5), (0,), (0,), (1,), 10, -1, "frame comparison key channel out of range"),
    (T, (0,), fn(0), fr(start_channel=1), (0,), (0,), (1,), 10, -1, "a frame bound and its comparison key differ in type"),
    (T, (0,), fn(0), fr(end_channel=3, end_key=4), (0,), (0,), (1,), 10, -1, "a frame bound and its comparison key differ in type"),   # INTEGER against DATE
    (T, (0,), fn(0), fr(start_channel=2, start_key=2), (0,), (0,), (1,), 10, -1, "a RANGE frame bound must be BIGINT, INTEGER, DATE or DOUBLE"),
    # the other frames are checked as the framed native checks them
    (T, (0,), fn(0), fr(kind=1, start_channel=1), (0,), (0,), (1,), 10, -1, "a frame offset must be BIGINT or INTEGER"),
    (T, (0,), fn(0), fr(kind=2, end_channel=7), (0,), (0,), (1,), 10, -1, "frame offset channel out of range"),
    (T, (0,), fn(9, agg=4, args=(1,)), fr(), (0,), (0,), (1,), 10, -8, "sum(double) and avg are not supported as window aggregates"),
    (T, (0,), fn(8, args=(2,), ignore_nulls=1), fr(), (0,), (0,), (1,), 10, -8, "IGNORE NULLS is not supported"),
    (T, (0,), fn(0), fr(), (0,), (0,), (1,), 0, -1, "expected positions must be positive"),
]


def call(jvm, name, types, outputs, functions, frames, partitions, sorts, orders, expected_positions):
    return jvm.call(name, C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), ints(jvm, *outputs), ints(jvm, *functions), ints(jvm, *frames),
                    ints(jvm, *partitions), ints(jvm, *sorts), ints(jvm, *orders), C.c_int32(expected_positions))


@pytest.mark.parametrize("types, outputs, functions, frames, partitions, sorts, orders, expected_positions, code, why", BAD)
def test_arguments_are_checked_in_front_of_the_library(jvm, types, outputs, functions, frames, partitions, sorts, orders, expected_positions, code, why):
    assert call(jvm, "createRangeWindowFactory", types, outputs, functions, frames, partitions, sorts, orders, expected_positions) == 0
    assert jvm.pending_code() == code and jvm.pending_message() == "window: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


def test_the_ranged_native_accepts_what_the_framed_one_refuses(jvm):
    """RANGE offsets pass the ranged shim's checks and reach the library, which refuses the null context handle (not one of the shim's own "window: .."
    messages); the framed native keeps refusing them"""
    old = call(jvm, "createFramedWindowFactory", T, (0,), fn(0), (0, 1, 0, 2, -1), (), (0,), (1,), 10)
    assert old == 0 and jvm.pending_code() == -8 and jvm.pending_message() == "window: RANGE frames with an offset are not supported"
    jvm.clear()
    for functions, frames in ((fn(9, agg=3, args=(0,)), fr()), (fn(8, args=(2,)), fr(start=0, end=1, end_channel=1, end_key=1)),
                              (fn(10, args=(2, 0)), fr(start=3, end=4, start_channel=4, start_key=4)), (fn(11, args=(0,)), fr(kind=1, start=0, end=2, start_channel=-1)),
                              (fn(0), fr(start=2, end=2, start_channel=-1, end_channel=-1, start_key=-1, end_key=-1))):
        assert call(jvm, "createRangeWindowFactory", T, (0,), functions, frames, (), (0,), (1,), 10) == 0   # the null context
        assert jvm.pending_code() != 0 and not (jvm.pending_message() or "").startswith("window: ")
        jvm.clear()
        assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0

"""RowNumberOperator / LimitOperator without a GPU: the expected-value helper (tests/row_number_expected.py) reproduces the facts the reference
asserts for its four row-number cases and its two limit cases (tests/golden/row_number_vectors.json), so the yardstick of the GPU tests is itself
checked; tgpu.h declares the two factories, libtgpu.so exports them, _lib.py binds them and the package exports the Python factories; the JNI
shim rejects bad channels, limits and sizes with a pending NativeError before the library is called (a call with the null context handle would
reach it otherwise)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from jni_harness import FakeJvm, build_fake_jni, header_symbols
from row_number_expected import expected_limit, expected_row_numbers

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "row_number_vectors.json")))
NEW_SYMBOLS = ["tgpu_row_number_factory_create", "tgpu_limit_factory_create"]
ROW_NUMBER_CASES = [c for c in GOLD["cases"] if c["operator"] == "row_number"]
LIMIT_CASES = [c for c in GOLD["cases"] if c["operator"] == "limit"]


@pytest.mark.parametrize("case", ROW_NUMBER_CASES, ids=lambda c: c["name"])
def test_helper_reproduces_row_number_case(oracle, case):
    keys = [[oracle.Col(1, np.array([r[ch] for r in page], dtype=np.int64)) for ch in case["partition_channels"]] for page in case["pages"]]
    got = expected_row_numbers(oracle, [1] * len(case["partition_channels"]), keys, [len(p) for p in case["pages"]], case["max_rows_per_partition"])
    numbers = [v for page in got if page is not None for v in page[1]]
    rows = [tuple(page[i][ch] for ch in case["output_channels"]) for page, out in zip(case["pages"], got) if out is not None for i in out[0]]
    assert len(numbers) == case["row_number_count"] == len(rows)
    if case["max_row_number"] is not None:
        assert max(numbers) <= case["max_row_number"]
    for s in case["row_sets"]:
        want = {tuple(r) for r in s["rows"]}
        assert len(want & set(rows)) == s["intersection"]
        if s.get("exact"):
            assert sorted(rows) == sorted(want)


def test_helper_numbers_in_row_order_and_saturates(oracle):
    """the two loops on one stream: numbers continue across pages; with max = 2 a group's first two rows are kept and a full page is no page"""
    pages = [[5, 7, 5, 5, 7], [5, 5], [9, 7, 9, 9]]
    keys = [[oracle.Col(1, np.array(p, dtype=np.int64))] for p in pages]
    sizes = [len(p) for p in pages]
    assert expected_row_numbers(oracle, [1], keys, sizes) == [([0, 1, 2, 3, 4], [1, 1, 2, 3, 2]), ([0, 1], [4, 5]), ([0, 1, 2, 3], [1, 3, 2, 3])]
    assert expected_row_numbers(oracle, [1], keys, sizes, 2) == [([0, 1, 2, 4], [1, 1, 2, 2]), None, ([0, 2], [1, 2])]
    assert expected_row_numbers(oracle, [1], keys, sizes, 0) == [None, None, None]
    assert expected_row_numbers(oracle, [], [[], [], []], sizes) == [([0, 1, 2, 3, 4], [1, 2, 3, 4, 5]), ([0, 1], [6, 7]), ([0, 1, 2, 3], [8, 9, 10, 11])]
    assert expected_row_numbers(oracle, [], [[], [], []], sizes, 6) == [([0, 1, 2, 3, 4], [1, 2, 3, 4, 5]), ([0], [6])]   # then finished: page 2 is not taken
    assert expected_row_numbers(oracle, [], [[], [], []], sizes, 0) == []


def test_helper_uses_the_multi_channel_hash_for_other_keys(oracle):
    """(INTEGER, VARCHAR) keys with nulls: a null key is a partition like any other"""
    a = oracle.Col(2, np.array([1, 1, 2, 1, 0], dtype=np.int32), np.array([0, 0, 0, 0, 1], dtype=np.uint8))
    b = oracle.Col(6, ["x", "x", "x", None, None])
    a2 = oracle.Col(2, np.array([0, 2, 1], dtype=np.int32), np.array([1, 0, 0], dtype=np.uint8))
    b2 = oracle.Col(6, [None, "x", "x"])
    assert expected_row_numbers(oracle, [2, 6], [[a, b], [a2, b2]], [5, 3]) == [([0, 1, 2, 3, 4], [1, 2, 1, 1, 1]), ([0, 1, 2], [2, 2, 3])]


@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: c["name"])
def test_helper_reproduces_limit_case(case):
    takes = expected_limit([len(p) for p in case["pages"]], case["limit"])
    assert [p[:k] for p, k in zip(case["pages"], takes)] == case["expected_pages"]


def test_limit_arithmetic():
    assert expected_limit([3, 2, 2], 0) == []
    assert expected_limit([3, 2, 2], 100) == [3, 2, 2]
    assert expected_limit([3, 0, 2], 4) == [3, 0, 1]


def test_header_library_and_binding_have_the_row_number_and_limit_operators(pkg):
    declared = set(header_symbols())
    L = pkg._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in pkg._lib.SYMBOLS, name
    for name in ("RowNumberOperatorFactory", "LimitOperatorFactory"):
        assert hasattr(pkg, name), name


@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


# (types, output channels, partition channels, maxRowsPerPartition, hashChannel, expectedPositions, message)
BAD_ROW_NUMBER = [
    ((1, 4), (0, -1), (0,), -1, -1, 10, "output channel out of range"),
    ((1, 4), (2,), (0,), -1, -1, 10, "output channel out of range"),
    ((1, 4), (0,), (-1,), -1, -1, 10, "partition channel out of range"),
    ((1, 4), (0,), (0, 2), -1, -1, 10, "partition channel out of range"),
    ((1, 1), (0,), (), -1, 1, 10, "hash channel without partition channels"),
    ((1, 1), (0,), (0,), -1, 2, 10, "hash channel out of range"),
    ((1, 4), (0,), (0,), -1, 1, 10, "hash channel is not BIGINT"),
    ((1, 4), (0,), (0,), -2, -1, 10, "negative max rows per partition"),
    ((1, 4), (0,), (0,), 3, -1, 0, "expected positions must be positive"),
    ((1, 4), (0,), (0,), 3, -1, -5, "expected positions must be positive"),
    ((), (), (), -1, -1, 10, "empty type array"),
]


@pytest.mark.parametrize("types, outputs, partitions, max_rows, hash_channel, expected_positions, why", BAD_ROW_NUMBER)
def test_row_number_arguments_are_checked_in_front_of_the_library(jvm, types, outputs, partitions, max_rows, hash_channel, expected_positions, why):
    r = jvm.call("createRowNumberFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), ints(jvm, *outputs), ints(jvm, *partitions),
                 C.c_int64(max_rows), C.c_int32(hash_channel), C.c_int32(expected_positions))
    assert r == 0
    assert jvm.pending_code() == -1 and jvm.pending_message() == "row number: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


@pytest.mark.parametrize("types, limit, why", [((1,), -1, "negative limit"), ((), 5, "empty type array")])
def test_limit_arguments_are_checked_in_front_of_the_library(jvm, types, limit, why):
    r = jvm.call("createLimitFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), C.c_int64(limit))
    assert r == 0
    assert jvm.pending_code() == -1 and jvm.pending_message() == "limit: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0

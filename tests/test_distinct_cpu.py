"""MarkDistinctOperator / DistinctLimitOperator without a GPU: the expected-value helper (tests/distinct_expected.py) reproduces the reference's
four data cases (tests/golden/distinct_vectors.json), so the yardstick of the GPU tests is itself checked; tgpu.h declares the two factories,
libtgpu.so exports them, _lib.py binds them and the package exports the Python factories; the JNI shim rejects bad channels and limits with a
pending NativeError before the library is called (a call with the null context handle would reach it otherwise)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from distinct_expected import expected_distinct_limit, expected_marks
from jni_harness import FakeJvm, build_fake_jni, header_symbols

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "distinct_vectors.json")))
NEW_SYMBOLS = ["tgpu_mark_distinct_factory_create", "tgpu_distinct_limit_factory_create"]


def case(name):
    return next(c for c in GOLD["cases"] if c["name"] == name)


def key_pages(oracle, c):
    return [[oracle.Col(1, np.array(p, dtype=np.int64))] for p in c["pages"]]


def test_helper_reproduces_mark_distinct(oracle):
    c = case("testMarkDistinct")
    marks = expected_marks(oracle, [1], key_pages(oracle, c))
    rows = [[v, bool(m)] for page, pm in zip(c["pages"], marks) for v, m in zip(page, pm)]
    assert rows == c["expected"]


@pytest.mark.parametrize("name", ["testDistinctLimit", "testDistinctLimitWithPageAlignment", "testDistinctLimitValuesLessThanLimit"])
def test_helper_reproduces_distinct_limit(oracle, name):
    c = case(name)
    kept = expected_distinct_limit(oracle, [1], key_pages(oracle, c), c["limit"])
    rows = [[page[i]] for page, positions in zip(c["pages"], kept) for i in positions]
    assert rows == c["expected"]


def test_helper_uses_the_multi_channel_hash_for_other_keys(oracle):
    """(INTEGER, VARCHAR) keys with nulls: a null key is a group like any other"""
    a = oracle.Col(2, np.array([1, 1, 2, 1, 0], dtype=np.int32), np.array([0, 0, 0, 0, 1], dtype=np.uint8))
    b = oracle.Col(6, ["x", "x", "x", None, None])
    a2 = oracle.Col(2, np.array([0, 2, 3], dtype=np.int32), np.array([1, 0, 0], dtype=np.uint8))
    b2 = oracle.Col(6, [None, "x", "y"])
    marks = expected_marks(oracle, [2, 6], [[a, b], [a2, b2]])
    assert [m.tolist() for m in marks] == [[True, False, True, True, True], [False, False, True]]
    assert expected_distinct_limit(oracle, [2, 6], [[a, b], [a2, b2]], 3) == [[0, 2, 3]]
    assert expected_distinct_limit(oracle, [2, 6], [[a, b], [a2, b2]], 5) == [[0, 2, 3, 4], [2]]
    assert expected_distinct_limit(oracle, [2, 6], [[a, b], [a2, b2]], 0) == []


def test_header_library_and_binding_have_the_distinct_operators(pkg):
    declared = set(header_symbols())
    L = pkg._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in pkg._lib.SYMBOLS, name
    for name in ("MarkDistinctOperatorFactory", "DistinctLimitOperatorFactory"):
        assert hasattr(pkg, name), name


def test_factories_fail_loudly_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.TgpuError):
        pkg.MarkDistinctOperatorFactory(pkg.Context(0), 1, [pkg.BIGINT], [0])


@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


BAD_CHANNELS = [
    ((1,), (), -1, "empty channel list"),
    ((), (0,), -1, "empty type array"),
    ((1,), (1,), -1, "channel out of range"),
    ((1, 1), (0, -1), -1, "channel out of range"),
    ((1, 1), (0,), 2, "hash channel out of range"),
    ((1, 1), (0,), -2, "hash channel out of range"),
    ((1, 2), (0,), 1, "hash channel is not BIGINT"),
]


@pytest.mark.parametrize("types, channels, hash_channel, why", BAD_CHANNELS)
def test_mark_distinct_channels_are_checked_in_front_of_the_library(jvm, types, channels, hash_channel, why):
    r = jvm.call("createMarkDistinctFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), ints(jvm, *channels), C.c_int32(hash_channel))
    assert r == 0
    assert jvm.pending_code() == -1 and jvm.pending_message() == "mark distinct: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


@pytest.mark.parametrize("types, channels, hash_channel, why", BAD_CHANNELS)
def test_distinct_limit_channels_are_checked_in_front_of_the_library(jvm, types, channels, hash_channel, why):
    r = jvm.call("createDistinctLimitFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, *types), ints(jvm, *channels), C.c_int64(5),
                 C.c_int32(hash_channel))
    assert r == 0
    assert jvm.pending_code() == -1 and jvm.pending_message() == "distinct limit: " + why
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


def test_distinct_limit_negative_limit_is_checked_in_front_of_the_library(jvm):
    r = jvm.call("createDistinctLimitFactory", C.c_int64, C.c_int64(0), C.c_int32(1), ints(jvm, 1), ints(jvm, 0), C.c_int64(-1), C.c_int32(-1))
    assert r == 0
    assert jvm.pending_code() == -1 and jvm.pending_message() == "distinct limit: negative limit"
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0

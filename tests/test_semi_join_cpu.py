"""The semi join's C ABI without a GPU: tgpu.h declares the set builder / semi join entry points, libtgpu.so exports them, _lib.py binds them
and the package exports the factories; the JNI shim rejects bad channels with a pending NativeError before the library is called (a call with
the null context handle would reach it otherwise), without leaking pins or local frames."""
import ctypes as C

import numpy as np
import pytest

from jni_harness import FakeJvm, build_fake_jni, header_symbols

NEW_SYMBOLS = ["tgpu_set_builder_factory_create", "tgpu_hash_semi_join_factory_create", "tgpu_set_supplier_stats", "tgpu_set_supplier_destroy"]


def test_header_library_and_binding_have_the_semi_join(pkg):
    declared = set(header_symbols())
    L = pkg._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in pkg._lib.SYMBOLS, name
    for name in ("SetBuilderOperatorFactory", "HashSemiJoinOperatorFactory", "SetSupplier"):
        assert hasattr(pkg, name), name
    assert (pkg.SET_BITMAP, pkg.SET_HASH, pkg.SET_GENERIC) == (0, 1, 2)


def test_factories_fail_loudly_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.TgpuError):
        pkg.SetBuilderOperatorFactory(pkg.Context(0), 1, [pkg.BIGINT], 0)


@pytest.fixture(scope="module")
def jvm():
    return FakeJvm(build_fake_jni())


def ints(jvm, *v):
    return jvm.array(np.array(v, dtype=np.int32))


@pytest.mark.parametrize("types, set_channel, hash_channel", [((1,), -1, -1), ((1,), 1, -1), ((1, 1), 0, 2), ((1, 1), 0, -2), ((), 0, -1)])
def test_set_builder_channels_are_checked_in_front_of_the_library(jvm, types, set_channel, hash_channel):
    arr = ints(jvm, *types) if types else jvm.array(np.zeros(0, dtype=np.int32))
    r = jvm.call("createSetBuilderFactory", C.c_void_p, C.c_int64(0), C.c_int32(1), arr, C.c_int32(set_channel), C.c_int32(hash_channel), C.c_int32(10))
    assert r is None
    assert jvm.pending_code() == -1 and "set builder" in jvm.pending_message()
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


@pytest.mark.parametrize("types, join_channel, hash_channel", [((1,), -1, -1), ((1, 1), 2, -1), ((1, 1), 0, 2), ((1,), 0, -3), ((), 0, -1)])
def test_semi_join_channels_are_checked_in_front_of_the_library(jvm, types, join_channel, hash_channel):
    arr = ints(jvm, *types) if types else jvm.array(np.zeros(0, dtype=np.int32))
    r = jvm.call("createHashSemiJoinFactory", C.c_int64, C.c_int64(0), C.c_int32(2), C.c_int64(0), arr, C.c_int32(join_channel), C.c_int32(hash_channel))
    assert r == 0
    assert jvm.pending_code() == -1 and "semi join" in jvm.pending_message()
    jvm.clear()
    assert jvm.outstanding_pins() == 0 and jvm.open_frames() == 0 and jvm.calls_while_pinned() == 0


def test_stats_of_a_null_supplier_is_an_error_not_a_crash(jvm):
    out = jvm.array(np.zeros(4, dtype=np.int64))
    jvm.call("setSupplierStats", None, C.c_int64(0), out)
    assert jvm.pending_code() == -1
    jvm.clear()
    jvm.call("destroySetSupplier", None, C.c_int64(0))   # a null handle is ignored
    assert jvm.pending_code() == 0

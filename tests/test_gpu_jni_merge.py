"""A MergeOperator over two sorted streams, driven through the JNI shim on the GPU against the fake JVM, as a JVM host would: createContext ->
createMergeFactory -> createOperator -> mergeAddPageSource (one GpuPageSource per stream: nextPage / isFinished / isBlocked / loadBlock / close
are upcalls, every channel loaded at once) -> mergeNoMoreSplits -> getOutput -> blockInfo / copyBlocks, against the model of
tests/merge_expected.py; afterwards every source closed once, no global reference, no array left pinned and no local frame open."""
import ctypes as C

import numpy as np
import pytest

import merge_expected as M
from test_gpu_jni_shim import I32, I64, clean, drain, heap_blocks, ints, jctx, jvm  # noqa: F401  (jvm and jctx are fixtures)

pytestmark = pytest.mark.gpu


def test_a_two_stream_merge_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    B, D = pkg.BIGINT, pkg.DOUBLE
    rng = np.random.default_rng(21)
    # stream s: three pages of a sorted key with duplicates across the streams, and a payload that names (stream, row)
    streams = []
    for s in range(2):
        keys = np.sort(rng.integers(0, 400, 2500)).astype(np.int64)
        payload = (s * 10_000 + np.arange(2500)).astype(np.float64)
        streams.append([(keys[a:b], payload[a:b]) for a, b in ((0, 1000), (1000, 1001), (1001, 2500))])
    states = []

    def adapter(pages):
        state = {"i": -1, "closed": 0, "keep": [], "loaded": 0}

        def next_page():
            if state["i"] + 1 >= len(pages):
                return -1
            state["i"] += 1
            return len(pages[state["i"]][0])

        def load_block(ch):
            state["loaded"] += 1
            parts = jvm.object_array([jvm.array(np.array([0, 0, 0], dtype=np.int32)), jvm.array(pages[state["i"]][ch]), None, None, None, None, None, None])
            state["keep"].append(parts)
            return parts.value

        def close():
            state["closed"] += 1

        states.append(state)
        return jvm.adapter(next_page, lambda: state["i"] + 1 >= len(pages), lambda: 0, load_block, close)

    fac = I64(jvm.checked("createMergeFactory", I64, jctx, I32(9), ints(jvm, B, D), ints(jvm, 1, 0), ints(jvm, 0), ints(jvm, pkg.ASC_NULLS_FIRST)))
    op = I64(jvm.checked("createOperator", I64, fac))
    assert not jvm.checked("needsInput", C.c_uint8, op) and jvm.checked("isBlocked", C.c_uint8, op)   # blockedOnSplits
    for pages in streams:
        jvm.checked("mergeAddPageSource", None, op, adapter(pages), ints(jvm, B, D))
    jvm.checked("mergeNoMoreSplits", None, op)
    with pytest.raises(RuntimeError, match="noMoreSplits has been called already"):
        jvm.checked("mergeAddPageSource", None, op, adapter(streams[0]), ints(jvm, B, D))
    states.pop()
    outs = drain(jvm, op)
    got_p = np.concatenate([heap_blocks(jvm, p)[0][0] for p in outs])
    got_k = np.concatenate([heap_blocks(jvm, p)[1][0] for p in outs])
    want_k, want_p = M.merge_ascending_bigint([np.concatenate([k for k, _ in s]) for s in streams], [np.concatenate([p for _, p in s]).astype(np.int64) for s in streams])
    assert np.array_equal(got_k, want_k) and np.array_equal(got_p.astype(np.int64), want_p)
    assert [st["loaded"] for st in states] == [6, 6] and [st["closed"] for st in states] == [1, 1]
    for p in outs:
        jvm.call("releasePage", None, I64(p))
    jvm.call("close", None, op)
    assert [st["closed"] for st in states] == [1, 1] and jvm.global_refs() == 0
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    clean(jvm)

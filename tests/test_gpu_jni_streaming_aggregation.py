"""The reference's TestStreamingAggregationOperator.test driven through the JNI shim on the GPU against the fake JVM, as a JVM host would:
createContext -> createStreamingAggregationFactory -> createOperator -> addInput (heap arrays) / getOutput page by page -> finish -> getOutput ->
blockInfo / copyBlocks; afterwards no global reference, no array left pinned and no local frame open."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import key_cases as K
import streaming_aggregation_expected as S
from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, heap_blocks, ints, jctx, jvm  # noqa: F401  (jvm and jctx are fixtures)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_aggregation_vectors.json")


def test_the_reference_test_case_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    case = [c for c in json.load(open(GOLDEN))["cases"] if c["name"] == "test"][0]
    types, pages = S.golden_pages(case)
    aggs = S.golden_aggs(case)
    flat_aggs = [x for f, ch in aggs for x in (f, ch, -1)]
    fac = I64(jvm.checked("createStreamingAggregationFactory", I64, jctx, I32(5), ints(jvm, *types), ints(jvm, *case["group_by_channels"]), I32(pkg.SINGLE), ints(jvm, *flat_aggs)))
    op = I64(jvm.checked("createOperator", I64, fac))
    wb = jvm.empty(1, np.uint8)
    outs = []
    for page in pages:
        assert jvm.checked("needsInput", C.c_uint8, op)
        add_flat_page(jvm, op, types, [c.values for c in page], [c.nulls for c in page])
        h = jvm.checked("getOutput", I64, op, wb)
        if h:
            outs.append(h)
    jvm.checked("finish", None, op)
    outs += drain(jvm, op)
    assert jvm.checked("isFinished", C.c_uint8, op) and not jvm.checked("needsInput", C.c_uint8, op)
    blocks = [heap_blocks(jvm, p) for p in outs]
    key_bits = np.concatenate([b[0][0].view(np.uint64) for b in blocks]).tolist()
    key_nulls = np.concatenate([b[0][1] for b in blocks]).tolist()
    counts = np.concatenate([b[1][0] for b in blocks]).tolist()
    sums = np.concatenate([b[2][0] for b in blocks]).tolist()
    expected = S.golden_expected(case)
    got_keys = [None if nl else ("NaN" if K.is_nan_bits(v) else K.bits_to_doubles([v])[0].item()) for v, nl in zip(key_bits, key_nulls)]
    assert got_keys == [r[0] for r in expected] and counts == [r[1] for r in expected] and sums == [r[2] for r in expected]
    # malformed aggregate triples are refused by the shim itself
    with pytest.raises(RuntimeError, match="malformed aggregate array"):
        jvm.checked("createStreamingAggregationFactory", I64, jctx, I32(5), ints(jvm, *types), ints(jvm, 1), I32(pkg.SINGLE), ints(jvm, 1, -1))
    jvm.clear()
    for p in outs:
        jvm.call("releasePage", None, I64(p))
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    assert jvm.global_refs() == 0
    clean(jvm)

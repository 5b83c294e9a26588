"""A framed WindowOperator driven through the JNI shim on the GPU against the fake JVM, as a JVM host would: createContext ->
createFramedWindowFactory -> createOperator -> addInput(heap arrays) -> finish -> getOutput -> blockInfo / copyBlocks.  sum and min under ROWS BETWEEN 1
PRECEDING AND 2 FOLLOWING, nth_value and ntile, against tests/window_frames_expected.py; afterwards no array left pinned and no local frame open."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, heap_blocks, ints, jctx, jvm  # noqa: F401  (jvm and jctx are fixtures)
from window_expected import AGGREGATE, MIN_BIGINT, SUM_BIGINT, Fn
from window_frames_expected import FOLLOWING, NTH_VALUE, NTILE, PRECEDING, ROWS, Frame, expected_output

pytestmark = pytest.mark.gpu


def test_a_framed_window_operator_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    B = pkg.BIGINT
    rng = np.random.default_rng(12)
    n = 3000
    cols = [rng.integers(0, 5, n).astype(np.int64), rng.permutation(n).astype(np.int64), rng.integers(-100, 100, n).astype(np.int64), np.full(n, 1, dtype=np.int64),
            np.full(n, 2, dtype=np.int64)]
    frame = (pkg.FRAME_TYPE_ROWS, pkg.BOUND_PRECEDING, 3, pkg.BOUND_FOLLOWING, 4)
    whole = (pkg.FRAME_TYPE_ROWS, pkg.BOUND_UNBOUNDED_PRECEDING, -1, pkg.BOUND_UNBOUNDED_FOLLOWING, -1)
    functions = (pkg.WINDOW_AGGREGATE, pkg.SUM_BIGINT, 0, 1, 2, 0, 0, 0) + (pkg.WINDOW_AGGREGATE, pkg.MIN_BIGINT, 0, 1, 2, 0, 0, 0) + (pkg.WINDOW_NTH_VALUE, 0, 0, 2, 2, 4, 0, 0) + \
        (pkg.WINDOW_NTILE, 0, 0, 1, 4, 0, 0, 0)
    fac = I64(jvm.checked("createFramedWindowFactory", I64, jctx, I32(7), ints(jvm, B, B, B, B, B), ints(jvm, 1, 0), ints(jvm, *functions), ints(jvm, *(frame + frame + frame + whole)),
                          ints(jvm, 0), ints(jvm, 1), ints(jvm, pkg.ASC_NULLS_LAST), I32(10)))
    op = I64(jvm.checked("createOperator", I64, fac))
    assert jvm.checked("needsInput", C.c_uint8, op)
    add_flat_page(jvm, op, [B] * 5, [c[:1000] for c in cols])
    add_flat_page(jvm, op, [B] * 5, [c[1000:] for c in cols])
    jvm.checked("finish", None, op)
    pages = drain(jvm, op)
    assert len(pages) == 1
    blocks = heap_blocks(jvm, pages[0])
    got = [tuple(None if nl[i] else int(v[i]) for v, nl in blocks) for i in range(n)]
    f = Frame(ROWS, PRECEDING, FOLLOWING, 3, 4)
    want = expected_output([1] * 5, [list(zip(*[c.tolist() for c in cols]))], [1, 0],
                           [Fn(AGGREGATE, (2,), f, SUM_BIGINT), Fn(AGGREGATE, (2,), f, MIN_BIGINT), Fn(NTH_VALUE, (2, 4), f), Fn(NTILE, (4,), 0)], [0], [1], [1])
    assert got == want
    jvm.call("releasePage", None, I64(pages[0]))
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    clean(jvm)

"""A WindowOperator with a RANGE frame whose bounds are values, driven through the JNI shim on the GPU against the fake JVM, as a JVM host would:
createContext -> createRangeWindowFactory -> createOperator -> addInput(heap arrays) -> finish -> getOutput -> blockInfo / copyBlocks.  sum, count and
last_value under RANGE BETWEEN 2 PRECEDING AND 3 FOLLOWING beside a ROWS frame, against the walk of tests/window_range_expected.py; afterwards no array
left pinned and no local frame open."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, heap_blocks, ints, jctx, jvm  # noqa: F401  (jvm and jctx are fixtures)
from window_expected import AGGREGATE, COUNT_ALL, LAST_VALUE, SUM_BIGINT, Fn
from window_frames_expected import FOLLOWING, PRECEDING, ROWS, Frame
from window_range_expected import RangeFrame, expected_output

pytestmark = pytest.mark.gpu


def test_a_ranged_window_operator_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    B = pkg.BIGINT
    rng = np.random.default_rng(13)
    n = 3000
    keys = rng.integers(0, 200, n).astype(np.int64)
    # channels: 0 partition, 1 sort key, 2 values, 3 / 4 the bounds key - 2 / key + 3, 5 the ROWS offset
    cols = [rng.integers(0, 5, n).astype(np.int64), keys, rng.integers(-100, 100, n).astype(np.int64), keys - 2, keys + 3, np.full(n, 1, dtype=np.int64)]
    ranged = (pkg.FRAME_TYPE_RANGE, pkg.BOUND_PRECEDING, 3, pkg.BOUND_FOLLOWING, 4, 1, 1)
    rows = (pkg.FRAME_TYPE_ROWS, pkg.BOUND_PRECEDING, 5, pkg.BOUND_FOLLOWING, 5, -1, -1)
    functions = (pkg.WINDOW_AGGREGATE, pkg.SUM_BIGINT, 0, 1, 2, 0, 0, 0) + (pkg.WINDOW_AGGREGATE, pkg.COUNT_ALL, 0, 0, 0, 0, 0, 0) + (pkg.WINDOW_LAST_VALUE, 0, 0, 1, 2, 0, 0, 0) + \
        (pkg.WINDOW_AGGREGATE, pkg.SUM_BIGINT, 0, 1, 2, 0, 0, 0)
    fac = I64(jvm.checked("createRangeWindowFactory", I64, jctx, I32(7), ints(jvm, B, B, B, B, B, B), ints(jvm, 1, 0), ints(jvm, *functions), ints(jvm, *(ranged + ranged + ranged + rows)),
                          ints(jvm, 0), ints(jvm, 1), ints(jvm, pkg.ASC_NULLS_LAST), I32(10)))
    op = I64(jvm.checked("createOperator", I64, fac))
    assert jvm.checked("needsInput", C.c_uint8, op)
    add_flat_page(jvm, op, [B] * 6, [c[:1000] for c in cols])
    add_flat_page(jvm, op, [B] * 6, [c[1000:] for c in cols])
    jvm.checked("finish", None, op)
    pages = drain(jvm, op)
    assert len(pages) == 1
    blocks = heap_blocks(jvm, pages[0])
    got = [tuple(None if nl[i] else int(v[i]) for v, nl in blocks) for i in range(n)]
    f, r = RangeFrame(PRECEDING, FOLLOWING, 3, 4, 1, 1), Frame(ROWS, PRECEDING, FOLLOWING, 5, 5)
    want = expected_output([1] * 6, [list(zip(*[c.tolist() for c in cols]))], [1, 0],
                           [Fn(AGGREGATE, (2,), f, SUM_BIGINT), Fn(AGGREGATE, (), f, COUNT_ALL), Fn(LAST_VALUE, (2,), f), Fn(AGGREGATE, (2,), r, SUM_BIGINT)], [0], [1], [1])
    assert got == want
    jvm.call("releasePage", None, I64(pages[0]))
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    clean(jvm)

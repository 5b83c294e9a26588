"""One filter / project program full of math functions driven through the JNI shim on the GPU against the fake JVM: createContext ->
createFilterProjectFactory (the node arrays carry the op values 33 - 51; nothing in front of the library rejects them) -> createOperator ->
addInput (heap arrays) -> finish -> getOutput -> blockInfo / copyBlocks, and the abs failure as a NativeError.  Expected values from the plain
Python model (tests/math_fn_expected.py)."""
import ctypes as C

import numpy as np
import pytest

import math_fn_expected as X
from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, heap_blocks, ints, jctx, jvm, program  # noqa: F401  (jvm and jctx are fixtures)

pytestmark = pytest.mark.gpu


def test_math_program_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    f, D, B = pkg.field, pkg.DOUBLE, pkg.BIGINT
    rng = np.random.default_rng(9)
    n = 1025
    xs = np.round(rng.uniform(-1000, 1000, n), 3)
    xs[:8] = [2.5, -2.5, 0.49999999999999994, -0.0, float("nan"), float("inf"), 1.005, 5e-324]
    ks = rng.integers(-10**6, 10**6, n).astype(np.int64)
    x_nulls = (np.arange(n) % 11 == 3).astype(np.uint8)
    x, k = f(0, D), f(1, B)
    exprs = [pkg.round_(x, 2), pkg.abs_(k), pkg.floor(x), pkg.sqrt(pkg.abs_(x)), pkg.sign(k), pkg.is_nan(x), pkg.round_(k, -2), pkg.power(x, 2.0), pkg.power(x, 1.5), pkg.ln(pkg.abs_(x))]
    filt = pkg.not_(pkg.is_infinite(x))
    fac = I64(jvm.checked("createFilterProjectFactory", I64, jctx, I32(0), ints(jvm, D, B), *program(jvm, pkg, filt, exprs)))
    op = I64(jvm.checked("createOperator", I64, fac))
    add_flat_page(jvm, op, [D, B], [xs, ks], [x_nulls, None])
    jvm.checked("finish", None, op)
    pages = drain(jvm, op)
    blocks = [heap_blocks(jvm, p) for p in pages]
    got = [[None if nl[i] else v[i].item() for v, nl in (b[ch] for b in blocks) for i in range(len(nl))] for ch in range(len(exprs))]
    rows = [(None if x_nulls[r] else float(xs[r]), int(ks[r])) for r in range(n)]
    rows = [(a, b) for a, b in rows if a is not None and not X.is_infinite(a)]
    model = [lambda a, b: X.round_(a, 2), lambda a, b: abs(b), lambda a, b: X.floor(a), lambda a, b: X.sqrt(X.abs_(a)), lambda a, b: X.sign(b), lambda a, b: X.is_nan(a),
             lambda a, b: X.round_(b, -2), lambda a, b: a * a]           # power(x, 2.0) is the one correctly rounded product
    assert len(rows) == n - int(x_nulls.sum()) - 1
    for ch, m in enumerate(model):
        want = [m(a, b) for a, b in rows]
        assert len(got[ch]) == len(want)
        for g, w in zip(got[ch], want):
            assert X.same(bool(g) if isinstance(w, bool) else g, w), (ch, g, w)
    # the host's pow and ln and the device's: each within 1 ulp of the truth, so at most two doubles apart
    assert max(X.ulp_distance(g, X.power(a, 1.5)) for g, (a, b) in zip(got[8], rows)) <= 2
    assert max(X.ulp_distance(g, X.ln(X.abs_(a))) for g, (a, b) in zip(got[9], rows)) <= 2
    for p in pages:
        jvm.call("releasePage", None, I64(p))
    # abs of the minimum comes back as NativeError(NUMERIC_VALUE_OUT_OF_RANGE = -2, the reference's message)
    op2 = I64(jvm.checked("createOperator", I64, fac))
    ks2 = ks.copy()
    ks2[700] = -2**63
    none = jvm.object_array([None] * 2)
    jvm.call("addInput", None, op2, I32(n), ints(jvm, D, B), ints(jvm, 0, 0), ints(jvm, 0, 0), ints(jvm, 0, 0), jvm.object_array([jvm.array(xs), jvm.array(ks2)]),
             jvm.object_array([jvm.array(x_nulls), None]), none, none, none, none, none)
    if jvm.pending_code() == 0:       # the error may surface at addInput or at getOutput; one of them must have raised
        jvm.call("getOutput", I64, op2, jvm.empty(1, np.uint8))
    assert jvm.pending_code() == -2
    jvm.clear()
    jvm.call("close", None, op2)
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    clean(jvm)

"""TGPU_TIMESTAMP through the JNI shim on the GPU against the fake JVM: one filter / project program of the TIMESTAMP functions (the node
arrays carry type code 7, the op values 52 - 56 and the precision of date_add / CAST in the node's long), and one hash aggregation grouped by a
TIMESTAMP key with min / max over TIMESTAMP (function codes 17 and 18).  createContext -> create...Factory -> createOperator -> addInput
(heap long[] arrays) -> finish -> getOutput -> blockInfo / copyBlocks.  Expected values from the plain Python model
(tests/timestamp_fn_expected.py)."""
import ctypes as C
import struct

import numpy as np
import pytest

import timestamp_fn_cases as TC
import timestamp_fn_expected as X
from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, ints, jctx, jvm, program  # noqa: F401  (jvm and jctx are fixtures)

pytestmark = pytest.mark.gpu


def heap_blocks(jvm, page):  # noqa: F811
    """GpuPages.toHeapBlocks for fixed-width channels, TIMESTAMP among them (long[] like BIGINT): blockInfo per channel, then ONE copyBlocks"""
    page = I64(page)
    channels = jvm.checked("pageChannelCount", I32, page)
    positions = jvm.checked("pagePositionCount", I32, page)
    info = jvm.empty(3, np.int64)
    vals, nls, meta = [], [], []
    for ch in range(channels):
        jvm.checked("blockInfo", None, page, I32(ch), info)
        t, _, may = (int(x) for x in jvm.read(info, np.int64))
        dt = {1: np.int64, 7: np.int64, 4: np.float64, 2: np.int32, 3: np.int32, 5: np.uint8}[t]
        vals.append(jvm.empty(positions, dt))
        nls.append(jvm.empty(positions, np.uint8) if may else None)
        meta.append((t, dt))
    jvm.checked("copyBlocks", None, page, jvm.object_array(vals), jvm.object_array(nls), jvm.object_array([None] * channels))
    out = []
    for ch, (t, dt) in enumerate(meta):
        nl = jvm.read(nls[ch], np.uint8).astype(bool) if nls[ch] is not None else np.zeros(positions, dtype=bool)
        out.append((jvm.read(vals[ch], dt), nl, t))
    return out


def columns_of(jvm, pages, n, types=None):  # noqa: F811
    blocks = [heap_blocks(jvm, p) for p in pages]
    if types is not None:
        assert all([t for _, _, t in b] == types for b in blocks)
    blocks = [[(v, nl) for v, nl, _ in b] for b in blocks]
    return [[None if nl[i] else v[i].item() for v, nl in (b[ch] for b in blocks) for i in range(len(nl))] for ch in range(n)]


def test_timestamp_program_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    xs = [t for t in TC.instants() if abs(t) < 2**62][:1025]
    n = len(xs)
    ts = np.array(xs, dtype=np.int64)
    ks = ((np.arange(n) * 37) % 61 - 30).astype(np.int64)
    t_nulls = (np.arange(n) % 11 == 3).astype(np.uint8)
    t, k = f(0, T), f(1, B)
    exprs = [pkg.hour(t), pkg.minute(t), pkg.second(t), pkg.millisecond(t), pkg.to_unixtime(t), pkg.year(t), pkg.date_trunc("hour", t), pkg.date_add("month", k, t, 2),
             pkg.date_diff("day", t, pkg.constant(0, T)), pkg.cast(t, T, 3), pkg.cast(t, pkg.DATE), t]
    filt = pkg.not_(pkg.between(pkg.hour(t), 3, 4))
    fac = I64(jvm.checked("createFilterProjectFactory", I64, jctx, I32(0), ints(jvm, T, B), *program(jvm, pkg, filt, exprs)))
    op = I64(jvm.checked("createOperator", I64, fac))
    add_flat_page(jvm, op, [T, B], [ts, ks], [t_nulls, None])
    jvm.checked("finish", None, op)
    pages = drain(jvm, op)
    got = columns_of(jvm, pages, len(exprs), [B, B, B, B, pkg.DOUBLE, B, T, T, B, T, pkg.DATE, T])
    rows = [(int(a), int(b)) for a, b, nu in zip(ts, ks, t_nulls) if not nu and not 3 <= X.hour(int(a)) <= 4]
    model = [lambda a, b: X.hour(a), lambda a, b: X.minute(a), lambda a, b: X.second(a), lambda a, b: X.millisecond(a), lambda a, b: X.to_unixtime(a), lambda a, b: X.year(a),
             lambda a, b: X.date_trunc("hour", a), lambda a, b: X.date_add("month", b, a, 2), lambda a, b: X.date_diff("day", a, 0), lambda a, b: X.cast_precision(a, 3),
             lambda a, b: X.to_date(a), lambda a, b: a]
    assert 800 < len(rows) < n
    for ch, m in enumerate(model):
        want = [m(a, b) for a, b in rows]
        if ch == 4:
            assert [struct.pack("<d", g) for g in got[ch]] == [struct.pack("<d", w) for w in want]
        else:
            assert got[ch] == want, ch
    for p in pages:
        jvm.call("releasePage", None, I64(p))
    # a date_add whose result leaves the microsecond range comes back as NativeError(NUMERIC_VALUE_OUT_OF_RANGE = -2)
    op2 = I64(jvm.checked("createOperator", I64, fac))
    ts2 = ts.copy()
    ts2[700], ks[700] = X.INT64_MAX - 5 * 3_600_000_000, 30          # 23:00 of the range's last whole day, plus 30 months
    assert X.hour(int(ts2[700])) == 23
    none = jvm.object_array([None] * 2)
    jvm.call("addInput", None, op2, I32(n), ints(jvm, T, B), ints(jvm, 0, 0), ints(jvm, 0, 0), ints(jvm, 0, 0), jvm.object_array([jvm.array(ts2), jvm.array(ks)]),
             jvm.object_array([jvm.array(np.zeros(n, dtype=np.uint8)), None]), none, none, none, none, none)
    if jvm.pending_code() == 0:       # the error may surface at addInput or at getOutput; one of them must have raised
        jvm.call("getOutput", I64, op2, jvm.empty(1, np.uint8))
    assert jvm.pending_code() == -2
    jvm.clear()
    jvm.call("close", None, op2)
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    clean(jvm)


def test_aggregation_grouped_by_a_timestamp_key_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    T, B = pkg.TIMESTAMP, pkg.BIGINT
    rng = np.random.default_rng(78)
    n, ngroups = 4000, 9
    key_pool = np.array([X.INT64_MIN, X.INT64_MAX, 0, -1, 1 << 32, TC.at(2020, 5, 10, 12), TC.at(1969, 12, 31, 23, 59, 59, 999_000), 86_400_000_000, -86_400_000_000], dtype=np.int64)
    keys = key_pool[rng.integers(0, ngroups, n)]
    key_nulls = (np.arange(n) % 17 == 4).astype(np.uint8)
    vals = rng.integers(-10**17, 10**17, n).astype(np.int64)
    val_nulls = ((keys == 0) | (rng.random(n) < 0.2)).astype(np.uint8)           # one group without a value
    aggs = [(pkg.MIN_TIMESTAMP, 1), (pkg.MAX_TIMESTAMP, 1), (pkg.COUNT_COLUMN, 1)]
    flat = [x for fn, ch in aggs for x in (fn, ch, -1)]
    fac = I64(jvm.checked("createHashAggregationFactory", I64, jctx, I32(3), ints(jvm, T), ints(jvm, 0), I32(-1), I32(pkg.SINGLE), ints(jvm, *flat), I32(ngroups), C.c_uint8(0)))
    op = I64(jvm.checked("createOperator", I64, fac))
    add_flat_page(jvm, op, [T, T], [keys, vals], [key_nulls, val_nulls])
    jvm.checked("finish", None, op)
    pages = drain(jvm, op)
    got = list(zip(*columns_of(jvm, pages, 4, [T, T, T, B])))
    want = {}
    for kk, kn, v, vn in zip(keys, key_nulls, vals, val_nulls):
        g = None if kn else int(kk)
        lo, hi, c = want.get(g, (None, None, 0))
        if not vn:
            lo, hi, c = (int(v) if lo is None else min(lo, int(v))), (int(v) if hi is None else max(hi, int(v))), c + 1
        want[g] = (lo, hi, c)
    assert got == [(g,) + w for g, w in want.items()] and want[0] == (None, None, 0) and None in want and len(want) == ngroups + 1
    jvm.clear()
    for p in pages:
        jvm.call("releasePage", None, I64(p))
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    assert jvm.global_refs() == 0
    clean(jvm)

"""One hash aggregation with min / max over INTEGER, DATE and VARCHAR driven through the JNI shim on the GPU against the fake JVM, SINGLE
and PARTIAL -> FINAL: createContext -> createHashAggregationFactory -> createOperator -> addInput (heap arrays) -> finish -> getOutput ->
blockInfo / copyBlocks.  Nothing in front of the library rejects the function codes 11 - 16; expected values from the plain Python model
(tests/minmax_expected.py)."""
import ctypes as C

import numpy as np

import minmax_expected as M
import pytest
from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, heap_blocks, ints, jctx, jvm  # noqa: F401  (jvm and jctx are fixtures)

pytestmark = pytest.mark.gpu

FUNCTIONS = [(M.MIN_INTEGER, 1), (M.MAX_INTEGER, 1), (M.MIN_DATE, 2), (M.MAX_DATE, 2), (M.MIN_VARCHAR, 3), (M.MAX_VARCHAR, 3)]


def varchar_arrays(values):
    """list of bytes / None -> (byte pool, offsets, nulls)"""
    bs = [b"" if v is None else v for v in values]
    offs = np.zeros(len(bs) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(b) for b in bs])
    pool = np.frombuffer(b"".join(bs) or b"\x00", dtype=np.uint8).copy()
    return pool, offs, np.array([v is None for v in values], dtype=np.uint8)


def run(pkg, jvm, jctx, step, aggs, types, columns, nulls, offsets, ngroups):  # noqa: F811
    flat = [x for f, ch in aggs for x in (f, ch, -1)]
    fac = I64(jvm.checked("createHashAggregationFactory", I64, jctx, I32(3), ints(jvm, pkg.BIGINT), ints(jvm, 0), I32(-1), I32(step), ints(jvm, *flat), I32(ngroups), C.c_uint8(0)))
    op = I64(jvm.checked("createOperator", I64, fac))
    add_flat_page(jvm, op, types, columns, nulls, offsets)
    jvm.checked("finish", None, op)
    pages = drain(jvm, op)
    blocks = [heap_blocks(jvm, p) for p in pages]
    rows = []
    for b in blocks:
        cols = [[None if nl[i] else (v[i] if isinstance(v, list) else v[i].item()) for i in range(len(nl))] for v, nl in b]
        rows += list(zip(*cols))
    jvm.clear()
    for p in pages:
        jvm.call("releasePage", None, I64(p))
    jvm.call("close", None, op)
    jvm.call("noMoreOperators", None, fac)
    jvm.call("destroyFactory", None, fac)
    return rows


def test_all_six_functions_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    rng = np.random.default_rng(77)
    n, ngroups = 4000, 7
    gids = rng.integers(0, ngroups, n).astype(np.int64)
    ints_ = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    dates = rng.integers(-20_000, 20_000, n).astype(np.int32)
    ints_[:2] = [-2 ** 31, 2 ** 31 - 1]
    int_nulls = (rng.random(n) < 0.2).astype(np.uint8)
    int_nulls[:2] = 0
    date_nulls = (gids == 3).astype(np.uint8)                       # one group without a date
    words = [b"", b"a", b"a ", b"https://x", b"https://y", b"https://x/longer/than/seven", b"zebra", b"Zebra"]
    texts = [None if rng.random() < 0.2 else words[int(rng.integers(0, len(words)))] for _ in range(n)]
    pool, offs, text_nulls = varchar_arrays(texts)
    B, I, DT, V = pkg.BIGINT, pkg.INTEGER, pkg.DATE, pkg.VARCHAR
    types = [B, I, DT, V]
    model_cols = {1: [None if nu else int(v) for v, nu in zip(ints_, int_nulls)], 2: [None if nu else int(v) for v, nu in zip(dates, date_nulls)], 3: texts}
    want = {g: tuple(M.single([(model_cols[ch], gids.tolist(), None)], f, ngroups)[g][1] for f, ch in FUNCTIONS) for g in range(ngroups)}
    want = {g: tuple(v.decode() if isinstance(v, bytes) else v for v in row) for g, row in want.items()}
    args = (types, [gids, ints_, dates, pool], [None, int_nulls, date_nulls, text_nulls], [None, None, None, offs])
    single = run(pkg, jvm, jctx, pkg.SINGLE, FUNCTIONS, *args, ngroups)
    assert {r[0]: tuple(r[1:]) for r in single} == want
    assert want[3][2] is None and want[3][3] is None
    # PARTIAL: key, then (count BIGINT, value BIGINT | VARCHAR) per function; the same intermediate rows twice into FINAL
    partial = run(pkg, jvm, jctx, pkg.PARTIAL, FUNCTIONS, *args, ngroups)
    assert len(partial) == ngroups and all(len(r) == 13 for r in partial)
    cols = list(zip(*partial))
    ptypes, pcols, pnulls, poffs = [B], [np.array(cols[0] * 2, dtype=np.int64)], [None], [None]
    for k, (f, _) in enumerate(FUNCTIONS):
        counts, values = cols[1 + 2 * k] * 2, cols[2 + 2 * k] * 2
        ptypes += [B, V if M.is_varchar(f) else B]
        pcols.append(np.array(counts, dtype=np.int64))
        pnulls.append(None)
        poffs.append(None)
        if M.is_varchar(f):
            assert all((v is None) == (c == 0) for v, c in zip(values, counts))
            vp, vo, vn = varchar_arrays([None if v is None else v.encode() for v in values])
            pcols.append(vp)
            pnulls.append(vn)
            poffs.append(vo)
        else:
            assert all(v == 0 for v, c in zip(values, counts) if c == 0)
            pcols.append(np.array(values, dtype=np.int64))
            pnulls.append(None)
            poffs.append(None)
    final_aggs = [(f, 1 + 2 * k) for k, (f, _) in enumerate(FUNCTIONS)]
    final = run(pkg, jvm, jctx, pkg.FINAL, final_aggs, ptypes, pcols, pnulls, poffs, ngroups)
    assert {r[0]: tuple(r[1:]) for r in final} == want
    assert jvm.global_refs() == 0
    clean(jvm)

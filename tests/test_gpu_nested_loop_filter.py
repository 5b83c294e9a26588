"""FilterProjectNestedLoopJoinOperator on the device: NestedLoopJoin(all channels) -> FilterAndProject as one operator.  Expected values are
nested_loop_expected.filtered -- expr_fuzz.run_program over every reference page in order -- compared cell by cell with expr_fuzz.bits, a
Failure by its error code; every program is also run as the unfused PAIR of operators on the device and must give the same.  Which route a
program took is proven by profile scope: nlj_pair_count / nlj_pair_emit (the predicate over the virtual product) or nlj_product (product
pieces, then the page processor)."""
import ctypes as C
import random

import numpy as np
import pytest

import expr_fuzz as F
import expr_harness as H
import nested_loop_expected as NL
import nested_loop_gpu as G
from expr_fuzz import BIGINT as B, BOOLEAN as BO, DATE as DT, DOUBLE as D
from test_gpu_jni_shim import I32, I64, add_flat_page, clean, drain, heap_blocks, ints, jctx, jvm, program as jni_program  # noqa: F401  (jvm and jctx are fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    cx = pkg.Context(0)
    yield cx
    cx.close()


def rows_of(cols):
    return [tuple(c[i] for c in cols) for i in range(len(cols[0]))] if cols else []


def run_fused(pkg, ctx, prog, n_probe, probe_pages, build_pages, max_rows=0, profile=False):
    """probe_pages / build_pages: per page its columns.  -> (output pages on the host, error or None, profile or None)"""
    types = list(prog.types)
    pt, bt = types[:n_probe], types[n_probe:]
    bf, bop = G.build(pkg, ctx, bt, [G.page_of(pkg, bt, pg) for pg in build_pages])
    _, filt, projs = F.lower(prog, pkg.expressions)
    jf = pkg.FilterProjectNestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, pt, filt, projs, max_product_rows=max_rows)
    jop = jf.createOperator()
    if profile:
        ctx.profile_enable(True)
        ctx.profile_reset()
    outs, err = H.drive_pages(pkg, jop, [G.page_of(pkg, pt, pg) for pg in probe_pages])
    prof = None
    if profile:
        prof = ctx.profile()
        ctx.profile_enable(False)
    jop.close()   # after an error too: clean
    G.end(bf, bop, jf)
    return outs, err, prof


def run_unfused_pair(pkg, ctx, prog, n_probe, probe_pages, build_pages):
    """NestedLoopJoinOperator -> FilterAndProjectOperator, page by page on the device.  The join hands on the channels the program reads
    (the two sides together have more channels than a page processor takes) and the program addresses them by their place in that page.
    One probe page, one build page; the join's output pages are cut at the large side's row count, i.e. they ARE the reference's pages:
    which error the pair raises depends on its pages (FilterAndProject reports a page's filter failure before any projection's)."""
    assert len(probe_pages) == 1 and len(build_pages) == 1
    types = list(prog.types)
    pt, bt = types[:n_probe], types[n_probe:]
    trees = ([] if prog.filter is None else [prog.filter]) + list(prog.projections)
    read = sorted({t[1] for tree in trees for t in F.walk(tree) if t[0] == "in"})
    place = {ch: k for k, ch in enumerate(read)}
    move = lambda tree: F.map_inputs(tree, lambda ch, t: ("in", place[ch], t))
    narrow = F.Program(prog.name, tuple(types[ch] for ch in read), None if prog.filter is None else move(prog.filter), tuple(move(p) for p in prog.projections))
    bf, bop = G.build(pkg, ctx, bt, [G.page_of(pkg, bt, pg) for pg in build_pages])
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, pt, [ch for ch in read if ch < n_probe], [ch - n_probe for ch in read if ch >= n_probe],
                                           max_output_rows=max(len(probe_pages[0][0]), len(build_pages[0][0])))
    jop = jf.createOperator()
    joined = pkg.to_pages(jop, [G.page_of(pkg, pt, pg) for pg in probe_pages], to_host=False)
    ff = pkg.FilterAndProjectOperatorFactory(ctx, 3, *F.lower(narrow, pkg.expressions))
    fop = ff.createOperator()
    outs, err = H.drive_pages(pkg, fop, joined)
    for o in joined:
        o.release()
    fop.close()
    ff.close()
    jop.close()
    G.end(bf, bop, jf)
    return outs, err


def check(prog, outs, err, want, what):
    if isinstance(want, F.Failure):
        assert err is not None, (prog.name, what, "no error; the model raises", want)
        assert err[0].code == want.code, (prog.name, what, err[0].code, str(err[0]), want)
        return
    assert err is None, (prog.name, what, str(err[0]) if err else None)
    assert sum(o.position_count for o in outs) == len(want.positions), (prog.name, what, sum(o.position_count for o in outs), len(want.positions))
    got = G.bits_columns([F.type_of(p) for p in prog.projections], outs)
    for k, (p, col) in enumerate(zip(prog.projections, want.columns)):
        exp = [F.bits(F.type_of(p), v) for v in col]
        if got[k] != exp:
            bad = [i for i, (x, y) in enumerate(zip(got[k], exp)) if x != y][:3]
            raise AssertionError((prog.name, what, "projection %d" % k, [(want.positions[i], got[k][i], exp[i]) for i in bad]))


def assert_route(prof, fused, what):
    if fused:
        assert "nlj_pair_count" in prof and "nlj_product" not in prof, (what, sorted(prof))
    else:
        assert "nlj_product" in prof and "nlj_pair_count" not in prof and "nlj_pair_emit" not in prof, (what, sorted(prof))


# ---- programs that must take the fused route ------------------------------------------------------------------------------------------
# probe: 0 x BIGINT, 1 d DATE, 2 v DOUBLE, 3 f BOOLEAN; build: 4 lo BIGINT, 5 hi BIGINT, 6 d DATE, 7 v DOUBLE, 8 f BOOLEAN
FT = (B, DT, D, BO, B, B, DT, D, BO)
NP = 4
_in = lambda ch: ("in", ch, FT[ch])
_call = lambda name, t, *a: ("call", name, t, tuple(a))
_sf = lambda form, t, *a, items=None: ("sf", form, t, tuple(a), items)
PROJ = (_in(0), _in(4), _call("ADD", D, _in(2), _in(7)), _in(6), _sf("IS_NULL", BO, _in(8)))
FUSED = [
    F.Program("band", FT, _sf("BETWEEN", BO, _in(0), _in(4), _in(5)), PROJ),
    F.Program("date_less", FT, _call("LESS_THAN", BO, _in(1), _in(6)), PROJ),
    F.Program("double_compare", FT, _sf("OR", BO, _call("LESS_THAN", BO, _in(2), _in(7)), _call("EQUAL", BO, _in(7), _in(2))), PROJ),
    F.Program("double_not_equal", FT, _call("NOT_EQUAL", BO, _in(2), _in(7)), PROJ[:3]),
    F.Program("probe_side_only", FT, _call("GREATER_THAN", BO, _in(0), ("const", 0, B)), PROJ),
    F.Program("build_side_only", FT, _call("NOT", BO, _sf("IS_NULL", BO, _in(5))), PROJ),
    F.Program("constant_true", FT, ("const", True, BO), PROJ[:2]),
    F.Program("constant_null", FT, ("const", None, BO), PROJ[:2]),
    F.Program("in_constants", FT, _sf("IN", BO, _in(0), items=(("const", -3, B), ("const", 2, B), ("const", None, B), ("const", 4, B))), PROJ),
    F.Program("and_or_with_nulls", FT, _sf("AND", BO, _in(3), _sf("OR", BO, _in(8), ("const", None, BO))), PROJ),
    F.Program("if_coalesce_cast", FT, _sf("IF", BO, _call("LESS_THAN", BO, _sf("COALESCE", D, _in(2), _call("CAST", D, _in(0))), _in(7)), _in(3), _in(8)), PROJ[:3]),
]
DOUBLES = [float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 1.5, -1.5, 2.0]


def side(types, n, salt):
    r = random.Random(1000 * salt + n)
    cols = []
    for t in types:
        pick = {B: lambda: r.randint(-5, 5), DT: lambda: r.randint(9000, 9004), D: lambda: r.choice(DOUBLES), BO: lambda: r.random() < 0.5}[t]
        cols.append([None if r.random() < 0.15 else pick() for _ in range(n)])
    return cols


@pytest.mark.parametrize("L,S,build_large", [(L, S, bl) for L in G.LARGE for S in G.SMALL if S <= L for bl in ((False,) if S == L else (False, True))])
def test_fused_programs_over_the_shapes(pkg, ctx, L, S, build_large):
    p, b = (S, L) if build_large else (L, S)
    probe, build = side(FT[:NP], p, 1), side(FT[NP:], b, 2)
    for prog in FUSED:
        want = NL.filtered(prog, [rows_of(probe)], [rows_of(build)])
        assert isinstance(want, F.Values)
        for max_rows in (0, 1000):
            outs, err, prof = run_fused(pkg, ctx, prog, NP, [probe], [build], max_rows, profile=True)
            check(prog, outs, err, want, "max_product_rows %d" % max_rows)
            assert_route(prof, True, prog.name)
            assert ("nlj_pair_emit" in prof) == bool(want.positions), (prog.name, sorted(prof))


def test_fused_programs_over_several_pages(pkg, ctx):
    probe = [side(FT[:NP], n, 3 + n) for n in (65, 0, 2, 130)]
    build = [side(FT[NP:], n, 4 + n) for n in (0, 64, 3, 131)]
    for prog in FUSED:
        want = NL.filtered(prog, [rows_of(pg) for pg in probe], [rows_of(pg) for pg in build])
        outs, err, _ = run_fused(pkg, ctx, prog, NP, probe, build, 777)
        check(prog, outs, err, want, "3 x 3 pages")


# ---- random programs: the 13 expr_fuzz channels dealt to the two sides ----------------------------------------------------------------------
SEEDED = [("quiet", s) for s in F.QUIET_SEEDS] + [("loud", s) for s in F.LOUD_SEEDS]
N13 = len(F.TYPES)
# (probe rows, build rows): 1, 64, 65 on one side and 3, 257 on the other, each way round; the two largest products go to every fourth
# program (the plain evaluator takes seconds over their 16 000 rows)
SIZES = [(65, 3), (3, 64), (1, 257), (257, 1), (64, 3), (3, 1)]
LARGE_SIZES = [(65, 257), (257, 64)]


def split_program(prog):
    """channels 0-6 are the probe side's, 7-12 the build side's: the program as it stands"""
    return prog, 7, lambda n: [vals for _, vals in F.page(n)[:7]], lambda n: [vals for _, vals in F.page(n)[7:]]


def dealt_program(prog, seed):
    """every input reference goes to the probe side's copy of its channel or to the build side's, reference by reference (as expr_fuzz.join_filter deals)"""
    r = random.Random("deal%s" % seed)
    deal = lambda tree: F.map_inputs(tree, lambda ch, t: ("in", ch + (N13 if r.random() < 0.5 else 0), t))
    dealt = F.Program(prog.name + "_dealt", F.TYPES + F.TYPES, None if prog.filter is None else deal(prog.filter), tuple(deal(p) for p in prog.projections))
    cols = lambda n: [vals for _, vals in F.page(n)]
    return dealt, N13, cols, lambda n: [list(reversed(vals)) for _, vals in F.page(n)]   # (the build side's rows in another order than the probe side's)


@pytest.mark.parametrize("dealing", ["split", "dealt"])
@pytest.mark.parametrize("mode,seed", SEEDED, ids=["%s%s" % s for s in SEEDED])
def test_random_programs(pkg, ctx, mode, seed, dealing):
    base = F.program(seed, mode)
    prog, n_probe, probe_cols, build_cols = split_program(base) if dealing == "split" else dealt_program(base, seed)
    sizes = SIZES + (LARGE_SIZES if SEEDED.index((mode, seed)) % 4 == 0 else [])
    for p, b in sizes:
        probe, build = probe_cols(p), build_cols(b)
        want = NL.filtered(prog, [rows_of(probe)], [rows_of(build)])
        outs, err, prof = run_fused(pkg, ctx, prog, n_probe, [probe], [build], 0, profile=True)
        check(prog, outs, err, want, "%d x %d" % (p, b))
        assert ("nlj_pair_count" in prof) != ("nlj_product" in prof), (prog.name, sorted(prof))   # one route or the other, whichever: it is compared
        outs2, err2 = run_unfused_pair(pkg, ctx, prog, n_probe, [probe], [build])
        check(prog, outs2, err2, want, "%d x %d as NestedLoopJoin -> FilterAndProject" % (p, b))
        # pieces smaller than a reference page, and cut inside one
        outs3, err3, _ = run_fused(pkg, ctx, prog, n_probe, [probe], [build], 100)
        check(prog, outs3, err3, want, "%d x %d, max_product_rows 100" % (p, b))


def test_routes_of_filters_the_generator_declines(pkg, ctx):
    x, lo, s = ("in", 0, B), ("in", 1, B), ("in", 2, F.VARCHAR)
    types = (B, B, F.VARCHAR)
    probe, build = [[1, 2, None, 4]], [[0, 3, 1], ["ab", None, "b"]]
    for name, filt, fused in [("none", None, False),
                              ("raising", _call("GREATER_THAN", BO, _call("ADD", B, x, lo), ("const", 2, B)), False),
                              ("like", _call("LIKE", BO, s, ("const", "a%", F.VARCHAR)), False),
                              ("plain", _call("GREATER_THAN", BO, x, lo), True)]:
        prog = F.Program(name, types, filt, (x, s, lo))
        outs, err, prof = run_fused(pkg, ctx, prog, 1, [probe], [build], 0, profile=True)
        check(prog, outs, err, NL.filtered(prog, [rows_of(probe)], [rows_of(build)]), name)
        assert_route(prof, fused, name)


# ---- which error wins ---------------------------------------------------------------------------------------------------------------------------
def error_case(pkg, ctx, prog, n_probe, probe, build, code):
    want = NL.filtered(prog, [rows_of(probe)], [rows_of(build)])
    assert isinstance(want, F.Failure) and want.code == code, want
    for max_rows in (0, 50):
        outs, err, _ = run_fused(pkg, ctx, prog, n_probe, [probe], [build], max_rows)
        check(prog, outs, err, want, "max_product_rows %d" % max_rows)
    outs, err = run_unfused_pair(pkg, ctx, prog, n_probe, [probe], [build])
    check(prog, outs, err, want, "NestedLoopJoin -> FilterAndProject")
    # the context stays usable
    ok = F.Program("ok", prog.types, None, (("in", 0, prog.types[0]),))
    outs, err, _ = run_fused(pkg, ctx, ok, n_probe, [probe], [build])
    assert err is None and sum(o.position_count for o in outs) == len(probe[0]) * len(build[0])


def test_an_earlier_page_failing_in_a_projection_beats_a_later_one_failing_in_the_filter(pkg, ctx):
    x, y = ("in", 0, B), ("in", 1, B)
    probe, build = [list(range(1, 71))], [[1, 2, 0]]   # the build page is the small side: one reference page per y
    overflow = _call("MULTIPLY", B, x, ("const", 2**62, B))                                   # x >= 2: NUMERIC_VALUE_OUT_OF_RANGE
    # unfused route: the filter divides by y (page y = 0, the LAST one, fails in the filter); projection 1 overflows in the FIRST page
    raising = F.Program("filter_later", (B, B), _call("GREATER_THAN_OR_EQUAL", BO, _call("DIVIDE", B, ("const", 7, B), y), ("const", 0, B)), (x, overflow))
    error_case(pkg, ctx, raising, 1, probe, build, F.RANGE)
    # fused route: the filter cannot raise; projection 1 fails in the first page, projection 0 (of lower rank) in the second, y = 2
    div = _call("DIVIDE", B, ("const", 7, B), _call("SUBTRACT", B, y, ("const", 2, B)))
    quiet = F.Program("projection_later", (B, B), _call("GREATER_THAN", BO, x, ("const", 0, B)), (div, overflow))
    error_case(pkg, ctx, quiet, 1, probe, build, F.RANGE)


@pytest.mark.parametrize("k", range(F.ORDER_PROGRAMS))
def test_order_programs_within_one_reference_page(pkg, ctx, k):
    """expr_fuzz.order_program: projection j fails while projection j + 1 fails on an EARLIER row with another code -- one build row, so the
    2049 probe rows are one reference page"""
    prog, n_probe, probe_cols, build_cols = split_program(F.order_program(k))
    probe, build = probe_cols(max(F.ROW_COUNTS)), build_cols(1)
    want = NL.filtered(prog, [rows_of(probe)], [rows_of(build)])
    assert isinstance(want, F.Failure)
    for max_rows in (0, 600):
        outs, err, _ = run_fused(pkg, ctx, prog, n_probe, [probe], [build], max_rows)
        check(prog, outs, err, want, "max_product_rows %d" % max_rows)


# ---- through the JNI shim ---------------------------------------------------------------------------------------------------------------------------
def test_build_probe_fused_and_stats_through_the_shim(pkg, jvm, jctx):  # noqa: F811
    f = pkg.field
    x = np.arange(-40, 60, dtype=np.int64)                  # probe: 100 rows
    lo, hi = np.array([-10, 5, 30], dtype=np.int64), np.array([-5, 5, 41], dtype=np.int64)
    handles = jvm.checked("createNestedLoopBuildFactory", I64, jctx, I32(1), ints(jvm, B, B))
    bfac, bridge = (I64(int(v)) for v in jvm.read(C.c_void_p(handles), np.int64))
    bop = I64(jvm.checked("createOperator", I64, bfac))
    add_flat_page(jvm, bop, [B, B], [lo, hi])
    jvm.checked("finish", None, bop)
    stats = jvm.empty(3, np.int64)
    jvm.checked("nestedLoopBridgeStats", None, bridge, stats)
    assert [int(v) for v in jvm.read(stats, np.int64)] == [1, 3, 48]
    # the plain join: probe channel 0, build channels 1, 0
    jfac = I64(jvm.checked("createNestedLoopJoinFactory", I64, jctx, I32(2), bridge, ints(jvm, B), ints(jvm, 0), ints(jvm, 1, 0), I64(64)))
    jop = I64(jvm.checked("createOperator", I64, jfac))
    assert not jvm.checked("isBlocked", C.c_uint8, jop)
    add_flat_page(jvm, jop, [B], [x])
    jvm.checked("finish", None, jop)
    pages = drain(jvm, jop)
    assert len(pages) == 5   # 300 rows in pieces of at most 64
    got = [np.concatenate([heap_blocks(jvm, p)[c][0] for p in pages]) for c in range(3)]
    assert np.array_equal(got[0], np.tile(x, 3)) and np.array_equal(got[1], np.repeat(hi, 100)) and np.array_equal(got[2], np.repeat(lo, 100))
    # the fused operator: x BETWEEN lo AND hi, projecting x and lo
    ffac = I64(jvm.checked("createFilterProjectNestedLoopJoinFactory", I64, jctx, I32(3), bridge, ints(jvm, B),
                           *jni_program(jvm, pkg, pkg.between(f(0, B), f(1, B), f(2, B)), [f(0, B), f(1, B)]), I64(0)))
    fop = I64(jvm.checked("createOperator", I64, ffac))
    add_flat_page(jvm, fop, [B], [x])
    jvm.checked("finish", None, fop)
    fpages = drain(jvm, fop)
    fgot = [np.concatenate([heap_blocks(jvm, p)[c][0] for p in fpages]) for c in range(2)]
    want = [(int(v), int(a)) for a, b in zip(lo, hi) for v in x if a <= v <= b]
    assert list(zip(fgot[0].tolist(), fgot[1].tolist())) == want and len(want) == 6 + 1 + 12
    for p in pages + fpages:
        jvm.call("releasePage", None, I64(p))
    for o in (fop, jop):
        jvm.call("close", None, o)
    for fct in (ffac, jfac):
        jvm.call("noMoreOperators", None, fct)
    assert jvm.checked("isFinished", C.c_uint8, bop)
    jvm.call("close", None, bop)
    for fct in (ffac, jfac, bfac):
        jvm.call("destroyFactory", None, fct)
    jvm.call("destroyNestedLoopBridge", None, bridge)
    clean(jvm)

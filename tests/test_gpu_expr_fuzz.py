"""The expression kernel generator (csrc/jit.cpp) against the plain evaluator of expr_fuzz.py on seeded random programs: compositions of
special forms, NULL and error flags crossing them, casts inside comparisons inside BETWEEN, subtrees shared by the filter and several
projections -- what the one-operator lists of the other expression tests never reach.  One program is one test: one compile, a few launches
on pages of at most 2049 rows.  Every cell is compared by bit pattern (NaN == NaN); where the evaluator raises, the library must raise the
same code, and on a flat page name the same input position.  test_expr_fuzz_cpu.py checks the evaluator itself against the C oracle."""
import numpy as np
import pytest

import expr_fuzz as F
import expr_harness as H

pytestmark = pytest.mark.gpu
SEEDED = [("quiet", s) for s in F.QUIET_SEEDS] + [("loud", s) for s in F.LOUD_SEEDS]
CUTS = (1, 63, 0, 961, 1024)      # the 2049-row input as pages of these sizes
FULL = max(F.ROW_COUNTS)


@pytest.fixture(scope="module")
def ctx(pkg):
    cx = pkg.Context(0)
    yield cx
    cx.close()


def flat_blocks(pkg, page):
    return [pkg.Block(t, vals) for t, vals in page]


def run(pkg, fac, block_pages):
    op = fac.createOperator()
    outs, err = H.drive_pages(pkg, op, [pkg.Page(*blocks) for blocks in block_pages])
    op.close()
    return outs, err


def check(prog, outs, err, want, what, position=True, one_input_page=True):
    """outs / err: what drive_pages gave; want: Values or Failure of the evaluator"""
    if isinstance(want, F.Failure):
        assert err is not None, (prog.name, what, "no error; the evaluator raises", want)
        assert err[0].code == want.code, (prog.name, what, err[0].code, str(err[0]), want)
        if position:
            assert err[2] == want.position, (prog.name, what, str(err[0]), want)
        return
    assert err is None, (prog.name, what, str(err[0]) if err else None)
    if one_input_page:
        assert len(outs) == (1 if want.positions else 0) and sum(o.position_count for o in outs) == len(want.positions), (prog.name, what, len(outs))
    for k, (p, col) in enumerate(zip(prog.projections, want.columns)):
        t = F.type_of(p)
        got = [F.bits(t, v) for o in outs for v in o.getBlock(k).to_list()]
        exp = [F.bits(t, v) for v in col]
        if got != exp:
            bad = [i for i, (x, y) in enumerate(zip(got, exp)) if x != y][:3]
            raise AssertionError((prog.name, what, "projection %d" % k, len(got), len(exp), [(want.positions[i], got[i], exp[i]) for i in bad]))


def cut_outcome(prog):
    """the evaluator over the cut pages in order: Values over all of them, or (the first Failure, the index of its page)"""
    full = F.page(FULL)
    at, positions, columns = 0, [], [[] for _ in prog.projections]
    for k, n in enumerate(CUTS):
        if n:
            o = F.run_program(prog, [(t, vals[at:at + n]) for t, vals in full])
            if isinstance(o, F.Failure):
                return o, k
            positions += [at + i for i in o.positions]
            for col, part in zip(columns, o.columns):
                col += part
        at += n
    return F.Values(positions, columns), None


@pytest.mark.parametrize("mode,seed", SEEDED, ids=["%s%s" % s for s in SEEDED])
def test_filter_and_project_matches_the_evaluator(pkg, ctx, mode, seed):
    prog = F.program(seed, mode)
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, *F.lower(prog, pkg.expressions))
    for n in F.ROW_COUNTS:
        outs, err = run(pkg, fac, [flat_blocks(pkg, F.page(n))])
        check(prog, outs, err, F.outcome(prog, n), "%d rows" % n)
    # the 2049 rows cut into pages and fed to one operator: the same rows, or the error of the page that holds the failing row
    full, at, pages = F.page(FULL), 0, []
    for n in CUTS:
        pages.append(flat_blocks(pkg, [(t, vals[at:at + n]) for t, vals in full]))
        at += n
    assert at == FULL
    outs, err = run(pkg, fac, pages)
    want, failing_page = cut_outcome(prog)
    check(prog, outs, err, want, "cut into pages", one_input_page=False)
    if failing_page is not None:
        assert err[1] == failing_page, (prog.name, "raised while page %d was the last one added, the failing row is in page %d" % (err[1], failing_page))
    fac.close()


# ---- encoded inputs ------------------------------------------------------------------------------------------------------------------
UNREFERENCED = {F.BIGINT: [F.I64_MIN, 2**62], F.INTEGER: [F.I32_MIN], F.DOUBLE: [float("nan"), 2.0**63]}   # entries no row refers to, which fail in many programs


def dictionary_blocks(pkg, page):
    """every channel as a DictionaryBlock: its distinct values, a NULL entry the NULL rows refer to, then a NULL and failing entries that
    no row refers to"""
    blocks = []
    for t, vals in page:
        entries, index = [], {}
        for v in vals:
            key = F.bits(t, v)
            if key not in index:
                index[key] = len(entries)
                entries.append(v)
        ids = [index[F.bits(t, v)] for v in vals]
        entries += [None] + UNREFERENCED.get(t, [])
        blocks.append(pkg.DictionaryBlock(pkg.Block(t, entries), ids))
    return blocks


def rle_blocks(pkg, page):
    n = len(page[0][1])
    return [pkg.RunLengthEncodedBlock(pkg.Block(t, vals[:1]), n) for t, vals in page]


ENCODED = [("quiet", 2, None), ("quiet", 6, None), ("loud", 106, None), ("loud", "order0", None)] + [(m, s, ch) for m, s, ch in F.SINGLE_CHANNEL]
# enough of the single-channel programs cannot raise, so that the dictionary-aware path itself (not only its fallback) is compared
assert sum(not any(F.can_raise(r) for r in ([p.filter] if p.filter is not None else []) + list(p.projections)) for p in (F.program(s, m, ch) for m, s, ch in F.SINGLE_CHANNEL)) >= 4


@pytest.mark.parametrize("mode,seed,only", ENCODED, ids=["%s%s%s" % (m, s, "" if ch is None else "_ch%d" % ch) for m, s, ch in ENCODED])
def test_dictionary_and_rle_inputs_match_the_flat_run(pkg, ctx, mode, seed, only):
    """a program that reads one channel takes the dictionary-aware path (the expressions over the dictionary's entries, then a gather) and
    falls back to the flat evaluation when an entry raises; every other program decodes its input"""
    prog = F.program(seed, mode, only)
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, *F.lower(prog, pkg.expressions))
    cannot_raise = not any(F.can_raise(r) for r in ([prog.filter] if prog.filter is not None else []) + list(prog.projections))
    for n in (64, 1025):
        page = F.page(n)
        op = fac.createOperator()
        outs, err = H.drive_pages(pkg, op, [pkg.Page(*dictionary_blocks(pkg, page))])
        taken = pkg._lib.lib().tgpu_debug_dictionary_pages(op.handle)
        op.close()
        check(prog, outs, err, F.run_program(prog, page), "dictionary blocks, %d rows" % n, position=False)
        if only is not None and cannot_raise and n == 1025:
            # no entry can raise and the dictionary is far shorter than the page: the expressions ran over the entries, not over the rows
            assert taken == 1, (prog.name, "the dictionary-aware path was not taken")
        if only is None:
            assert taken == 0, (prog.name, "several channels are read: there is no single dictionary to evaluate")
    full = F.page(FULL)
    for row in (3, 13, 28, 40):      # a run of one row's values, NULLs as they come
        page = [(t, [vals[row]] * 65) for t, vals in full]
        outs, err = run(pkg, fac, [rle_blocks(pkg, page)])
        check(prog, outs, err, F.run_program(prog, page), "run-length blocks of row %d" % row, position=False)
    fac.close()


# ---- the fused aggregation --------------------------------------------------------------------------------------------------------------
FUSED = [("quiet", s) for s in F.QUIET_SEEDS[:6]] + [("loud", s) for s in F.LOUD_SEEDS[:4]]


def aggregation_program(prog, stays_fused):
    """projection 0 becomes the BIGINT key (channel 2, never NULL); -> (program, aggregates as (name, input, mask)): count / sum / min over
    the other BIGINT projections, count / sum over the DOUBLE ones, one sum under the first BOOLEAN projection as its mask.
    A projection that can raise and that the aggregation drops, or evaluates under a mask, keeps the unfused composition (jit.cpp
    FusedAggGpu); stays_fused leaves those out: no BOOLEAN projection that can raise, the mask over an input that cannot."""
    numeric = [p for p in prog.projections if F.type_of(p) in (F.BIGINT, F.DOUBLE)][:5]          # 16 aggregates at the most
    masks = [p for p in prog.projections if F.type_of(p) == F.BOOLEAN and not (stays_fused and F.can_raise(p))]
    projections = (("in", 2, F.BIGINT),) + tuple(numeric) + tuple(masks)
    mask = 1 + len(numeric) if masks else -1
    aggs = [("count_all", -1, -1)]
    for k, p in enumerate(numeric, 1):
        masked = mask if not (stays_fused and F.can_raise(p)) else -1
        if F.type_of(p) == F.BIGINT:
            aggs += [("sum_bigint", k, masked), ("count", k, -1), ("min_bigint", k, -1)]
        else:
            aggs += [("sum_double", k, masked), ("count", k, -1)]
        if masked >= 0:
            mask = -1
    return F.Program(prog.name + "_agg", prog.types, prog.filter, projections), aggs


def fused_scopes(cx):
    return sorted(k for k in cx.profile() if k.startswith("fused_"))


@pytest.mark.parametrize("plan", ["every_projection", "stays_fused"])
@pytest.mark.parametrize("mode,seed", FUSED, ids=["%s%s" % s for s in FUSED])
def test_fused_aggregation_matches_the_unfused_composition(pkg, mode, seed, plan):
    """FilterProjectHashAggregationOperatorFactory against run_program followed by a plain group-by in Python: the groups, the counts and
    the BIGINT sums and minima exactly; a DOUBLE sum where it does not depend on the order (every addend a multiple of 0.25 below 2^40,
    no negative zero); the error code where the evaluator raises -- a raise must never turn into rows.  The stays_fused plans must run
    the fused kernels (their profile scopes), so that it is the generated aggregation that is compared and not the fallback."""
    import math
    prog, aggs = aggregation_program(F.program(seed, mode), plan == "stays_fused")
    fn = {"count_all": pkg.COUNT_ALL, "count": pkg.COUNT_COLUMN, "sum_bigint": pkg.SUM_BIGINT, "sum_double": pkg.SUM_DOUBLE, "min_bigint": pkg.MIN_BIGINT}
    n = 1025
    want = F.run_program(prog, F.page(n))
    cx = pkg.Context(0)
    cx.profile_enable(True)
    fac = pkg.FilterProjectHashAggregationOperatorFactory(cx, 0, *F.lower(prog, pkg.expressions), [F.BIGINT], [0], [(fn[a], ch, mask) for a, ch, mask in aggs])
    outs, err = run(pkg, fac, [flat_blocks(pkg, F.page(n))])
    fac.close()
    scopes = fused_scopes(cx)
    cx.close()
    if plan == "stays_fused" and (isinstance(want, F.Failure) or want.positions):
        assert scopes, (prog.name, "the plan was not fused")
    if isinstance(want, F.Failure):
        assert err is not None, (prog.name, "a raise turned into rows", want)
        assert err[0].code == want.code, (prog.name, err[0].code, str(err[0]), want)
        return
    groups = {}
    for i in range(len(want.positions)):
        groups.setdefault(want.columns[0][i], []).append(i)
    expected, total_overflows = {}, False
    for key, rows in groups.items():
        vals = []
        for a, ch, mask in aggs:
            if a == "count_all":
                vals.append(len(rows))
                continue
            xs = [want.columns[ch][i] for i in rows if want.columns[ch][i] is not None and (mask < 0 or want.columns[mask][i])]
            if a == "count":
                vals.append(len(xs))
            elif a == "min_bigint":
                vals.append(min(xs) if xs else None)
            elif a == "sum_bigint":
                total_overflows = total_overflows or not (F.I64_MIN <= sum(xs) <= F.I64_MAX)
                vals.append(sum(xs) if xs else None)
            else:
                order_free = all(float(x * 4).is_integer() and abs(x) < 2.0**40 and not (x == 0 and math.copysign(1.0, x) < 0) for x in xs)
                vals.append((math.fsum(xs) if xs else None) if order_free else "unchecked")
        expected[key] = vals
    if total_overflows:       # sum(bigint): only a group's exact total decides, and one that leaves 64 bits raises
        assert err is not None and err[0].code == F.RANGE, (prog.name, "the total of a group leaves 64 bits", str(err[0]) if err else None)
        return
    assert err is None, (prog.name, str(err[0]) if err else None)
    got = {}
    for o in outs:
        for r in o.rows():
            got[r[0]] = list(r[1:])
    assert sorted(got) == sorted(expected), (prog.name, sorted(got), sorted(expected))
    for key, vals in expected.items():
        for (a, ch, mask), g, w in zip(aggs, got[key], vals):
            if w == "unchecked":
                continue
            t = F.DOUBLE if a == "sum_double" else F.BIGINT
            assert F.bits(t, g) == F.bits(t, w), (prog.name, "key %d" % key, a, ch, mask, g, w)


# ---- the scan operator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,seed", FUSED, ids=["%s%s" % s for s in FUSED])
def test_scan_operator_matches_the_evaluator(pkg, ctx, mode, seed):
    """ScanFilterAndProjectOperator over a page source that hands out the 2049 rows as the cut pages: the same rows, or the same code"""
    prog = F.program(seed, mode)
    full, at, pages = F.page(FULL), 0, []
    for n in CUTS:
        pages.append(pkg.Page(*flat_blocks(pkg, [(t, vals[at:at + n]) for t, vals in full])))
        at += n
    fac = pkg.ScanFilterAndProjectOperatorFactory(ctx, 0, *F.lower(prog, pkg.expressions))
    op = fac.createOperator()
    op.addSplit(pkg.PageSource(pages))
    op.noMoreSplits()
    outs, err = [], None
    try:
        for _ in range(100_000):
            if op.isFinished():
                break
            o = op.getOutput()
            if o is not None:
                if o.position_count > 0:
                    outs.append(o.to_host())
                o.release()
        assert op.isFinished()
    except pkg.TgpuError as e:
        err = (e, None, None)
    op.close()
    fac.close()
    check(prog, outs, err, cut_outcome(prog)[0], "scan", position=False, one_input_page=False)


# ---- a raising operator in every place of a fused plan: ExprProgram::can_raise of csrc/jit.cpp, the one predicate both fused plans ask ----
ROWS, BAD = 65, 40      # one failing row


def _col(bad, good):
    return [bad if i == BAD else good for i in range(ROWS)]


def raising_operators():
    """name -> (tree, {channel: values}, code); channels: 0 key BIGINT, 1 / 2 BIGINT operands, 3 / 4 INTEGER operands, 5 DOUBLE, 6 BOOLEAN mask"""
    B, I, D = F.BIGINT, F.INTEGER, F.DOUBLE
    x, y, xi, yi, d = ("in", 1, B), ("in", 2, B), ("in", 3, I), ("in", 4, I), ("in", 5, D)
    out = {}
    for t, a, b, lo, hi, ca, cb in ((B, x, y, F.I64_MIN, F.I64_MAX, 1, 2), (I, xi, yi, F.I32_MIN, F.I32_MAX, 3, 4)):
        n = "bigint" if t == B else "integer"
        out["add_" + n] = (("call", "ADD", t, (a, b)), {ca: _col(hi, 1), cb: _col(1, 1)}, F.RANGE)
        out["subtract_" + n] = (("call", "SUBTRACT", t, (a, b)), {ca: _col(lo, 1), cb: _col(1, 1)}, F.RANGE)
        out["multiply_" + n] = (("call", "MULTIPLY", t, (a, b)), {ca: _col(hi, 1), cb: _col(2, 2)}, F.RANGE)
        out["divide_" + n] = (("call", "DIVIDE", t, (a, b)), {ca: _col(7, 7), cb: _col(0, 1)}, F.DIV0)
        out["modulus_" + n] = (("call", "MODULUS", t, (a, b)), {ca: _col(7, 7), cb: _col(0, 2)}, F.DIV0)
        out["negate_" + n] = (("call", "NEGATE", t, (a,)), {ca: _col(lo, 1), cb: _col(1, 1)}, F.RANGE)
    out["cast_bigint_integer"] = (("call", "CAST", I, (x,)), {1: _col(2**31, 5)}, F.RANGE)
    out["cast_double_bigint"] = (("call", "CAST", B, (d,)), {5: _col(float("nan"), 1.5)}, F.BADCAST)
    out["cast_double_integer"] = (("call", "CAST", I, (d,)), {5: _col(float("inf"), 1.5)}, F.RANGE)
    return out


MATRIX_TYPES = (F.BIGINT, F.BIGINT, F.BIGINT, F.INTEGER, F.INTEGER, F.DOUBLE, F.BOOLEAN)
PLACES = ["filter", "aggregate_input", "masked_in", "masked_out", "aggregation_drops_it", "join_key", "join_keeps_it", "join_drops_it"]


def matrix_page(columns, mask_at_bad, key_at_bad):
    page = [(F.BIGINT, [key_at_bad if i == BAD else i % 5 for i in range(ROWS)]), (F.BIGINT, [1] * ROWS), (F.BIGINT, [1] * ROWS), (F.INTEGER, [1] * ROWS),
            (F.INTEGER, [1] * ROWS), (F.DOUBLE, [1.5] * ROWS), (F.BOOLEAN, _col(mask_at_bad, True))]
    for ch, vals in columns.items():
        page[ch] = (page[ch][0], vals)
    return page


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", sorted(raising_operators()))
def test_a_raise_never_turns_into_rows(pkg, ctx, name, place):
    """the unfused composition evaluates every projection on every row the filter keeps, so it raises in every one of these places -- also
    where the fused plan would skip the failing row (masked out, no match in the join) or the whole projection (dropped)"""
    tree, columns, code = raising_operators()[name]
    K, X, MASK = ("in", 0, F.BIGINT), ("in", 1, F.BIGINT), ("in", 6, F.BOOLEAN)
    wide = tree if F.type_of(tree) == F.BIGINT else ("call", "CAST", F.BIGINT, (tree,))       # sum / min take a BIGINT
    page = matrix_page(columns, place != "masked_out", 99 if place in ("join_keeps_it", "join_drops_it") else BAD % 5)
    filt = ("call", "NOT", F.BOOLEAN, (("sf", "IS_NULL", F.BOOLEAN, (tree,), None),)) if place == "filter" else None
    if place == "join_key":
        prog = F.Program(name, MATRIX_TYPES, filt, (tree, X))
    elif place.startswith("join"):
        prog = F.Program(name, MATRIX_TYPES, filt, (K, tree, X))
    else:
        prog = F.Program(name, MATRIX_TYPES, filt, (K, X if place == "filter" else wide, MASK, X))
    want = F.run_program(prog, page)
    assert isinstance(want, F.Failure) and want.code == code and want.position == BAD, want       # the composition's answer
    args = F.lower(prog, pkg.expressions)
    blocks = [flat_blocks(pkg, page)]
    if place.startswith("join"):
        kt = F.type_of(prog.projections[0])
        bf = pkg.HashBuilderOperatorFactory(ctx, 0, [kt], [0], [0])
        b = bf.createOperator()
        b.addInput(pkg.Page(pkg.Block(kt, [0, 1, 2, 3, 4, 5, 6, 7])))      # where the key is a column, the failing row's key (99) finds no match
        b.finish()
        fac = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, *args, [0], probe_output_channels=[0, 2] if place == "join_drops_it" else [0, 1])
        outs, err = run(pkg, fac, blocks)
        fac.noMoreOperators()
        b.close()
        fac.close()
        bf.close()
    else:
        aggs = {"filter": [(pkg.SUM_BIGINT, 1)], "aggregate_input": [(pkg.SUM_BIGINT, 1), (pkg.MIN_BIGINT, 1)], "masked_in": [(pkg.SUM_BIGINT, 1, 2)],
                "masked_out": [(pkg.SUM_BIGINT, 1, 2)], "aggregation_drops_it": [(pkg.SUM_BIGINT, 3)]}[place]
        fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, *args, [F.BIGINT], [0], aggs + [(pkg.COUNT_ALL, -1)])
        outs, err = run(pkg, fac, blocks)
        fac.close()
    assert err is not None, (name, place, "a raise turned into rows", [o.rows() for o in outs])
    assert err[0].code == code, (name, place, err[0].code, str(err[0]))


# ---- the fused probe -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["every_output", "outputs_that_cannot_raise"])
@pytest.mark.parametrize("mode,seed", FUSED, ids=["%s%s" % s for s in FUSED])
def test_fused_probe_matches_the_unfused_composition(pkg, mode, seed, outputs):
    """FilterProjectLookupJoinOperatorFactory (inner join, unique build keys) against run_program followed by a plain look-up: projection 0
    is the key (channel 0: -50..50 with NULLs, a NULL key matches nothing), the other fixed-width projections are the probe outputs, the
    build side adds key * 10.  A program that raises must raise the same code, whether the plan was fused or fell back: an output that can
    raise keeps the unfused composition, so the second variant drops those and leaves what the fused kernel itself generates."""
    base = F.program(seed, mode)
    kept = [p for p in base.projections if F.type_of(p) != F.VARCHAR and not (outputs == "outputs_that_cannot_raise" and F.can_raise(p))]
    prog = F.Program(base.name + "_join", base.types, base.filter, ((("in", 0, F.BIGINT),) + tuple(kept))[:7])
    n = 1025
    want = F.run_program(prog, F.page(n))
    keys = list(range(-50, 51, 2))
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    bf = pkg.HashBuilderOperatorFactory(ctx, 0, [F.BIGINT, F.BIGINT], [1], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(F.BIGINT, keys), pkg.Block(F.BIGINT, [k * 10 for k in keys])))
    b.finish()
    fac = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, *F.lower(prog, pkg.expressions), [0])
    outs, err = run(pkg, fac, [flat_blocks(pkg, F.page(n))])
    fac.noMoreOperators()
    b.close()
    fac.close()
    bf.close()
    scopes = fused_scopes(ctx)
    ctx.close()
    if outputs == "outputs_that_cannot_raise":
        assert scopes, (prog.name, "the plan was not fused")
    if isinstance(want, F.Failure):
        assert err is not None, (prog.name, "a raise turned into rows", want)
        assert err[0].code == want.code, (prog.name, err[0].code, str(err[0]), want)
        return
    assert err is None, (prog.name, str(err[0]))
    types = [F.type_of(p) for p in prog.projections] + [F.BIGINT]
    expected = [[col[i] for col in want.columns] + [want.columns[0][i] * 10] for i in range(len(want.positions)) if want.columns[0][i] is not None and want.columns[0][i] % 2 == 0]
    got = [list(r) for o in outs for r in o.rows()]
    as_bits = lambda rows: [[F.bits(t, v) for t, v in zip(types, r)] for r in rows]
    assert as_bits(got) == as_bits(expected), (prog.name, len(got), len(expected))


# ---- the join filter function ------------------------------------------------------------------------------------------------------------------
JOIN_BUILD, JOIN_PROBE = (0, 120), (120, 720)        # rows of the 2049-row page: duplicate build keys (chains), NULL probe keys


@pytest.mark.parametrize("join_type", ["INNER", "PROBE_OUTER"])
@pytest.mark.parametrize("mode,seed", F.JOIN_FILTER_SEEDS, ids=["%s%s" % s for s in F.JOIN_FILTER_SEEDS])
def test_join_filter_function_matches_the_evaluator(pkg, ctx, oracle, mode, seed, join_type):
    """LookupSourceFactory.setJoinFilter with a seeded BOOLEAN tree over (build channels..., probe channels...): the library gathers the
    channels the tree reads at the key-equal candidate pairs, renumbers them and runs a page processor of its own over the candidates.
    Expectation: the candidates in the oracle's order (PagesHash.probe: a key's chain newest -> oldest), `evaluate` on every pair; the
    surviving pairs by their row numbers, a PROBE_OUTER row without one once with a NULL build side, or the code of the first failing
    candidate.  Build key: channel 2 (never NULL), probe key: channel 0."""
    tree = F.join_filter(seed, mode)
    full = F.page(FULL)
    side = lambda lo, hi: [(t, vals[lo:hi]) for t, vals in full] + [(F.BIGINT, list(range(hi - lo)))]
    build, probe = side(*JOIN_BUILD), side(*JOIN_PROBE)
    nb, npr = len(build[0][1]), len(probe[0][1])
    brows = [[vals[i] for _, vals in build] for i in range(nb)]
    prows = [[vals[i] for _, vals in probe] for i in range(npr)]
    cand_p, cand_b = oracle.PagesHash([oracle.Col(F.BIGINT, np.array(build[2][1], dtype=np.int64))]).probe(
        [oracle.Col(F.BIGINT, np.array([0 if v is None else v for v in probe[0][1]], dtype=np.int64), np.array([v is None for v in probe[0][1]], dtype=np.uint8))])
    assert len(cand_p) > 400 and all(prows[p][0] == brows[q][2] for p, q in zip(cand_p, cand_b))
    want, kept = None, {}
    for p, q in zip(cand_p, cand_b):
        try:
            if F.evaluate(tree, brows[q] + prows[p]) is True:
                kept.setdefault(int(p), []).append(int(q))
        except F.ExprError as e:
            want = e.code
            break
    last = len(F.JOIN_TYPES) - 1
    bf = pkg.HashBuilderOperatorFactory(ctx, 0, list(F.JOIN_TYPES), [last], [2])
    bf.lookup_source_factory.setJoinFilter(list(F.JOIN_TYPES), F.to_expr(tree, pkg.expressions))
    b = bf.createOperator()
    b.addInput(pkg.Page(*flat_blocks(pkg, build)))
    b.finish()
    jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, list(F.JOIN_TYPES), [0], probe_output_channels=[last], join_type=getattr(pkg, join_type))
    outs, err = run(pkg, jf, [flat_blocks(pkg, probe)])
    jf.noMoreOperators()
    b.close()
    jf.close()
    bf.close()
    if want is not None:
        assert err is not None, (seed, "a raise turned into rows", want)
        assert err[0].code == want, (seed, err[0].code, str(err[0]), want)
        return
    assert err is None, (seed, str(err[0]) if err else None)
    expected = []
    for p in range(npr):
        expected += [(p, q) for q in kept.get(p, [])] or ([(p, None)] if join_type == "PROBE_OUTER" else [])
    got = [tuple(r) for o in outs for r in o.rows()]
    assert got == expected, (seed, len(got), len(expected), [x for x in zip(got, expected) if x[0] != x[1]][:3])

"""The random expression programs without a GPU: the Python evaluator of expr_fuzz.py against the C oracle (which is pinned on the
reference's own vectors), the conditions the fixed seed lists must meet so that the GPU differential is worth its time, and the
generated source of a sample of the programs through hiprtc for gfx950."""
from collections import Counter

import numpy as np
import pytest

import expr_fuzz as F

FORMS = ("AND", "OR", "IF", "IS_NULL", "COALESCE", "BETWEEN", "IN")
CALLS = F.ARITH + ("NEGATE", "NOT", "CAST") + F.CMPS + F.STRING_OPS
FULL = max(F.ROW_COUNTS)


def roots(p):
    return ([p.filter] if p.filter is not None else []) + list(p.projections)


def oracle_outcome(oracle, E, prog, page):
    """the page processor on the C oracle: o_filter, then o_project per projection over the selected positions"""
    types, filt, projs = F.lower(prog, E)
    flat = E.FlatProgram(filt, projs)
    pool = bytes(flat.pool)

    def col(t, vals):
        if t == F.VARCHAR:
            return oracle.Col(t, vals)
        nulls = np.array([v is None for v in vals], dtype=np.uint8)
        return oracle.Col(t, np.array([0 if v is None else v for v in vals], dtype=oracle._NP[t]), nulls if nulls.any() else None)

    cols = [col(t, vals) for t, vals in page]
    n = len(page[0][1])
    positions = list(range(n))
    if flat.filter_root >= 0:
        try:
            positions = [int(i) for i in oracle.filter_positions(flat.nodes, flat.filter_root, pool, cols)]
        except oracle.OracleError as e:
            return F.Failure(e.code, e.row, "filter")
    if not positions:
        return F.Values([], [[] for _ in projs])
    out = []
    for k, r in enumerate(flat.projection_roots):
        nd = flat.nodes[r]
        if nd["kind"] == 0:
            out.append([page[nd["op"]][1][i] for i in positions])
            continue
        try:
            v, nl = oracle.project(flat.nodes, r, pool, cols, positions)
        except oracle.OracleError as e:
            return F.Failure(e.code, e.row, k)
        conv = float if nd["type"] == F.DOUBLE else (bool if nd["type"] == F.BOOLEAN else int)
        out.append([None if nl[i] else conv(v[i]) for i in range(len(positions))])
    return F.Values(positions, out)


def same(prog, got, want):
    if isinstance(want, F.Failure) or isinstance(got, F.Failure):
        return got == want
    if got.positions != want.positions:
        return False
    return all([F.bits(F.type_of(p), x) for x in g] == [F.bits(F.type_of(p), x) for x in w] for p, g, w in zip(prog.projections, got.columns, want.columns))


@pytest.mark.parametrize("n", [FULL, 64])
def test_evaluator_matches_the_c_oracle(pkg, oracle, n):
    E = pkg.expressions
    checked = 0
    for prog in F.all_programs():
        rewritten, page = F.rewrite_for_oracle(prog, F.page(n))
        assert not any(F.is_stringy(t) for r in roots(rewritten) for t in F.walk(r))
        got = F.run_program(prog, F.page(n))
        want = oracle_outcome(oracle, E, rewritten, page)
        assert same(prog, got, want), (prog.name, got if isinstance(got, F.Failure) else "values", want if isinstance(want, F.Failure) else "values")
        checked += 1
    assert checked == len(F.QUIET_SEEDS) + len(F.LOUD_SEEDS)


def test_evaluator_edges():
    ev = lambda tree, *row: F.evaluate(tree, list(row))
    x = ("in", 0, F.DOUBLE)
    to_big, to_int = ("call", "CAST", F.BIGINT, (x,)), ("call", "CAST", F.INTEGER, (x,))
    assert [ev(to_big, v) for v in (0.5, -0.5, 2.5, -2.5, 0.49999999999999994, 9223372036854774784.0, -2.0**63)] == [1, -1, 3, -3, 0, 9223372036854774784, -2**63]
    assert [ev(to_int, v) for v in (2147483647.49, -2147483648.49, 1.5)] == [2**31 - 1, -2**31, 2]
    for tree, v, code in ((to_big, float("nan"), F.BADCAST), (to_big, float("inf"), F.BADCAST), (to_big, 2.0**63, F.BADCAST), (to_int, float("nan"), F.BADCAST),
                          (to_int, float("inf"), F.RANGE), (to_int, 2147483647.5, F.RANGE), (to_int, -2147483648.5, F.RANGE)):
        with pytest.raises(F.ExprError) as e:
            ev(tree, v)
        assert e.value.code == code, (tree, v)
    a, b = ("in", 0, F.BIGINT), ("in", 1, F.BIGINT)
    div0 = ("call", "DIVIDE", F.BIGINT, (a, ("const", 0, F.BIGINT)))
    ovf = ("call", "MULTIPLY", F.BIGINT, (b, ("const", 2**62, F.BIGINT)))
    gt = lambda t: ("call", "GREATER_THAN", F.BOOLEAN, (t, ("const", 1, F.BIGINT)))
    # the first EVALUATED failure: left before right, a NULL argument skips what follows it
    for form in ("AND", "OR"):
        with pytest.raises(F.ExprError) as e:
            ev(("sf", form, F.BOOLEAN, (gt(div0), gt(ovf)), None), 1, 4)
        assert e.value.code == F.DIV0
    assert ev(("call", "ADD", F.BIGINT, (a, ovf)), None, 4) is None
    assert ev(("sf", "AND", F.BOOLEAN, (("const", False, F.BOOLEAN), gt(div0)), None), 1, 4) is False
    assert ev(("call", "MODULUS", F.BIGINT, (a, b)), -7, 2) == -1 and ev(("call", "DIVIDE", F.BIGINT, (a, b)), -7, 2) == -3
    with pytest.raises(F.ExprError) as e:
        ev(("call", "DIVIDE", F.BIGINT, (a, b)), -2**63, -1)
    assert e.value.code == F.RANGE
    assert ev(("call", "MODULUS", F.BIGINT, (a, b)), -2**63, -1) == 0


def test_page_semantics():
    a = ("in", 0, F.BIGINT)
    div = ("call", "DIVIDE", F.BIGINT, (("const", 7, F.BIGINT), a))
    mul = ("call", "MULTIPLY", F.BIGINT, (a, ("const", 2**62, F.BIGINT)))
    page = [(F.BIGINT, [1, 1, 0, 1, 5, None])]
    run = lambda filt, *projs: F.run_program(F.Program("t", (F.BIGINT,), filt, projs), page)
    assert run(None, mul, div) == F.Failure(F.RANGE, 4, 0)          # projection 0 first, though projection 1 fails on an earlier row
    assert run(None, div, mul) == F.Failure(F.DIV0, 2, 0)
    assert run(("call", "GREATER_THAN", F.BOOLEAN, (div, ("const", 0, F.BIGINT))), mul) == F.Failure(F.DIV0, 2, "filter")
    assert run(("call", "EQUAL", F.BOOLEAN, (a, ("const", 1, F.BIGINT))), a, div, mul) == F.Values([0, 1, 3], [[1, 1, 1], [7, 7, 7], [2**62] * 3])
    assert run(("call", "EQUAL", F.BOOLEAN, (a, ("const", 9, F.BIGINT))), div) == F.Values([], [[]])


def test_the_seed_lists_meet_their_conditions():
    quiet = [F.program(s, "quiet") for s in F.QUIET_SEEDS]
    loud = [F.program(s, "loud") for s in F.LOUD_SEEDS]
    assert len(quiet) >= 24 and len(loud) >= 16
    for p in quiet + loud:
        assert 1 <= len(p.projections) <= F.MAX_PROJ and len(p.types) <= F.MAX_COLS
        assert all(F.height(r) <= F.MAX_DEPTH for r in roots(p))
        assert sum(F.type_of(r) == F.VARCHAR and r[0] != "in" for r in p.projections) <= F.MAX_VARCHAR_PROJ
    # the same subtree in the filter and in projections
    assert sum(any(t[0] != "in" and t[0] != "const" and any(t in set(F.walk(q)) for q in p.projections) for t in F.walk(p.filter)) for p in quiet + loud if p.filter is not None) >= 5
    seen = Counter()
    for p in quiet + loud:
        names = set()
        for r in roots(p):
            names |= F.operators(r)
        seen.update(names)
    assert all(seen[n] >= 3 for n in CALLS + FORMS + ("INPUT", "CONST", "NULL", "IN_NULL", "IN_PLAIN", "LIKE_ESCAPE", "LIKE_PLAIN")), sorted((seen[n], n) for n in CALLS + FORMS)[:5]
    assert all(seen[(op, t)] >= 2 for op in F.ARITH + ("NEGATE",) for t in (F.BIGINT, F.INTEGER, F.DOUBLE))
    assert all(seen[("CMP", t)] >= 2 for t in (F.BIGINT, F.INTEGER, F.DATE, F.DOUBLE, F.BOOLEAN, F.VARCHAR))
    assert all(seen[("COALESCE", k)] >= 2 for k in (1, 2, 3, 4))
    assert all(seen[("CAST",) + pair] >= 2 for pair in F.CAST_PAIRS), [pair for pair in F.CAST_PAIRS if seen[("CAST",) + pair] < 2]
    outcomes = {p.name: F.outcome(p, FULL) for p in quiet + loud}
    assert sum(isinstance(outcomes[p.name], F.Values) for p in quiet) * 3 >= len(quiet) * 2
    cells = [v for o in outcomes.values() if isinstance(o, F.Values) for col in o.columns for v in col]
    nulls = sum(v is None for v in cells)
    assert len(cells) > 100_000 and nulls * 10 >= len(cells) and (len(cells) - nulls) * 10 >= len(cells), (len(cells), nulls)
    codes = Counter(outcomes[p.name].code for p in loud if isinstance(outcomes[p.name], F.Failure))
    assert all(codes[c] >= 3 for c in (F.RANGE, F.DIV0, F.BADCAST)), codes
    # a projection of index >= 1 fails while a later one fails on an earlier row with another code
    full = F.page(FULL)
    rows = [[vals[i] for _, vals in full] for i in range(FULL)]
    crossing = 0
    for p in loud:
        o = outcomes[p.name]
        if not isinstance(o, F.Failure) or o.where == "filter" or o.where < 1:
            continue
        selected = [i for i in range(FULL) if p.filter is None or F.evaluate(p.filter, rows[i])]
        later = [F.first_failure(q, [rows[i] for i in selected]) for q in p.projections[o.where + 1:]]
        crossing += any(f is not None and selected[f[0]] < o.position and f[1] != o.code for f in later)
    assert crossing >= 4, crossing


def test_page_sizes_are_prefixes_with_the_stated_pools():
    full = F.page(FULL)
    assert [t for t, _ in full] == list(F.TYPES) and len(full) <= F.MAX_COLS
    for n in F.ROW_COUNTS:
        assert [vals[:n] for _, vals in full] == [vals for _, vals in F.page(n)]
    assert all(v is not None for v in full[2][1]) and all(v is None for v in full[12][1])
    for ch in (0, 1, 3, 4, 5, 6, 7, 8, 10, 11):
        frac = sum(v is None for v in full[ch][1]) / FULL
        assert 0.1 < frac < 0.2, (ch, frac)
    assert {len(s.encode()) for s in F.EDGE_STRINGS} == {0, 7, 8, 9, 64, 300}
    assert {len(c.encode()) for s in F.EDGE_STRINGS for c in s} == {1, 2, 3, 4}
    assert set(F.bits(F.DOUBLE, v) for v in full[6][1] if v is not None) == set(F.bits(F.DOUBLE, v) for v in F.EDGE_DOUBLES)


COMPILED = [("quiet", s) for s in F.QUIET_SEEDS[:4]] + [("loud", s) for s in F.LOUD_SEEDS[:4]]


@pytest.mark.parametrize("mode,seed", COMPILED, ids=["%s%s" % c for c in COMPILED])
def test_seeded_programs_compile_for_gfx950(pkg, mode, seed):
    """hiprtc cross-compiles without a device; a program the generator of csrc/jit.cpp refuses is an error of expr_fuzz.Generator"""
    pkg.precompile_page_processor(*F.lower(F.program(seed, mode), pkg.expressions))

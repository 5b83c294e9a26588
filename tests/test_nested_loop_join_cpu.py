"""The nested loop join without a GPU: the plain model (nested_loop_expected.py) against the cases of the reference's
TestNestedLoopJoinOperator (tests/golden/nested_loop_join_vectors.json), its tie-break and its re-cut of channel-less build pages; and the
pair filter generator, which compiles through hiprtc here and says which filters it does not fuse."""
import json
import os

import pytest

import expr_fuzz as F
import nested_loop_expected as NL
import seqpages

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nested_loop_join_vectors.json")))
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def golden_pages(types, pages):
    out = []
    for pg in pages:
        if "sequence" in pg:
            cols = seqpages.sequence_page(types, pg["sequence"][0], *pg["sequence"][1:])
            cols = [[v if isinstance(v, str) else int(v) for v in col] for col in cols]
            out.append([tuple(col[i] for col in cols) for i in range(pg["sequence"][0])])
        else:
            out.append([tuple(r) for r in pg["rows"]])
    return out


def test_golden_file_holds_every_case_of_the_reference_test():
    assert len(CASES) == 11   # ten page-level tests, testNestedLoopJoin in both orientations
    assert {c["name"].split("_")[0] for c in GOLDEN["cases"]} == {
        "testNestedLoopJoin", "testColumnReordering", "testCrossJoinWithNullProbe", "testCrossJoinWithNullBuild", "testCrossJoinWithNullOnBothSides",
        "testBuildMultiplePages", "testProbeMultiplePages", "testProbeAndBuildMultiplePages", "testEmptyProbePage", "testEmptyBuildPage"}
    assert [c["expected_total"] for c in GOLDEN["count"]] == [4500, (2**31 - 11) * 45]


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_the_golden_rows_in_order(name):
    c = CASES[name]
    got = NL.reference_rows(golden_pages(c["probe_types"], c["probe_pages"]), golden_pages(c["build_types"], c["build_pages"]), c["probe_channels"], c["build_channels"])
    assert got == [tuple(r) for r in c["expected"]]


@pytest.mark.parametrize("count", GOLDEN["count"], ids=lambda c: c["name"])
def test_model_counts(count):
    pages = NL.reference_pages([count["probe_positions"]], [count["build_positions"]], [], [])
    assert sum(p.positions for p in pages) == count["expected_total"]


def test_a_tie_makes_the_probe_page_large():
    probe, build = [(1,), (2,), (3,)], [("a",), ("b",), ("c",)]
    pages = list(NL.reference_pages([probe], [build], [0], [0]))
    assert [p.rows() for p in pages] == [[(1, s), (2, s), (3, s)] for s in "abc"]
    # ... unless the probe side has no output channel: the build page is repeated (PageRepeatingIterator)
    assert NL.reference_rows([probe], [build], [], [0]) == [("a",), ("b",), ("c",)] * 3
    assert NL.reference_rows([probe], [build], [0], []) == [(1,), (2,), (3,)] * 3
    # one row more on the build side turns the pair round
    assert NL.reference_rows([probe], [build + [("d",)]], [0], [0]) == [(i, s) for i in (1, 2, 3) for s in "abcd"]


def test_zero_channel_build_pages_are_recut_to_8192_positions():
    assert NL.build_side([10_000]) == [8192, 1808]
    assert NL.build_side([5000, 0, 5000, 6384]) == [8192, 8192]
    assert NL.build_side([[], [(1,)], []]) == [[(1,)]]
    probe = [(i,) for i in range(5000)]
    pages = list(NL.reference_pages([probe], [10_000], [0], []))
    # 8192 > 5000: the build page is large, one page of 8192 positions per probe row; 1808 <= 5000: the probe page 1808 times
    assert len(pages) == 5000 + 1808
    assert all(p.positions == 8192 and len(p.probe) == 1 for p in pages[:5000]) and [p.probe[0] for p in pages[:5000]] == probe
    assert all(p.positions == 5000 and p.probe == probe for p in pages[5000:])
    assert sum(p.positions for p in pages) == 5000 * 10_000


def test_filtered_applies_the_program_page_by_page():
    B = F.BIGINT
    lt = ("call", "LESS_THAN", F.BOOLEAN, (("in", 0, B), ("in", 1, B)))
    div = ("call", "DIVIDE", B, (("const", 10, B), ("in", 1, B)))
    prog = F.Program("p", (B, B), lt, (("in", 0, B), div))
    probe, build = [(1,), (5,)], [(3,), (0,), (7,)]
    got = NL.filtered(prog, [probe], [build])
    assert got == F.Values([0, 2, 5], [[1, 1, 5], [3, 1, 1]])   # build large: (1,3) (1,0) (1,7) (5,3) (5,0) (5,7)
    # a failing page ends it: 1 < 2 selects the row whose projection divides by zero -- but only in the page it is in
    bad = NL.filtered(prog, [[(-1,)]], [[(3,)], [(0,)]])
    assert bad == F.Failure(F.DIV0, 0, 1)


def test_pair_filter_source_compiles_without_a_gpu(pkg):
    f, B = pkg.field, pkg.BIGINT
    band = pkg.and_(f(2, B) <= f(0, B), f(0, B) < f(3, B))   # b.lo <= a.x AND a.x < b.hi over probe (x, y), build (lo, hi)
    src = pkg.nested_loop_filter_source([B, B], [B, B], band)
    assert "nlj_pair_count" in src and "nlj_pair_emit" in src and "tg_pair_filter" in src and "__ballot" in src
    # the lane's own row and the wave-uniform row are loaded into registers by one loader per side; the predicate reads registers only
    assert "tg_load_probe" in src and "tg_load_build" in src and "R.c0" in src
    body = src[src.index("tg_pair_filter(const FpArgs& A, const NlRow& R)"):src.index("#define NL_STRIP")]
    assert "[row]" not in body and "col_values" not in body
    pkg.precompile_nested_loop_filter([B, B], [B, B], band)
    pkg.precompile_nested_loop_filter([B, B], [B, B], pkg.between(f(0, B), f(2, B), f(3, B)))


def test_filters_the_generator_does_not_fuse_say_so(pkg):
    f, B, V = pkg.field, pkg.BIGINT, pkg.VARCHAR
    for probe, build, filt, why in [([B], [B], (f(0, B) + f(1, B)) > 3, "can raise"),
                                    ([V], [B], pkg.like(f(0, V), "a%"), "VARCHAR"),
                                    ([V], [V], f(0, V).eq(f(1, V)), "VARCHAR")]:
        with pytest.raises(pkg.TgpuError) as e:
            pkg.nested_loop_filter_source(probe, build, filt)
        assert e.value.code == -8 and "not fused" in str(e.value) and why in str(e.value), str(e.value)

"""NestedLoopBuildOperator + NestedLoopJoinOperator on the device against the reference's own cases (tests/golden/nested_loop_join_vectors.json)
and against the plain model (nested_loop_expected.py) on the shapes at which a wave, a tile or a 16-byte store can go wrong.  The row SEQUENCE
is compared, not a set: the operator must give the rows of the reference's output pages in their order, however it cuts them into pages."""
import pytest

import nested_loop_gpu as G
from nested_loop_gpu import B, D, SIX, V
from test_nested_loop_join_cpu import CASES, GOLDEN, golden_pages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    cx = pkg.Context(0)
    yield cx
    cx.close()


def rows_page(pkg, types, rows):
    return G.page_of(pkg, types, [[r[c] for r in rows] for c in range(len(types))], len(rows))


def drain(op, cap=None):
    """-> the operator's output pages on the host, until it needs input again or has finished"""
    outs = []
    for _ in range(1_000_000):
        o = op.getOutput()
        if o is None:
            if op.needsInput() or op.isFinished():
                break
            continue
        assert o.position_count > 0 and (cap is None or o.position_count <= cap)
        outs.append(o.to_host())
        o.release()
    return outs


@pytest.mark.parametrize("max_rows", [0, 1, 7])
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_with_the_protocol_step_by_step(pkg, ctx, name, max_rows):
    c = CASES[name]
    pt, bt = c["probe_types"], c["build_types"]
    bf = pkg.NestedLoopBuildOperatorFactory(ctx, 1, bt)
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, pt, c["probe_channels"], c["build_channels"], max_output_rows=max_rows)
    bop, jop = bf.createOperator(), jf.createOperator()
    # the probe waits for the build side
    assert jop.isBlocked() and not jop.needsInput() and jop.getOutput() is None and not jop.isFinished()
    assert bop.needsInput() and not bop.isBlocked() and not bop.isFinished()
    for rows in golden_pages(bt, c["build_pages"]):
        bop.addInput(rows_page(pkg, bt, rows))
        assert bop.getOutput() is None and bop.needsInput()
    bop.finish()
    # published: the builder stays, blocked and unfinished, until the probes are done
    assert not bop.needsInput() and bop.isBlocked() and not bop.isFinished() and bop.getOutput() is None
    assert not jop.isBlocked() and jop.needsInput()
    stats = bf.bridge.stats()
    kept = [r for r in golden_pages(bt, c["build_pages"]) if r]
    assert stats["pages"] == len(kept) and stats["positions"] == sum(len(r) for r in kept)
    assert bop.memoryBytes() == stats["bytes"] and (stats["bytes"] > 0) == bool(kept)
    outs = []
    for rows in golden_pages(pt, c["probe_pages"]):
        assert jop.needsInput()
        jop.addInput(rows_page(pkg, pt, rows))
        if rows and kept:
            assert not jop.needsInput() and not jop.isFinished()   # the page still has output to give
        outs += drain(jop, max_rows or None)
        assert jop.needsInput()
    jop.finish()
    assert jop.isFinished() and not jop.needsInput() and not jop.isBlocked() and jop.getOutput() is None
    got = [row for o in outs for row in o.rows()]
    assert got == [tuple(r) for r in c["expected"]]
    jop.close()
    assert bop.isBlocked() and not bop.isFinished()   # the factory may still create operators
    G.end(bf, bop, jf)


def run_join(pkg, ctx, probe_types, probe_pages, build_types, build_pages, probe_channels, build_channels, max_rows=0):
    """pages: per page its columns (or, for a side without types, its position count)"""
    mk = lambda types, pg: G.page_of(pkg, types, pg if types else None, None if types else pg)
    bf, bop = G.build(pkg, ctx, build_types, [mk(build_types, pg) for pg in build_pages])
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, probe_types, probe_channels, build_channels, max_output_rows=max_rows)
    jop = jf.createOperator()
    outs = pkg.to_pages(jop, [mk(probe_types, pg) for pg in probe_pages])
    if max_rows:
        assert all(o.position_count <= max_rows for o in outs)
    jop.close()
    G.end(bf, bop, jf)
    return outs


def check_join(pkg, ctx, probe_types, probe_pages, build_types, build_pages, probe_channels, build_channels, max_rows=0):
    outs = run_join(pkg, ctx, probe_types, probe_pages, build_types, build_pages, probe_channels, build_channels, max_rows)
    size = lambda pg: pg if isinstance(pg, int) else len(pg[0])
    pairs = G.index_pairs([size(p) for p in probe_pages], [size(p) for p in build_pages], probe_channels, build_channels, bool(build_types))
    out_types = [probe_types[c] for c in probe_channels] + [build_types[c] for c in build_channels]
    assert sum(o.position_count for o in outs) == len(pairs)
    got = G.bits_columns(out_types, outs)
    want = G.expected_columns(probe_types, probe_pages, build_types, build_pages, probe_channels, build_channels, pairs)
    for c, (g, w) in enumerate(zip(got, want)):
        if g != w:
            bad = [i for i, (x, y) in enumerate(zip(g, w)) if x != y][:3]
            raise AssertionError(("output channel %d" % c, len(g), len(w), [(i, g[i], w[i]) for i in bad]))


# every (large, small) size in both orientations; S == L is the tie, which makes the probe page large whichever way round
SHAPES = [(L, S, bl) for L in G.LARGE for S in G.SMALL if S <= L for bl in ((False,) if S == L else (False, True))]


@pytest.mark.parametrize("L,S,build_large", SHAPES, ids=["%dx%d_%s" % (L, S, "build_large" if bl else "probe_large") for L, S, bl in SHAPES])
def test_shapes_every_type_on_both_sides(pkg, ctx, L, S, build_large):
    p, b = (S, L) if build_large else (L, S)
    probe, build = G.columns(SIX, p, "some", 1), G.columns(SIX, b, "some", 2)
    check_join(pkg, ctx, SIX, [probe], SIX, [build], list(range(6)), list(range(6)))
    # pieces that end inside a small row's run and inside a 16-byte chunk
    check_join(pkg, ctx, SIX, [probe], SIX, [build], [0, 5, 4], [5, 1, 4], max_rows=999 if L > 64 else 5)


@pytest.mark.parametrize("probe_nulls,build_nulls", [("none", "none"), ("some", "all"), ("all", "some"), ("none", "some"), ("all", "all")])
@pytest.mark.parametrize("p,b", [(65, 3), (3, 65), (64, 64), (257, 64)])
def test_null_vectors(pkg, ctx, p, b, probe_nulls, build_nulls):
    check_join(pkg, ctx, SIX, [G.columns(SIX, p, probe_nulls, 1)], SIX, [G.columns(SIX, b, build_nulls, 2)], list(range(6)), list(range(6)), max_rows=1000)


def test_no_null_vector_without_nulls(pkg, ctx):
    outs = run_join(pkg, ctx, [B, V], [G.columns([B, V], 70, "none")], [D], [G.columns([D], 5, "some")], [0, 1], [0])
    assert all(o.getBlock(0).nulls is None and o.getBlock(1).nulls is None and o.getBlock(2).nulls is not None for o in outs)


@pytest.mark.parametrize("probe_channels,build_channels", [([0, 0, 1], [2, 2]), ([5, 3, 0], [4, 5, 1, 0]), ([], [0, 5]), ([1, 5], []), ([], [])])
@pytest.mark.parametrize("p,b", [(65, 3), (3, 65), (64, 64)])
def test_channel_lists(pkg, ctx, p, b, probe_channels, build_channels):
    for max_rows in (0, 50):
        check_join(pkg, ctx, SIX, [G.columns(SIX, p, "some", 1)], SIX, [G.columns(SIX, b, "some", 2)], probe_channels, build_channels, max_rows)


def test_three_probe_pages_by_three_build_pages_with_empty_ones(pkg, ctx):
    probe = [G.columns(SIX, n, "some", n) for n in (65, 0, 2, 130)]
    build = [G.columns(SIX, n, "some", n + 1) for n in (0, 64, 3, 0, 131)]
    check_join(pkg, ctx, SIX, probe, SIX, build, [0, 5, 3], [5, 4, 0])
    check_join(pkg, ctx, SIX, probe, SIX, build, [5], [0], max_rows=100)


def test_zero_channel_build_side_is_counted_and_recut(pkg, ctx):
    probe = [G.columns([B, V], 70, "some", 1)]
    # 8192 + 8: the first kept page is larger than the probe page (one run per probe row), the remainder is smaller (the probe page 8 times)
    bf, bop = G.build(pkg, ctx, [], [pkg.Page(position_count=n) for n in (5000, 0, 3200)])
    assert bf.bridge.stats() == dict(pages=2, positions=8200, bytes=0)
    G.end(bf, bop)
    check_join(pkg, ctx, [B, V], probe, [], [5000, 0, 3200], [1, 0], [], max_rows=100_000)


def test_dictionary_and_rle_input_blocks(pkg, ctx):
    flat = G.columns([B, V, D], 6, "some", 4)
    ids = [5, 0, 0, 3, 2, 5, 1, 4, 4, 2] * 7
    probe_blocks = [pkg.DictionaryBlock(pkg.Block(t, list(c)), ids) for t, c in zip([B, V, D], flat)]
    rle = [pkg.RunLengthEncodedBlock(pkg.Block(V, ["é漢 run"]), 3), pkg.RunLengthEncodedBlock(pkg.Block(B, [None]), 3)]
    bf, bop = G.build(pkg, ctx, [V, B], [pkg.Page(*rle)])
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, [B, V, D], [0, 1, 2], [0, 1])
    jop = jf.createOperator()
    outs = pkg.to_pages(jop, [pkg.Page(*probe_blocks)])
    jop.close()
    G.end(bf, bop, jf)
    probe_cols = [[c[i] for i in ids] for c in flat]
    pairs = G.index_pairs([70], [3], True, True)
    want = G.expected_columns([B, V, D], [probe_cols], [V, B], [[["é漢 run"] * 3, [None] * 3]], [0, 1, 2], [0, 1], pairs)
    assert G.bits_columns([B, V, D, V, B], outs) == want


@pytest.mark.parametrize("count", GOLDEN["count"], ids=lambda c: c["name"])
def test_count(pkg, ctx, count):
    """testCount: pages without channels on both sides; (2^31 - 11) * 45 positions come out as counts, no device memory grows"""
    bf, bop = G.build(pkg, ctx, [], [pkg.Page(position_count=count["build_positions"])])
    assert bf.bridge.stats()["positions"] == count["build_positions"] and bop.memoryBytes() == 0
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, [], [], [], max_output_rows=2**31 - 1)
    jop = jf.createOperator()
    jop.addInput(pkg.Page(position_count=count["probe_positions"]))
    total, pages = 0, 0
    while not jop.needsInput():
        o = jop.getOutput()
        assert o is not None and 0 < o.position_count <= 2**31 - 1 and o.channel_count == 0
        assert jop.memoryBytes() == 0
        total += o.position_count
        pages += 1
        o.release()
    assert total == count["expected_total"] and pages <= 46
    jop.finish()
    assert jop.isFinished()
    jop.close()
    G.end(bf, bop, jf)


def test_output_pages_stay_on_the_device_for_the_next_operator(pkg, ctx):
    p, b = 300, 70
    bf, bop = G.build(pkg, ctx, [B], [G.page_of(pkg, [B], G.columns([B], b, "none"))])
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, [B], [0], [0], max_output_rows=4096)
    jop = jf.createOperator()
    outs = pkg.to_pages(jop, [G.page_of(pkg, [B], G.columns([B], p, "none"))], to_host=False)
    assert len(outs) > 1
    af = pkg.HashAggregationOperatorFactory(ctx, 3, [], [], [(pkg.COUNT_ALL, -1)])
    aop = af.createOperator()
    res = pkg.to_pages(aop, outs)
    for o in outs:
        o.release()
    assert [r[0] for pg in res for r in pg.rows()] == [p * b]
    aop.close()
    af.close()
    jop.close()
    G.end(bf, bop, jf)


def test_lifecycle_duplicate_two_probes_close_before_drain(pkg, ctx):
    probe, build = G.columns([B], 5, "none", 1), G.columns([B], 3, "none", 2)
    bf, bop = G.build(pkg, ctx, [B], [G.page_of(pkg, [B], build)])
    jf = pkg.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, [B], [0], [0], max_output_rows=4)
    dup = jf.duplicate()
    a, b2, c = jf.createOperator(), jf.createOperator(), dup.createOperator()
    want = G.expected_columns([B], [probe], [B], [build], [0], [0], G.index_pairs([5], [3], True, True))
    for op in (a, c):
        assert G.bits_columns([B, B], pkg.to_pages(op, [G.page_of(pkg, [B], probe)])) == want
    # closed with output still to give: clean, and it counts as done
    b2.addInput(G.page_of(pkg, [B], probe))
    first = b2.getOutput()
    assert first.position_count == 4 and not b2.needsInput() and not b2.isFinished()
    first.release()
    b2.close()
    a.close()
    jf.noMoreOperators()
    assert bop.isBlocked() and not bop.isFinished()   # the duplicate's operator is open and its factory may create more
    c.close()
    assert bop.isBlocked() and not bop.isFinished()
    dup.noMoreOperators()
    assert bop.isFinished() and not bop.isBlocked() and bop.memoryBytes() == 0
    bop.close()
    for h in (dup, jf, bf.bridge, bf):
        h.close()


def test_a_second_build_operator_cannot_publish(pkg, ctx):
    bf = pkg.NestedLoopBuildOperatorFactory(ctx, 1, [B])
    first, second = bf.createOperator(), bf.createOperator()
    first.addInput(G.page_of(pkg, [B], [[1, 2]]))
    second.addInput(G.page_of(pkg, [B], [[3]]))
    first.finish()
    with pytest.raises(pkg.TgpuError) as e:
        second.finish()
    assert e.value.code == -5 and "pagesFuture already set" in str(e.value)
    assert bf.bridge.stats()["positions"] == 2
    with pytest.raises(pkg.TgpuError):
        bf.duplicate()
    second.close()
    first.close()
    bf.bridge.close()
    bf.close()
    # the context is still usable
    check_join(pkg, ctx, [B], [G.columns([B], 2, "none")], [B], [G.columns([B], 2, "none")], [0], [0])


def test_an_empty_build_side_gives_nothing(pkg, ctx):
    assert run_join(pkg, ctx, [B], [G.columns([B], 4, "none")], [B], [], [0], [0]) == []
    assert run_join(pkg, ctx, [B], [G.columns([B], 4, "none")], [], [0], [0], []) == []

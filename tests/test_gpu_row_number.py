"""RowNumberOperator on the GPU: the reference's TestRowNumberOperator data cases (tests/golden/row_number_vectors.json), random streams of every key
type against the oracle's GroupByHash plus the reference's two loops (tests/row_number_expected.py), a ladder of group counts on both sides of the
LDS / sort threshold, counts carried across the switch between the two paths, saturation at the limit, the operator without partition channels,
the equivalence RowNumber -> Filter(rn <= 3) == RowNumber(max = 3), block encodings, channel selection and the protocol.  Every comparison is
exact: values, nulls, page boundaries and which pages are absent."""
import json
import os

import numpy as np
import pytest

from distinct_gpu import DOMAINS, KEY_SPECS, key_block, key_cols, key_pages, with_hash
from row_number_expected import RowNumberOracle

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "row_number_vectors.json")))
ROW_NUMBER_CASES = [c for c in GOLD["cases"] if c["operator"] == "row_number"]
PAGE_SIZES = [1, 63, 64, 65, 255, 257, 1023, 1025, 4097]
MAXES = [None, 0, 1, 3, 1000]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def drive(op, pages):
    """per page the operator takes: its output page on the host, or None; stops offering pages when needsInput turns false"""
    outs = []
    for p in pages:
        if not op.needsInput():
            break
        assert not op.isFinished()
        op.addInput(p)
        assert not op.needsInput() or op.getOutput() is None   # one page at a time: a pending result blocks the next page
        o = op.getOutput()
        assert op.getOutput() is None
        if o is None:
            outs.append(None)
        else:
            outs.append(o.to_host())
            o.release()
    return outs


def same_cells(pkg, got, want, positions):
    """block `got` == the rows `positions` of block `want`, nulls included; fixed-width values bit for bit (NaN, -0.0)"""
    want = want.flatten()
    got = got.flatten()
    assert got.type == want.type
    if want.type == pkg.VARCHAR:
        w = want.to_list()
        assert got.to_list() == [w[i] for i in positions]
        return
    idx = np.asarray(positions, dtype=np.int64)
    wn = np.zeros(len(idx), dtype=bool) if want.nulls is None else want.nulls[idx].astype(bool)
    gn = np.zeros(len(idx), dtype=bool) if got.nulls is None else got.nulls.astype(bool)
    assert np.array_equal(gn, wn)
    a, b = np.ascontiguousarray(got.values[~gn]), np.ascontiguousarray(want.values[idx][~wn])
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(pkg, oracle, types, output_channels, partition_channels, max_rows, pages, outs):
    """outs against the reference's loops over the helper's group ids; returns (rows produced, the helper)"""
    o = RowNumberOracle(oracle, [types[c] for c in partition_channels], max_rows)
    taken, total = 0, 0
    for page in pages:
        if o.finished_early():
            break
        n = page.getPositionCount()
        want = o.page(key_cols(oracle, page, partition_channels), n)
        assert taken < len(outs)
        got = outs[taken]
        taken += 1
        if want is None:
            assert got is None   # no output page for a page that keeps no row
            continue
        positions, numbers = want
        assert got is not None and got.getPositionCount() == len(positions)
        assert got.getChannelCount() == len(output_channels) + 1
        rn = got.getBlock(len(output_channels))
        assert rn.type == pkg.BIGINT and (rn.nulls is None or not rn.nulls.any())
        assert np.array_equal(rn.values, np.asarray(numbers, dtype=np.int64)), np.nonzero(rn.values != np.asarray(numbers, dtype=np.int64))[0][:10]
        for i, ch in enumerate(output_channels):
            same_cells(pkg, got.getBlock(i), page.getBlock(ch), positions)
        total += len(positions)
    assert taken == len(outs)
    return total, o


def run(pkg, ctx, oracle, types, output_channels, partition_channels, max_rows, pages, hash_channel=-1, expected_positions=10):
    op = pkg.RowNumberOperatorFactory(ctx, 1, types, output_channels, partition_channels, max_rows, hash_channel, expected_positions).createOperator()
    outs = drive(op, pages)
    total, _ = check(pkg, oracle, types, output_channels, partition_channels, max_rows, pages, outs)
    return op, total, outs


def finish(op):
    op.finish()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()


def bigint_pages(pkg, key_arrays):
    """(types, pages): channel 0 = the BIGINT key, channel 1 = a DOUBLE payload that tells the rows apart"""
    pages, at = [], 0
    for k in key_arrays:
        k = np.asarray(k, dtype=np.int64)
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, k), pkg.Block(pkg.DOUBLE, np.arange(at, at + len(k), dtype=np.float64))))
        at += len(k)
    return [pkg.BIGINT, pkg.DOUBLE], pages


# ---- 1. the reference's cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, hash_enabled", [(c, h) for c in ROW_NUMBER_CASES for h in ((False, True) if c["hash_parametrised"] else (False,))],
                         ids=lambda v: v["name"] if isinstance(v, dict) else ("hash" if v else "nohash"))
def test_reference_cases(pkg, ctx, oracle, case, hash_enabled):
    types = [getattr(pkg, t) for t in case["types"]]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.array([r[0] for r in p], dtype=np.int64)), pkg.Block(pkg.DOUBLE, np.array([r[1] for r in p], dtype=np.float64)))
             for p in case["pages"]]
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, case["partition_channels"]) for p in pages], len(types), types + [pkg.BIGINT]
    op, total, outs = run(pkg, ctx, oracle, types, case["output_channels"], case["partition_channels"], case["max_rows_per_partition"], pages, hc,
                          case["expected_positions"])
    rows = [tuple(r[:-1]) for o in outs if o is not None for r in o.rows()]
    numbers = [r[-1] for o in outs if o is not None for r in o.rows()]
    assert len(numbers) == case["row_number_count"] == total
    if case["max_row_number"] is not None:
        assert max(numbers) <= case["max_row_number"]
    for s in case["row_sets"]:
        assert len({tuple(r) for r in s["rows"]} & set(rows)) == s["intersection"]
    op.close()


# ---- 2. random streams against the helper -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_enabled", [False, True])
@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("spec", KEY_SPECS, ids=[s[0] for s in KEY_SPECS])
def test_random_streams_match_helper(pkg, ctx, oracle, spec, domain, hash_enabled):
    name, type_names, null_frac = spec
    rng = np.random.default_rng(5000 + 10 * [s[0] for s in KEY_SPECS].index(name) + list(DOMAINS).index(domain))
    sizes = [int(s) for s in rng.choice(PAGE_SIZES, 3)]
    types, pages = key_pages(pkg, rng, type_names, DOMAINS[domain], null_frac, sizes)
    channels = list(range(len(types)))
    pages = [p.appendColumn(pkg.Block(pkg.BIGINT, np.arange(p.getPositionCount(), dtype=np.int64))) for p in pages]   # a payload channel
    types = types + [pkg.BIGINT]
    outputs = list(range(len(types)))
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, channels) for p in pages], len(types), types + [pkg.BIGINT]
    rows = sum(sizes)
    for max_rows in MAXES:
        op, total, outs = run(pkg, ctx, oracle, types, outputs, channels, max_rows, pages, hc)
        assert len(outs) == 3 and op.needsInput() and not op.isFinished()   # a partitioned operator never finishes early
        if max_rows is None:
            assert total == rows
        if max_rows == 0:
            assert outs == [None, None, None]
        finish(op)


@pytest.mark.parametrize("groups", [7, 1500, 40_000])
def test_a_page_of_several_blocks_and_chunks(pkg, ctx, oracle, groups):
    """70 001 rows: several workgroups and several 64-row steps per wave take part, behind a small page that seeds the counts"""
    rng = np.random.default_rng(groups)
    types, pages = bigint_pages(pkg, [rng.integers(0, groups, 300), rng.integers(0, groups, 70_001)])
    for max_rows in (None, 3):
        op, total, outs = run(pkg, ctx, oracle, types, [1, 0], [0], max_rows, pages)
        finish(op)


# ---- 3. group-count ladder ---------------------------------------------------------------------------------------------------------------
def ladder_keys(pattern, groups, rng):
    n = max(3001, groups + 777)
    if pattern == "one_group":
        return [np.full(n, 42), np.full(n, 42), np.full(n, 42)]
    if pattern == "distinct":   # every row of the stream a group of its own
        m = max(groups, 1)
        return [np.arange(k * m, (k + 1) * m) * 3 for k in range(3)]
    if pattern == "sorted_runs":
        return [np.sort(rng.integers(0, groups, n)) for _ in range(3)]
    if pattern == "interleave":
        return [np.arange(n) % groups, (np.arange(n) + 5) % groups, np.arange(n) % groups]
    if pattern == "absent_then_back":   # the first half of the groups sits out page 1
        half = max(1, groups // 2)
        return [np.arange(n) % groups, half + np.arange(n) % max(1, groups - half) if groups > 1 else np.full(n, 999), np.arange(n) % groups]
    raise ValueError(pattern)


@pytest.mark.parametrize("pattern", ["one_group", "distinct", "sorted_runs", "interleave", "absent_then_back"])
@pytest.mark.parametrize("groups", [1, 2, 3, 64, 65, 1000, 5000, 70_000])
def test_group_count_ladder(pkg, ctx, oracle, groups, pattern):
    """three pages each, so that carried counts matter; 70 000 groups need a 17-bit sort key; 1000 / 5000 sit on either side of any threshold
    in 1024..4096"""
    rng = np.random.default_rng(100 + groups)
    types, pages = bigint_pages(pkg, ladder_keys(pattern, groups, rng))
    for max_rows in (None, 3):
        op, total, outs = run(pkg, ctx, oracle, types, [1, 0], [0], max_rows, pages)
        assert len(outs) == 3
        finish(op)


# ---- 4. counts carried across the switch of paths ------------------------------------------------------------------------------------------
LDS, SORT = "row_number_lds", "row_number_sort"


def ranking_scopes(ctx, fn):
    """(fn(), the ranking scopes the profile saw while fn ran): which of the two paths the pages took"""
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        result = fn()
        ctx.synchronize()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    return result, {k for k, v in prof.items() if k in (LDS, SORT) and v["count"] > 0}


def drive_with_paths(ctx, op, pages):
    """drive() page by page + the ranking path every page took"""
    outs, paths = [], []
    for p in pages:
        got, scopes = ranking_scopes(ctx, lambda: drive(op, [p]))
        outs.extend(got)
        paths.append(scopes)
    return outs, paths


@pytest.mark.parametrize("max_rows", [None, 3, 40])
def test_group_count_grows_across_the_threshold(pkg, ctx, oracle, max_rows):
    """100 groups, then 1500, 5000 and 10 000: the early pages take the LDS path, the late ones the sort path, and a last small page of old
    groups (the group count stays at 10 000: sort path) still sees every count"""
    rng = np.random.default_rng(77)
    keys = [rng.integers(0, g, n) for g, n in ((100, 5000), (1500, 9000), (5000, 20_000), (10_000, 30_000))] + [rng.integers(0, 100, 700)]
    types, pages = bigint_pages(pkg, keys)
    op = pkg.RowNumberOperatorFactory(ctx, 1, types, [1, 0], [0], max_rows).createOperator()
    outs, paths = drive_with_paths(ctx, op, pages)
    assert paths == [{LDS}, {LDS}, {SORT}, {SORT}, {SORT}]   # 100 and 1500 groups <= the threshold < 5000
    check(pkg, oracle, types, [1, 0], [0], max_rows, pages, outs)
    assert len(outs) == 5
    finish(op)


@pytest.mark.parametrize("max_rows", [None, 3])
@pytest.mark.parametrize("groups", [1, 4, 1000])
def test_forced_sort_path_with_few_groups(pkg, ctx, oracle, groups, max_rows):
    """TGPU_ROW_NUMBER_PATH=sort (read when the operator is created): the measurement tool's baseline.  One group sorts on a 1-bit key."""
    rng = np.random.default_rng(groups)
    types, pages = bigint_pages(pkg, [rng.integers(0, groups, n) for n in (3001, 65, 5000)])
    os.environ["TGPU_ROW_NUMBER_PATH"] = "sort"
    try:
        op = pkg.RowNumberOperatorFactory(ctx, 1, types, [1, 0], [0], max_rows).createOperator()
    finally:
        del os.environ["TGPU_ROW_NUMBER_PATH"]
    outs, paths = drive_with_paths(ctx, op, pages)
    assert paths == [{SORT}] * 3
    check(pkg, oracle, types, [1, 0], [0], max_rows, pages, outs)
    finish(op)
    op = pkg.RowNumberOperatorFactory(ctx, 1, types, [1, 0], [0], max_rows).createOperator()   # without the variable: by group count
    outs, paths = drive_with_paths(ctx, op, pages[:1])
    assert paths == [{LDS}]
    finish(op)


# ---- 5. saturation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [LDS, SORT])
def test_saturation_with_max_3(pkg, ctx, oracle, path):
    """LDS path (504 filler groups, at most 509 groups in all): page 0 has 5000 rows = 12 waves of 448-row chunks (ceil(5000 / 512) = 10
    waves rounded up to 3 blocks of 4; ceil(5000 / 12) = 417 rows rounded up to 7 steps of 64), so wave w owns rows [448 w, 448 w + 448)
    and walks them in steps of 64 from 448 w.  The marked groups reach 3 inside one 64-row step, in the middle of a chunk, across steps
    and across chunks.  Sort path: every filler row a group of its own (5000 groups), the same marked rows."""
    n = 5000
    filler = 1_000_000 + (np.arange(n) % 504 if path == LDS else np.arange(n))
    page0 = filler.copy()
    page0[[10, 20, 30, 40, 50]] = 7            # all in wave 0's first step: the third row sits in the middle of the 64 lanes
    page0[[600, 700, 800, 900, 2000]] = 8      # third row in the middle of chunk 1 (rows 448..895), two more in chunks 2 and 4
    page0[[63, 64, 127, 128]] = 9              # steps 0, 1, 1, 2 of chunk 0
    page0[[447, 448, 895, 896]] = 10           # chunks 0, 1, 1, 2
    page1 = np.repeat([7, 8, 9, 10], 1000)     # every group saturated, over several chunks and blocks
    page2 = np.concatenate([np.full(10, 7), np.full(200, 11), np.full(5, 8)])     # a new group still gets 1, 2, 3
    types, pages = bigint_pages(pkg, [page0, page1, page2])
    op = pkg.RowNumberOperatorFactory(ctx, 1, types, [1, 0], [0], 3).createOperator()
    outs = []
    for p in pages:
        assert op.needsInput()
        got, scopes = ranking_scopes(ctx, lambda: drive(op, [p]))
        assert scopes == {path}
        outs.extend(got)
        assert op.needsInput() and not op.isFinished()   # also after the page that produced nothing
    check(pkg, oracle, types, [1, 0], [0], 3, pages, outs)
    assert outs[1] is None
    keys0 = outs[0].getBlock(1).values
    for key, rows in ((7, [10, 20, 30]), (8, [600, 700, 800]), (9, [63, 64, 127]), (10, [447, 448, 895])):
        assert outs[0].getBlock(0).values[keys0 == key].tolist() == [float(r) for r in rows]   # the payload is the row's position
        assert outs[0].getBlock(2).values[keys0 == key].tolist() == [1, 2, 3]
    assert outs[2].getBlock(1).values.tolist() == [11, 11, 11] and outs[2].getBlock(2).values.tolist() == [1, 2, 3]
    finish(op)


# ---- 6. no partition channels ------------------------------------------------------------------------------------------------------------
def test_unpartitioned_numbers_continue_across_pages(pkg, ctx, oracle):
    rng = np.random.default_rng(3)
    types, pages = bigint_pages(pkg, [rng.integers(0, 9, n) for n in (1, 65, 4097, 0, 300)])
    op, total, outs = run(pkg, ctx, oracle, types, [1, 0], [], None, pages)
    assert total == 4463 and outs[3].getPositionCount() == 0
    assert outs[4].getBlock(2).values.tolist() == list(range(4164, 4464))
    assert op.needsInput() and not op.isFinished() and op.memoryBytes() > 0
    finish(op)


def test_unpartitioned_limit_cuts_the_crossing_page(pkg, ctx, oracle):
    types, pages = bigint_pages(pkg, [np.arange(100), np.arange(100), np.arange(100)])
    pages = [p.appendColumn(pkg.Block(pkg.VARCHAR, [None if i % 7 == 0 else "v%d" % i for i in range(100)])) for p in pages]
    types = types + [pkg.VARCHAR]
    op, total, outs = run(pkg, ctx, oracle, types, [2, 0], [], 130, pages)
    assert total == 130 and len(outs) == 2 and outs[1].getPositionCount() == 30   # the third page is not taken
    assert outs[1].getBlock(2).values.tolist() == list(range(101, 131))
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()


def test_unpartitioned_limit_reached_at_a_page_end_and_limit_0(pkg, ctx, oracle):
    types, pages = bigint_pages(pkg, [np.arange(5), np.arange(5)])
    op, total, outs = run(pkg, ctx, oracle, types, [0], [], 5, pages)
    assert total == 5 and len(outs) == 1 and op.isFinished() and not op.needsInput()
    op.close()
    op = pkg.RowNumberOperatorFactory(ctx, 1, types, [0], [], 0).createOperator()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None   # finished at once
    op.close()
    op = pkg.RowNumberOperatorFactory(ctx, 1, types, [0], [], 9).createOperator()   # finish() before the limit
    outs = drive(op, pages[:1])
    assert outs[0].getPositionCount() == 5 and op.needsInput() and not op.isFinished()
    finish(op)


# ---- 7. RowNumber -> Filter(rn <= 3) == RowNumber(max = 3) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [40, 6000])
def test_filter_on_the_row_number_equals_the_limit(pkg, ctx, oracle, groups):
    f, B, D = pkg.field, pkg.BIGINT, pkg.DOUBLE
    rng = np.random.default_rng(groups)
    types, pages = bigint_pages(pkg, [rng.integers(0, groups, n) for n in (3000, 9000, 2000)])
    numberer = pkg.RowNumberOperatorFactory(ctx, 1, types, [1, 0], [0]).createOperator()
    numbered = pkg.to_pages(numberer, pages, to_host=False)   # device-resident OutputPages
    keep = pkg.FilterAndProjectOperatorFactory(ctx, 2, [D, B, B], f(2, B) <= 3, [f(0, D), f(1, B), f(2, B)]).createOperator()
    filtered = pkg.to_pages(keep, numbered)
    for o in numbered:
        o.release()
    limited = pkg.RowNumberOperatorFactory(ctx, 3, types, [1, 0], [0], 3).createOperator()
    direct = pkg.to_pages(limited, pages)
    assert [p.rows() for p in filtered if p.getPositionCount()] == [p.rows() for p in direct]
    assert sum(p.getPositionCount() for p in direct) > 0
    for op in (numberer, keep, limited):
        op.close()


def test_device_resident_input_with_limit(pkg, ctx, oracle):
    f, B, D = pkg.field, pkg.BIGINT, pkg.DOUBLE
    rng = np.random.default_rng(8)
    types, pages = bigint_pages(pkg, [rng.integers(0, 50, n) for n in (3000, 2000)])
    head = pkg.FilterAndProjectOperatorFactory(ctx, 10, types, None, [f(0, B), f(1, D)]).createOperator()
    resident = pkg.to_pages(head, pages, to_host=False)
    for max_rows in (None, 2):
        op = pkg.RowNumberOperatorFactory(ctx, 11, types, [1], [0], max_rows).createOperator()
        outs = drive(op, resident)
        check(pkg, oracle, types, [1], [0], max_rows, pages, outs)
        finish(op)
    for o in resident:
        o.release()
    head.close()


# ---- 8. encodings, empty pages, channel selection ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rows", [None, 2])
@pytest.mark.parametrize("type_name", ["BIGINT", "DOUBLE", "VARCHAR"])
def test_dictionary_and_rle_blocks(pkg, ctx, oracle, type_name, max_rows):
    rng = np.random.default_rng(19)
    t = getattr(pkg, type_name)
    dictionary = pkg.DictionaryBlock(key_block(pkg, rng, t, 40, 30, 0.1), rng.integers(0, 40, 2000).astype(np.int32))
    payload_dictionary = pkg.DictionaryBlock(key_block(pkg, rng, pkg.VARCHAR, 10, 10, 0.2), rng.integers(0, 10, 2000).astype(np.int32))
    rle = pkg.RunLengthEncodedBlock(pkg.Block(t, [dictionary.flatten().get(3)]), 500)
    payload_rle = pkg.RunLengthEncodedBlock(pkg.Block(pkg.VARCHAR, ["same"]), 500)
    pages = [pkg.Page(dictionary, payload_dictionary), pkg.Page(rle, payload_rle), pkg.Page(key_block(pkg, rng, t, 1000, 60, 0.1), key_block(pkg, rng, pkg.VARCHAR, 1000, 5, 0.1))]
    op, total, outs = run(pkg, ctx, oracle, [t, pkg.VARCHAR], [0, 1], [0], max_rows, pages)
    finish(op)


@pytest.mark.parametrize("max_rows", [None, 2])
def test_zero_row_page(pkg, ctx, oracle, max_rows):
    types, pages = bigint_pages(pkg, [[4, 4, 5], [], [4, 5, 5, 6]])
    op, total, outs = run(pkg, ctx, oracle, types, [0, 1], [0], max_rows, pages)
    if max_rows is None:
        assert outs[1].getPositionCount() == 0 and outs[1].getChannelCount() == 3
    else:
        assert outs[1] is None
    finish(op)


@pytest.mark.parametrize("max_rows", [None, 2])
@pytest.mark.parametrize("outputs", [[2, 0, 1], [2], [], [1, 1]])
def test_output_channels_reordered_and_subset(pkg, ctx, oracle, outputs, max_rows):
    """always len(outputChannels) + 1 channels, never the input's channel count + 1"""
    rng = np.random.default_rng(41)
    n = 1025
    page = pkg.Page(key_block(pkg, rng, pkg.VARCHAR, n, 6, 0.1), pkg.Block(pkg.DOUBLE, rng.random(n)), key_block(pkg, rng, pkg.INTEGER, n, 5, 0.1))
    types = [pkg.VARCHAR, pkg.DOUBLE, pkg.INTEGER]
    op, total, outs = run(pkg, ctx, oracle, types, outputs, [2, 0], max_rows, [page, page])
    assert all(o.getChannelCount() == len(outputs) + 1 for o in outs if o is not None)
    assert [outs[0].getBlock(i).type for i in range(len(outputs))] == [types[c] for c in outputs]
    finish(op)


# ---- 9. protocol -------------------------------------------------------------------------------------------------------------------------
def test_protocol_memory_and_duplicate(pkg, ctx):
    f = pkg.RowNumberOperatorFactory(ctx, 1, [pkg.BIGINT], [0], [0], 2)
    f2 = f.duplicate()
    a, b = f.createOperator(), f2.createOperator()
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array([4, 4, 9, 4, 1], dtype=np.int64)))
    for op in (a, b):   # independent hashes and counts
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None
        op.addInput(page)
        assert not op.needsInput() and not op.isFinished()   # a page is pending
        with pytest.raises(pkg.TgpuError):
            op.addInput(page)
        o = op.getOutput()
        assert o.to_host().rows() == [(4, 1), (4, 2), (9, 1), (1, 1)]
        o.release()
        assert op.needsInput() and not op.isFinished() and op.memoryBytes() > 0
    a.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.array([4, 4], dtype=np.int64))))   # saturated: no output page, the next page is taken at once
    assert a.getOutput() is None and a.needsInput()
    a.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.array([9], dtype=np.int64))))
    a.finish()
    assert not a.isFinished() and not a.needsInput()   # finishing with a page pending
    o = a.getOutput()
    assert o.to_host().rows() == [(9, 2)]
    o.release()
    assert a.isFinished()
    with pytest.raises(pkg.TgpuError):
        a.addInput(page)
    for op in (a, b):
        op.close()


@pytest.mark.parametrize("types, outputs, partitions, max_rows, hash_channel, expected_positions", [
    ([1], [1], [0], None, -1, 10), ([1], [-1], [0], None, -1, 10), ([1], [0], [1], None, -1, 10), ([1], [0], [-1], None, -1, 10),
    ([1, 1], [0], [], None, 1, 10), ([1, 1], [0], [0], None, 2, 10), ([1, 2], [0], [0], None, 1, 10), ([1], [0], [0], -2, -1, 10),
    ([1], [0], [0], 3, -1, 0), ([], [], [], None, -1, 10)])
def test_factory_argument_errors(pkg, ctx, types, outputs, partitions, max_rows, hash_channel, expected_positions):
    with pytest.raises(pkg.TgpuError) as e:
        pkg.RowNumberOperatorFactory(ctx, 1, types, outputs, partitions, max_rows, hash_channel, expected_positions)
    assert e.value.code == -1   # TGPU_ERR_INVALID_ARGUMENT


def test_max_rows_0_is_legal_and_keeps_nothing(pkg, ctx, oracle):
    types, pages = bigint_pages(pkg, [[1, 2, 1], [3]])
    op, total, outs = run(pkg, ctx, oracle, types, [0, 1], [0], 0, pages)
    assert outs == [None, None] and total == 0 and op.needsInput()
    finish(op)

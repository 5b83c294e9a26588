"""TopNRankingOperator on the GPU: the reference's data cases (tests/golden/top_n_ranking_vectors.json) through the C ABI, random streams of every
partition key type and every sort channel type against the oracle's GroupByHash plus a Python restatement of the reference's comparator
(tests/top_n_ranking_expected.py), ties, the cutoff's worst and best cases, every path (prefilter off, compaction after every page, no compaction
before the result, pages cut into slices) with byte-identical output, equivalences with OrderBy -> RowNumber and TopN, block encodings, channel selection and the
protocol.  Every comparison is exact: values bit for bit, nulls, row order, ranking values."""
import json
import os

import numpy as np
import pytest

from distinct_gpu import KEY_SPECS, key_block, key_cols, key_pages, with_hash
from top_n_ranking_expected import expected_output, golden_case_inputs, tokens

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "top_n_ranking_vectors.json")))
PAGE_SIZES = [1, 63, 64, 65, 255, 257, 1023, 1025, 4097]
ORDERS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}
ROW_NUMBER, RANK = 0, 1
PREFILTER, COMPACT, SLICE = "TGPU_TOP_N_RANKING_PREFILTER", "TGPU_TOP_N_RANKING_COMPACT_ROWS", "TGPU_TOP_N_RANKING_SLICE_ROWS"
# the default, the prefilter off, a compaction after every page, no compaction before result(), and pages cut into slices of 100 and 64 rows (the
# library's slice is 2^20 rows: a page that large is prefiltered and selected slice by slice)
PATHS = [{}, {PREFILTER: "off"}, {COMPACT: "1"}, {COMPACT: "1000000000"}, {PREFILTER: "off", COMPACT: "1"}, {SLICE: "100"}, {SLICE: "64", COMPACT: "1"}]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def create(pkg, ctx, ranking, types, outputs, partitions, sorts, orders, n, partial=False, hash_channel=-1, expected_positions=10, env=None):
    """one operator; the two switches are read when it is created"""
    env = env or {}
    os.environ.update(env)
    try:
        return pkg.TopNRankingOperatorFactory(ctx, 1, ranking, types, outputs, partitions, sorts, orders, n, partial, hash_channel, expected_positions).createOperator()
    finally:
        for k in env:
            del os.environ[k]


def drive(op, pages):
    """the operator's one output page on the host (None = no page), with the protocol checked on the way"""
    for p in pages:
        assert op.needsInput() and not op.isFinished()
        op.addInput(p)
        assert op.getOutput() is None   # nothing before finish()
    op.finish()
    assert not op.needsInput()
    o = op.getOutput()
    assert op.getOutput() is None and op.isFinished() and not op.needsInput()
    if o is None:
        return None
    page = o.to_host()
    o.release()
    return page


def run(pkg, ctx, ranking, types, outputs, partitions, sorts, orders, n, pages, partial=False, hash_channel=-1, expected_positions=10, env=None):
    op = create(pkg, ctx, ranking, types, outputs, partitions, sorts, orders, n, partial, hash_channel, expected_positions, env)
    out = drive(op, pages)
    assert op.memoryBytes() >= 0
    op.close()
    if out is None:
        return []
    assert out.getPositionCount() > 0 and out.getChannelCount() == len(outputs) + (0 if partial else 1)
    assert [out.getBlock(i).type for i in range(len(outputs))] == [types[c] for c in outputs]
    if not partial:
        rank = out.getBlock(len(outputs))
        assert rank.type == pkg.BIGINT and (rank.nulls is None or not rank.nulls.any())
    return tokens(out.rows())


def want(oracle, ranking, types, outputs, partitions, sorts, orders, n, pages, partial=False, expected_positions=10):
    rows = [p.rows() for p in pages]
    keys = [key_cols(oracle, p, partitions) for p in pages]
    return tokens(expected_output(oracle, types, rows, keys, outputs, partitions, sorts, orders, ranking, n, partial, expected_positions))


def check(pkg, ctx, oracle, ranking, types, outputs, partitions, sorts, orders, n, pages, partial=False, hash_channel=-1, paths=({},), oracle_pages=None):
    """every path gives the helper's rows; returns them"""
    expected = want(oracle, ranking, types, outputs, partitions, sorts, orders, n, oracle_pages or pages, partial)
    for env in paths:
        got = run(pkg, ctx, ranking, types, outputs, partitions, sorts, orders, n, pages, partial, hash_channel, env=env)
        assert got == expected, (env, [i for i, (a, b) in enumerate(zip(got, expected)) if a != b][:5], len(got), len(expected))
    return expected


def stream(pkg, rng, sizes, groups, sort_domain):
    """(types, pages): channel 0 the BIGINT partition key, 1 a BIGINT sort key from a small domain (many ties), 2 a DOUBLE that tells the rows apart"""
    pages, at = [], 0
    for n in sizes:
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, groups, n).astype(np.int64)), pkg.Block(pkg.BIGINT, rng.integers(0, sort_domain, n).astype(np.int64)),
                              pkg.Block(pkg.DOUBLE, np.arange(at, at + n, dtype=np.float64))))
        at += n
    return [pkg.BIGINT, pkg.BIGINT, pkg.DOUBLE], pages


# ---- 1. the reference's cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, hash_enabled", [(c, h) for c in GOLD["cases"] for h in ((False, True) if c["hash_parametrised"] else (False,))],
                         ids=lambda v: v["name"] if isinstance(v, dict) else ("hash" if v else "nohash"))
def test_reference_cases(pkg, ctx, oracle, case, hash_enabled):
    types, pages_rows, expected = golden_case_inputs(case)
    pages = [pkg.Page(*[pkg.Block(t, [r[c] for r in rows]) if t == pkg.VARCHAR else
                        pkg.Block(t, np.array([0 if r[c] is None else r[c] for r in rows], dtype={1: np.int64, 4: np.float64}[t]),
                                  np.array([r[c] is None for r in rows], dtype=np.uint8) if any(r[c] is None for r in rows) else None)
                        for c, t in enumerate(types)]) for rows in pages_rows]
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, case["partition_channels"]) for p in pages], len(types), types + [pkg.BIGINT]
    got = run(pkg, ctx, {"ROW_NUMBER": 0, "RANK": 1}[case["ranking_type"]], types, case["output_channels"], case["partition_channels"], case["sort_channels"],
              [ORDERS[o] for o in case["sort_orders"]], case["max_rank_per_partition"], pages, case["partial"], hc, case["expected_positions"])
    assert got == tokens(expected)


# ---- 2. random streams against the helper, on every path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n, groups", [(1, 1), (2, 2), (3, 63), (64, 64), (65, 65), (1000, 1000), (2, 10**9), (3, 5)])
def test_random_streams_match_helper_on_every_path(pkg, ctx, oracle, n, groups):
    """3-6 pages of the ladder's sizes; n = 1000 exceeds every partition; 10^9 possible keys = more groups than rows; both ranking types, partial and final"""
    rng = np.random.default_rng(7000 + n + groups % 1000)
    sizes = [int(s) for s in rng.choice(PAGE_SIZES, int(rng.integers(3, 7)))]
    types, pages = stream(pkg, rng, sizes, groups, 40)
    for ranking in (ROW_NUMBER, RANK):
        final = check(pkg, ctx, oracle, ranking, types, [2, 0, 1], [0], [1], [1], n, pages, paths=PATHS)
        partial = run(pkg, ctx, ranking, types, [2, 0, 1], [0], [1], [1], n, pages, partial=True)
        assert partial == [r[:-1] for r in final] and len(final) > 0


def test_a_page_of_many_blocks(pkg, ctx, oracle):
    """70 001 rows in one page behind a small one: several workgroups in every kernel, the merge sort's several passes"""
    rng = np.random.default_rng(31)
    types, pages = stream(pkg, rng, [300, 70_001], 700, 1000)
    for ranking in (ROW_NUMBER, RANK):
        check(pkg, ctx, oracle, ranking, types, [2], [0], [1], [0], 3, pages, paths=[{}, {COMPACT: "1"}])


# ---- 3. partition keys ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", KEY_SPECS, ids=[s[0] for s in KEY_SPECS])
def test_every_partition_key_type_with_and_without_the_hash_channel(pkg, ctx, oracle, spec):
    name, type_names, null_frac = spec
    rng = np.random.default_rng(8000 + [s[0] for s in KEY_SPECS].index(name))
    sizes = [257, 1025, 63]
    types, pages = key_pages(pkg, rng, type_names, 50, null_frac, sizes)
    partitions = list(range(len(types)))
    pages = [p.appendColumn(pkg.Block(pkg.DOUBLE, rng.integers(0, 30, p.getPositionCount()).astype(np.float64))) for p in pages]
    types = types + [pkg.DOUBLE]
    sort = [len(types) - 1]
    outputs = list(range(len(types)))
    hashed = [with_hash(pkg, oracle, p, partitions) for p in pages]
    for ranking in (ROW_NUMBER, RANK):
        plain = check(pkg, ctx, oracle, ranking, types, outputs, partitions, sort, [3], 2, pages, paths=[{}, {COMPACT: "1"}])
        got = run(pkg, ctx, ranking, types + [pkg.BIGINT], outputs, partitions, sort, [3], 2, hashed, hash_channel=len(types))
        assert got == plain


# ---- 4. sort channels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE", "DOUBLE", "BOOLEAN", "VARCHAR"])
def test_every_sort_channel_type_under_every_sort_order(pkg, ctx, oracle, type_name):
    """10 % nulls; DOUBLE sort keys carry NaN and both zeros for ROW_NUMBER; for RANK the negative zeros become positive ones"""
    rng = np.random.default_rng(9000 + len(type_name))
    t = getattr(pkg, type_name)
    pages, rank_pages = [], []
    for n in (255, 1025):
        key = pkg.Block(pkg.BIGINT, rng.integers(0, 5, n).astype(np.int64))
        payload = pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64))
        sort_block = key_block(pkg, rng, t, n, 40, 0.1)
        pages.append(pkg.Page(key, sort_block, payload))
        if t == pkg.DOUBLE:
            sort_block = pkg.Block(pkg.DOUBLE, np.where(sort_block.values == 0, 0.0, sort_block.values), sort_block.nulls)
        rank_pages.append(pkg.Page(key, sort_block, payload))
    types = [pkg.BIGINT, t, pkg.BIGINT]
    if t == pkg.DOUBLE:
        zeros = np.concatenate([p.getBlock(1).values[p.getBlock(1).values == 0] for p in pages])
        assert np.signbit(zeros).any() and not np.signbit(zeros).all() and any(np.isnan(p.getBlock(1).values).any() for p in pages)
    for order in range(4):
        check(pkg, ctx, oracle, ROW_NUMBER, types, [1, 2, 0], [0], [1], [order], 7, pages, paths=[{}, {COMPACT: "1"}])
        check(pkg, ctx, oracle, RANK, types, [1, 2, 0], [0], [1], [order], 7, rank_pages, paths=[{}, {COMPACT: "1"}])


@pytest.mark.parametrize("sorts, orders", [([1, 2], [0, 3]), ([3, 1, 2], [2, 1, 0]), ([1, 3, 4], [3, 3, 1])])
def test_multi_key_sorts_whose_leading_keys_tie(pkg, ctx, oracle, sorts, orders):
    """channel 1 INTEGER from 3 values, 2 VARCHAR from 6, 3 BOOLEAN, 4 DOUBLE from 4: the order code of the first key decides next to nothing"""
    rng = np.random.default_rng(sum(sorts))
    pages = []
    for n in (1023, 65, 257):
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, 9, n).astype(np.int64)), key_block(pkg, rng, pkg.INTEGER, n, 3, 0.1),
                              key_block(pkg, rng, pkg.VARCHAR, n, 6, 0.1), key_block(pkg, rng, pkg.BOOLEAN, n, 2, 0.1),
                              pkg.Block(pkg.DOUBLE, rng.integers(0, 4, n).astype(np.float64)), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64))))
    types = [pkg.BIGINT, pkg.INTEGER, pkg.VARCHAR, pkg.BOOLEAN, pkg.DOUBLE, pkg.BIGINT]
    for ranking in (ROW_NUMBER, RANK):
        check(pkg, ctx, oracle, ranking, types, [5, 1, 2, 3, 4], [0], sorts, orders, 4, pages, paths=PATHS[:3])


@pytest.mark.parametrize("kind", ["suffix", "length"])
def test_varchar_keys_the_order_code_cannot_tell_apart(pkg, ctx, oracle, kind):
    """keys that agree in their first 8 bytes and differ after, and keys that differ only in length: every code is equal, also to the cutoff"""
    rng = np.random.default_rng(len(kind))
    make = (lambda k: "abcdefgh%03d" % k) if kind == "suffix" else (lambda k: "a" * (8 + k))
    pages = []
    for n in (257, 1025, 64):
        ks = rng.integers(0, 60, n)
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, 4, n).astype(np.int64)), pkg.Block(pkg.VARCHAR, [None if k == 0 else make(int(k)) for k in ks]),
                              pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64))))
    types = [pkg.BIGINT, pkg.VARCHAR, pkg.BIGINT]
    for ranking in (ROW_NUMBER, RANK):
        for order in (1, 2):
            check(pkg, ctx, oracle, ranking, types, [1, 2], [0], [1], [order], 3, pages, paths=PATHS[:3])


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------------
def test_one_partition_whose_sort_keys_are_all_equal(pkg, ctx, oracle):
    sizes = [65, 1, 257]
    pages, at = [], 0
    for n in sizes:
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, np.full(n, 7, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.arange(at, at + n, dtype=np.int64))))
        at += n
    types = [pkg.BIGINT, pkg.BIGINT]
    for partitions in ([], [0]):
        for n in (1, 66, 70):   # 66: the last kept row is the only row of page 1
            got = check(pkg, ctx, oracle, ROW_NUMBER, types, [1], partitions, [0], [1], n, pages, paths=PATHS)
            assert got == [(i, i + 1) for i in range(n)]   # the first n arrivals across the pages
        got = check(pkg, ctx, oracle, RANK, types, [1], partitions, [0], [1], 1, pages, paths=PATHS)
        assert got == [(i, 1) for i in range(sum(sizes))]   # all of them with rank 1


def test_rank_boundary_tie_that_straddles_two_pages(pkg, ctx, oracle):
    """n = 3 and sort keys 1 2 | 3 3 9 | 3 | 9: the three 3s share rank 3; a last page with a 0 pushes all of them out"""
    keys = [[1, 2], [3, 3, 9], [3], [9]]
    pages, at = [], 0
    for k in keys:
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, np.array(k, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.arange(at, at + len(k), dtype=np.int64))))
        at += len(k)
    types = [pkg.BIGINT, pkg.BIGINT]
    got = check(pkg, ctx, oracle, RANK, types, [0, 1], [], [0], [1], 3, pages, paths=PATHS)
    assert got == [(1, 0, 1), (2, 1, 2), (3, 2, 3), (3, 3, 3), (3, 5, 3)]   # three peers at the boundary, from two pages: more than n rows
    got = check(pkg, ctx, oracle, ROW_NUMBER, types, [0, 1], [], [0], [1], 3, pages, paths=PATHS)
    assert got == [(1, 0, 1), (2, 1, 2), (3, 2, 3)]
    last = pkg.Page(pkg.Block(pkg.BIGINT, np.array([0], dtype=np.int64)), pkg.Block(pkg.BIGINT, np.array([99], dtype=np.int64)))
    got = check(pkg, ctx, oracle, RANK, types, [0, 1], [], [0], [1], 3, pages + [last], paths=PATHS)
    assert got == [(0, 99, 1), (1, 0, 2), (2, 1, 3)]


# ---- 6. the cutoff's worst and best cases ----------------------------------------------------------------------------------------------------
def dropped_rows(ctx, fn):
    """(fn(), rows the prefilter saw, rows it dropped) from the profile's notes"""
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        result = fn()
        ctx.synchronize()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    return result, prof["top_n_ranking_rows_seen"]["count"], prof["top_n_ranking_rows_dropped"]["count"]


@pytest.mark.parametrize("ranking", [ROW_NUMBER, RANK])
def test_cutoff_worst_best_and_equal(pkg, ctx, oracle, ranking):
    """4 groups, n = 3, three pages of 400 rows; sort keys two apart (the order code drops a key's lowest bit)"""
    types = [pkg.BIGINT, pkg.BIGINT, pkg.BIGINT]
    group = np.arange(400, dtype=np.int64) % 4

    def pages_of(key_of):
        return [pkg.Page(pkg.Block(pkg.BIGINT, group), pkg.Block(pkg.BIGINT, key_of(p).astype(np.int64)), pkg.Block(pkg.BIGINT, np.arange(400, dtype=np.int64) + 400 * p))
                for p in range(3)]
    descending = pages_of(lambda p: 2 * (1200 - 400 * p - np.arange(400)))
    ascending = pages_of(lambda p: 2 * (400 * p + np.arange(400)))
    equal = pages_of(lambda p: np.full(400, 5))
    for pages, want_dropped in ((descending, 0), (ascending, 800), (equal, 0)):
        expected, seen, dropped = dropped_rows(ctx, lambda: check(pkg, ctx, oracle, ranking, types, [1, 2], [0], [1], [1], 3, pages))
        assert seen == 1200 and dropped == want_dropped   # ascending: every row of the later pages; page 0 only sets the cutoffs
        assert len(expected) == (12 if not (ranking == RANK and pages is equal) else 1200)
        check(pkg, ctx, oracle, ranking, types, [1, 2], [0], [1], [1], 3, pages, paths=PATHS[1:])
    # one ascending page in slices of 100 rows: the first slice sets the cutoffs, the other three are dropped whole
    env = {SLICE: "100"}
    expected, seen, dropped = dropped_rows(ctx, lambda: check(pkg, ctx, oracle, ranking, types, [1, 2], [0], [1], [1], 3, ascending[:1], paths=[env]))
    assert (seen, dropped, len(expected)) == (400, 300, 12)


# ---- 7. equivalences with operators that were there before -----------------------------------------------------------------------------------
def test_partitioned_row_number_equals_order_by_feeding_row_number(pkg, ctx, oracle):
    """sort keys unique per partition; compared per partition as ordered lists (OrderBy emits the partitions in key order, the operator in arrival order)"""
    rng = np.random.default_rng(12)
    sizes, n = [1025, 257, 4097], 5
    total = sum(sizes)
    sort_keys = rng.permutation(total).astype(np.float64) - 2000.0
    pages, at = [], 0
    for s in sizes:
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, 300, s).astype(np.int64)), pkg.Block(pkg.DOUBLE, sort_keys[at:at + s])))
        at += s
    types = [pkg.BIGINT, pkg.DOUBLE]
    got = run(pkg, ctx, ROW_NUMBER, types, [0, 1], [0], [1], [3], n, pages, env={COMPACT: "2000"})
    order_by = pkg.OrderByOperatorFactory(ctx, 2, types, [0, 1], 10, [0, 1], [1, 3]).createOperator()
    ordered = pkg.to_pages(order_by, pages, to_host=False)
    numberer = pkg.RowNumberOperatorFactory(ctx, 3, types, [0, 1], [0], n).createOperator()
    composed = [r for p in pkg.to_pages(numberer, ordered) for r in tokens(p.rows())]
    for o in ordered:
        o.release()
    order_by.close()
    numberer.close()

    def by_partition(rows):
        out = {}
        for r in rows:
            out.setdefault(r[0], []).append(r)
        return out
    assert by_partition(got) == by_partition(composed) and len(got) == len(composed) > 300


def test_unpartitioned_row_number_equals_top_n(pkg, ctx, oracle):
    rng = np.random.default_rng(13)
    types, pages = stream(pkg, rng, [1023, 4097, 65], 10, 25)
    for n in (1, 64, 6000):
        top = pkg.TopNOperatorFactory(ctx, 2, types, n, [1, 0], [3, 0]).createOperator()
        rows = [r for p in pkg.to_pages(top, pages) for r in tokens(p.rows())]
        top.close()
        got = run(pkg, ctx, ROW_NUMBER, types, [0, 1, 2], [], [1, 0], [3, 0], n, pages)
        assert got == [r + (i + 1,) for i, r in enumerate(rows)] and len(got) == min(n, 5185)


def test_rank_with_n_at_least_the_largest_partition_returns_every_row(pkg, ctx, oracle):
    rng = np.random.default_rng(14)
    types, pages = stream(pkg, rng, [257, 1025, 63], 6, 30)
    got = check(pkg, ctx, oracle, RANK, types, [2], [0], [1], [0], 1345, pages, paths=PATHS[:3])
    assert sorted(r[0] for r in got) == sorted(("double", np.float64(i).tobytes()) for i in range(1345))


# ---- 8. encodings, channel selection, the protocol ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [[2, 0, 1], [2], [], [1, 1]])
def test_output_channels_reordered_and_subset(pkg, ctx, oracle, outputs):
    rng = np.random.default_rng(41)
    n = 1025
    page = pkg.Page(key_block(pkg, rng, pkg.VARCHAR, n, 6, 0.1), pkg.Block(pkg.DOUBLE, rng.integers(0, 50, n).astype(np.float64)), key_block(pkg, rng, pkg.INTEGER, n, 5, 0.1))
    types = [pkg.VARCHAR, pkg.DOUBLE, pkg.INTEGER]
    for partial in (False, True):
        if outputs or not partial:
            check(pkg, ctx, oracle, ROW_NUMBER, types, outputs, [2, 0], [1], [1], 2, [page, page], partial=partial)


@pytest.mark.parametrize("type_name", ["BIGINT", "DOUBLE", "VARCHAR"])
def test_dictionary_and_rle_blocks(pkg, ctx, oracle, type_name):
    rng = np.random.default_rng(19)
    t = getattr(pkg, type_name)
    dictionary = pkg.DictionaryBlock(key_block(pkg, rng, t, 40, 30, 0.1), rng.integers(0, 40, 2000).astype(np.int32))
    sort_dictionary = pkg.DictionaryBlock(key_block(pkg, rng, pkg.VARCHAR, 10, 10, 0.2), rng.integers(0, 10, 2000).astype(np.int32))
    rle = pkg.RunLengthEncodedBlock(pkg.Block(t, [dictionary.flatten().get(3)]), 500)
    sort_rle = pkg.RunLengthEncodedBlock(pkg.Block(pkg.VARCHAR, ["same"]), 500)
    pages = [pkg.Page(dictionary, sort_dictionary), pkg.Page(rle, sort_rle), pkg.Page(key_block(pkg, rng, t, 1000, 60, 0.1), key_block(pkg, rng, pkg.VARCHAR, 1000, 5, 0.1))]
    flat = [pkg.Page(*[b.flatten() for b in p.blocks]) for p in pages]
    for ranking in (ROW_NUMBER, RANK):
        check(pkg, ctx, oracle, ranking, [t, pkg.VARCHAR], [0, 1], [0], [1], [0], 2, pages, oracle_pages=flat)


def test_protocol_empty_input_duplicate_and_factory_close(pkg, ctx):
    f = pkg.TopNRankingOperatorFactory(ctx, 1, RANK, [pkg.BIGINT, pkg.BIGINT], [1], [0], [1], [1], 1)
    f2 = f.duplicate()
    a, b, empty, zero = f.createOperator(), f2.createOperator(), f.createOperator(), f2.createOperator()
    f.noMoreOperators()
    with pytest.raises(pkg.TgpuError):
        f.createOperator()
    f.close()    # the factories go first: their operators live on
    f2.close()
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array([4, 4, 9, 4, 9], dtype=np.int64)), pkg.Block(pkg.BIGINT, np.array([5, 3, 8, 3, 9], dtype=np.int64)))
    for op in (a, b):   # independent hashes and stores
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None
        op.addInput(page)
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None and op.memoryBytes() > 0
    a.addInput(page)
    for op, rows in ((a, [(3, 1)] * 4 + [(8, 1)] * 2), (b, [(3, 1)] * 2 + [(8, 1)])):
        op.finish()
        assert not op.needsInput() and not op.isFinished()   # the page has not been handed out yet
        with pytest.raises(pkg.TgpuError) as e:
            op.addInput(page)
        assert e.value.code == -5   # a state error
        o = op.getOutput()
        assert o.to_host().rows() == rows
        o.release()
        assert op.isFinished() and op.getOutput() is None
        op.close()
    # empty input, and input of zero-row pages only: no page
    empty.finish()
    assert empty.isFinished() and not empty.needsInput() and empty.getOutput() is None and empty.isFinished()
    zero.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.zeros(0, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.zeros(0, dtype=np.int64))))
    zero.finish()
    assert zero.isFinished() and zero.getOutput() is None
    empty.close()
    zero.close()


# (ranking type, types, outputs, partitions, sort channels, sort orders, max rank, hash channel, expected positions)
BAD = [
    (2, [1, 4], [0], [0], [1], [1], 3, -1, 10),                  # DENSE_RANK
    (3, [1, 4], [0], [0], [1], [1], 3, -1, 10), (-1, [1, 4], [0], [0], [1], [1], 3, -1, 10),   # unknown ranking types
    (0, [1, 4], [0], [0], [1], [1], 0, -1, 10), (0, [1, 4], [0], [0], [1], [1], -1, -1, 10), (1, [1, 4], [0], [0], [1], [1], 2**31, -1, 10),
    (0, [1, 4], [0], [0], [1], [1], 3, -1, 0), (0, [1, 4], [0], [0], [1], [1], 3, -1, -4),
    (0, [1, 4], [0], [0], [], [], 3, -1, 10), (0, [1, 4], [0], [0], [1] * 9, [1] * 9, 3, -1, 10),
    (0, [1, 4], [0], [0] * 9, [1], [1], 3, -1, 10),
    (0, [1, 4], [2], [0], [1], [1], 3, -1, 10), (0, [1, 4], [-1], [0], [1], [1], 3, -1, 10), (0, [1, 4], [0], [2], [1], [1], 3, -1, 10),
    (0, [1, 4], [0], [0], [2], [1], 3, -1, 10), (0, [1, 4], [0], [0], [-1], [1], 3, -1, 10),
    (0, [1, 4], [0], [0], [1], [4], 3, -1, 10), (0, [1, 4], [0], [0], [1], [-1], 3, -1, 10),
    (0, [1, 4], [0], [0], [1], [1], 3, 1, 10), (0, [1, 1], [0], [], [0], [1], 3, 1, 10), (0, [1, 1], [0], [0], [0], [1], 3, 2, 10),
    (0, [], [], [], [0], [1], 3, -1, 10), (0, [1, 9], [0], [0], [0], [1], 3, -1, 10),
]


@pytest.mark.parametrize("ranking, types, outputs, partitions, sorts, orders, max_rank, hash_channel, expected_positions", BAD)
def test_factory_argument_errors(pkg, ctx, ranking, types, outputs, partitions, sorts, orders, max_rank, hash_channel, expected_positions):
    with pytest.raises(pkg.TgpuError) as e:
        pkg.TopNRankingOperatorFactory(ctx, 1, ranking, types, outputs, partitions, sorts, orders, max_rank, False, hash_channel, expected_positions)
    assert e.value.code == -1   # TGPU_ERR_INVALID_ARGUMENT


def test_valid_edges_of_the_arguments(pkg, ctx):
    """8 partition channels, 8 sort channels, the largest limit"""
    types = [pkg.BIGINT] * 8
    op = pkg.TopNRankingOperatorFactory(ctx, 1, ROW_NUMBER, types, [0], list(range(8)), list(range(8)), [0] * 8, 2**31 - 1).createOperator()
    page = pkg.Page(*[pkg.Block(pkg.BIGINT, np.array([c, 1, c], dtype=np.int64)) for c in range(8)])
    out = drive(op, [page])
    assert out.rows() == [(0, 1), (0, 2), (1, 1)]
    op.close()

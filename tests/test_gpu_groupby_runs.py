"""The group-by's run route (groupby.hip "Run route"): pages whose rows are clustered by the group key, the keys ascending from run to run,
get their first-seen group ids from the runs themselves -- no hash table.  Every case compares the ids with oracle.MultiChannelGroupByHash,
group count / capacity / rehash count / appendValues with the oracle's, runs the same input again with TGPU_GBH_RUNS=0 (the table route)
and asserts from the profile which route each page took: `gbh_runs` without `gbh_insert` = run route, both = an attempt that failed and fell
back, `gbh_insert` alone = the table route (run mode is left for the life of the object).

Choices the route leaves open and these tests pin down: a key cell that is null makes the page ineligible (it falls back); the heads
kernel's tile is 2048 rows (RUN_TILE)."""
import argparse
import importlib

import numpy as np
import pytest

from gpu_common import drive_with_revokes, ocol

pytestmark = pytest.mark.gpu

RUN_TILE = 2048   # rows per tile of the heads / publish kernels (groupby.hip kRunTile)
RUNS, FALLBACK, TABLE = "runs", "fallback", "table"
I64_MIN, I64_MAX = -(2**63), 2**63 - 1


# ---------------------------------------------------------------------------------------------------------------------
# the bench.py pipeline (first in the file: bench.py brings torch up before the library touches the device, as its own main does)
# ---------------------------------------------------------------------------------------------------------------------
def test_q3_pipeline_takes_the_run_route_and_saves_two_readbacks(monkeypatch):
    """bench.py's Q3 at SF 0.02: the aggregation behind the lineitem join takes the run route, and a step makes two host <- device
    read-backs fewer than with TGPU_GBH_RUNS=0 (the sort check's and the mode decision's).  The join output of SF 0.02 is 590 rows in
    225 groups, fewer than the 65,536 rows of the mode prefix, so TGPU_MODE_PREFIX_ROWS (the operator's own switch for tests) puts the
    mark inside the page, behind more groups than the few-group mode holds -- the situation of the full-scale step (row-order mode,
    asserted below) -- for both settings alike."""
    pytest.importorskip("torch")
    bench_mod = importlib.import_module("bench")
    monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "256")
    b = bench_mod.Bench(argparse.Namespace())
    try:
        b.setup_q3(0.02)
        b.ctx.profile_enable(True)
        seen = {}
        for setting in ("on", "off"):
            if setting == "off":
                monkeypatch.setenv("TGPU_GBH_RUNS", "0")
            else:
                monkeypatch.delenv("TGPU_GBH_RUNS", raising=False)
            _, prof = b.timed(b.step_q3, 2, 1)
            seen[setting] = (b.last_readbacks_per_step, set(prof), dict(b.q3_stats))
            for o in b.q3_result:
                o.release()
            b.q3_result = None
        print("q3 readbacks per step:", {k: v[0] for k, v in seen.items()})
        assert seen["on"][2] == seen["off"][2] and seen["on"][2]["lineitem_join_rows"] > 256
        assert "gbh_runs" in seen["on"][1] and "gbh_insert" not in seen["on"][1], sorted(seen["on"][1])
        assert "gbh_runs" not in seen["off"][1] and "gbh_insert" in seen["off"][1], sorted(seen["off"][1])
        assert "agg_accumulate_ordered" in seen["on"][1] and "agg_accumulate_ordered" in seen["off"][1]
        assert seen["off"][0] - seen["on"][0] == 2, seen
    finally:
        b.ctx.close()


def clustered(rng, n, lo=1, hi=7, first_id=0):
    """group index per row: runs of lo..hi rows, ids ascending from first_id"""
    lens = rng.integers(lo, hi + 1, n)
    return (first_id + np.repeat(np.arange(n), lens)[:n]).astype(np.int64)


def q3_keys(ids):
    """(BIGINT, DATE, INTEGER) key columns of the Q3 shape for group indices `ids`: the first channel ascends with the index"""
    return [(ids * 4 + 1).astype(np.int64), (8000 + ids % 2000).astype(np.int32), (ids % 3).astype(np.int32)]


def check_stream(pkg, oracle, monkeypatch, type_names, pages, routes, expected_size=16, with_hash=False, probes=()):
    """pages: one list of (values, nulls-or-None) per page; routes: the route each page must take with the run route enabled.
    probes: (page of one row, present?) pairs for contains() after the last page, then the last page is fed again and they are asked again"""
    tids = [getattr(pkg, t) for t in type_names]
    results = {}
    for setting in ("on", "off"):
        if setting == "off":
            monkeypatch.setenv("TGPU_GBH_RUNS", "0")
        else:
            monkeypatch.delenv("TGPU_GBH_RUNS", raising=False)
        ctx = pkg.Context(0)
        ctx.profile_enable(True)
        gbh = pkg.GroupByHash(ctx, tids, list(range(len(tids))), input_hash_channel=len(tids) if with_hash else None, expected_size=expected_size)
        o = oracle.MultiChannelGroupByHash(tids, expected_size)
        all_ids, all_hashes, all_cols = [], [], [[] for _ in tids]
        for page_cols, route in zip(pages, routes):
            blocks = [pkg.Block(t, v, None if nl is None else np.asarray(nl, dtype=np.uint8)) for t, (v, nl) in zip(tids, page_cols)]
            ocols = [ocol(oracle, b) for b in blocks]
            hashes = oracle.hash_rows(ocols)
            page = pkg.Page(*(blocks + ([pkg.Block(pkg.BIGINT, hashes)] if with_hash else [])))
            ctx.profile_reset()
            got = gbh.getGroupIds(page)
            prof = ctx.profile()
            want = o.get_group_ids(ocols, hashes if with_hash else None)
            assert np.array_equal(got, want), (setting, route)
            assert gbh.getGroupCount() == o.group_count
            assert gbh.getCapacity() == o.capacity
            assert gbh.getRehashCount() == o.rehash_count
            took = (("gbh_runs" in prof), ("gbh_insert" in prof))
            if setting == "off":
                assert took == (False, True), (setting, sorted(prof))
            else:
                assert took == {RUNS: (True, False), FALLBACK: (True, True), TABLE: (False, True)}[route], (route, sorted(prof))
            all_ids.append(want)
            all_hashes.append(hashes)
            for c, (v, nl) in enumerate(page_cols):
                all_cols[c].append((np.asarray(v), np.zeros(len(v), dtype=bool) if nl is None else np.asarray(nl, dtype=bool)))
        # appendValues: the key of group g is the key of the first row that got id g
        ids = np.concatenate(all_ids)
        _, first = np.unique(ids, return_index=True)
        out = gbh.appendValues()
        assert out.position_count == o.group_count == len(first)
        for c in range(len(tids)):
            vals = np.concatenate([v for v, _ in all_cols[c]])[first]
            nulls = np.concatenate([nl for _, nl in all_cols[c]])[first]
            want_keys = [None if isnull else (bool(x) if tids[c] == pkg.BOOLEAN else int(x)) for x, isnull in zip(vals, nulls)]
            got_keys = out.getBlock(c).to_list()
            if tids[c] == pkg.BOOLEAN:
                got_keys = [None if x is None else bool(x) for x in got_keys]
            assert got_keys == want_keys, (setting, c)
        if with_hash:
            assert np.array_equal(out.getBlock(len(tids)).values, np.concatenate(all_hashes)[first])
        answers = []
        for again in (False, True):
            if again and probes:   # more groups by the same route, then the same questions: the table follows the store
                last = pages[-1]
                bump = [(np.asarray(v) + (np.asarray(v).max() - np.asarray(v).min() + 1 if c == 0 else 0)).astype(np.asarray(v).dtype) for c, (v, _) in enumerate(last)]
                blocks = [pkg.Block(t, v) for t, v in zip(tids, bump)]
                ocols = [ocol(oracle, b) for b in blocks]
                ctx.profile_reset()
                got = gbh.getGroupIds(pkg.Page(*blocks))
                prof = ctx.profile()
                assert np.array_equal(got, o.get_group_ids(ocols, None))
                if setting == "on":
                    assert "gbh_runs" in prof and "gbh_insert" not in prof, sorted(prof)
            for cols, present in probes:
                blocks = [pkg.Block(t, np.asarray([v], dtype=np.asarray(pages[0][c][0]).dtype)) for c, (t, v) in enumerate(zip(tids, cols))]
                got = gbh.contains(0, pkg.Page(*blocks))
                assert got == present, (setting, again, cols)
                answers.append(got)
        results[setting] = (ids, answers)
        gbh.close()
        ctx.close()
    assert np.array_equal(results["on"][0], results["off"][0]) and results["on"][1] == results["off"][1]


Q3 = ["BIGINT", "DATE", "INTEGER"]


def page_of(cols):
    return [(c, None) for c in cols]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2 * RUN_TILE + 1])
def test_row_counts(pkg, oracle, monkeypatch, n):
    ids = clustered(np.random.default_rng(n), n)
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(q3_keys(ids))], [RUNS], with_hash=(n == 257))


def test_runs_straddle_every_wave_workgroup_and_tile_edge(pkg, oracle, monkeypatch):
    # runs of four rows starting at rows 2, 6, 10, ...: every multiple of 64 (so every wave, workgroup and tile edge) lies inside a run
    n = 2 * RUN_TILE + 100
    ids = (np.arange(n) + 2) // 4
    assert all(ids[b - 1] == ids[b] for b in range(64, n, 64))
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(q3_keys(ids))], [RUNS])


@pytest.mark.parametrize("shape", ["one_group", "all_distinct"])
def test_extremes(pkg, oracle, monkeypatch, shape):
    n = 5000
    ids = np.zeros(n, dtype=np.int64) if shape == "one_group" else np.arange(n, dtype=np.int64)
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(q3_keys(ids))], [RUNS])


@pytest.mark.parametrize("channel,descending", [(1, False), (2, False), (1, True)])
def test_heads_that_differ_in_one_channel_only(pkg, oracle, monkeypatch, channel, descending):
    n = 3000
    ids = clustered(np.random.default_rng(3), n)
    cols = [np.full(n, 7, dtype=np.int64), np.full(n, 9000, dtype=np.int32), np.full(n, 5, dtype=np.int32)]
    step = -1 if descending else 1
    cols[channel] = (cols[channel] + step * ids).astype(cols[channel].dtype)
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(cols)], [FALLBACK if descending else RUNS])


@pytest.mark.parametrize("where", ["row_1", "last_row", "recurs", "last_row_of_third_tile"])
def test_where_the_violation_falls(pkg, oracle, monkeypatch, where):
    if where == "recurs":
        ids = np.array([1, 1, 2, 2, 1], dtype=np.int64)
    else:
        n = 2 * RUN_TILE + 77 if where == "last_row_of_third_tile" else 300
        ids = clustered(np.random.default_rng(4), n, first_id=10)
        ids[1 if where == "row_1" else n - 1] = 3
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(q3_keys(ids))], [FALLBACK])


def test_negative_keys_and_the_int64_extremes(pkg, oracle, monkeypatch):
    ids = clustered(np.random.default_rng(5), 500)
    neg = [(ids * 3 - 10_000).astype(np.int64), (ids - 700).astype(np.int32), (-ids % 5 - 2).astype(np.int32)]
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(neg)], [RUNS])
    # a difference would overflow: INT64_MIN < -1 < 0 < INT64_MAX by comparison only
    b = np.array([I64_MIN, I64_MIN, -1, 0, 0, I64_MAX, I64_MAX], dtype=np.int64)
    d = np.array([-(2**31), -(2**31), 0, 0, 0, 2**31 - 1, 2**31 - 1], dtype=np.int32)
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of([b, d, d])], [RUNS])
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of([b[::-1].copy(), d, d])], [FALLBACK])
    # equal first channel, the second one steps from INT32_MIN to INT32_MAX
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of([np.zeros(7, dtype=np.int64), d, d])], [RUNS])


def test_null_vectors(pkg, oracle, monkeypatch):
    n = 700
    ids = clustered(np.random.default_rng(6), n)
    cols = q3_keys(ids)
    none_set = [(c, np.zeros(n, dtype=np.uint8)) for c in cols]
    check_stream(pkg, oracle, monkeypatch, Q3, [none_set], [RUNS])
    # a null key cell makes the page ineligible (the documented choice): whole runs of nulls in the second channel, one null in the last row
    nl = (ids % 11 == 0).astype(np.uint8)
    check_stream(pkg, oracle, monkeypatch, Q3, [[(cols[0], None), (cols[1], nl), (cols[2], None)]], [FALLBACK])
    last = np.zeros(n, dtype=np.uint8)
    last[-1] = 1
    check_stream(pkg, oracle, monkeypatch, Q3, [[(cols[0], last), (cols[1], None), (cols[2], None)]], [FALLBACK])


def test_boolean_key(pkg, oracle, monkeypatch):
    ids = clustered(np.random.default_rng(7), 600)
    flag = (np.arange(600) >= 301).astype(np.uint8)            # false rows, then true rows: the second channel starts over, the first one rose
    big = np.where(flag == 0, ids, ids - ids[301]).astype(np.int64)
    check_stream(pkg, oracle, monkeypatch, ["BOOLEAN", "BIGINT"], [page_of([flag, big])], [RUNS])
    check_stream(pkg, oracle, monkeypatch, ["BOOLEAN"], [page_of([np.array([0, 0, 0, 1, 1], dtype=np.uint8)])], [RUNS])
    check_stream(pkg, oracle, monkeypatch, ["BOOLEAN"], [page_of([np.array([1, 0], dtype=np.uint8)])], [FALLBACK])


@pytest.mark.parametrize("second", ["continues", "above", "below"])
def test_streams(pkg, oracle, monkeypatch, second):
    rng = np.random.default_rng(8)
    a = clustered(rng, 900)
    first2 = {"continues": a[-1], "above": a[-1] + 5, "below": a[-1] - 3}[second]
    b = clustered(rng, 700, first_id=first2)
    c = clustered(rng, 500, first_id=b[-1] + 1)
    pages = [page_of(q3_keys(x)) for x in (a, b, c)]
    routes = [RUNS, RUNS, RUNS] if second != "below" else [RUNS, FALLBACK, TABLE]
    check_stream(pkg, oracle, monkeypatch, Q3, pages, routes)


def test_contains_builds_the_table_on_first_need(pkg, oracle, monkeypatch):
    ids = clustered(np.random.default_rng(9), 1500)
    k = q3_keys(ids)
    present = [(int(k[0][r]), int(k[1][r]), int(k[2][r])) for r in (0, 700, 1499)]
    absent = [(int(k[0][0]) - 4, int(k[1][0]), int(k[2][0])), (int(k[0][5]), int(k[1][5]) + 1, int(k[2][5])), (int(k[0][-1]) + 2, 8000, 0)]
    probes = [(p, True) for p in present] + [(p, False) for p in absent]
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(k)], [RUNS], probes=probes)


def test_small_sub_batches(pkg, oracle, monkeypatch):
    monkeypatch.setenv("TGPU_GBH_SUBBATCH", "1000")
    ids = clustered(np.random.default_rng(10), 5000)
    check_stream(pkg, oracle, monkeypatch, Q3, [page_of(q3_keys(ids))], [RUNS], expected_size=4)


# ---------------------------------------------------------------------------------------------------------------------
# through HashAggregationOperator
# ---------------------------------------------------------------------------------------------------------------------
def agg_both(pkg, monkeypatch, run):
    """run(ctx) -> (rows, profile names) with the run route on and off; the rows must be equal bit for bit"""
    out = {}
    for setting in ("on", "off"):
        if setting == "off":
            monkeypatch.setenv("TGPU_GBH_RUNS", "0")
        else:
            monkeypatch.delenv("TGPU_GBH_RUNS", raising=False)
        ctx = pkg.Context(0)
        ctx.profile_enable(True)
        rows = run(ctx)
        prof = ctx.profile()
        out[setting] = (rows, prof)
        ctx.close()
    (rows_on, prof_on), (rows_off, prof_off) = out["on"], out["off"]
    assert "gbh_runs" in prof_on and "gbh_insert" not in prof_on, sorted(prof_on)
    assert "gbh_runs" not in prof_off and "gbh_insert" in prof_off, sorted(prof_off)
    assert bits(rows_on) == bits(rows_off)
    # the accumulate side decided the same mode and took the same kernels
    assert {k for k in prof_on if k.startswith("agg_")} == {k for k in prof_off if k.startswith("agg_")}, (sorted(prof_on), sorted(prof_off))
    return rows_on, prof_on, prof_off


def bits(rows):
    return [tuple(np.float64(x).view(np.int64) if isinstance(x, float) else x for x in r) for r in rows]


def oracle_rows(oracle, ids, vals):
    """what a SINGLE aggregation over (BIGINT, DATE, INTEGER) keys + SUM_DOUBLE + COUNT gives in Java row order"""
    k = q3_keys(ids)
    cols = [oracle.Col(oracle.BIGINT, k[0]), oracle.Col(oracle.DATE, k[1]), oracle.Col(oracle.INTEGER, k[2])]
    g = oracle.MultiChannelGroupByHash([oracle.BIGINT, oracle.DATE, oracle.INTEGER], 100)
    gids = g.get_group_ids(cols, None)
    cnt, sums = oracle.agg_double_sum(gids, vals, g.group_count)
    _, first = np.unique(gids, return_index=True)
    return [(int(k[0][r]), int(k[1][r]), int(k[2][r]), float(s), int(c)) for r, s, c in zip(first, sums, cnt)]


def q3_page(pkg, ids, vals):
    k = q3_keys(ids)
    return pkg.Page(pkg.Block(pkg.BIGINT, k[0]), pkg.Block(pkg.DATE, k[1]), pkg.Block(pkg.INTEGER, k[2]), pkg.Block(pkg.DOUBLE, vals))


def single_agg(pkg, ids, vals, cuts, java_order):
    def run(ctx):
        if java_order:
            ctx.set_double_sum_order(pkg.SUM_ORDER_JAVA)
        f = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT, pkg.DATE, pkg.INTEGER], [0, 1, 2], [(pkg.SUM_DOUBLE, 3), (pkg.COUNT_ALL, -1)], expected_groups=100)
        op = f.createOperator()
        pages = [q3_page(pkg, ids[a:z], vals[a:z]) for a, z in zip(cuts[:-1], cuts[1:])]
        rows = [r for p in pkg.to_pages(op, pages) for r in p.rows()]
        op.close()
        return rows
    return run


def test_agg_single_run_beyond_the_handoff(pkg, oracle, monkeypatch):
    n = 5000                                                   # one group of more than kOrdHandoffRows (4096) rows
    rng = np.random.default_rng(20)
    ids, vals = np.zeros(n, dtype=np.int64), rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    rows, _, _ = agg_both(pkg, monkeypatch, single_agg(pkg, ids, vals, [0, n], java_order=True))
    assert bits(rows) == bits(oracle_rows(oracle, ids, vals))


@pytest.mark.parametrize("groups_in_prefix", [1, 3000])
def test_agg_prefix_decision(pkg, oracle, monkeypatch, groups_in_prefix):
    """70,000 rows; the mode is decided from the groups among the first 65,536 rows, which the run route reports itself: one group there
    (few-group mode) or 3,000 (row-order mode), 3,000 more groups behind the mark either way.  The values are multiples of 2^-10 below 2^21,
    so every partial sum is exact and the Java-order oracle holds in both modes; that the mode is the table route's is asserted from the
    accumulate kernels' names (agg_both)."""
    n, mark = 70_000, 65_536
    head = np.zeros(mark, dtype=np.int64) if groups_in_prefix == 1 else (np.arange(mark) * groups_in_prefix // mark).astype(np.int64)
    tail = head[-1] + 1 + np.arange(n - mark) * 3000 // (n - mark)
    ids = np.concatenate([head, tail]).astype(np.int64)
    assert len(np.unique(ids[:mark])) == groups_in_prefix and len(np.unique(ids)) == groups_in_prefix + 3000
    vals = np.random.default_rng(21).integers(-(2**20), 2**20, n) / 1024.0
    rows, prof_on, _ = agg_both(pkg, monkeypatch, single_agg(pkg, ids, vals, [0, n], java_order=False))
    assert ("agg_accumulate_ordered" in prof_on) == (groups_in_prefix == 3000), sorted(prof_on)
    assert bits(rows) == bits(oracle_rows(oracle, ids, vals))


def test_agg_many_small_pages_are_coalesced(pkg, oracle, monkeypatch):
    rng = np.random.default_rng(22)
    n = 20_000
    ids = clustered(rng, n)
    vals = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    cuts = [0] + sorted(rng.choice(np.arange(1, n), 39, replace=False).tolist()) + [n]      # 40 pages; groups continue across the cuts
    rows, _, _ = agg_both(pkg, monkeypatch, single_agg(pkg, ids, vals, cuts, java_order=True))
    assert bits(rows) == bits(oracle_rows(oracle, ids, vals))


def test_agg_partial_with_hash_channel_then_final(pkg, oracle, monkeypatch):
    rng = np.random.default_rng(23)
    n = 6000
    ids = clustered(rng, n)
    vals = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    k = q3_keys(ids)
    ocols = [oracle.Col(oracle.BIGINT, k[0]), oracle.Col(oracle.DATE, k[1]), oracle.Col(oracle.INTEGER, k[2])]
    hashes = oracle.hash_rows(ocols)
    want = oracle_rows(oracle, ids, vals)
    _, first = np.unique(ids, return_index=True)
    cuts = [0, 2500, 2501, n]
    inter = {}

    def partial(ctx):
        ctx.set_double_sum_order(pkg.SUM_ORDER_JAVA)
        f = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT, pkg.DATE, pkg.INTEGER], [0, 1, 2], [(pkg.SUM_DOUBLE, 4), (pkg.COUNT_ALL, -1)], step=pkg.PARTIAL,
                                               hash_channel=3, expected_groups=100)
        op = f.createOperator()
        pages = [pkg.Page(pkg.Block(pkg.BIGINT, k[0][a:z]), pkg.Block(pkg.DATE, k[1][a:z]), pkg.Block(pkg.INTEGER, k[2][a:z]), pkg.Block(pkg.BIGINT, hashes[a:z]),
                          pkg.Block(pkg.DOUBLE, vals[a:z])) for a, z in zip(cuts[:-1], cuts[1:])]
        out = pkg.to_pages(op, pages)
        op.close()
        inter["pages"] = out
        return [r for p in out for r in p.rows()]
    rows, _, _ = agg_both(pkg, monkeypatch, partial)
    # PARTIAL output: keys, hash, then per aggregate its intermediate state (SUM_DOUBLE: count, sum; COUNT: count)
    assert [r[:3] for r in rows] == [w[:3] for w in want]
    assert [r[3] for r in rows] == [int(h) for h in hashes[first]]
    assert bits([(r[5], r[6]) for r in rows]) == bits([(w[3], w[4]) for w in want])

    def final(ctx):
        ctx.set_double_sum_order(pkg.SUM_ORDER_JAVA)
        f = pkg.HashAggregationOperatorFactory(ctx, 1, [pkg.BIGINT, pkg.DATE, pkg.INTEGER], [0, 1, 2], [(pkg.SUM_DOUBLE, 4), (pkg.COUNT_ALL, 6)], step=pkg.FINAL,
                                               hash_channel=3, expected_groups=100)
        op = f.createOperator()
        out = [r for p in pkg.to_pages(op, inter["pages"]) for r in p.rows()]
        op.close()
        return out
    frows, _, _ = agg_both(pkg, monkeypatch, final)
    # FINAL output: keys, hash, sum, count -- one intermediate row per group, so the sums pass through unchanged
    assert bits([r[:3] + r[4:] for r in frows]) == bits(want)


def test_agg_spill_after_a_run_route_page(pkg, oracle, monkeypatch):
    rng = np.random.default_rng(24)
    n = 9000
    ids = clustered(rng, n)
    vals = rng.integers(-(2**20), 2**20, n) / 1024.0            # exact partial sums: merged runs (raw-hash order, exact merge) equal the row-order sums
    cuts = [0, 3000, 6000, n]

    def run(ctx):
        ctx.set_double_sum_order(pkg.SUM_ORDER_JAVA)
        f = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT, pkg.DATE, pkg.INTEGER], [0, 1, 2], [(pkg.SUM_DOUBLE, 3), (pkg.COUNT_ALL, -1)], expected_groups=100,
                                               spill_enabled=True)
        op = f.createOperator()
        pages = [q3_page(pkg, ids[a:z], vals[a:z]) for a, z in zip(cuts[:-1], cuts[1:])]
        op.addInput(pages[0])
        assert op.getOutput() is None
        op.startMemoryRevoke()                                   # the first page's groups leave as a run: keys and hashes the run route stored
        op.finishMemoryRevoke()
        rows = drive_with_revokes(op, pages[1:], revoke=False)
        assert op.spillStats()[0] >= 1
        op.close()
        return rows
    out = {}
    for setting in ("on", "off"):
        if setting == "off":
            monkeypatch.setenv("TGPU_GBH_RUNS", "0")
        else:
            monkeypatch.delenv("TGPU_GBH_RUNS", raising=False)
        ctx = pkg.Context(0)
        ctx.profile_enable(True)
        out[setting] = (run(ctx), ctx.profile())
        ctx.close()
    assert "gbh_runs" in out["on"][1] and "gbh_runs" not in out["off"][1]
    assert bits(out["on"][0]) == bits(out["off"][0])              # merged output: raw-hash order, the same by either route
    assert sorted(bits(out["on"][0])) == sorted(bits(oracle_rows(oracle, ids, vals)))

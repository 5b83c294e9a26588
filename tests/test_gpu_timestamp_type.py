"""TGPU_TIMESTAMP as BIGINT's twin wherever a value is only carried, compared, hashed or ordered: every drive below runs twice, once with a
TIMESTAMP channel and once with a BIGINT channel over the same int64 values (ShortTimestampType declares BIGINT's EQUAL, HASH_CODE, XX_HASH_64
and COMPARISON: include/tgpu.h at the enum), the rows must be equal and the TIMESTAMP run's channel must come out typed 7.  Then min / max
over TIMESTAMP on the aggregation paths of tests/agg_paths.py, each proven by its profile scope, PARTIAL -> FINAL, spilled and streaming, and
every refusal with its code and message."""
import json

import numpy as np
import pytest

import agg_paths as P
import gpu_common as G
import key_cases as K

pytestmark = pytest.mark.gpu
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
ORDERS = ("ASC_NULLS_FIRST", "ASC_NULLS_LAST", "DESC_NULLS_FIRST", "DESC_NULLS_LAST")


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    yield c
    c.close()


def instants(n, seed, distinct=200, nulls=True):
    """int64 microseconds: negative values, the int64 ends and values that differ in the high word only; every 13th row NULL"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(-10**15, 10**15, distinct - 6), np.array([INT64_MIN, INT64_MAX, 0, -1, 1 << 32, -(1 << 32)])]).astype(np.int64)
    v = pool[rng.integers(0, len(pool), n)]
    mask = (np.arange(n) % 13 == 5).astype(np.uint8) if nulls else None
    return v, mask


def rows_of(pages):
    return [tuple(r) for pg in pages for r in pg.rows()]


def twin(pkg, drive, channels):
    """drive(T) -> output pages, for T = TIMESTAMP and T = BIGINT: equal rows, and `channels` of the TIMESTAMP run typed TIMESTAMP (BIGINT in the other)"""
    got, want = drive(pkg.TIMESTAMP), drive(pkg.BIGINT)
    assert rows_of(got) == rows_of(want) and len(rows_of(got)) > 0
    for ch in channels:
        assert {pg.getBlock(ch).type for pg in got} == {pkg.TIMESTAMP} and {pg.getBlock(ch).type for pg in want} == {pkg.BIGINT}, ch
    return rows_of(got)


def drain_source(op, limit=10_000):
    """a source operator (scan, merge): getOutput until it is finished -> host pages"""
    pages = []
    for _ in range(limit):
        if op.isFinished():
            break
        o = op.getOutput()
        if o is not None:
            if o.position_count > 0:
                pages.append(o.to_host())
            o.release()
    assert op.isFinished()
    return pages


def paged(pkg, types, cols, size):
    """cols: (values, nulls) per channel"""
    n = len(cols[0][0])
    return [pkg.Page(*[pkg.Block(t, v[a:a + size], None if m is None else m[a:a + size]) for t, (v, m) in zip(types, cols)]) for a in range(0, n, size)]


# ---- group-by keys ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["table", "table_with_hash", "run_route", "two_channels", "payload_only"])
def test_group_by_key(pkg, ctx, shape):
    n = 20_000
    v, m = instants(n, 1)
    pay = np.arange(n, dtype=np.int64)
    if shape == "run_route":                       # clustered ascending keys, no nulls: the groups are the runs (two key channels: one integer key takes its table)
        v, m = np.sort(v), None

    def drive(T):
        if shape == "two_channels":
            second = (pay % 3).astype(np.int32)
            pages = paged(pkg, [pkg.INTEGER, T, pkg.BIGINT], [(second, None), (v, m), (pay, None)], 4097)
            fac = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.INTEGER, T], [0, 1], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 2), (pkg.COUNT_COLUMN, 1)])
        elif shape == "payload_only":               # the TIMESTAMP channel is counted, never a key
            pages = paged(pkg, [pkg.BIGINT, T], [(pay % 7, None), (v, m)], 4097)
            fac = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT], [0], [(pkg.COUNT_COLUMN, 1), (pkg.COUNT_ALL, -1)])
        elif shape == "run_route":
            pages = paged(pkg, [T, pkg.BIGINT, pkg.BIGINT], [(v, m), (np.zeros(n, dtype=np.int64), None), (pay, None)], 4097)
            fac = pkg.HashAggregationOperatorFactory(ctx, 0, [T, pkg.BIGINT], [0, 1], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 2)])
        elif shape == "table_with_hash":
            from oracle import oracle
            h = oracle.hash_rows([oracle.Col(oracle.BIGINT, v, m)])      # the raw hash of the same int64 values: one hash for both types
            pages = paged(pkg, [T, pkg.BIGINT, pkg.BIGINT], [(v, m), (pay, None), (h, None)], 4097)
            fac = pkg.HashAggregationOperatorFactory(ctx, 0, [T], [0], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)], hash_channel=2)
        else:
            pages = paged(pkg, [T, pkg.BIGINT], [(v, m), (pay, None)], 4097)
            fac = pkg.HashAggregationOperatorFactory(ctx, 0, [T], [0], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)])
        return pkg.to_pages(fac.createOperator(), pages)

    if shape == "run_route":                       # the TIMESTAMP drive alone under the profile: its own pages took the run route
        ctx.profile_enable(True)
        ctx.profile_reset()
        alone = drive(pkg.TIMESTAMP)
        prof = ctx.profile()
        ctx.profile_enable(False)
        prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
        assert "gbh_runs" in prof and len(rows_of(alone)) > 100, sorted(prof)
    rows = twin(pkg, drive, [] if shape == "payload_only" else [1] if shape == "two_channels" else [0])
    if shape == "run_route":
        rows = [(k, c, s) for k, _, c, s in rows]
    if shape in ("table", "run_route"):
        first = {}
        for r, (key, null) in enumerate(zip(v, m if m is not None else np.zeros(n, dtype=np.uint8))):
            k = None if null else int(key)
            c, s = first.get(k, (0, 0))
            first[k] = (c + 1, s + r)
        assert rows == [(k, c, s) for k, (c, s) in first.items()]      # groups in first-seen order


# ---- join, semi join and the partitioning operators ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("join", ["inner", "probe_outer", "two_key_channels", "semi", "nested_loop_payload"])
def test_join_keys(pkg, ctx, join):
    bv, bm = instants(3000, 2, distinct=400)
    pv, pm = instants(9000, 3, distinct=600)
    bpay, ppay = np.arange(3000, dtype=np.int64), np.arange(9000, dtype=np.int64)

    def drive(T):
        if join == "semi":
            sf = pkg.SetBuilderOperatorFactory(ctx, 0, [T], 0)
            sb = sf.createOperator()
            for pg in paged(pkg, [T], [(bv, bm)], 1000):
                sb.addInput(pg)
            sb.finish()
            return pkg.to_pages(pkg.HashSemiJoinOperatorFactory(ctx, 1, sf.set_supplier, [T, pkg.BIGINT], 0).createOperator(), paged(pkg, [T, pkg.BIGINT], [(pv, pm), (ppay, None)], 4097))
        if join == "nested_loop_payload":
            bridge_f = pkg.NestedLoopBuildOperatorFactory(ctx, 0, [T])
            b = bridge_f.createOperator()
            b.addInput(pkg.Page(pkg.Block(T, bv[:7], bm[:7])))
            b.finish()
            return pkg.to_pages(pkg.NestedLoopJoinOperatorFactory(ctx, 1, bridge_f.bridge, [T], [0], [0]).createOperator(), paged(pkg, [T], [(pv[:300], pm[:300])], 128))
        if join == "two_key_channels":
            b2, p2 = (bpay % 2).astype(np.int64), (ppay % 2).astype(np.int64)
            bf = pkg.HashBuilderOperatorFactory(ctx, 0, [T, pkg.BIGINT, pkg.BIGINT], [0, 2], [0, 1])
            build_pages = paged(pkg, [T, pkg.BIGINT, pkg.BIGINT], [(bv, bm), (b2, None), (bpay, None)], 1000)
            jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, [T, pkg.BIGINT, pkg.BIGINT], [0, 1])
            probe_pages = paged(pkg, [T, pkg.BIGINT, pkg.BIGINT], [(pv, pm), (p2, None), (ppay, None)], 4097)
        else:
            bf = pkg.HashBuilderOperatorFactory(ctx, 0, [T, pkg.BIGINT], [0, 1], [0])
            build_pages = paged(pkg, [T, pkg.BIGINT], [(bv, bm), (bpay, None)], 1000)
            kw = {"join_type": pkg.PROBE_OUTER} if join == "probe_outer" else {}
            jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, [T, pkg.BIGINT], [0], **kw)
            probe_pages = paged(pkg, [T, pkg.BIGINT], [(pv, pm), (ppay, None)], 4097)
        b = bf.createOperator()
        for pg in build_pages:
            b.addInput(pg)
        b.finish()
        return pkg.to_pages(jf.createOperator(), probe_pages)

    twin(pkg, drive, [0])


@pytest.mark.parametrize("op", ["mark_distinct", "distinct_limit", "row_number", "top_n_ranking", "dynamic_filter", "merge_pages", "partitioned_output"])
def test_partition_keys(pkg, ctx, op):
    n = 10_000
    v, m = instants(n, 4, distinct=300)
    pay = np.arange(n, dtype=np.int64)

    def drive(T):
        types, pages = [T, pkg.BIGINT], paged(pkg, [T, pkg.BIGINT], [(v, m), (pay, None)], 4097)
        if op == "mark_distinct":
            fac = pkg.MarkDistinctOperatorFactory(ctx, 0, types, [0])
        elif op == "distinct_limit":
            fac = pkg.DistinctLimitOperatorFactory(ctx, 0, [T], [0], 1000)      # (more than the 301 distinct values: every page is consumed)
            pages = paged(pkg, [T], [(v, m)], 4097)
        elif op == "row_number":
            fac = pkg.RowNumberOperatorFactory(ctx, 0, types, [0, 1], [0], max_rows_per_partition=3)
        elif op == "top_n_ranking":
            fac = pkg.TopNRankingOperatorFactory(ctx, 0, pkg.ROW_NUMBER, [pkg.BIGINT, T], [0, 1], [0], [1], [pkg.DESC_NULLS_LAST], 2)
            pages = paged(pkg, [pkg.BIGINT, T], [(pay % 11, None), (v, m)], 4097)
        elif op == "dynamic_filter":
            fac = pkg.DynamicFilterSourceOperatorFactory(ctx, 0, types, [0], 10, 1 << 20, 100_000)     # more than 10 distinct values: min / max are collected
        elif op == "merge_pages":
            fac = pkg.MergePagesOperatorFactory(ctx, 0, types, 1 << 20, 3000)
            pages = paged(pkg, types, [(v, m), (pay, None)], 257)
        else:
            fac = pkg.PartitionedOutputOperatorFactory(ctx, 0, types, [0], 4)
            o = fac.createOperator()
            for pg in pages:
                o.addInput(pg)
            o.finish()
            out = []
            while True:
                got = o.poll()
                if got is None:
                    break
                part, page = got
                host = page.to_host()
                out.append(pkg.Page(*(host.blocks + [pkg.Block(pkg.BIGINT, np.full(host.position_count, part, dtype=np.int64))])))
            return out
        operator = fac.createOperator()
        out = pkg.to_pages(operator, pages)
        if op == "dynamic_filter":
            summary = operator.filter() if hasattr(operator, "filter") else None
            assert summary is None or summary is not False
        return out

    twin(pkg, drive, [1] if op == "top_n_ranking" else [0])


# ---- the inputs of key_cases.py with their BIGINT key channel retyped: GroupByHash itself, the aggregation, the fused tiers, the partitioner ----
SCHEMA = "DOUBLE_BIGINT"                           # the schema of key_cases.py with a BIGINT key channel: [DOUBLE, BIGINT]


def kc_types(pkg, T):
    return [T if t == K.BIGINT else t for t in K.KEY_SCHEMAS[SCHEMA]]


def kc_page(pkg, cols, T, retype, extra=()):
    """a page of KeyCols; the channels `retype` (BIGINT ones) become T"""
    return pkg.Page(*([pkg.Block(T if i in retype else c.type, c.values, c.nulls) for i, c in enumerate(cols)] + list(extra)))


def tokens(pages):
    """rows as bit tokens (key_cases.cells: NaN payloads and zero signs stay visible); a TIMESTAMP block as its int64 values"""
    out = []
    for pg in pages:
        cols = []
        for b in pg.blocks:
            if b.type == 7:
                f = b.flatten()
                b = type("Col", (), {"type": K.BIGINT, "values": f.values, "nulls": f.nulls, "offsets": None})()
            cols.append(K.cells(b))
        out += list(zip(*cols))
    return out


def twin_tokens(pkg, drive, channels):
    got, want = drive(pkg.TIMESTAMP), drive(pkg.BIGINT)
    assert tokens(got) == tokens(want) and len(tokens(got)) > 0
    for ch in channels:
        assert {pg.getBlock(ch).type for pg in got} == {pkg.TIMESTAMP} and {pg.getBlock(ch).type for pg in want} == {pkg.BIGINT}, ch
    return tokens(got)


@pytest.mark.parametrize("with_hash", [False, True])
def test_key_cases_group_by_hash(pkg, ctx, with_hash):
    """pages of 1, 257, 20 000 and 3 rows through one GroupByHash: ids and group count after every page, appendValues() at the end"""
    from oracle import oracle
    pages = K.group_by_hash_pages(SCHEMA)
    runs = {}
    for T in (pkg.TIMESTAMP, pkg.BIGINT):
        gbh = pkg.GroupByHash(ctx, kc_types(pkg, T), [0, 1], input_hash_channel=2 if with_hash else None, expected_size=16)
        ids = []
        for cols in pages:
            hashes = oracle.hash_rows([K.to_ocol(oracle, c) for c in cols])
            ids.append(np.array(gbh.getGroupIds(kc_page(pkg, cols, T, {1}, [pkg.Block(pkg.BIGINT, hashes)] if with_hash else []))))
            ids.append(np.array([gbh.getGroupCount()]))
        keys = gbh.appendValues()
        assert keys.getBlock(1).type == T
        runs[T] = (np.concatenate(ids).tolist(), tokens([keys]))
        gbh.close()
    assert runs[pkg.TIMESTAMP] == runs[pkg.BIGINT] and runs[pkg.BIGINT][0][-1] > 10


def test_key_cases_hash_aggregation(pkg, ctx):
    def drive(T):
        pages = [kc_page(pkg, cols, T, {1}) for cols in K.aggregation_pages(SCHEMA)]
        op = pkg.HashAggregationOperatorFactory(ctx, 0, kc_types(pkg, T), [0, 1], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 2), (pkg.COUNT_COLUMN, 3)]).createOperator()
        out = pkg.to_pages(op, pages)
        op.close()
        return out
    twin_tokens(pkg, drive, [1])


@pytest.mark.parametrize("tier", K.fused_tiers(SCHEMA))
def test_key_cases_fused_aggregation_tiers(pkg, ctx, monkeypatch, tier):
    """key_cases' twelve pages per tier (4 | 5, 16 | 17, 300 groups: the register records, the LDS records, the table) with a TIMESTAMP key
    channel beside the DOUBLE one, through the fused operator; the fused kernels ran for the TIMESTAMP drive"""
    monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "5000")
    monkeypatch.setenv("TGPU_ONEPASS_BATCH_ROWS", "1")
    f = pkg.field
    cols_pages = K.fused_aggregation_pages(SCHEMA, tier)

    def drive(T):
        types = kc_types(pkg, T)
        nk = len(types)
        filt = f(nk, pkg.BIGINT) > 1
        projs = [f(i, t) for i, t in enumerate(types)] + [f(nk + 2, pkg.DOUBLE), f(nk + 1, pkg.BIGINT)]
        aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_DOUBLE, nk), (pkg.COUNT_COLUMN, nk + 1)]
        fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, types + [pkg.BIGINT, pkg.BIGINT, pkg.DOUBLE], filt, projs, types, list(range(nk)), aggs)
        op = fac.createOperator()
        if T == pkg.TIMESTAMP:
            ctx.profile_enable(True)
            ctx.profile_reset()
        out = pkg.to_pages(op, [kc_page(pkg, cols, T, {1}) for cols in cols_pages])
        if T == pkg.TIMESTAMP:
            prof = ctx.profile()
            ctx.profile_enable(False)
            prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
            assert any(k.startswith("fused_project_accumulate") or k.startswith("fused_filter_group_accumulate") for k in prof), sorted(prof)
        op.close()
        fac.close()
        return out
    assert len(twin_tokens(pkg, drive, [1])) == tier


@pytest.mark.parametrize("groups", [4, 5, 16, 17, 300])
def test_fused_aggregation_keyed_by_timestamps_that_differ_in_the_high_word(pkg, ctx, monkeypatch, groups):
    """ONE TIMESTAMP group key in the fused filter / project aggregation, the keys equal in their low 32 bits (k << 32 | 5, both signs) and a
    NULL group: a record signature or an LDS record that kept 32 bits of the key would merge them.  Expected values from numpy."""
    monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "5000")
    T, B = pkg.TIMESTAMP, pkg.BIGINT
    f = pkg.field
    n, size = 36_000, 9000
    rng = np.random.default_rng(50 + groups)
    pool = np.array([((k - groups // 2) << 32) | 5 for k in range(groups - 1)], dtype=np.int64)
    g = rng.integers(0, groups, n)
    g[:groups] = np.arange(groups)
    keys = np.where(g == groups - 1, 0, pool[np.minimum(g, groups - 2)]).astype(np.int64)
    key_nulls = (g == groups - 1).astype(np.uint8)                 # the last group is the NULL key, lying over value 0
    vals = rng.integers(-10**6, 10**6, n).astype(np.int64)
    keep = rng.integers(0, 10, n).astype(np.int64)
    keep[:groups] = 9
    pages = [pkg.Page(pkg.Block(T, keys[a:a + size], key_nulls[a:a + size]), pkg.Block(B, keep[a:a + size]), pkg.Block(B, vals[a:a + size])) for a in range(0, n, size)]
    fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [T, B, B], f(1, B) > 1, [f(0, T), f(2, B)], [T], [0], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)])
    op = fac.createOperator()
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = pkg.to_pages(op, pages)
    prof = ctx.profile()
    ctx.profile_enable(False)
    op.close()
    fac.close()
    prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
    assert any(k.startswith("fused_project_accumulate") or k.startswith("fused_filter_group_accumulate") for k in prof), sorted(prof)
    assert {pg.getBlock(0).type for pg in out} == {T}
    want = {}
    for r in np.nonzero(keep > 1)[0]:
        k = None if key_nulls[r] else int(keys[r])
        c, t = want.get(k, (0, 0))
        want[k] = (c + 1, t + int(vals[r]))
    assert rows_of(out) == [(k, c, t) for k, (c, t) in want.items()] and len(want) == groups          # first-seen order, no two keys merged


def test_key_cases_partitioner(pkg, ctx):
    """key_cases' partition input [BIGINT, DOUBLE with specials, VARCHAR] with channel 0 retyped: PartitionedOutput (the remote and the local
    partition function), the page partitioner and the one-rank exchange give every row the partition of the same int64 as BIGINT"""
    import importlib
    ex_mod = importlib.import_module("presto-1_amd.exchange")
    cols = K.partition_input(5000)

    def drive(T):
        types = [T, pkg.DOUBLE, pkg.VARCHAR]
        page = kc_page(pkg, cols, T, {0})
        out = []
        for channels, local in (([0], False), ([0, 1], False), ([0], True)):
            o = pkg.PartitionedOutputOperatorFactory(ctx, 0, types, channels, 4, local=local).createOperator()
            o.addInput(page)
            o.finish()
            while True:
                got = o.poll()
                if got is None:
                    break
                host = got[1].to_host()
                out.append(pkg.Page(*(host.blocks + [pkg.Block(pkg.BIGINT, np.full(host.position_count, got[0], dtype=np.int64))])))
            o.close()
        counts, parted = ctx.partition_page(page, [0], 8)
        host = parted.to_host()
        parted.release()
        out.append(pkg.Page(*(host.blocks + [pkg.Block(pkg.BIGINT, np.repeat(np.arange(8), counts))])))
        ex = ex_mod.Exchange.over_rccl(ctx, 0, 1, lambda payload: payload)
        moved = ex.repartition(page, [0])
        host = moved.to_host()
        moved.release()
        ex.close()
        out.append(pkg.Page(*(host.blocks + [pkg.Block(pkg.BIGINT, np.zeros(host.position_count, dtype=np.int64))])))
        return out
    twin_tokens(pkg, drive, [0])


@pytest.mark.parametrize("join_type", ["LOOKUP_OUTER", "FULL_OUTER"])
def test_lookup_outer(pkg, ctx, join_type):
    """two probe operators over one lookup source, then LookupOuterOperator's unmatched build rows"""
    bv, bm = instants(3000, 8, distinct=400)
    pv, pm = instants(6000, 9, distinct=300)
    runs = {}
    for T in (pkg.TIMESTAMP, pkg.BIGINT):
        types = [T, pkg.BIGINT]
        build = paged(pkg, types, [(bv, bm), (np.arange(3000, dtype=np.int64), None)], 1000)
        probes = [paged(pkg, types, [(pv[a:a + 3000], pm[a:a + 3000]), (np.arange(a, a + 3000, dtype=np.int64), None)], 1024) for a in (0, 3000)]
        probe_pages, outer_page, _ = G.outer_join(pkg, ctx, build, probes, types, types, [0], [0], getattr(pkg, join_type), [0, 1], [0, 1], as_pages=True)
        assert outer_page is not None and outer_page.getBlock(2).type == T and {pg.getBlock(0).type for part in probe_pages for pg in part} == {T}
        runs[T] = ([rows_of(part) for part in probe_pages], outer_page.rows())
    assert runs[pkg.TIMESTAMP] == runs[pkg.BIGINT] and len(runs[pkg.BIGINT][1]) > 100


def test_partitioned_build(pkg, ctx):
    """the build side as four HashBuilderOperators behind a local exchange on the TIMESTAMP key, probed FULL_OUTER"""
    bv, bm = instants(3000, 12, distinct=400)
    pv, pm = instants(6000, 13, distinct=600)

    def drive(T):
        types = [T, pkg.BIGINT]
        bf = pkg.HashBuilderOperatorFactory(ctx, 0, types, [0, 1], [0], partition_count=4)
        jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, types, [0], join_type=pkg.FULL_OUTER)
        builders = [bf.createOperator() for _ in range(4)]
        probe = jf.createOperator()
        ex = pkg.PartitionedOutputOperatorFactory(ctx, 2, types, [0], 4, local=True).createOperator()
        seen = [0] * 4
        for pg in paged(pkg, types, [(bv, bm), (np.arange(3000, dtype=np.int64), None)], 700):
            ex.addInput(pg)
            while True:
                polled = ex.poll()
                if polled is None:
                    break
                seen[polled[0]] += polled[1].position_count
                builders[polled[0]].addInput(polled[1])
                polled[1].release()
        for b in builders:
            b.finish()
        assert min(seen) > 0 and sum(seen) == 3000
        out = pkg.to_pages(probe, paged(pkg, types, [(pv, pm), (np.arange(6000, dtype=np.int64), None)], 2048))
        probe.close()
        ex.close()
        return out
    twin(pkg, drive, [0, 2])


# ---- sort keys: all four orders, nulls, negative values --------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("op", ["top_n", "order_by", "merge", "window_order"])
def test_sort_keys(pkg, ctx, op, order):
    n = 6000
    v, m = instants(n, 5, distinct=2000)
    pay = np.arange(n, dtype=np.int64)
    so = getattr(pkg, order)

    def drive(T):
        types = [T, pkg.BIGINT]
        pages = paged(pkg, types, [(v, m), (pay, None)], 1000)
        if op == "top_n":
            return pkg.to_pages(pkg.TopNOperatorFactory(ctx, 0, types, 777, [0], [so]).createOperator(), pages)
        if op == "order_by":
            return pkg.to_pages(pkg.OrderByOperatorFactory(ctx, 0, types, [0, 1], 10, [0], [so]).createOperator(), pages)
        if op == "window_order":
            fns = [pkg.WindowFunction(pkg.WINDOW_RANK), pkg.WindowFunction(pkg.WINDOW_LAG, (0,)), pkg.WindowFunction(pkg.WINDOW_FIRST_VALUE, (0,)),
                   pkg.WindowFunction(pkg.WINDOW_LAST_VALUE, (0,), pkg.FRAME_PARTITION), pkg.WindowFunction(pkg.WINDOW_LEAD, (0,))]
            pages = paged(pkg, [T, pkg.BIGINT], [(v, m), (pay % 5, None)], 1000)
            out = pkg.to_pages(pkg.WindowOperatorFactory(ctx, 0, types, [0, 1], fns, [1], [0], [so]).createOperator(), pages)
            assert {out[0].getBlock(ch).type for ch in (3, 4, 5, 6)} == {T}
            # nth_value over the channel (the framed entry point), and the channel as the PARTITION key with the BIGINT channel as the sort key
            whole = pkg.WindowFrame(pkg.FRAME_TYPE_ROWS, pkg.BOUND_UNBOUNDED_PRECEDING, pkg.BOUND_UNBOUNDED_FOLLOWING)
            nth_pages = paged(pkg, [T, pkg.BIGINT, pkg.BIGINT], [(v, m), (pay % 5, None), (np.full(n, 2, dtype=np.int64), None)], 1000)
            nth = pkg.to_pages(pkg.WindowOperatorFactory(ctx, 0, [T, pkg.BIGINT, pkg.BIGINT], [0, 1], [pkg.WindowFunction(pkg.WINDOW_NTH_VALUE, (0, 2), whole)], [1], [0],
                                                         [so]).createOperator(), nth_pages)
            assert {pg.getBlock(2).type for pg in nth} == {T}
            keyed = pkg.to_pages(pkg.WindowOperatorFactory(ctx, 0, types, [0, 1], [pkg.WindowFunction(pkg.WINDOW_ROW_NUMBER), pkg.WindowFunction(pkg.WINDOW_LAG, (0,))], [0], [1],
                                                           [so]).createOperator(), paged(pkg, types, [(v, m), (pay, None)], 1000))
            assert {pg.getBlock(0).type for pg in keyed} == {T} and {pg.getBlock(3).type for pg in keyed} == {T}
            # (one row list for the twin: the three windows' rows one after the other, padded to one width)
            tail = [pkg.Page(pkg.Block(T, [r[0] for r in rws]), pkg.Block(pkg.BIGINT, [r[1] for r in rws]), pkg.Block(pkg.BIGINT, [0 if r[2] is None else 1 for r in rws]),
                             *[pkg.Block(T, [r[k] for r in rws]) for k in (2, 2, 2, 2)]) for rws in ([(a, b, c) for a, b, c in rows_of(nth)], [(a, b, d) for a, b, c, d in rows_of(keyed)])]
            return out + tail
        # merge: sorted streams in, one sorted stream out
        streams = []
        for s in range(3):
            vs, ms = v[s::3], m[s::3]
            sorted_pages = pkg.to_pages(pkg.OrderByOperatorFactory(ctx, 0, types, [0, 1], 10, [0, 1], [so, pkg.ASC_NULLS_LAST]).createOperator(),
                                        paged(pkg, types, [(vs, ms), (pay[s::3], None)], 700))
            streams.append(sorted_pages)
        fac = pkg.MergeOperatorFactory(ctx, 1, types, [0, 1], [0, 1], [so, pkg.ASC_NULLS_LAST])
        return merge_streams(pkg, fac, streams)

    rows = twin(pkg, drive, [0])
    if op in ("order_by", "merge"):
        keys = [r[0] for r in rows]
        nulls_first, desc = "NULLS_FIRST" in order, order.startswith("DESC")
        body = [k for k in keys if k is not None]
        assert body == sorted(body, reverse=desc) and len(body) < len(keys) and (keys[0] is None) == nulls_first and min(body) < 0


def merge_streams(pkg, fac, streams):
    op = fac.createOperator()
    for pages in streams:
        op.addSplit(pkg.PageSource(pages))
    op.noMoreSplits()
    return drain_source(op)


# ---- wire and scan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lz4", [False, True])
def test_serialize_round_trip(pkg, ctx, lz4):
    n = 5000
    v, m = instants(n, 6, distinct=50)

    def drive(T):
        page = pkg.Page(pkg.Block(T, v, m), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64)))
        if lz4 and hasattr(ctx, "set_serde_compression"):
            ctx.set_serde_compression(True)
        try:
            wire = ctx.serialize_page(page)
        finally:
            if lz4 and hasattr(ctx, "set_serde_compression"):
                ctx.set_serde_compression(False)
        back = ctx.deserialize_page(bytes(wire), [T, pkg.BIGINT])
        host = back.to_host()
        back.release()
        return [host], bytes(wire)

    (got, wire_t), (want, wire_b) = drive(pkg.TIMESTAMP), drive(pkg.BIGINT)
    assert rows_of(got) == rows_of(want) == [(None if mm else int(x), r) for r, (x, mm) in enumerate(zip(v, m))]
    assert got[0].getBlock(0).type == pkg.TIMESTAMP and wire_t == wire_b and b"LONG_ARRAY" in wire_t          # the same bytes on the wire


def test_scan_with_a_lazy_block_and_encodings(pkg, ctx):
    n = 4097
    v, m = instants(n, 7, distinct=40)
    f = pkg.field

    def drive(T):
        lazy = pkg.LazyBlock(T, n, lambda: pkg.Block(T, v, m))
        dict_ids = (np.arange(n) % 40).astype(np.int32)
        page = pkg.Page(lazy, pkg.DictionaryBlock(pkg.Block(T, v[:40], m[:40]), dict_ids), pkg.RunLengthEncodedBlock(pkg.Block(T, [int(v[0])]), n), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64)))
        fac = pkg.ScanFilterAndProjectOperatorFactory(ctx, 0, [T, T, T, pkg.BIGINT], f(3, pkg.BIGINT) > 99, [f(0, T), f(1, T), f(2, T), f(3, pkg.BIGINT)])
        op = fac.createOperator()
        op.addSplit(pkg.PageSource([page]))
        op.noMoreSplits()
        out = drain_source(op)
        assert op.stats()["lazyBlocksLoaded"] == 1
        return out

    rows = twin(pkg, drive, [0, 1, 2])
    cell = lambda r: None if m[r] else int(v[r])
    assert rows == [(cell(r), cell(r % 40), int(v[0]), r) for r in range(100, n)]


# ---- min / max over TIMESTAMP: every path of agg_paths.py, each proven by its profile scope ---------------------------------------------------
FILTER_BELOW = 0.8
HEAVY_GROUP, ALL_NULL_GROUP, ALL_MASKED_GROUP = 7, 2, 3
EDGES = np.array([INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, -1, 0, 1 << 32, -(1 << 32)], dtype=np.int64)


def mm_aggs(pkg):
    return [(pkg.MIN_TIMESTAMP, 1), (pkg.MAX_TIMESTAMP, 1), (pkg.MIN_TIMESTAMP, 1, 2), (pkg.MAX_TIMESTAMP, 1, 2), (pkg.COUNT_COLUMN, 1), (pkg.COUNT_ALL, -1)]


def mm_fused_spec(pkg):
    f = pkg.field
    B, T, BO, D = pkg.BIGINT, pkg.TIMESTAMP, pkg.BOOLEAN, pkg.DOUBLE
    return [B, T, BO, D], f(3, D) < FILTER_BELOW, [f(0, B), f(1, T), f(2, BO)]


class Stream:
    """n rows: gids, a TIMESTAMP column with nulls (values over the whole int64 range, ties, both ends), a mask with nulls, the fused filter column"""

    def __init__(self, rng, ngroups, n, first_row=None, heavy=False):
        g = rng.integers(0, ngroups, n)
        if heavy:                                   # a tenth of the rows: more than a lane walks (agg.h kOrdHandoffRows) in every page
            g = np.where(rng.random(n) < 0.1, HEAVY_GROUP, g)
        if first_row is not None:                   # the last group arrives late (agg_paths.late_group_first_row)
            late = ngroups - 1
            g[:first_row[late]][g[:first_row[late]] == late] = 0
        self.gids, self.n, self.ngroups = g.astype(np.int64), n, ngroups
        v = rng.integers(INT64_MIN, INT64_MAX, n, endpoint=True)
        v = np.where(rng.random(n) < 0.2, rng.integers(-3, 4, n), v)
        v = np.where(rng.random(n) < 0.05, EDGES[rng.integers(0, len(EDGES), n)], v).astype(np.int64)
        self.nulls = (rng.random(n) < 0.15).astype(np.uint8)
        self.mask = (rng.random(n) < 0.5).astype(np.uint8)
        self.mask_nulls = (rng.random(n) < 0.1).astype(np.uint8)
        if ngroups > ALL_MASKED_GROUP:
            self.nulls[g == ALL_NULL_GROUP] = 1
            self.mask[g == ALL_MASKED_GROUP] = 0
        self.filt = rng.random(n)
        for k, want in enumerate(EDGES[:2]):        # both ends are there, kept by the filter and not null (group 0 or 1)
            rows = np.nonzero(g == k % min(ngroups, 2))[0]           # (many groups: a group has a handful of rows)
            i = int(rows[min(k, len(rows) - 1)])
            v[i], self.nulls[i], self.filt[i] = want, 0, 0.0
        self.values = v

    def pages(self, pkg, sizes, fused):
        out, at = [], 0
        for m in sizes:
            z = slice(at, at + m)
            cols = [pkg.Block(pkg.BIGINT, self.gids[z]), pkg.Block(pkg.TIMESTAMP, self.values[z], self.nulls[z]), pkg.Block(pkg.BOOLEAN, self.mask[z], self.mask_nulls[z])]
            if fused:
                cols.append(pkg.Block(pkg.DOUBLE, self.filt[z]))
            out.append(pkg.Page(*cols))
            at += m
        assert at == self.n
        return out

    def states(self, rows):
        """per group over the rows `rows`: [(count, min, max) unmasked, (count, min, max) under the mask, rows]"""
        g, v = self.gids[rows], self.values[rows]
        ok = self.nulls[rows] == 0
        out = []
        for sel in (ok, ok & (self.mask[rows] == 1) & (self.mask_nulls[rows] == 0)):
            cnt = np.bincount(g[sel], minlength=self.ngroups)
            lo, hi = np.full(self.ngroups, INT64_MAX, dtype=np.int64), np.full(self.ngroups, INT64_MIN, dtype=np.int64)
            np.minimum.at(lo, g[sel], v[sel])
            np.maximum.at(hi, g[sel], v[sel])
            out.append((cnt, lo, hi))
        return out + [np.bincount(g, minlength=self.ngroups)]

    def expected(self, rows):
        """{group: (min, max, masked min, masked max, count(x), count(*))} of SINGLE, for the groups with a row"""
        (c, lo, hi), (cm, lom, him), present = self.states(rows)
        val = lambda n, x: int(x) if n else None
        return {g: (val(c[g], lo[g]), val(c[g], hi[g]), val(cm[g], lom[g]), val(cm[g], him[g]), int(c[g]), int(present[g])) for g in range(self.ngroups) if present[g]}


def mm_cells():
    out = [(path, 1 if path == "global" else 5) for path in P.PATHS + (P.FUSED_GENERAL,)]
    out += [(path, P.ORDERED_GROUPS[path.rsplit("_", 1)[1]]) for path in P.ORDERED_PATHS + (P.PARTIAL_FINAL_MANY,)]
    return [pytest.param(p, g, id="%s-%d" % (p, g)) for p, g in out]


def mm_partial_final(pkg, ctx, s, pages, sizes, aggs, path):
    """PARTIAL operators over disjoint page sets (many groups: one per page), their intermediate rows checked -- min(bigint)'s layout, every
    channel BIGINT -- into one FINAL"""
    ends = np.cumsum(sizes)
    if path == P.PARTIAL_FINAL_MANY:
        sets = [([pg], np.arange(e - m, e)) for pg, m, e in zip(pages, sizes, ends)]
    else:
        sets = [(pages[:1], np.arange(0, sizes[0])), (pages[1:], np.arange(sizes[0], s.n))]
    partials = []
    for pgs, rows in sets:
        out = P.run_partials(pkg, ctx, [pgs], s.ngroups, aggs)[0]
        (c, lo, hi), (cm, lom, him), present = s.states(rows)
        z = lambda n, x: int(x) if n else 0
        want = {g: (int(c[g]), z(c[g], lo[g]), int(c[g]), z(c[g], hi[g]), int(cm[g]), z(cm[g], lom[g]), int(cm[g]), z(cm[g], him[g]), int(c[g]), int(present[g]))
                for g in range(s.ngroups) if present[g]}
        got = {}
        for p in out:
            assert [b.type for b in p.blocks] == [pkg.BIGINT] * (1 + 2 * 4 + 2)      # key, (count, extreme) x 4, count(x), count(*)
            got.update({r[0]: tuple(r[1:]) for r in p.rows()})
        assert got == want
        partials += out
    rows = P.run_final(pkg, ctx, partials, s.ngroups, aggs)
    assert ("agg_combine_ordered" if path == P.PARTIAL_FINAL_MANY else "agg_combine") in ctx.profile(), sorted(ctx.profile())
    return rows


@pytest.mark.parametrize("path,ngroups", mm_cells())
def test_min_max_timestamp_on_every_path(pkg, monkeypatch, path, ngroups):
    sizes = P.page_sizes(path)
    fused = P.is_fused(path)
    rng = np.random.default_rng(9300 + len(path) + ngroups % 89)
    s = Stream(rng, ngroups, sum(sizes), first_row=P.late_group_first_row(path, ngroups), heavy=path.endswith("handoff"))
    pages = s.pages(pkg, sizes, fused)
    aggs = mm_aggs(pkg)
    want = s.expected(np.nonzero(s.filt < FILTER_BELOW)[0] if fused else np.arange(s.n))
    flat = [x for row in want.values() for x in row[:4]]
    assert INT64_MIN in flat and INT64_MAX in flat
    if ngroups > ALL_MASKED_GROUP and ALL_NULL_GROUP in want and ALL_MASKED_GROUP in want:      # (20 000 groups: a group may draw no row)
        assert want[ALL_NULL_GROUP][:5] == (None, None, None, None, 0) and want[ALL_MASKED_GROUP][2:4] == (None, None) and want[ALL_MASKED_GROUP][0] is not None
    got = P.drive(pkg, monkeypatch, path, ngroups, pages, aggs, mm_fused_spec, partial_final=lambda ctx: mm_partial_final(pkg, ctx, s, pages, sizes, aggs, path))
    if got.error is not None:
        raise got.error
    assert {r[0]: tuple(r[1:]) for r in got.rows} == want
    P.assert_profile(path, got.profile, ngroups)


def test_min_max_output_types(pkg, ctx):
    """SINGLE / FINAL: a TIMESTAMP channel; PARTIAL: count BIGINT, extreme BIGINT -- on the pages the operators themselves hand out: plain, global,
    fused, spilled, streaming"""
    T, B = pkg.TIMESTAMP, pkg.BIGINT
    page = pkg.Page(pkg.Block(B, [0, 0, 1, 1, 2]), pkg.Block(T, [INT64_MIN, INT64_MAX, -1, 0, None]))
    aggs = [(pkg.MIN_TIMESTAMP, 1), (pkg.MAX_TIMESTAMP, 1), (pkg.COUNT_COLUMN, 1)]
    rows = [(0, INT64_MIN, INT64_MAX, 2), (1, -1, 0, 2), (2, None, None, 0)]

    def check(pages, types, want):
        assert [[b.type for b in p.blocks] for p in pages] == [types] and sorted(pages[0].rows()) == want

    op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], aggs).createOperator()
    check(pkg.to_pages(op, [page]), [B, T, T, B], rows)
    op.close()
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], aggs, step=pkg.PARTIAL).createOperator()
    partial = pkg.to_pages(op, [page])
    op.close()
    assert [[b.type for b in p.blocks] for p in partial] == [[B] * 6]
    assert sorted(partial[0].rows()) == [(0, 2, INT64_MIN, 2, INT64_MAX, 2), (1, 2, -1, 2, 0, 2), (2, 0, 0, 0, 0, 0)]
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], P.final_aggs(pkg, aggs), step=pkg.FINAL).createOperator()
    final = pkg.to_pages(op, partial + partial)
    op.close()
    check(final, [B, T, T, B], [r[:3] + (2 * r[3],) for r in rows])
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [], [], aggs).createOperator()
    glob = pkg.to_pages(op, [page])
    op.close()
    assert [b.type for b in glob[0].blocks] == [T, T, B] and glob[0].rows() == [(INT64_MIN, INT64_MAX, 4)]
    fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [B, T], None, [pkg.field(0, B), pkg.field(1, T)], [B], [0], aggs)
    op = fac.createOperator()
    check(pkg.to_pages(op, [page]), [B, T, T, B], rows)
    op.close()
    fac.close()
    op = pkg.StreamingAggregationOperatorFactory(ctx, 0, [B, T], [0], pkg.SINGLE, aggs).createOperator()
    out = pkg.to_pages(op, [page])
    op.close()
    assert {tuple(b.type for b in p.blocks) for p in out} == {(B, T, T, B)} and rows_of(out) == rows
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], aggs, expected_groups=3, spill_enabled=True).createOperator()
    spilled = G.drive_with_revokes(op, [page, page], True, as_pages=True)
    assert op.spillStats()[0] >= 1
    op.close()
    assert {tuple(b.type for b in p.blocks) for p in spilled} == {(B, T, T, B)} and sorted(rows_of(spilled)) == [r[:3] + (2 * r[3],) for r in rows]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def refused(pkg, make):
    with pytest.raises(pkg.TgpuError) as e:
        made = make()
        if made is not None and hasattr(made, "createOperator"):
            made.createOperator()
    return e.value.code, str(e.value)


def test_refusals(pkg, ctx):
    T, B = pkg.TIMESTAMP, pkg.BIGINT
    NOT_SUPPORTED, INVALID = -8, -1
    # RANGE frames with an offset over a TIMESTAMP sort key
    frame = pkg.WindowRangeFrame(pkg.BOUND_PRECEDING, pkg.BOUND_CURRENT_ROW, start_channel=1, start_sort_key_channel=0)
    code, msg = refused(pkg, lambda: pkg.WindowOperatorFactory(ctx, 0, [T, T], [0], [pkg.WindowFunction(pkg.WINDOW_AGGREGATE, (), frame, pkg.COUNT_ALL)], [], [0], [pkg.ASC_NULLS_LAST]))
    assert code == NOT_SUPPORTED and "TIMESTAMP" in msg and "RANGE" in msg
    # window aggregates over TIMESTAMP
    for agg in (pkg.MIN_BIGINT, pkg.MAX_BIGINT, pkg.SUM_BIGINT):
        code, msg = refused(pkg, lambda: pkg.WindowOperatorFactory(ctx, 0, [T], [0], [pkg.WindowFunction(pkg.WINDOW_AGGREGATE, (0,), pkg.FRAME_RANGE_TO_CURRENT, agg)], [], [0], [pkg.ASC_NULLS_LAST]))
        assert code == NOT_SUPPORTED and "window aggregates over TIMESTAMP" in msg
    for agg in (pkg.MIN_TIMESTAMP, pkg.MAX_TIMESTAMP):           # ids above 10 stay unknown to the window
        code, msg = refused(pkg, lambda: pkg.WindowOperatorFactory(ctx, 0, [T], [0], [pkg.WindowFunction(pkg.WINDOW_AGGREGATE, (0,), pkg.FRAME_RANGE_TO_CURRENT, agg)], [], [0], [pkg.ASC_NULLS_LAST]))
        assert code == INVALID and "unknown aggregate function" in msg
    # sum / avg over TIMESTAMP, min / max(timestamp) over BIGINT: a wrong input type
    page = pkg.Page(pkg.Block(B, [1, 2]), pkg.Block(T, [5, 6]))
    for agg, ch, types in ((pkg.SUM_BIGINT, 1, [B, T]), (pkg.AVG_BIGINT, 1, [B, T]), (pkg.SUM_DOUBLE, 1, [B, T]), (pkg.MIN_TIMESTAMP, 0, [B, T]), (pkg.MIN_BIGINT, 1, [B, T])):
        op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], [(agg, ch)]).createOperator()
        with pytest.raises(pkg.TgpuError) as e:
            pkg.to_pages(op, [page])
        named = "timestamp" if ch == 1 else "bigint"      # the message names the type it met
        assert e.value.code == INVALID and ("aggregate input: unexpected channel type " + named) in str(e.value), (agg, str(e.value))
        op.close()
        code, msg = refused(pkg, lambda: pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, types, None, [pkg.field(0, B), pkg.field(1, T)], [B], [0], [(agg, ch)]))
        assert code == INVALID and "aggregate input type mismatch" in msg
        if agg == pkg.MIN_TIMESTAMP:                 # the streaming factory knows its source types: refused at creation
            code, msg = refused(pkg, lambda: pkg.StreamingAggregationOperatorFactory(ctx, 0, types, [0], pkg.SINGLE, [(agg, ch)]))
            assert code == INVALID and "aggregate input type mismatch" in msg
        else:                                        # ... the kernels' functions meet the channel with the first page
            op = pkg.StreamingAggregationOperatorFactory(ctx, 0, types, [0], pkg.SINGLE, [(agg, ch)]).createOperator()
            with pytest.raises(pkg.TgpuError) as e:
                pkg.to_pages(op, [page])
            assert e.value.code == INVALID and "aggregate input: unexpected channel type timestamp" in str(e.value), (agg, str(e.value))
            op.close()
    # min / max over VARCHAR meets a TIMESTAMP channel: named as well
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], [(pkg.MIN_VARCHAR, 1)]).createOperator()
    with pytest.raises(pkg.TgpuError) as e:
        pkg.to_pages(op, [page])
    assert e.value.code == INVALID and "timestamp" in str(e.value), str(e.value)
    op.close()
    # type codes past TIMESTAMP stay unknown
    code, msg = refused(pkg, lambda: pkg.TopNOperatorFactory(ctx, 0, [8], 1, [0], [pkg.ASC_NULLS_LAST]))
    assert code == INVALID and "unknown type" in msg

"""Special-value and mixed-type keys on every group-by and join path (run with -m gpu on an MI355X).

Grouping is IS NOT DISTINCT FROM (every NaN one group, -0.0 and +0.0 one group, NULL its own group; a group's key = the raw cells of the
row that opened it), joins are EQUAL (-0.0 matches +0.0, NaN and NULL match nothing).  The inputs come from key_cases.py -- NaNs of four
payloads, both zeros, infinities, denormals, NULLs over arbitrary bytes, key schemas for every signature layout of the fused kernels -- and
test_key_semantics_cpu.py shows, without a GPU, that each of them separates these semantics from grouping / matching by raw bits and with
`=`.  The yardstick is the CPU oracle (MultiChannelGroupByHash, PagesHash, the exact aggregates); every comparison is on bits
(key_cases.cells / same_bits), never on doubles."""
import numpy as np
import pytest

import key_cases as kc
from gpu_common import drive_with_revokes, outer_join, run_join

pytestmark = pytest.mark.gpu


def _page(pkg, cols, extra=()):
    return pkg.Page(*([kc.to_block(pkg, c) for c in cols] + list(extra)))


def _ocols(oracle, cols):
    return [kc.to_ocol(oracle, c) for c in cols]


def _out_cols(pages, n_channels):
    """the channels of a list of host pages, concatenated, as KeyCols"""
    if not pages:
        return None
    return [kc.concat([kc.from_block(pg.getBlock(c)) for pg in pages]) for c in range(n_channels)]


def _i64_tokens(a):
    return np.asarray(a, dtype=np.int64).view(np.uint64).tolist()


def _f64_tokens(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# (a) GroupByHash
# ---------------------------------------------------------------------------------------------------------------------
_RUN_TYPES = (kc.BIGINT, kc.INTEGER, kc.DATE, kc.BOOLEAN)      # key types of the run route (groupby.hip run_key_type)
_GBH_CASES = [(s, "default") for s in kc.KEY_SCHEMAS] + [("DOUBLE", "subbatch"), ("INTEGER_DATE", "subbatch")] + \
             [(s, "runs_off") for s, ts in kc.KEY_SCHEMAS.items() if all(t in _RUN_TYPES for t in ts)]


@pytest.mark.parametrize("with_hash", [False, True])
@pytest.mark.parametrize("schema,variant", _GBH_CASES)
def test_group_by_hash(pkg, oracle, monkeypatch, schema, variant, with_hash):
    """pages of 1, 257, 20 000 and 3 rows through one GroupByHash: ids, group count and capacity after every page; appendValues() = the
    first row's cells bit for bit; contains() across zero signs and NaN payloads; sub-batches of 1000 rows; the table route forced"""
    if variant == "subbatch":
        monkeypatch.setenv("TGPU_GBH_SUBBATCH", "1000")
    if variant == "runs_off":
        monkeypatch.setenv("TGPU_GBH_RUNS", "0")
    types = kc.KEY_SCHEMAS[schema]
    nk = len(types)
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    gbh = pkg.GroupByHash(ctx, types, list(range(nk)), input_hash_channel=nk if with_hash else None, expected_size=16)
    o = oracle.MultiChannelGroupByHash(types, 16)
    pages = kc.group_by_hash_pages(schema)
    all_ids = []
    for cols in pages:
        oc = _ocols(oracle, cols)
        hashes = oracle.hash_rows(oc)
        got = gbh.getGroupIds(_page(pkg, cols, [pkg.Block(pkg.BIGINT, hashes)] if with_hash else []))
        want = o.get_group_ids(oc, hashes if with_hash else None)
        assert np.array_equal(got, want), cols[0].n
        assert gbh.getGroupCount() == o.group_count
        assert gbh.getCapacity() == o.capacity
        all_ids.append(want)
    cat = kc.concat_pages(pages)
    keys = kc.first_row_keys(cat, np.concatenate(all_ids))
    out = gbh.appendValues()
    assert out.position_count == o.group_count == len(keys)
    assert kc.row_tokens(out.blocks[:nk]) == keys
    key_cols = [kc.col_from_tokens(t, [k[c] for k in keys]) for c, t in enumerate(types)]
    for c in range(nk):                                     # the same once more per channel: null flags + uint64 / int32 / uint8 views
        (got_nulls, got_bits), (want_nulls, want_bits) = kc.block_bits(out.getBlock(c)), kc.block_bits(key_cols[c])
        assert np.array_equal(got_nulls, want_nulls) and len(got_bits) == len(want_bits) and all(g == w for g, w in zip(got_bits, want_bits)), c
    if with_hash:
        assert np.array_equal(out.getBlock(nk).values, oracle.hash_rows(_ocols(oracle, key_cols)))

    def contains(row):
        cols = [kc.col_from_tokens(t, [row[c]]) for c, t in enumerate(types)]
        extra = [pkg.Block(pkg.BIGINT, oracle.hash_rows(_ocols(oracle, cols)))] if with_hash else []
        return gbh.contains(0, _page(pkg, cols, extra))

    assert contains(keys[0]) and contains(keys[-1])
    for c, t in enumerate(types):
        if t != kc.DOUBLE:
            continue
        opened_by_neg_zero = next(k for k in keys if k[c] == kc.NEG_ZERO)
        assert contains(opened_by_neg_zero[:c] + (kc.POS_ZERO,) + opened_by_neg_zero[c + 1:])
        nan_group = next(k for k in keys if k[c] is not None and kc.is_nan_bits(k[c]))
        assert contains(nan_group[:c] + (kc.NAN_NEVER_INSERTED,) + nan_group[c + 1:])
        assert not contains(keys[0][:c] + (int(np.array([12345.5]).view(np.uint64)[0]),) + keys[0][c + 1:])
    prof = ctx.profile()
    if kc.DOUBLE in types or kc.VARCHAR in types or variant == "runs_off":
        assert "gbh_runs" not in prof, sorted(prof)          # DOUBLE (and VARCHAR) keys leave the run route on their own
    elif schema != "INTEGER":                                # (a single INTEGER key has its own table and never enters the run route)
        assert "gbh_runs" in prof, sorted(prof)              # ... and run-eligible keys do start on it: "runs_off" is another path
    gbh.close()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# (b) HashAggregationOperator, unfused
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agg_expected(oracle):
    """per schema: (pages, expected rows as tokens in group order) -- the oracle's ids on the concatenated stream + exact aggregates"""
    memo = {}

    def get(schema):
        if schema not in memo:
            types = kc.KEY_SCHEMAS[schema]
            nk = len(types)
            pages = kc.aggregation_pages(schema)
            cat = kc.concat_pages(pages)
            o = oracle.MultiChannelGroupByHash(types, 100)
            gids = o.get_group_ids(_ocols(oracle, cat[:nk]))
            ng = o.group_count
            count = oracle.agg_count(gids, cat[0].n, ng)
            lc, ls = oracle.agg_long_sum(gids, cat[nk].values, ng, nulls=cat[nk].nulls)
            dc, ds = oracle.agg_double_sum_exact(gids, cat[nk + 1].values, ng, nulls=cat[nk + 1].nulls)
            keys = kc.first_row_keys(cat[:nk], gids)
            rows = [k + (c, s if n1 else None, d if n2 else None)
                    for k, c, s, n1, d, n2 in zip(keys, _i64_tokens(count), _i64_tokens(ls), lc.tolist(), _f64_tokens(ds), dc.tolist())]
            memo[schema] = (pages, rows)
        return memo[schema]
    return get


@pytest.mark.parametrize("plan", ["single", "partial_final", "spilled"])
@pytest.mark.parametrize("schema", kc.AGG_SCHEMAS)
def test_hash_aggregation(pkg, oracle, agg_expected, schema, plan):
    """count(*), sum(bigint), sum(double over integer values): results that do not depend on the order of the rows, so all that is under
    test is which rows land in which group, in which order the groups come out and with which key bits.  partial_final: the keys travel
    through the intermediate page and are grouped again; spilled: every page becomes a run and the merge groups the runs' keys again
    (output in raw-hash order: compared as a map from key bits to totals)"""
    types = kc.KEY_SCHEMAS[schema]
    nk = len(types)
    cols_pages, want = agg_expected(schema)
    pages = [_page(pkg, cols) for cols in cols_pages]
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, nk), (pkg.SUM_DOUBLE, nk + 1)]
    gch = list(range(nk))
    ctx = pkg.Context(0)
    if plan == "single":
        op = pkg.HashAggregationOperatorFactory(ctx, 0, types, gch, aggs, expected_groups=100).createOperator()
        out = pkg.to_pages(op, pages)
        op.close()
    elif plan == "partial_final":
        fp = pkg.HashAggregationOperatorFactory(ctx, 0, types, gch, aggs, step=pkg.PARTIAL, expected_groups=100)
        partial = []
        for chunk in (pages[:2], pages[2:]):
            op = fp.createOperator()
            partial.extend(pkg.to_pages(op, chunk))
            op.close()
        # intermediate layout: keys, count | (count, sum) per aggregate
        final_aggs = [(pkg.COUNT_ALL, nk), (pkg.SUM_BIGINT, nk + 1), (pkg.SUM_DOUBLE, nk + 3)]
        op = pkg.HashAggregationOperatorFactory(ctx, 1, types, gch, final_aggs, step=pkg.FINAL, expected_groups=100).createOperator()
        out = pkg.to_pages(op, partial)
        op.close()
    else:
        op = pkg.HashAggregationOperatorFactory(ctx, 0, types, gch, aggs, expected_groups=100, spill_enabled=True).createOperator()
        out = drive_with_revokes(op, pages, True, as_pages=True)
        assert op.spillStats()[0] == len(pages)
        op.close()
    got = [r for pg in out for r in kc.row_tokens(pg.blocks)]
    assert len(got) == len(want)                       # the number of groups equals the oracle's
    if plan == "spilled":
        assert len({r[:nk] for r in got}) == len(got)
        assert {r[:nk]: r[nk:] for r in got} == {r[:nk]: r[nk:] for r in want}
    else:
        assert got == want
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) fused filter + project + aggregation
# ---------------------------------------------------------------------------------------------------------------------
_FUSED_MODES = {"default": None, "no_onepass": "TGPU_DISABLE_ONEPASS", "no_speculation": "TGPU_DISABLE_SPECULATION", "unfused": "TGPU_DISABLE_FUSION"}


def _fused_program(pkg, types):
    """input = keys, filter column, BIGINT value, DOUBLE value; projections = keys, DOUBLE value, BIGINT value.
    Aggregates: count(*), sum(double over integer values), count(bigint) -- ONE wide (hi, lo) state and three counts per group, 8 KiB of
    lane-private LDS, so that 16 groups fit a one-pass launch (FusedAggregation::onepass_groups) and the one-pass limit is FG_LDS_GROUPS
    itself; a second sum would lower that limit to 13 and move the boundary away from the tier under test"""
    f = pkg.field
    nk = len(types)
    T = list(types) + [pkg.BIGINT, pkg.BIGINT, pkg.DOUBLE]
    filt = f(nk, pkg.BIGINT) > 1
    projs = [f(i, t) for i, t in enumerate(types)] + [f(nk + 2, pkg.DOUBLE), f(nk + 1, pkg.BIGINT)]
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_DOUBLE, nk), (pkg.COUNT_COLUMN, nk + 1)]
    return T, filt, projs, aggs


@pytest.mark.parametrize("schema,tier", [(s, t) for s in kc.KEY_SCHEMAS for t in kc.fused_tiers(s)])
def test_fused_aggregation(pkg, oracle, monkeypatch, schema, tier):
    """twelve pages of 9000 rows, a filter that rejects a fifth of them, a late page that opens a NaN (or ordinary), a NULL and an ordinary
    group, group counts on both sides of FG_REG_GROUPS (4 | 5), of FG_LDS_GROUPS = the one-pass limit (16 | 17) and past the one-byte ids
    (300): the default path, the two-launch path, the path without speculation and the unfused composition give the same rows bit for
    bit, and those are the oracle's (filter_positions -> MultiChannelGroupByHash -> exact aggregates), keys = the cells of the first row
    the filter KEEPS"""
    monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "5000")
    monkeypatch.setenv("TGPU_ONEPASS_BATCH_ROWS", "1")
    types = kc.KEY_SCHEMAS[schema]
    nk = len(types)
    T, filt, projs, aggs = _fused_program(pkg, types)
    cols_pages = kc.fused_aggregation_pages(schema, tier)
    pages = [_page(pkg, cols) for cols in cols_pages]
    # the oracle composition
    prog = pkg.expressions.FlatProgram(filt, projs)
    cat = kc.concat_pages(cols_pages)
    pos = oracle.filter_positions(prog.nodes, prog.filter_root, b"", _ocols(oracle, cat))
    kept = [kc.take(c, pos) for c in cat]
    o = oracle.MultiChannelGroupByHash(types, 100)
    gids = o.get_group_ids(_ocols(oracle, kept[:nk]))
    ng = o.group_count
    assert ng == tier
    count = oracle.agg_count(gids, len(pos), ng)
    dc, ds = oracle.agg_double_sum_exact(gids, kept[nk + 2].values, ng, nulls=kept[nk + 2].nulls)
    lc = oracle.agg_count(gids, len(pos), ng, nulls=kept[nk + 1].nulls)
    want = [k + (c, d if n else None, l) for k, c, d, n, l in
            zip(kc.first_row_keys(kept[:nk], gids), _i64_tokens(count), _f64_tokens(ds), dc.tolist(), _i64_tokens(lc))]
    results = {}
    for mode, env in _FUSED_MODES.items():
        if env:
            monkeypatch.setenv(env, "1")
        ctx = pkg.Context(0)
        ctx.profile_enable(True)
        fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, T, filt, projs, types, list(range(nk)), aggs)
        op = fac.createOperator()
        out = pkg.to_pages(op, pages)
        op.close()
        results[mode] = [r for pg in out for r in kc.row_tokens(pg.blocks)]
        prof = ctx.profile()
        onepass = prof.get("fused_filter_group_accumulate_onepass", {"count": 0})["count"]
        fused_accumulate = [k for k in prof if k.startswith("fused_project_accumulate_")]
        if mode == "default":
            assert (onepass >= 1) == (tier <= 16), (onepass, sorted(prof))
        else:
            assert onepass == 0
        assert bool(fused_accumulate) == (mode != "unfused"), sorted(prof)
        ctx.close()
        if env:
            monkeypatch.delenv(env)
    for mode in _FUSED_MODES:
        assert results[mode] == results["default"], mode
    assert results["default"] == want


# ---------------------------------------------------------------------------------------------------------------------
# (d) joins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def join_case(oracle):
    """per schema: the inputs, the oracle's table over the concatenated build side and its pair lists (computed once, left unchanged)"""
    memo = {}

    def get(schema):
        if schema not in memo:
            nk = len(kc.JOIN_SCHEMAS[schema])
            build, probe = kc.join_inputs(schema)
            bcat = kc.concat_pages(build)
            ph = oracle.PagesHash(_ocols(oracle, bcat[:nk]))
            pairs = {outer: ph.probe(_ocols(oracle, probe[:nk]), probe_outer=outer) for outer in (False, True)}
            memo[schema] = (build, probe, bcat, ph, pairs)
        return memo[schema]
    return get


def _assert_join_output(out_cols, probe, bcat, op, ob):
    """probe channels then build channels; every side's key cells come out with that side's own bits"""
    want = [kc.take(c, op) for c in probe] + [kc.take_or_null(c, ob) for c in bcat]
    assert out_cols is not None or len(op) == 0
    if out_cols is None:
        return
    assert out_cols[0].n == len(op)
    for ch, (g, w) in enumerate(zip(out_cols, want)):
        assert kc.same_bits(g, w), ch


def _assert_outer_output(outer_page, n_probe_channels, bcat, ob):
    """LookupOuterOperator: exactly the build rows nobody matched, ascending -- every NaN-key and every NULL-key row among them"""
    nb = bcat[0].n
    visited = np.zeros(nb, dtype=bool)
    visited[ob[ob >= 0]] = True
    unvisited = np.nonzero(~visited)[0]
    for c in bcat[:-1]:
        if c.nulls is not None:
            assert not visited[c.nulls != 0].any()
        if c.type == kc.DOUBLE:
            assert not visited[np.isnan(c.values)].any()
    assert outer_page is not None and outer_page.position_count == len(unvisited)
    for ch in range(n_probe_channels):
        blk = outer_page.getBlock(ch)
        assert blk.nulls is not None and blk.nulls.all()
    for ch, c in enumerate(bcat):
        assert kc.same_bits(outer_page.getBlock(n_probe_channels + ch), kc.take(c, unvisited)), ch


@pytest.mark.parametrize("join_type", ["INNER", "PROBE_OUTER", "LOOKUP_OUTER", "FULL_OUTER"])
@pytest.mark.parametrize("schema", list(kc.JOIN_SCHEMAS))
def test_joins(pkg, oracle, join_case, schema, join_type):
    """build pages of 700, 1 and 1500 rows, 5000 probe rows, both sides with a row-number payload and their own key channels in the output:
    the (probe row, build row) list, the link count and the outer operator's rows equal the oracle's"""
    types = kc.JOIN_SCHEMAS[schema]
    nk = len(types)
    build, probe, bcat, ph, pairs = join_case(schema)
    T = list(types) + [pkg.BIGINT]
    chans = list(range(nk + 1))
    ctx = pkg.Context(0)
    build_pages = [_page(pkg, cols) for cols in build]
    probe_page = _page(pkg, probe)
    op, ob = pairs[join_type in ("PROBE_OUTER", "FULL_OUTER")]
    if join_type in ("INNER", "PROBE_OUTER"):
        out, stats = run_join(pkg, ctx, build_pages, [probe_page], T, T, chans[:nk], chans[:nk], join_type=getattr(pkg, join_type), out_b=chans, out_p=chans,
                              as_pages=True)
        assert stats["link_count"] == ph.link_count and stats["positions"] == bcat[0].n
        _assert_join_output(_out_cols(out, 2 * (nk + 1)), probe, bcat, op, ob)
    else:
        probe_out, outer_page, stats = outer_join(pkg, ctx, build_pages, [[probe_page]], T, T, chans[:nk], chans[:nk], getattr(pkg, join_type), out_b=chans, out_p=chans,
                                           as_pages=True)
        assert stats["link_count"] == ph.link_count and stats["positions"] == bcat[0].n
        _assert_join_output(_out_cols(probe_out[0], 2 * (nk + 1)), probe, bcat, op, ob)
        _assert_outer_output(outer_page, nk + 1, bcat, ob)
    ctx.close()


def test_join_filter_function_with_double_keys(pkg, oracle, join_case):
    """DOUBLE keys with a join filter function over both sides' payloads (build.row < probe.row AND probe.row <> 7), PROBE_OUTER: a chain's
    positions are eligible only where the filter holds; a row without an eligible position comes out once with a NULL build side"""
    build, probe, bcat, ph, _ = join_case("DOUBLE")
    B, D = pkg.BIGINT, pkg.DOUBLE
    f = pkg.field
    filt = pkg.and_(f(1, B) < f(3, B), f(3, B).ne(7))          # channels 0, 1: build; 2, 3: probe
    ctx = pkg.Context(0)
    bf = pkg.HashBuilderOperatorFactory(ctx, 0, [D, B], [0, 1], [0])
    bf.lookup_source_factory.setJoinFilter([D, B], filt)
    b = bf.createOperator()
    for cols in build:
        b.addInput(_page(pkg, cols))
    b.finish()
    jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, [D, B], [0], join_type=pkg.PROBE_OUTER)
    out = pkg.to_pages(jf.createOperator(), [_page(pkg, probe)])
    prog = pkg.expressions.FlatProgram(filt, [])
    op, ob = oracle.probe_with_filter(ph, _ocols(oracle, probe[:1]), _ocols(oracle, bcat), _ocols(oracle, probe), prog.nodes, prog.filter_root, b"", probe_outer=True)
    assert 0 < int((ob >= 0).sum()) < len(ph.probe(_ocols(oracle, probe[:1]))[0])           # the filter rejects some key-equal pairs, not all
    _assert_join_output(_out_cols(out, 4), probe, bcat, op, ob)
    assert bf.lookup_source_factory.stats()["link_count"] == ph.link_count
    ctx.close()


def test_partitioned_lookup_source_with_double_keys(pkg, oracle, join_case):
    """the build side as four HashBuilderOperators behind a local exchange on the DOUBLE key: all rows of a key (both zeros!) sit in one
    partition, so the pairs are those of one table over the partition-major concatenation of the build rows"""
    build, probe, _, _, _ = join_case("DOUBLE")
    P = 4
    B, D = pkg.BIGINT, pkg.DOUBLE
    ctx = pkg.Context(0)
    bf = pkg.HashBuilderOperatorFactory(ctx, 0, [D, B], [0, 1], [0], partition_count=P)
    jf = pkg.LookupJoinOperatorFactory(ctx, 1, bf.lookup_source_factory, [D, B], [0], join_type=pkg.FULL_OUTER)
    builders = [bf.createOperator() for _ in range(P)]
    probe_op = jf.createOperator()
    ex = pkg.PartitionedOutputOperatorFactory(ctx, 2, [D, B], [0], P, local=True).createOperator()
    parts = [[] for _ in range(P)]
    for cols in build:
        ex.addInput(_page(pkg, cols))
        while True:
            polled = ex.poll()
            if polled is None:
                break
            part, out = polled
            parts[part].append(out.to_host())
            builders[part].addInput(out)
            out.release()
    for b in builders:
        b.finish()
    assert not probe_op.isBlocked()
    cat = _out_cols([pg for part in parts for pg in part], 2)
    part_of = np.concatenate([np.full(pg.position_count, p) for p, part in enumerate(parts) for pg in part])
    assert sorted(cat[1].values.tolist()) == list(range(sum(kc.JOIN_BUILD_ROWS)))          # the exchange lost and invented no row
    live = np.ones(cat[0].n, dtype=bool) if cat[0].nulls is None else cat[0].nulls == 0
    zeros = (cat[0].values == 0.0) & live
    assert len(set(cat[0].values.view(np.uint64)[zeros].tolist())) == 2 and len(set(part_of[zeros].tolist())) == 1      # -0.0 and +0.0: one partition
    ph = oracle.PagesHash(_ocols(oracle, cat[:1]))
    op, ob = ph.probe(_ocols(oracle, probe[:1]), probe_outer=True)
    out = pkg.to_pages(probe_op, [_page(pkg, probe)])
    _assert_join_output(_out_cols(out, 4), probe, cat, op, ob)
    jf.noMoreOperators()
    oo = pkg.LookupOuterOperatorFactory(ctx, 3, bf.lookup_source_factory, [D, B]).createOperator()
    o = oo.getOutput()
    host = o.to_host()
    o.release()
    _assert_outer_output(host, 2, cat, ob)                                       # partition by partition = ascending in the concatenation
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# (e) partitioning
# ---------------------------------------------------------------------------------------------------------------------
def _assert_specials_stay_together(cols, channels, pid):
    """all NaNs, and both zeros, of the DOUBLE channel land in one partition -- per value of the other partition channel, if there is one"""
    d = cols[1]
    live = np.ones(d.n, dtype=bool) if d.nulls is None else d.nulls == 0
    other = kc.cells(cols[0]) if 0 in channels else [0] * d.n
    checked = 0
    for name, sel in (("nan", np.isnan(d.values) & live), ("zero", (d.values == 0.0) & live)):
        where = {}
        for r in np.nonzero(sel)[0].tolist():
            where.setdefault(other[r], set()).add(int(pid[r]))
        assert where and all(len(v) == 1 for v in where.values()), name
        checked += len(where)
    assert checked >= 2


@pytest.mark.parametrize("channels", [[0, 1], [1]])
def test_partition_page_with_special_doubles(pkg, oracle, channels):
    cols = kc.partition_input()
    ctx = pkg.Context(0)
    page = _page(pkg, cols)
    raw = oracle.hash_rows([kc.to_ocol(oracle, cols[c]) for c in channels])
    for parts in (1, 2, 7, 8):
        counts, out = ctx.partition_page(page, channels, parts)
        host = out.to_host()
        out.release()
        pid = oracle.partition_remote(raw, parts)
        order = np.argsort(pid, kind="stable")
        assert list(counts) == [int((pid == p).sum()) for p in range(parts)]
        for ch, c in enumerate(cols):
            assert kc.same_bits(host.getBlock(ch), kc.take(c, order)), (parts, ch)      # counts, row order, bits unchanged
        _assert_specials_stay_together(cols, channels, pid)
    ctx.close()


@pytest.mark.parametrize("parts,local", [(1, False), (2, False), (7, False), (8, False), (8, True)])
def test_partitioned_output_operator_with_special_doubles(pkg, oracle, parts, local):
    cols = kc.partition_input()
    ctx = pkg.Context(0)
    types = [c.type for c in cols]
    fac = pkg.PartitionedOutputOperatorFactory(ctx, 31, types, [0, 1], parts, local=local)
    op = fac.createOperator()
    raw = oracle.hash_rows(_ocols(oracle, cols[:2]))
    want = oracle.PagePartitioner(parts, False, -1, local).partition_page(_ocols(oracle, cols), raw)
    op.addInput(_page(pkg, cols))
    got = {}
    while True:
        e = op.poll()
        if e is None:
            break
        p, out = e
        assert p not in got
        got[p] = out.to_host()
        out.release()
    pid = np.zeros(cols[0].n, dtype=np.int64)
    for p in range(parts):
        pid[want[p]] = p
        if not want[p]:
            assert p not in got
            continue
        for ch, c in enumerate(cols):
            assert kc.same_bits(got[p].getBlock(ch), kc.take(c, want[p])), (p, ch)
    _assert_specials_stay_together(cols, [0, 1], pid)
    op.finish()
    assert op.isFinished()
    op.close()
    fac.close()
    ctx.close()

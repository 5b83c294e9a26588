"""WindowOperator on the GPU, through the C ABI, against tests/window_expected.py (a Python restatement of the reference's row loop): the
reference's cases (tests/golden/window_vectors.json), every key type and sort order with nulls and uneven pages, random data with every function
in one operator (more aggregates than one scan launch carries), the scan's tile shapes under TGPU_WINDOW_TILE_ROWS=256 and at the default tile,
the sum's overflow rule, lag / lead offsets and defaults, equivalences with OrderBy -> RowNumber, TopNRanking and HashAggregation, and the
protocol.  Every comparison is exact: values bit for bit, nulls, row order."""
import json
import os

import numpy as np
import pytest

from distinct_gpu import key_block
from window_expected import (AGGREGATE, COUNT_ALL, COUNT_COLUMN, CUME_DIST, DENSE_RANK, FIRST_VALUE, FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT, LAG,
                             LAST_VALUE, LEAD, MAX_BIGINT, MAX_DOUBLE, MIN_BIGINT, MIN_DOUBLE, PERCENT_RANK, RANK, ROW_NUMBER, SUM_BIGINT, Fn, expected_output,
                             golden_case, tokens)

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "window_vectors.json")))
ORDERS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}
TILE = "TGPU_WINDOW_TILE_ROWS"
SMALL = {TILE: "256"}
DEFAULT_TILE = 2048   # WindowGpu::kTileRows
FRAMES = (FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT)
NP = {1: np.int64, 2: np.int32, 3: np.int32, 4: np.float64, 5: np.uint8}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def block_of(pkg, t, values):
    if t == pkg.VARCHAR:
        return pkg.Block(t, list(values))
    nulls = np.array([v is None for v in values], dtype=np.uint8)
    return pkg.Block(t, np.array([0 if v is None else v for v in values], dtype=NP[t]), nulls if nulls.any() else None)


def page_of(pkg, types, rows):
    return pkg.Page(*[block_of(pkg, t, [r[c] for r in rows]) for c, t in enumerate(types)])


def create(pkg, ctx, types, outputs, functions, partitions, sorts, orders, env=None):
    """one operator; the tile switch is read when it is created"""
    env = env or {}
    fns = [pkg.WindowFunction(f.function, f.args, f.frame, f.agg) for f in functions]
    os.environ.update(env)
    try:
        return pkg.WindowOperatorFactory(ctx, 1, types, outputs, fns, partitions, sorts, orders).createOperator()
    finally:
        for k in env:
            del os.environ[k]


def drive(op, pages):
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


def run(pkg, ctx, types, outputs, functions, partitions, sorts, orders, pages, env=None):
    op = create(pkg, ctx, types, outputs, functions, partitions, sorts, orders, env)
    try:
        out = drive(op, pages)
        assert op.memoryBytes() >= 0
    finally:
        op.close()
    if out is None:
        return []
    assert out.getChannelCount() == len(outputs) + len(functions)
    assert [out.getBlock(i).type for i in range(len(outputs))] == [types[c] for c in outputs]
    for i, f in enumerate(functions):
        b = out.getBlock(len(outputs) + i)
        if f.function in (ROW_NUMBER, RANK, DENSE_RANK) or (f.function == AGGREGATE and f.agg in (COUNT_ALL, COUNT_COLUMN)):
            assert b.type == pkg.BIGINT and (b.nulls is None or not b.nulls.any())
        elif f.function in (PERCENT_RANK, CUME_DIST):
            assert b.type == pkg.DOUBLE and (b.nulls is None or not b.nulls.any())
        elif f.function == AGGREGATE:
            assert b.type == (pkg.DOUBLE if f.agg in (MIN_DOUBLE, MAX_DOUBLE) else pkg.BIGINT)
        else:
            assert b.type == types[f.args[0]]
    return tokens(out.rows())


def check(pkg, ctx, types, outputs, functions, partitions, sorts, orders, pages, envs=({},)):
    expected = tokens(expected_output(types, [p.rows() for p in pages], outputs, functions, partitions, sorts, orders))
    for env in envs:
        got = run(pkg, ctx, types, outputs, functions, partitions, sorts, orders, pages, env)
        assert got == expected, (env, [(i, a, b) for i, (a, b) in enumerate(zip(got, expected)) if a != b][:3], len(got), len(expected))
    return expected


def all_functions(value, bigint, double, offset, default):
    """every in-scope function over the given channels: 8 running aggregates under all three frames and more (24 > one launch's 4) is too many for one
    operator's 16, so the aggregates rotate through the frames"""
    fns = [Fn(ROW_NUMBER), Fn(RANK), Fn(DENSE_RANK), Fn(PERCENT_RANK), Fn(CUME_DIST), Fn(LAG, (value, offset, default)), Fn(LEAD, (value, offset, default)),
           Fn(FIRST_VALUE, (value,), FRAME_ROWS_TO_CURRENT), Fn(LAST_VALUE, (value,), FRAME_RANGE_TO_CURRENT)]
    aggs = [(COUNT_ALL, ()), (COUNT_COLUMN, (value,)), (SUM_BIGINT, (bigint,)), (MIN_BIGINT, (bigint,)), (MAX_BIGINT, (bigint,)), (MIN_DOUBLE, (double,)),
            (MAX_DOUBLE, (double,))]
    return fns + [Fn(AGGREGATE, args, FRAMES[i % 3], agg) for i, (agg, args) in enumerate(aggs)]


def table(pkg, rng, sizes, partitions, sort_domain=20, nulls=0.1):
    """channels: 0 BIGINT partition key, 1 BIGINT sort key (ties), 2 BIGINT row id, 3 BIGINT values with nulls, 4 DOUBLE values with nulls / NaN / zeros,
    5 VARCHAR values with nulls, 6 BIGINT offsets 0 .. 3 with nulls, 7 VARCHAR defaults"""
    pages, at = [], 0
    for n in sizes:
        d = rng.integers(-3, 4, n).astype(np.float64)
        d[rng.random(n) < 0.05] = np.nan
        d[rng.random(n) < 0.05] = -0.0
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, partitions, n).astype(np.int64)), pkg.Block(pkg.BIGINT, rng.integers(0, sort_domain, n).astype(np.int64)),
                              pkg.Block(pkg.BIGINT, np.arange(at, at + n, dtype=np.int64)),
                              pkg.Block(pkg.BIGINT, rng.integers(-1000, 1000, n).astype(np.int64), (rng.random(n) < nulls).astype(np.uint8)),
                              pkg.Block(pkg.DOUBLE, d, (rng.random(n) < nulls).astype(np.uint8)), key_block(pkg, rng, pkg.VARCHAR, n, 30, nulls),
                              pkg.Block(pkg.BIGINT, rng.integers(0, 4, n).astype(np.int64), (rng.random(n) < nulls).astype(np.uint8)),
                              pkg.Block(pkg.VARCHAR, ["d%d" % i for i in range(at, at + n)])))
        at += n
    return [pkg.BIGINT, pkg.BIGINT, pkg.BIGINT, pkg.BIGINT, pkg.DOUBLE, pkg.VARCHAR, pkg.BIGINT, pkg.VARCHAR], pages


TABLE_FUNCTIONS = all_functions(5, 3, 4, 6, 7)


# ---- 1. the reference's cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_reference_cases(pkg, ctx, case):
    types, pages_rows, functions, expected = golden_case(case)
    pages = [page_of(pkg, types, rows) for rows in pages_rows]
    got = run(pkg, ctx, types, case["output_channels"], functions, case["partition_channels"], case["sort_channels"], [ORDERS[o] for o in case["sort_orders"]], pages)
    if case["ordered"]:
        assert got == tokens(expected)
    else:
        assert sorted(map(repr, got)) == sorted(map(repr, tokens(expected)))


# ---- 2. keys, orders, pages -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE", "DOUBLE", "BOOLEAN", "VARCHAR"])
def test_every_type_as_partition_key_and_as_sort_key_under_every_sort_order(pkg, ctx, type_name):
    """uneven pages, 10 % nulls in keys and arguments; DOUBLE keys carry NaN and both zeros: one partition / peers, the sort puts -0.0 first"""
    rng = np.random.default_rng(100 + len(type_name))
    t = getattr(pkg, type_name)
    pages, at = [], 0
    for n in (65, 257, 1, 300):
        pages.append(pkg.Page(key_block(pkg, rng, t, n, 6, 0.1), key_block(pkg, rng, t, n, 9, 0.1), pkg.Block(pkg.BIGINT, np.arange(at, at + n, dtype=np.int64)),
                              pkg.Block(pkg.BIGINT, rng.integers(-50, 50, n).astype(np.int64), (rng.random(n) < 0.1).astype(np.uint8))))
        at += n
    types = [t, t, pkg.BIGINT, pkg.BIGINT]
    if t == pkg.DOUBLE:
        zeros = np.concatenate([p.getBlock(c).values[p.getBlock(c).values == 0] for p in pages for c in (0, 1)])
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    functions = [Fn(ROW_NUMBER), Fn(RANK), Fn(DENSE_RANK), Fn(CUME_DIST), Fn(AGGREGATE, (3,), FRAME_RANGE_TO_CURRENT, SUM_BIGINT), Fn(LAG, (1,)),
                 Fn(LAST_VALUE, (2,), FRAME_RANGE_TO_CURRENT), Fn(AGGREGATE, (0,), FRAME_PARTITION, COUNT_COLUMN)]
    for order in range(4):
        check(pkg, ctx, types, [2, 0, 1], functions, [0], [1], [order], pages, envs=[SMALL])
    check(pkg, ctx, types, [2], functions, [], [1, 0], [3, 0], pages)
    check(pkg, ctx, types, [2], functions, [1, 0], [], [], pages)


@pytest.mark.parametrize("partitions", [1, 7, 5000])
def test_random_rows_with_every_function_in_one_operator(pkg, ctx, partitions):
    """5 000 rows in uneven pages; 16 functions, 7 of them running aggregates: two scan runs"""
    rng = np.random.default_rng(200 + partitions)
    types, pages = table(pkg, rng, [1023, 1, 2049, 640, 1287], partitions)
    assert sum(f.function == AGGREGATE for f in TABLE_FUNCTIONS) > 4 and len(TABLE_FUNCTIONS) == 16
    check(pkg, ctx, types, [2, 0], TABLE_FUNCTIONS, [0], [1], [1], pages, envs=[{}, SMALL])


def test_no_keys_is_one_partition_of_peers_in_arrival_order(pkg, ctx):
    rng = np.random.default_rng(3)
    types, pages = table(pkg, rng, [300, 5, 600], 4)
    expected = check(pkg, ctx, types, [2], TABLE_FUNCTIONS, [], [], [], pages, envs=[{}, SMALL])
    assert [r[0] for r in expected] == list(range(905)) and {r[2] for r in expected} == {1}   # arrival order; rank 1 everywhere


# ---- 3. tile shapes ---------------------------------------------------------------------------------------------------------------------------
SCAN_FUNCTIONS = [Fn(ROW_NUMBER), Fn(RANK), Fn(DENSE_RANK), Fn(AGGREGATE, (2,), FRAME_ROWS_TO_CURRENT, SUM_BIGINT), Fn(AGGREGATE, (2,), FRAME_RANGE_TO_CURRENT, SUM_BIGINT),
                  Fn(AGGREGATE, (2,), FRAME_PARTITION, MAX_BIGINT), Fn(AGGREGATE, (), FRAME_RANGE_TO_CURRENT, COUNT_ALL), Fn(CUME_DIST), Fn(LEAD, (2,)),
                  Fn(AGGREGATE, (2,), FRAME_ROWS_TO_CURRENT, MIN_BIGINT), Fn(AGGREGATE, (2,), FRAME_PARTITION, COUNT_COLUMN)]


def shaped(pkg, part_keys, sort_keys=None, seed=0):
    """one page: 0 the partition key, 1 the sort key, 2 BIGINT values with nulls; keys ascending so that the sort leaves the rows where they are"""
    n = len(part_keys)
    rng = np.random.default_rng(seed + n)
    sort_keys = np.arange(n) if sort_keys is None else sort_keys
    return [pkg.BIGINT] * 3, [pkg.Page(pkg.Block(pkg.BIGINT, np.asarray(part_keys, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.asarray(sort_keys, dtype=np.int64)),
                                       pkg.Block(pkg.BIGINT, rng.integers(-9, 10, n).astype(np.int64), (rng.random(n) < 0.1).astype(np.uint8)))]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 3 * 256 + 17])
def test_row_counts_around_wave_block_and_tile(pkg, ctx, n):
    for keys in (np.zeros(n), np.arange(n), np.arange(n) // 5):   # one partition across all tiles, every row its own, partitions of 5
        types, pages = shaped(pkg, keys, np.arange(n) // 3)
        check(pkg, ctx, types, [1], SCAN_FUNCTIONS, [0], [1], [1], pages, envs=[SMALL])


def test_heads_on_tile_edges_and_a_tile_without_a_head(pkg, ctx):
    """tiles of 256: partition heads exactly at rows 256 (first of tile 1) and 767 (last of tile 2), none in tile 3 although tiles 2 and 4 have one"""
    n = 5 * 256 + 9
    keys = np.zeros(n)
    for k, head in enumerate((256, 767, 1100)):
        keys[head:] = k + 1
    types, pages = shaped(pkg, keys, np.arange(n) // 4)
    assert not np.diff(keys[768:1024]).any() and keys[767] != keys[766] and keys[256] != keys[255]
    check(pkg, ctx, types, [1], SCAN_FUNCTIONS, [0], [1], [1], pages, envs=[SMALL])


def test_a_peer_group_across_a_tile_boundary_under_range_to_current(pkg, ctx):
    n = 700
    sort = np.arange(n)
    sort[250:262] = 250   # peers 250 .. 261 straddle the boundary at 256
    sort[500:520] = 500   # and the one at 512
    types, pages = shaped(pkg, np.zeros(n), sort)
    expected = check(pkg, ctx, types, [1], SCAN_FUNCTIONS, [0], [1], [1], pages, envs=[SMALL])
    # RANGE sums agree over the peers on both sides of the boundary, ROWS sums move along them
    assert len({expected[i][5] for i in range(250, 262)}) == 1 and len({expected[i][4] for i in range(250, 262)}) > 1


def test_the_carry_scan_takes_a_second_chunk(pkg, ctx):
    """256 tiles of 256 rows fill one trip of launch 2; one row more is the smallest input with a second"""
    n = 256 * 256 + 1
    types, pages = shaped(pkg, np.arange(n) // 40000, np.arange(n) // 2)
    check(pkg, ctx, types, [1], SCAN_FUNCTIONS[:7], [0], [1], [1], pages, envs=[SMALL])


def test_the_default_tile(pkg, ctx):
    n = 2 * DEFAULT_TILE + 3
    types, pages = shaped(pkg, np.arange(n) // 3000, np.arange(n) // 2)
    check(pkg, ctx, types, [1], SCAN_FUNCTIONS, [0], [1], [1], pages)


# ---- 4. sum overflow ------------------------------------------------------------------------------------------------------------------------
BIG = 2**63 - 1
SUM = [Fn(AGGREGATE, (0,), FRAME_ROWS_TO_CURRENT, SUM_BIGINT)]


def sums(pkg, ctx, values, partitions=None, frame=FRAME_ROWS_TO_CURRENT, env=None):
    cols = [pkg.Block(pkg.BIGINT, np.array(values, dtype=np.int64))]
    if partitions is not None:
        cols.append(pkg.Block(pkg.BIGINT, np.array(partitions, dtype=np.int64)))
    fn = [Fn(AGGREGATE, (0,), frame, SUM_BIGINT)]
    return run(pkg, ctx, [pkg.BIGINT] * len(cols), [], fn, [1] if partitions is not None else [], [], [], [pkg.Page(*cols)], env)


def test_a_prefix_beyond_int64_fails_and_only_a_prefix(pkg, ctx):
    with pytest.raises(pkg.TgpuError) as e:
        sums(pkg, ctx, [BIG, 1, -1])
    assert e.value.code == -2 and e.value.message == "bigint addition overflow"
    assert sums(pkg, ctx, [BIG, -1, 1]) == [(BIG,), (BIG - 1,), (BIG,)]
    for frame in (FRAME_PARTITION, FRAME_RANGE_TO_CURRENT):   # the frame grows through the same prefixes
        with pytest.raises(pkg.TgpuError) as e:
            sums(pkg, ctx, [BIG, 1, -1], frame=frame)
        assert e.value.code == -2
        assert sums(pkg, ctx, [BIG, -1, 1], frame=frame) == [(BIG,)] * 3


def test_a_tile_local_sum_beyond_int64_whose_prefixes_fit(pkg, ctx):
    """tiles 0 and 1 sum to -2^63; tile 2 holds 2^62 three times: its own sum is 3 * 2^62 > int64, every prefix of the partition fits"""
    values = [0] * 768
    values[10] = values[300] = -2**62
    values[512] = values[600] = values[767] = 2**62
    got = sums(pkg, ctx, values, env=SMALL)
    assert got == [(int(v),) for v in np.cumsum(np.array(values, dtype=object))] and got[299] == (-2**62,) and got[511] == (-2**63,) and got[767] == (2**62,)


def test_an_overflow_in_one_partition_fails_whatever_the_others_do(pkg, ctx):
    values = [1, 2, 3, BIG, 1, 5, 6]
    with pytest.raises(pkg.TgpuError) as e:
        sums(pkg, ctx, values, partitions=[0, 0, 0, 1, 1, 2, 2])
    assert e.value.code == -2 and e.value.message == "bigint addition overflow"
    assert sums(pkg, ctx, values, partitions=[0, 0, 0, 1, 2, 2, 2]) == [(1,), (3,), (6,), (BIG,), (1,), (6,), (12,)]   # the head resets the sum


# ---- 5. lag / lead --------------------------------------------------------------------------------------------------------------------------
def test_lag_and_lead_offsets_and_defaults(pkg, ctx):
    """partition 0 has 5 rows, partition 1 has 3; offsets null, 0, 1, beyond the partition and 2^62; defaults BIGINT / VARCHAR, some null"""
    types = [pkg.BIGINT, pkg.BIGINT, pkg.BIGINT, pkg.VARCHAR, pkg.BIGINT, pkg.VARCHAR]
    rows = [(0, i, 100 + i, "v%d" % i, o, None if i == 3 else "d%d" % i) for i, o in enumerate([None, 0, 1, 2, 2**62])]
    rows += [(1, i, 200 + i, None if i == 1 else "w%d" % i, o, "e%d" % i) for i, o in enumerate([7, 3, 1])]
    pages = [page_of(pkg, types, rows[:4]), page_of(pkg, types, rows[4:])]
    functions = [Fn(LAG, (2, 4)), Fn(LEAD, (2, 4)), Fn(LAG, (2, 4, 1)), Fn(LEAD, (2, 4, 1)), Fn(LAG, (3, 4, 5)), Fn(LEAD, (3, 4, 5)), Fn(LAG, (3,)), Fn(LEAD, (3,))]
    expected = check(pkg, ctx, types, [0, 1], functions, [0], [1], [1], pages)
    assert expected[0][2:] == (None,) * 6 + (None, "v1")          # a null offset is null, not the default
    assert expected[3][2:6] == (101, None, 101, 3) and expected[3][6:8] == ("v1", None)   # lead beyond the partition: the default cell, here BIGINT 3 / a null VARCHAR
    assert expected[4][2:6] == (None, None, 4, 4)                 # 2^62 lands outside both ways
    for bad in (-1, -2**63):
        rows[2] = rows[2][:4] + (bad,) + rows[2][5:]
        for f in (LAG, LEAD):
            with pytest.raises(pkg.TgpuError) as e:
                run(pkg, ctx, types, [0], [Fn(f, (2, 4))], [0], [1], [1], [page_of(pkg, types, rows)])
            assert e.value.code == -1 and e.value.message == "Offset must be at least 0"


# ---- 6. equivalences ------------------------------------------------------------------------------------------------------------------------
def rows_of(pkg, op, pages):
    out = pkg.to_pages(op, pages)
    op.close()
    return [r for p in out for r in p.rows()]


def test_row_number_equals_order_by_then_row_number(pkg, ctx):
    rng = np.random.default_rng(5)
    types, pages = table(pkg, rng, [700, 300, 1], 9)
    got = run(pkg, ctx, types, [2, 0, 1], [Fn(ROW_NUMBER)], [0], [1], [3], pages)
    ordered = pkg.to_pages(pkg.OrderByOperatorFactory(ctx, 2, types, [2, 0, 1], 10, [0, 1], [1, 3]).createOperator(), pages)
    numbered = rows_of(pkg, pkg.RowNumberOperatorFactory(ctx, 3, types[:3], [0, 1, 2], [1]).createOperator(), ordered)
    assert got == tokens(numbered)


def test_rank_up_to_n_equals_top_n_ranking(pkg, ctx):
    """BIGINT keys: the comparator and IS NOT DISTINCT FROM agree; TopNRanking's partitions come in arrival order, so both sides are ordered by key"""
    rng = np.random.default_rng(6)
    types, pages = table(pkg, rng, [900, 200], 11)
    got = [r for r in run(pkg, ctx, types, [0, 1, 2], [Fn(RANK)], [0], [1], [1], pages) if r[3] <= 3]
    top = rows_of(pkg, pkg.TopNRankingOperatorFactory(ctx, 4, pkg.RANK, types, [0, 1, 2], [0], [1], [1], 3).createOperator(), pages)
    assert got == tokens(sorted(top, key=lambda r: r[0]))   # stable: inside a partition TopNRanking's order stays


def test_partition_frame_aggregates_equal_hash_aggregation_joined_back(pkg, ctx):
    rng = np.random.default_rng(7)
    types, pages = table(pkg, rng, [500, 777], 13)
    aggs = [(COUNT_ALL, ()), (SUM_BIGINT, (3,)), (MIN_BIGINT, (3,)), (MAX_BIGINT, (3,)), (MIN_DOUBLE, (4,)), (MAX_DOUBLE, (4,))]
    got = run(pkg, ctx, types, [0], [Fn(AGGREGATE, args, FRAME_PARTITION, agg) for agg, args in aggs], [0], [], [], pages)
    grouped = rows_of(pkg, pkg.HashAggregationOperatorFactory(ctx, 5, [pkg.BIGINT], [0], [(agg, args[0] if args else -1) for agg, args in aggs]).createOperator(), pages)
    by_key = {r[0]: r for r in tokens(grouped)}
    assert got == [by_key[r[0]] for r in got] and len(got) == 1277


# ---- 7. lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_empty_input_finish_protocol_and_duplicate(pkg, ctx):
    types = [pkg.BIGINT, pkg.BIGINT]
    assert run(pkg, ctx, types, [0], [Fn(ROW_NUMBER)], [0], [1], [1], []) == []
    empty = pkg.Page(pkg.Block(pkg.BIGINT, np.zeros(0, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.zeros(0, dtype=np.int64)))
    assert run(pkg, ctx, types, [0], [Fn(ROW_NUMBER)], [0], [1], [1], [empty]) == []
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array([2, 1, 2], dtype=np.int64)), pkg.Block(pkg.BIGINT, np.array([5, 6, 4], dtype=np.int64)))
    factory = pkg.WindowOperatorFactory(ctx, 1, types, [1], [pkg.WindowFunction(pkg.WINDOW_ROW_NUMBER)], [0], [1], [pkg.ASC_NULLS_LAST])
    twin = factory.duplicate()
    for f in (factory, twin):
        op = f.createOperator()
        op.addInput(page)
        op.finish()
        with pytest.raises(pkg.TgpuError) as e:
            op.addInput(page)
        assert e.value.code == -5   # "Operator is already finishing"
        out = op.getOutput()
        assert out.to_host().rows() == [(6, 1), (4, 1), (5, 2)]
        out.release()
        assert op.isFinished()
        op.close()

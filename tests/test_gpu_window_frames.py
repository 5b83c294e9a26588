"""WindowOperator under frames with bounds on the GPU (tgpu_window_factory_create_framed), against tests/window_frames_expected.py (a row-by-row
Python restatement of the reference's getFrameRange that recomputes every function over its frame from scratch): the reference's cases
(tests/golden/window_frame_vectors.json), the three old frames through the framed entry point, random tables with every function under every valid
ROWS / GROUPS bound combination with per-row and constant offsets, row counts and partition heads around wave / block / tile edges under
TGPU_WINDOW_TILE_ROWS=256, min / max over frames inside a chunk of the range-extreme index, across two, across many and wider than the partition,
offsets beyond every partition, the sum's frame-local overflow rule, the offset and argument errors, nth_value over every type, ntile, one larger
shape checked in closed form, and the protocol.  Every comparison is exact: values bit for bit, nulls, row order."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from distinct_gpu import key_block
from window_expected import (AGGREGATE, COUNT_ALL, COUNT_COLUMN, CUME_DIST, DENSE_RANK, FIRST_VALUE, FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT, LAG, LAST_VALUE,
                             LEAD, MAX_BIGINT, MAX_DOUBLE, MIN_BIGINT, MIN_DOUBLE, PERCENT_RANK, RANK, ROW_NUMBER, SUM_BIGINT, Fn, tokens)
from window_frames_expected import (CURRENT_ROW, FOLLOWING, GROUPS, NTH_VALUE, NTILE, PRECEDING, RANGE, ROWS, UNBOUNDED_FOLLOWING, UNBOUNDED_PRECEDING, Frame, expected_output,
                                    golden_case, golden_group_case, valid_bounds)

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "window_frame_vectors.json")))
ORDERS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}
TILE = "TGPU_WINDOW_TILE_ROWS"
SMALL = {TILE: "256"}
NP = {1: np.int64, 2: np.int32, 3: np.int32, 4: np.float64, 5: np.uint8}
AGGS = (COUNT_ALL, COUNT_COLUMN, SUM_BIGINT, MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE)
COMBINATIONS = [(s, e) for s in range(5) for e in range(5) if valid_bounds(s, e)]   # 13
OLD_AS_FRAMES = {FRAME_PARTITION: Frame(RANGE, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING), FRAME_RANGE_TO_CURRENT: Frame(RANGE, UNBOUNDED_PRECEDING, CURRENT_ROW),
                 FRAME_ROWS_TO_CURRENT: Frame(ROWS, UNBOUNDED_PRECEDING, CURRENT_ROW)}


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


def window_function(pkg, f):
    frame = pkg.WindowFrame(f.frame.type, f.frame.start, f.frame.end, f.frame.start_channel, f.frame.end_channel) if isinstance(f.frame, Frame) else f.frame
    return pkg.WindowFunction(f.function, f.args, frame, f.agg)


def create(pkg, ctx, types, outputs, functions, partitions, sorts, orders, env=None):
    """one operator; the tile switch is read when it is created"""
    env = env or {}
    os.environ.update(env)
    try:
        return pkg.WindowOperatorFactory(ctx, 1, types, outputs, [window_function(pkg, f) for f in functions], partitions, sorts, orders).createOperator()
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
    for i, f in enumerate(functions):
        b = out.getBlock(len(outputs) + i)
        if f.function in (ROW_NUMBER, RANK, DENSE_RANK) or (f.function == AGGREGATE and f.agg in (COUNT_ALL, COUNT_COLUMN)):
            assert b.type == pkg.BIGINT and (b.nulls is None or not b.nulls.any())
        elif f.function in (PERCENT_RANK, CUME_DIST):
            assert b.type == pkg.DOUBLE
        elif f.function == AGGREGATE:
            assert b.type == (pkg.DOUBLE if f.agg in (MIN_DOUBLE, MAX_DOUBLE) else pkg.BIGINT)
        elif f.function == NTILE:
            assert b.type == pkg.BIGINT
        else:
            assert b.type == types[f.args[0]]
    return tokens(out.rows())


def check(pkg, ctx, types, outputs, functions, partitions, sorts, orders, pages, envs=({},), operators=None):
    """`functions` in operators of at most 16 (or as `operators` slices them), each against the helper's columns, which are computed once for all of them"""
    expected = tokens(expected_output(types, [p.rows() for p in pages], outputs, functions, partitions, sorts, orders))
    k = len(outputs)
    slices = operators or [(at, min(at + 16, len(functions))) for at in range(0, len(functions), 16)]
    for lo, hi in slices:
        want = [r[:k] + r[k + lo:k + hi] for r in expected]
        for env in envs:
            got = run(pkg, ctx, types, outputs, functions[lo:hi], partitions, sorts, orders, pages, env)
            assert got == want, (env, lo, hi, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:3], len(got), len(want))
    return expected


def table(pkg, rng, sizes, partitions, sort_domain=20, nulls=0.1):
    """channels: 0 BIGINT partition key, 1 BIGINT sort key (ties), 2 BIGINT row id, 3 BIGINT values with nulls, 4 DOUBLE values with nulls / NaN / zeros,
    5 VARCHAR values with nulls, 6 BIGINT offsets 0 .. 3 with nulls (lag / lead), 7 VARCHAR defaults, 8 BIGINT frame offsets 0 .. 4, 9 INTEGER frame offsets 0 .. 4,
    10 / 11 / 12 BIGINT constants 0 / 1 / 3, 13 BIGINT nth offsets 1 .. 4 with nulls, 14 BIGINT buckets 1 .. 9 with nulls"""
    pages, at = [], 0
    for n in sizes:
        d = rng.integers(-3, 4, n).astype(np.float64)
        d[rng.random(n) < 0.05] = np.nan
        d[rng.random(n) < 0.05] = -0.0
        const = lambda v: pkg.Block(pkg.BIGINT, np.full(n, v, dtype=np.int64))
        pages.append(pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, partitions, n).astype(np.int64)), pkg.Block(pkg.BIGINT, rng.integers(0, sort_domain, n).astype(np.int64)),
                              pkg.Block(pkg.BIGINT, np.arange(at, at + n, dtype=np.int64)),
                              pkg.Block(pkg.BIGINT, rng.integers(-1000, 1000, n).astype(np.int64), (rng.random(n) < nulls).astype(np.uint8)),
                              pkg.Block(pkg.DOUBLE, d, (rng.random(n) < nulls).astype(np.uint8)), key_block(pkg, rng, pkg.VARCHAR, n, 30, nulls),
                              pkg.Block(pkg.BIGINT, rng.integers(0, 4, n).astype(np.int64), (rng.random(n) < nulls).astype(np.uint8)),
                              pkg.Block(pkg.VARCHAR, ["d%d" % i for i in range(at, at + n)]),
                              pkg.Block(pkg.BIGINT, rng.integers(0, 5, n).astype(np.int64)), pkg.Block(pkg.INTEGER, rng.integers(0, 5, n).astype(np.int32)),
                              const(0), const(1), const(3),
                              pkg.Block(pkg.BIGINT, rng.integers(1, 5, n).astype(np.int64), (rng.random(n) < nulls).astype(np.uint8)),
                              pkg.Block(pkg.BIGINT, rng.integers(1, 10, n).astype(np.int64), (rng.random(n) < nulls).astype(np.uint8))))
        at += n
    return [pkg.BIGINT] * 4 + [pkg.DOUBLE, pkg.VARCHAR, pkg.BIGINT, pkg.VARCHAR, pkg.BIGINT, pkg.INTEGER] + [pkg.BIGINT] * 5, pages


def framed_functions(frame):
    """every function that reads its frame, under `frame`, over the channels of table()"""
    args = {COUNT_ALL: (), COUNT_COLUMN: (5,), SUM_BIGINT: (3,), MIN_BIGINT: (3,), MAX_BIGINT: (3,), MIN_DOUBLE: (4,), MAX_DOUBLE: (4,)}
    return [Fn(AGGREGATE, args[a], frame, a) for a in AGGS] + [Fn(FIRST_VALUE, (5,), frame), Fn(LAST_VALUE, (4,), frame), Fn(NTH_VALUE, (5, 13), frame)]


def every_frame():
    """ROWS and GROUPS frames of each valid bound combination; the offset sources rotate through the per-row BIGINT channel, the per-row INTEGER channel and
    the constants 0, 1 and 3, start and end one step apart, so that every source meets every bound type on both sides"""
    sources, frames, turn = (8, 10, 9, 11, 12), [], 0
    for kind in (ROWS, GROUPS):
        for s, e in COMBINATIONS:
            frames.append(Frame(kind, s, e, sources[turn % 5] if s in (PRECEDING, FOLLOWING) else -1, sources[(turn + 1) % 5] if e in (PRECEDING, FOLLOWING) else -1))
            turn += 1
    return frames


# ---- 1. the reference's cases ---------------------------------------------------------------------------------------------------------------
def multiset(rows):
    return sorted(map(repr, rows))


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_reference_cases(pkg, ctx, case):
    types, pages_rows, functions, expected = golden_case(case)
    pages = [page_of(pkg, types, rows) for rows in pages_rows]
    got = run(pkg, ctx, types, case["output_channels"], functions, case["partition_channels"], case["sort_channels"], [ORDERS[o] for o in case["sort_orders"]], pages)
    assert multiset(got) == multiset(tokens(expected))   # the reference compares these ignoring order


@pytest.mark.parametrize("case", GOLD["groups"], ids=lambda c: c["name"])
def test_reference_groups_cases(pkg, ctx, case):
    """count(*), count(a), first_value(a), last_value(a), min(a), max(a) derived from the listed array_agg(a) frames"""
    types, pages_rows, functions, expected = golden_group_case(case)
    pages = [page_of(pkg, types, rows) for rows in pages_rows]
    got = run(pkg, ctx, types, case["output_channels"], functions, case["partition_channels"], case["sort_channels"], [ORDERS[o] for o in case["sort_orders"]], pages)
    assert multiset(got) == multiset(tokens(expected))


# ---- 2. the old frames through the framed entry point -------------------------------------------------------------------------------------
def test_the_three_old_frames_through_the_framed_entry_point_give_the_old_page(pkg, ctx):
    rng = np.random.default_rng(21)
    types, pages = table(pkg, rng, [1023, 1, 2049, 640, 1287], 7)
    old = [Fn(ROW_NUMBER), Fn(RANK), Fn(DENSE_RANK), Fn(PERCENT_RANK), Fn(CUME_DIST), Fn(LAG, (5, 6, 7)), Fn(LEAD, (5, 6, 7)), Fn(FIRST_VALUE, (5,), FRAME_ROWS_TO_CURRENT),
           Fn(LAST_VALUE, (5,), FRAME_RANGE_TO_CURRENT)]
    args = {COUNT_ALL: (), COUNT_COLUMN: (5,), SUM_BIGINT: (3,), MIN_BIGINT: (3,), MAX_BIGINT: (3,), MIN_DOUBLE: (4,), MAX_DOUBLE: (4,)}
    old += [Fn(AGGREGATE, args[a], i % 3, a) for i, a in enumerate(AGGS)]
    framed = [Fn(f.function, f.args, OLD_AS_FRAMES[f.frame], f.agg) for f in old]
    assert len(old) == 16 and not any(window_function(pkg, f).framed() for f in old) and all(window_function(pkg, f).framed() for f in framed)
    for env in ({}, SMALL):
        a = run(pkg, ctx, types, [2, 0], old, [0], [1], [1], pages, env)
        b = run(pkg, ctx, types, [2, 0], framed, [0], [1], [1], pages, env)
        assert a == b and len(a) == 5000


# ---- 3. random tables, every function under every frame ------------------------------------------------------------------------------------
@pytest.mark.parametrize("partitions", [1, 7, 1000])
def test_random_rows_with_every_function_under_every_rows_and_groups_frame(pkg, ctx, partitions):
    """5 000 rows in uneven pages with sort ties, nulls, NaN and both zeros; 26 frames x 10 functions in operators of 10 (7 of them aggregates: two scan
    runs each), then the functions that ignore their frame with ntile in one operator"""
    rng = np.random.default_rng(300 + partitions)
    types, pages = table(pkg, rng, [1023, 1, 2049, 640, 1287], partitions)
    frames = every_frame()
    assert len(frames) == 26 and {f.start_channel for f in frames} | {f.end_channel for f in frames} == {-1, 8, 9, 10, 11, 12}
    functions = [f for frame in frames for f in framed_functions(frame)]
    some = frames[5]
    functions += [Fn(ROW_NUMBER, (), some), Fn(RANK, (), some), Fn(DENSE_RANK, (), some), Fn(PERCENT_RANK, (), some), Fn(CUME_DIST, (), some), Fn(LAG, (5, 6, 7), some),
                  Fn(LEAD, (5, 6, 7), some), Fn(NTILE, (14,), some), Fn(NTILE, (12,), FRAME_PARTITION)]
    operators = [(at, at + 10) for at in range(0, 260, 10)] + [(260, 269)]
    assert sum(f.function == AGGREGATE for f in functions[:10]) > 4
    check(pkg, ctx, types, [2, 0], functions, [0], [1], [1], pages, envs=[SMALL if partitions == 7 else {}], operators=operators)


# ---- 4. row counts and tile edges ---------------------------------------------------------------------------------------------------------------
def shaped(pkg, part_keys, sort_keys=None, seed=0):
    """one page: 0 the partition key, 1 the sort key, 2 BIGINT values with nulls, 3 / 4 the constants 2 / 1; keys ascending so that the sort leaves the rows where they are"""
    n = len(part_keys)
    rng = np.random.default_rng(seed + n)
    sort_keys = np.arange(n) if sort_keys is None else sort_keys
    return [pkg.BIGINT] * 5, [pkg.Page(pkg.Block(pkg.BIGINT, np.asarray(part_keys, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.asarray(sort_keys, dtype=np.int64)),
                                       pkg.Block(pkg.BIGINT, rng.integers(-9, 10, n).astype(np.int64), (rng.random(n) < 0.1).astype(np.uint8)),
                                       pkg.Block(pkg.BIGINT, np.full(n, 2, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.full(n, 1, dtype=np.int64)))]


ROWS_2_2 = Frame(ROWS, PRECEDING, FOLLOWING, 3, 3)       # ROWS BETWEEN 2 PRECEDING AND 2 FOLLOWING
GROUPS_1_1 = Frame(GROUPS, PRECEDING, FOLLOWING, 4, 4)   # GROUPS BETWEEN 1 PRECEDING AND 1 FOLLOWING
EDGE_FUNCTIONS = [Fn(AGGREGATE, a, frame, agg) for frame in (ROWS_2_2, GROUPS_1_1) for agg, a in ((COUNT_ALL, ()), (SUM_BIGINT, (2,)), (MIN_BIGINT, (2,)), (MAX_BIGINT, (2,)))] + \
                 [Fn(FIRST_VALUE, (2,), ROWS_2_2), Fn(LAST_VALUE, (2,), GROUPS_1_1)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 3 * 256 + 17])
def test_row_counts_around_wave_block_and_tile(pkg, ctx, n):
    """one partition across all tiles (frames straddle every tile edge); a partition head on each tile edge (rows 256 k) and partitions of one row"""
    on_edges = np.arange(n) // 256
    singles = np.where(np.arange(n) % 7 == 0, 2 * np.arange(n), 2 * (np.arange(n) // 7 * 7) + 1)   # every 7th row a partition of its own
    for keys in (np.zeros(n), on_edges, singles):
        types, pages = shaped(pkg, keys, np.arange(n) // 3)
        check(pkg, ctx, types, [1], EDGE_FUNCTIONS, [0], [1], [1], pages, envs=[SMALL])


# ---- 5. min / max over frames of every shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partition_sizes", [(1500,), (700, 1, 799)])
def test_min_and_max_over_frames_inside_a_chunk_across_chunks_and_wider_than_the_partition(pkg, ctx, partition_sizes):
    """frame widths 1, 2, 3, 255, 256, 257 and 1100 (a PRECEDING + b FOLLOWING + 1) over BIGINT and DOUBLE values with NaN, both zeros and runs of 300
    nulls: an all-null frame gives null"""
    n = 1500
    rng = np.random.default_rng(55)
    ints = rng.integers(-10**6, 10**6, n).astype(np.int64)
    d = rng.integers(-5, 6, n).astype(np.float64)
    d[rng.random(n) < 0.1] = np.nan
    d[rng.random(n) < 0.1] = -0.0
    nulls = (rng.random(n) < 0.05).astype(np.uint8)
    nulls[200:500] = 1
    nulls[900:1200] = 1
    d[520:700] = np.nan   # a run of NaN: min and max are NaN there
    keys = np.repeat(np.arange(len(partition_sizes)), partition_sizes)
    widths = [(0, 0), (1, 0), (1, 1), (127, 127), (100, 155), (128, 128), (500, 599)]
    assert [a + b + 1 for a, b in widths] == [1, 2, 3, 255, 256, 257, 1100]
    cols = [pkg.Block(pkg.BIGINT, keys.astype(np.int64)), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64)), pkg.Block(pkg.BIGINT, ints, nulls), pkg.Block(pkg.DOUBLE, d, nulls)]
    types = [pkg.BIGINT, pkg.BIGINT, pkg.BIGINT, pkg.DOUBLE]
    functions = []
    for a, b in widths:
        cols += [pkg.Block(pkg.BIGINT, np.full(n, a, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.full(n, b, dtype=np.int64))]
        types += [pkg.BIGINT, pkg.BIGINT]
        frame = Frame(ROWS, PRECEDING, FOLLOWING, len(cols) - 2, len(cols) - 1)
        functions += [Fn(AGGREGATE, (2,), frame, MIN_BIGINT), Fn(AGGREGATE, (2,), frame, MAX_BIGINT), Fn(AGGREGATE, (3,), frame, MIN_DOUBLE), Fn(AGGREGATE, (3,), frame, MAX_DOUBLE)]
    # both-bounded frames that start behind the partition's first row and end at its last, and the mirror image
    functions += [Fn(AGGREGATE, (2,), Frame(ROWS, PRECEDING, UNBOUNDED_FOLLOWING, 6), MAX_BIGINT), Fn(AGGREGATE, (3,), Frame(ROWS, FOLLOWING, UNBOUNDED_FOLLOWING, 6), MIN_DOUBLE),
                  Fn(AGGREGATE, (2,), Frame(ROWS, UNBOUNDED_PRECEDING, PRECEDING, -1, 6), MIN_BIGINT), Fn(AGGREGATE, (3,), Frame(ROWS, CURRENT_ROW, FOLLOWING, -1, 10), MAX_DOUBLE)]
    expected = check(pkg, ctx, types, [1], functions, [0], [1], [1], [pkg.Page(*cols)], envs=[SMALL])
    assert any(r[1] is None for r in expected) and not all(r[-1] is None for r in expected)


# ---- 6. offsets larger than the partition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [50, 2**40, 2**63 - 1])
def test_offsets_beyond_the_partition_under_each_bound(pkg, ctx, offset):
    n = 40
    rng = np.random.default_rng(6)
    cols = [pkg.Block(pkg.BIGINT, (np.arange(n) // 13).astype(np.int64)), pkg.Block(pkg.BIGINT, (np.arange(n) // 2).astype(np.int64)),
            pkg.Block(pkg.BIGINT, rng.integers(-9, 10, n).astype(np.int64), (rng.random(n) < 0.1).astype(np.uint8)), pkg.Block(pkg.BIGINT, np.full(n, offset, dtype=np.int64)),
            pkg.Block(pkg.BIGINT, np.full(n, 1, dtype=np.int64))]
    functions = []
    for kind in (ROWS, GROUPS):
        for s, e in COMBINATIONS:
            if s not in (PRECEDING, FOLLOWING) and e not in (PRECEDING, FOLLOWING):
                continue
            for big_start in (True, False):   # the large offset on one side, 1 on the other; on both sides where only one variant exists
                frame = Frame(kind, s, e, (3 if big_start else 4) if s in (PRECEDING, FOLLOWING) else -1, (4 if big_start else 3) if e in (PRECEDING, FOLLOWING) else -1)
                functions += [Fn(AGGREGATE, (), frame, COUNT_ALL), Fn(AGGREGATE, (2,), frame, SUM_BIGINT), Fn(AGGREGATE, (2,), frame, MAX_BIGINT), Fn(FIRST_VALUE, (2,), frame)]
            both = Frame(kind, s, e, 3 if s in (PRECEDING, FOLLOWING) else -1, 3 if e in (PRECEDING, FOLLOWING) else -1)
            functions += [Fn(AGGREGATE, (), both, COUNT_ALL), Fn(LAST_VALUE, (2,), both)]
    check(pkg, ctx, [pkg.BIGINT] * 5, [1], functions, [0], [1], [1], [pkg.Page(*cols)])


# ---- 7. sum --------------------------------------------------------------------------------------------------------------------------------------
TWO_ROWS = Frame(ROWS, PRECEDING, CURRENT_ROW, 2)   # ROWS BETWEEN 1 PRECEDING AND CURRENT ROW


def sums(pkg, ctx, values, partitions=None, frame=TWO_ROWS, env=None):
    n = len(values)
    cols = [pkg.Block(pkg.BIGINT, np.array([0 if v is None else v for v in values], dtype=np.int64), np.array([v is None for v in values], dtype=np.uint8)),
            pkg.Block(pkg.BIGINT, np.array(partitions if partitions is not None else [0] * n, dtype=np.int64)), pkg.Block(pkg.BIGINT, np.full(n, 1, dtype=np.int64))]
    got = run(pkg, ctx, [pkg.BIGINT] * 3, [], [Fn(AGGREGATE, (0,), frame, SUM_BIGINT)], [1], [], [], [pkg.Page(*cols)], env)
    return [r[0] for r in got]


def test_partition_prefixes_may_leave_int64_while_every_frame_fits(pkg, ctx):
    big = 2**62
    values = [big, big - 1, 5, big - 1, 3, None, big - 1, -big, -big, -big, -big, 7]   # prefixes reach 3 * 2^62 and come back below -2^62
    want = [big, 2 * big - 1, big + 4, big + 4, big + 2, 3, big - 1, -1, -2 * big, -2 * big, -2 * big, 7 - big]
    assert sums(pkg, ctx, values) == want and -2 * big == -2**63
    # across tiles of 256: the running sum's high word travels through the carries
    long = ([big, big - 1] + [0] * 300) * 3
    got = sums(pkg, ctx, long, env=SMALL)
    assert got == [(long[i] + (long[i - 1] if i else 0)) for i in range(len(long))] and max(got) == 2**63 - 1


def test_a_frame_whose_sum_is_2_to_the_63_fails(pkg, ctx):
    big = 2**62
    with pytest.raises(pkg.TgpuError) as e:
        sums(pkg, ctx, [1, big, big, -5])
    assert e.value.code == -2 and e.value.message == "bigint addition overflow"
    assert sums(pkg, ctx, [1, big, big - 1, -5]) == [1, big + 1, 2**63 - 1, big - 6]
    with pytest.raises(pkg.TgpuError) as e:   # below: -2^63 fits, -2^63 - 1 does not
        sums(pkg, ctx, [-big, -big - 1])
    assert e.value.code == -2
    assert sums(pkg, ctx, [-big, -big]) == [-big, -2**63]


def test_the_same_prefix_overflow_under_an_old_frame_still_fails(pkg, ctx):
    big = 2**62
    values = [big, big - 1, 5, big - 1]
    assert sums(pkg, ctx, values) == [big, 2 * big - 1, big + 4, big + 4]
    for frame in (FRAME_ROWS_TO_CURRENT, FRAME_RANGE_TO_CURRENT, FRAME_PARTITION, OLD_AS_FRAMES[FRAME_ROWS_TO_CURRENT], OLD_AS_FRAMES[FRAME_PARTITION]):
        with pytest.raises(pkg.TgpuError) as e:
            sums(pkg, ctx, values, frame=frame)
        assert e.value.code == -2 and e.value.message == "bigint addition overflow"


def test_an_overflow_in_one_partition_fails_whatever_the_others_do(pkg, ctx):
    big = 2**62
    values = [1, 2, 3, big, big, 5, 6]
    with pytest.raises(pkg.TgpuError) as e:
        sums(pkg, ctx, values, partitions=[0, 0, 0, 1, 1, 2, 2])
    assert e.value.code == -2 and e.value.message == "bigint addition overflow"
    assert sums(pkg, ctx, values, partitions=[0, 0, 0, 1, 2, 2, 2]) == [1, 3, 5, big, big, big + 5, 11]   # the head cuts the frame


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------
def failing(pkg, ctx, types, functions, rows, code, message):
    op = create(pkg, ctx, types, [0], functions, [], [0], [1])
    op.addInput(page_of(pkg, types, rows))
    op.finish()
    with pytest.raises(pkg.TgpuError) as e:
        op.getOutput()
    assert e.value.code == code and e.value.message == message
    op.close()   # the operator can be closed afterwards


def test_offset_and_argument_errors_fail_get_output(pkg, ctx):
    types = [pkg.BIGINT, pkg.BIGINT, pkg.BIGINT, pkg.INTEGER]
    rows = lambda bad, integer=1: [(i, 1 if i != 3 else bad, 1, 1 if i != 3 else integer) for i in range(6)]
    count = lambda frame: [Fn(AGGREGATE, (), frame, COUNT_ALL)]
    for kind in (ROWS, GROUPS):
        failing(pkg, ctx, types, count(Frame(kind, PRECEDING, FOLLOWING, 1, 2)), rows(None), -1, "Window frame starting offset must not be null")
        failing(pkg, ctx, types, count(Frame(kind, PRECEDING, FOLLOWING, 2, 1)), rows(None), -1, "Window frame ending offset must not be null")
        failing(pkg, ctx, types, count(Frame(kind, UNBOUNDED_PRECEDING, PRECEDING, -1, 1)), rows(None), -1, "Window frame ending offset must not be null")
        failing(pkg, ctx, types, count(Frame(kind, FOLLOWING, UNBOUNDED_FOLLOWING, 1)), rows(None), -1, "Window frame starting offset must not be null")
        for bad in (-1, -2**63):
            failing(pkg, ctx, types, count(Frame(kind, PRECEDING, FOLLOWING, 1, 2)), rows(bad), -1, "Window frame offset must not be negative")
            failing(pkg, ctx, types, count(Frame(kind, CURRENT_ROW, FOLLOWING, -1, 1)), rows(bad), -1, "Window frame offset must not be negative")
        failing(pkg, ctx, types, count(Frame(kind, PRECEDING, CURRENT_ROW, 3)), rows(1, None), -1, "Window frame starting offset must not be null")   # an INTEGER offset
        failing(pkg, ctx, types, count(Frame(kind, PRECEDING, CURRENT_ROW, 3)), rows(1, -7), -1, "Window frame offset must not be negative")
    whole = Frame(ROWS, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING)
    for bad in (0, -3):
        failing(pkg, ctx, types, [Fn(NTH_VALUE, (0, 1), whole)], rows(bad), -1, "Offset must be at least 1")
    for bad in (0, -1):
        failing(pkg, ctx, types, [Fn(NTILE, (1,), whole)], rows(bad), -1, "Buckets must be greater than 0")
    # a null nth offset or null buckets is a null, not an error; an offset below 1 in a row whose frame is empty is not looked at (NthValueFunction.java:44)
    got = run(pkg, ctx, types, [0], [Fn(NTH_VALUE, (0, 1), whole), Fn(NTILE, (1,), whole), Fn(NTH_VALUE, (0, 1), Frame(ROWS, FOLLOWING, FOLLOWING, 2, 2))], [], [0], [1],
              [page_of(pkg, types, rows(None))])
    assert got == [(0, 0, 1, 1), (1, 0, 1, 2), (2, 0, 1, 3), (3, None, None, None), (4, 0, 1, 5), (5, 0, 1, None)]
    got = run(pkg, ctx, types, [0], [Fn(NTH_VALUE, (0, 1), Frame(ROWS, FOLLOWING, FOLLOWING, 2, 2))], [], [0], [1], [page_of(pkg, types, [(0, 1, 1, 1), (1, 0, 1, 1)])])
    assert got == [(0, 1), (1, None)]


def test_creation_errors(pkg, ctx):
    types = [pkg.BIGINT, pkg.DOUBLE, pkg.INTEGER]
    make = lambda f: create(pkg, ctx, types, [0], [f], [], [0], [1])
    for frame, code, text in ((Frame(RANGE, PRECEDING, CURRENT_ROW, 0), -8, "RANGE frames with an offset are not supported"),
                              (Frame(RANGE, CURRENT_ROW, FOLLOWING, -1, 2), -8, "RANGE frames with an offset are not supported"),
                              (Frame(ROWS, CURRENT_ROW, PRECEDING, -1, 0), -1, "invalid window frame bounds"), (Frame(ROWS, FOLLOWING, CURRENT_ROW, 0), -1, "invalid window frame bounds"),
                              (Frame(GROUPS, UNBOUNDED_FOLLOWING, UNBOUNDED_FOLLOWING), -1, "invalid window frame bounds"),
                              (Frame(ROWS, UNBOUNDED_PRECEDING, UNBOUNDED_PRECEDING), -1, "invalid window frame bounds"), (Frame(3, 0, 2), -1, "unknown window frame type"),
                              (Frame(ROWS, 5, 2), -1, "unknown window frame bound"), (Frame(ROWS, PRECEDING, CURRENT_ROW, 3), -1, "frame offset channel out of range"),
                              (Frame(GROUPS, CURRENT_ROW, FOLLOWING, -1, 1), -1, "a frame offset must be BIGINT or INTEGER")):
        with pytest.raises(pkg.TgpuError) as e:
            make(Fn(AGGREGATE, (), frame, COUNT_ALL))
        assert (e.value.code, e.value.message) == (code, text)
    with pytest.raises(pkg.TgpuError) as e:
        make(Fn(NTH_VALUE, (0, 2), Frame(ROWS, UNBOUNDED_PRECEDING, CURRENT_ROW)))
    assert e.value.code == -1
    with pytest.raises(pkg.TgpuError) as e:   # the old entry point keeps refusing the new function codes
        h = C.c_void_p()
        spec = (pkg._lib.WindowFunctionSpec * 1)(pkg.WindowFunction(pkg.WINDOW_NTILE, (0,), FRAME_PARTITION).spec())
        t = (C.c_int32 * 3)(*types)
        o = (C.c_int32 * 1)(0)
        pkg._lib.check(pkg._lib.lib().tgpu_window_factory_create(ctx.handle, 1, 3, t, 1, o, 1, spec, 0, None, 1, o, (C.c_int32 * 1)(1), 10, C.byref(h)))
    assert e.value.code == -1 and e.value.message == "unknown window function"
    with pytest.raises(pkg.TgpuError) as e:
        pkg.WindowOperatorFactory(ctx, 1, types, [0], [pkg.WindowFunction(pkg.WINDOW_NTH_VALUE, (0, 0), pkg.WindowFrame(1, 0, 2), ignore_nulls=True)], [], [0], [1])
    assert e.value.code == -8 and e.value.message == "IGNORE NULLS is not supported"


# ---- 9. nth_value over every type, ntile ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE", "DOUBLE", "BOOLEAN", "VARCHAR"])
def test_nth_value_over_every_value_type(pkg, ctx, type_name):
    rng = np.random.default_rng(90 + len(type_name))
    t = getattr(pkg, type_name)
    n = 600
    cols = [pkg.Block(pkg.BIGINT, rng.integers(0, 9, n).astype(np.int64)), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64)), key_block(pkg, rng, t, n, 40, 0.15),
            pkg.Block(pkg.BIGINT, rng.integers(1, 7, n).astype(np.int64), (rng.random(n) < 0.1).astype(np.uint8)), pkg.Block(pkg.BIGINT, np.full(n, 2, dtype=np.int64))]
    types = [pkg.BIGINT, pkg.BIGINT, t, pkg.BIGINT, pkg.BIGINT]
    functions = [Fn(NTH_VALUE, (2, 3), Frame(ROWS, PRECEDING, FOLLOWING, 4, 4)), Fn(NTH_VALUE, (2, 3), Frame(ROWS, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING)),
                 Fn(NTH_VALUE, (2, 4), Frame(RANGE, UNBOUNDED_PRECEDING, CURRENT_ROW)), Fn(NTH_VALUE, (2, 3), Frame(GROUPS, CURRENT_ROW, FOLLOWING, -1, 4)),
                 Fn(NTH_VALUE, (2, 3), Frame(ROWS, FOLLOWING, FOLLOWING, 4, 4)), Fn(FIRST_VALUE, (2,), Frame(ROWS, PRECEDING, PRECEDING, 4, 4)),
                 Fn(LAST_VALUE, (2,), Frame(GROUPS, FOLLOWING, UNBOUNDED_FOLLOWING, 4))]
    check(pkg, ctx, types, [1], functions, [0], [1], [1], [pkg.Page(*cols)], envs=[SMALL])


def test_ntile_buckets(pkg, ctx):
    """buckets 1, equal to the rows, more than the rows, not dividing them, 2^62, per row, and null; partitions of 10, 1 and 7 rows"""
    sizes = (10, 1, 7)
    n = sum(sizes)
    keys = np.repeat(np.arange(3), sizes)
    per_partition = np.repeat(np.array(sizes), sizes)
    buckets = [np.full(n, 1), per_partition, per_partition + 5, np.full(n, 3), np.full(n, 4), np.full(n, 2**62), np.arange(n) % 5 + 1]
    cols = [pkg.Block(pkg.BIGINT, keys.astype(np.int64)), pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64))] + [pkg.Block(pkg.BIGINT, b.astype(np.int64)) for b in buckets]
    cols.append(pkg.Block(pkg.BIGINT, np.full(n, 3, dtype=np.int64), (np.arange(n) % 4 == 0).astype(np.uint8)))
    functions = [Fn(NTILE, (2 + i,), FRAME_RANGE_TO_CURRENT) for i in range(len(buckets) + 1)]
    expected = check(pkg, ctx, [pkg.BIGINT] * len(cols), [1], functions, [0], [1], [1], [pkg.Page(*cols)])
    assert [r[4] for r in expected[:10]] == [1, 1, 1, 1, 2, 2, 2, 3, 3, 3] and [r[5] for r in expected[:10]] == [1, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    assert [r[2] for r in expected[:10]] == list(range(1, 11)) and expected[10][1:8] == (1,) * 7 and expected[0][8] is None


# ---- 10. one larger shape at the default tile, in closed form --------------------------------------------------------------------------------------
def test_a_million_rows_in_closed_form(pkg, ctx):
    """2^20 rows in 1000 partitions, sorted by a unique id that is also the value; a partition holds consecutive ids: ROWS BETWEEN 5 PRECEDING AND 9 FOLLOWING
    from the row's position r and its partition's last position E alone"""
    n, parts = 2**20, 1000
    rng = np.random.default_rng(10)
    ids = rng.permutation(n).astype(np.int64)
    keys = ids * parts // n
    const = lambda v: pkg.Block(pkg.BIGINT, np.full(n, v, dtype=np.int64))
    page = pkg.Page(pkg.Block(pkg.BIGINT, keys), pkg.Block(pkg.BIGINT, ids), const(5), const(9))
    frame = pkg.WindowFrame(pkg.FRAME_TYPE_ROWS, pkg.BOUND_PRECEDING, pkg.BOUND_FOLLOWING, 2, 3)
    fns = [pkg.WindowFunction(pkg.WINDOW_AGGREGATE, a, frame, agg) for agg, a in ((pkg.COUNT_ALL, ()), (pkg.SUM_BIGINT, (1,)), (pkg.MIN_BIGINT, (1,)), (pkg.MAX_BIGINT, (1,)))]
    op = pkg.WindowOperatorFactory(ctx, 1, [pkg.BIGINT] * 4, [0, 1], fns, [0], [1], [pkg.ASC_NULLS_LAST]).createOperator()
    out = drive(op, [page])
    assert op.memoryBytes() > 0
    op.close()
    order = np.lexsort((ids, keys))
    k, v = keys[order], ids[order]
    assert np.array_equal(out.getBlock(0).values, k) and np.array_equal(out.getBlock(1).values, v)
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    sizes = np.diff(np.r_[starts, n])
    first = np.repeat(starts, sizes)
    r = np.arange(n) - first
    last = np.repeat(sizes, sizes) - 1
    lo, hi = first + np.maximum(r - 5, 0), first + np.minimum(r + 9, last)
    assert np.array_equal(out.getBlock(2).values, np.minimum(r, 5) + np.minimum(last - r, 9) + 1)
    assert np.array_equal(np.diff(v), np.ones(n - 1, dtype=np.int64)) and len(sizes) == parts
    assert np.array_equal(out.getBlock(3).values, (v[lo] + v[hi]) * (hi - lo + 1) // 2)   # an arithmetic series
    assert np.array_equal(out.getBlock(4).values, v[lo]) and np.array_equal(out.getBlock(5).values, v[hi])
    for c in (2, 3, 4, 5):
        assert out.getBlock(c).nulls is None or not out.getBlock(c).nulls.any()


# ---- 11. lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_empty_input_finish_protocol_and_duplicate(pkg, ctx):
    types = [pkg.BIGINT, pkg.BIGINT, pkg.BIGINT]
    count = [Fn(AGGREGATE, (), Frame(ROWS, PRECEDING, FOLLOWING, 2, 2), COUNT_ALL)]
    assert run(pkg, ctx, types, [0], count, [0], [1], [1], []) == []
    zero = lambda: pkg.Block(pkg.BIGINT, np.zeros(0, dtype=np.int64))
    assert run(pkg, ctx, types, [0], count, [0], [1], [1], [pkg.Page(zero(), zero(), zero())]) == []
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array([2, 1, 2, 2], dtype=np.int64)), pkg.Block(pkg.BIGINT, np.array([5, 6, 4, 7], dtype=np.int64)),
                    pkg.Block(pkg.BIGINT, np.array([1, 1, 1, 1], dtype=np.int64)))
    factory = pkg.WindowOperatorFactory(ctx, 1, types, [1], [window_function(pkg, count[0]), pkg.WindowFunction(pkg.WINDOW_NTILE, (2,))], [0], [1], [pkg.ASC_NULLS_LAST])
    twin = factory.duplicate()
    for f in (factory, twin):
        op = f.createOperator()
        op.addInput(page)
        op.finish()
        with pytest.raises(pkg.TgpuError) as e:
            op.addInput(page)
        assert e.value.code == -5   # "Operator is already finishing"
        out = op.getOutput()
        assert out.to_host().rows() == [(6, 1, 1), (4, 2, 1), (5, 3, 1), (7, 2, 1)]
        out.release()
        assert op.isFinished()
        op.close()

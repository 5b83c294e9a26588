"""WindowOperator under RANGE frames with k PRECEDING / k FOLLOWING bounds on the GPU (tgpu_window_factory_create_ranged), against the reference's
stateful walk restated in tests/window_range_expected.py: the reference's cases (tests/golden/window_range_vectors.json), the seeded corpus of
tests/window_range_cases.py (4 key types x 4 sort orders x 13 bound combinations), every function under such a frame, row counts and partition / null-run
edges around wave, block and tile edges under TGPU_WINDOW_TILE_ROWS=256 and the default, several pages, 16 mixed frames in one operator, shared and
separate comparison channels, the sum's frame-local overflow rule, the other frames through the new entry point, arbitrary bounds against the closed
form, the errors, the protocol, and a filter / project operator computing the bounds in front of the window.  Every comparison is exact: values bit
for bit, nulls, row order."""
import json
import os

import numpy as np
import pytest

import date_fn_expected as D
import window_range_cases as W
import window_range_expected as X
from window_expected import (AGGREGATE, COUNT_ALL, COUNT_COLUMN, CUME_DIST, DENSE_RANK, FIRST_VALUE, LAG, LAST_VALUE, LEAD, MAX_BIGINT, MAX_DOUBLE, MIN_BIGINT, MIN_DOUBLE,
                             PERCENT_RANK, RANK, ROW_NUMBER, SUM_BIGINT, Fn, NumericValueOutOfRange, tokens)
from window_frames_expected import CURRENT_ROW, FOLLOWING, GROUPS, NTH_VALUE, NTILE, PRECEDING, RANGE, ROWS, UNBOUNDED_FOLLOWING, UNBOUNDED_PRECEDING, Frame
from window_range_expected import RangeFrame

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "window_range_vectors.json")))
LIVE = [c for c in GOLD["cases"] if "skip" not in c]
TILE = "TGPU_WINDOW_TILE_ROWS"
ENVS = ({TILE: "256"}, {})
NP = {1: np.int64, 2: np.int32, 3: np.int32, 4: np.float64, 5: np.uint8}
B, I, DT, DBL, V = 1, 2, 3, 4, 6


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
    frame = f.frame
    if isinstance(frame, RangeFrame):
        frame = pkg.WindowRangeFrame(frame.start, frame.end, frame.start_channel, frame.end_channel, frame.start_key, frame.end_key)
    elif isinstance(frame, Frame):
        frame = pkg.WindowFrame(frame.type, frame.start, frame.end, frame.start_channel, frame.end_channel)
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
        op.addInput(p)
        assert op.getOutput() is None   # nothing before finish()
    op.finish()
    o = op.getOutput()
    assert op.getOutput() is None and op.isFinished()
    if o is None:
        return None
    page = o.to_host()
    o.release()
    return page


def run(pkg, ctx, types, outputs, functions, partitions, sorts, orders, rows_per_page, env=None):
    op = create(pkg, ctx, types, outputs, functions, partitions, sorts, orders, env)
    try:
        out = drive(op, [page_of(pkg, types, rows) for rows in rows_per_page])
    finally:
        op.close()
    return [] if out is None else tokens(out.rows())


def check(pkg, ctx, types, outputs, functions, partitions, sorts, orders, rows_per_page, envs=ENVS, how="walk"):
    """the device against the helper, in operators of at most 16 functions; returns the expected rows"""
    expected = tokens(X.expected_output(types, rows_per_page, outputs, functions, partitions, sorts, orders, how))
    k = len(outputs)
    for lo in range(0, len(functions), 16):
        hi = min(lo + 16, len(functions))
        want = [r[:k] + r[k + lo:k + hi] for r in expected]
        for env in envs:
            got = run(pkg, ctx, types, outputs, functions[lo:hi], partitions, sorts, orders, rows_per_page, env)
            assert got == want, (env, lo, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:3], len(got), len(want))
    return expected


def corpus_functions(frame):
    """over the tables of window_range_cases: 2 = the row id, 3 = BIGINT values with nulls"""
    return [Fn(AGGREGATE, (), frame, COUNT_ALL), Fn(AGGREGATE, (3,), frame, COUNT_COLUMN), Fn(AGGREGATE, (3,), frame, SUM_BIGINT), Fn(AGGREGATE, (3,), frame, MIN_BIGINT),
            Fn(AGGREGATE, (3,), frame, MAX_BIGINT), Fn(FIRST_VALUE, (2,), frame), Fn(LAST_VALUE, (2,), frame), Fn(RANK, (), frame)]


# ---- the reference's cases and the corpus --------------------------------------------------------------------------------------------------------
def test_reference_cases(pkg, ctx):
    for case in LIVE:
        types, rows, outputs, functions, partitions, order, listed = W.golden_table(case)
        expected = check(pkg, ctx, types, outputs, functions, partitions, [0], [order], [rows])
        assert sorted(map(repr, expected)) == sorted(map(repr, tokens(listed))), case["sql"]   # matches() ignores row order


@pytest.mark.parametrize("key_type", W.KEY_TYPES)
def test_corpus_against_the_walk(pkg, ctx, key_type):
    cases = [c for c in W.corpus(20260101, per_combination=1) if c["types"][1] == key_type]
    assert len(cases) == 4 * 13
    for c in cases:
        check(pkg, ctx, c["types"], [0, 1, 2], corpus_functions(c["frame"]), [0], [1], [c["order"]], [c["rows"]])


def test_arbitrary_bounds_give_the_closed_form(pkg, ctx):
    cases = W.corpus(77, per_combination=1, conforming=False)[::3]
    for c in cases:
        check(pkg, ctx, c["types"], [0, 1, 2], corpus_functions(c["frame"]), [0], [1], [c["order"]], [c["rows"]], how="closed")


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------------
def key_table(rng, sizes, null_counts, order, domain=12, offsets=(2, 3)):
    """partitions of the given sizes whose first null_counts[p] keys are null; channels: 0 partition, 1 BIGINT key, 2 row id, 3 BIGINT values, 4 / 5 the
    bounds of <offsets[0]> PRECEDING / <offsets[1]> FOLLOWING, 6 DOUBLE values"""
    rows, asc = [], X.ascending(order)
    for p, (size, nulls) in enumerate(zip(sizes, null_counts)):
        for i in range(size):
            k = None if i < nulls else int(rng.integers(0, domain))
            v = None if rng.random() < 0.1 else int(rng.integers(-1000, 1000))
            d = None if rng.random() < 0.1 else (float("nan"), -0.0, 0.0, 1.5, -2.5, 7.0)[int(rng.integers(6))]
            rows.append((p, k, len(rows), v, W.bound_value(B, k, offsets[0], asc), W.bound_value(B, k, offsets[1], not asc), d))
    order_of = rng.permutation(len(rows))
    return [rows[i] for i in order_of]


TABLE_TYPES = [B, B, B, B, B, B, DBL]
BOTH = RangeFrame(PRECEDING, FOLLOWING, 4, 5, 1, 1)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 513, 1000])
def test_row_counts_around_wave_block_and_tile_edges(pkg, ctx, n):
    rng = np.random.default_rng(n)
    for sizes, nulls, order in (([n], [n // 5], 1), ([n], [0], 2), ([n - n // 2, n // 2], [1, n // 4], 0)):
        sizes, nulls = zip(*[(s, k) for s, k in zip(sizes, nulls) if s > 0])
        rows = key_table(rng, sizes, nulls, order)
        check(pkg, ctx, TABLE_TYPES, [0, 1, 2], corpus_functions(BOTH), [0], [1], [order], [rows])


def test_partition_heads_and_the_null_edge_on_and_next_to_wave_block_and_tile_edges(pkg, ctx):
    """sorted positions: partition p starts at the sum of the sizes before it; under NULLS FIRST its non-null run starts null_counts[p] later, under NULLS LAST
    it ends that much before the partition does"""
    rng = np.random.default_rng(5)
    sizes = [63, 1, 1, 63, 127, 1, 255, 2, 255, 257]           # heads at 63, 64, 65, 128, 255, 256, 511, 513, 768
    nulls = [1, 0, 1, 62, 1, 0, 192, 1, 255, 1]                # null edges at 64, 127 / 128 .., a whole partition of nulls
    for order in (0, 1, 2, 3):
        rows = key_table(rng, sizes, nulls, order)
        for frame in (BOTH, RangeFrame(FOLLOWING, UNBOUNDED_FOLLOWING, 5, -1, 1, -1), RangeFrame(UNBOUNDED_PRECEDING, PRECEDING, -1, 4, -1, 1)):
            check(pkg, ctx, TABLE_TYPES, [0, 1, 2], corpus_functions(frame), [0], [1], [order], [rows])


def test_one_partition_over_several_tiles_and_frames_wider_than_it(pkg, ctx):
    rng = np.random.default_rng(6)
    for order in (1, 2):
        rows = key_table(rng, [1100], [37], order, domain=400, offsets=(50, 10**9))
        fns = corpus_functions(BOTH) + [Fn(AGGREGATE, (6,), BOTH, MIN_DOUBLE), Fn(AGGREGATE, (6,), BOTH, MAX_DOUBLE)]
        check(pkg, ctx, TABLE_TYPES, [1, 2], fns, [], [1], [order], [rows])
        wide = key_table(rng, [700, 400], [0, 5], order, domain=50, offsets=(10**12, 10**12))
        check(pkg, ctx, TABLE_TYPES, [0, 1, 2], corpus_functions(BOTH), [0], [1], [order], [wide])


def test_several_input_pages(pkg, ctx):
    rows = key_table(np.random.default_rng(7), [300, 200, 41], [10, 0, 41], 0)
    check(pkg, ctx, TABLE_TYPES, [0, 1, 2], corpus_functions(BOTH), [0], [1], [0], [rows[:100], rows[100:101], rows[101:400], rows[400:]])


# ---- functions and frames ------------------------------------------------------------------------------------------------------------------------
def test_every_function_under_a_range_frame(pkg, ctx):
    """channels 7 / 8 / 9: nth offsets 1 .. 4 with nulls, lag / lead offsets, ntile buckets"""
    rng = np.random.default_rng(8)
    rows = [r + (None if rng.random() < 0.1 else int(rng.integers(1, 5)), int(rng.integers(0, 4)), int(rng.integers(1, 9))) for r in key_table(rng, [200, 90, 10], [20, 0, 3], 1)]
    types = TABLE_TYPES + [B, B, B]
    aggs = [Fn(AGGREGATE, (), BOTH, COUNT_ALL)] + [Fn(AGGREGATE, (3,), BOTH, a) for a in (COUNT_COLUMN, SUM_BIGINT, MIN_BIGINT, MAX_BIGINT)]
    aggs += [Fn(AGGREGATE, (6,), BOTH, a) for a in (COUNT_COLUMN, MIN_DOUBLE, MAX_DOUBLE)]
    values = [Fn(FIRST_VALUE, (6,), BOTH), Fn(LAST_VALUE, (3,), BOTH), Fn(NTH_VALUE, (2, 7), BOTH), Fn(NTH_VALUE, (6, 7), RangeFrame(CURRENT_ROW, FOLLOWING, -1, 5, -1, 1))]
    ranking = [Fn(f, (), BOTH) for f in (ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST)] + [Fn(LAG, (2, 8), BOTH), Fn(LEAD, (3, 8), BOTH), Fn(NTILE, (9,), BOTH)]
    for order in (1, 2):
        rows_o = [r[:4] + (W.bound_value(B, r[1], 2, X.ascending(order)), W.bound_value(B, r[1], 3, not X.ascending(order))) + r[6:] for r in rows]
        check(pkg, ctx, types, [0, 1, 2], aggs + values + ranking, [0], [1], [order], [rows_o])


def test_sixteen_functions_with_different_frames_in_one_operator(pkg, ctx):
    """channel 7: BIGINT offsets 0 .. 3 for the ROWS / GROUPS frames; 8 / 9: the bounds of 0 PRECEDING / 5 FOLLOWING"""
    rng = np.random.default_rng(9)
    rows = [r + (int(rng.integers(0, 4)), W.bound_value(B, r[1], 0, True), W.bound_value(B, r[1], 5, False)) for r in key_table(rng, [300, 150, 7], [30, 0, 7], 0)]
    types = TABLE_TYPES + [B, B, B]
    frames = [BOTH, RangeFrame(PRECEDING, CURRENT_ROW, 4, -1, 1, -1), RangeFrame(CURRENT_ROW, FOLLOWING, -1, 5, -1, 1), RangeFrame(PRECEDING, PRECEDING, 4, 8, 1, 1),
              RangeFrame(FOLLOWING, FOLLOWING, 8, 9, 1, 1), RangeFrame(UNBOUNDED_PRECEDING, FOLLOWING, -1, 9, -1, 1), RangeFrame(PRECEDING, UNBOUNDED_FOLLOWING, 4, -1, 1, -1),
              RangeFrame(FOLLOWING, UNBOUNDED_FOLLOWING, 9, -1, 1, -1), RangeFrame(UNBOUNDED_PRECEDING, PRECEDING, -1, 8, -1, 1),
              Frame(ROWS, PRECEDING, FOLLOWING, 7, 7), Frame(ROWS, UNBOUNDED_PRECEDING, PRECEDING, -1, 7), Frame(GROUPS, PRECEDING, CURRENT_ROW, 7), Frame(GROUPS, FOLLOWING, FOLLOWING, 7, 7),
              Frame(RANGE, CURRENT_ROW, CURRENT_ROW), Frame(RANGE, UNBOUNDED_PRECEDING, CURRENT_ROW), RangeFrame(CURRENT_ROW, UNBOUNDED_FOLLOWING)]
    assert len(frames) == 16
    aggs = (SUM_BIGINT, MIN_BIGINT, MAX_BIGINT, COUNT_COLUMN)
    functions = [Fn(AGGREGATE, (3,), frame, aggs[i % 4]) for i, frame in enumerate(frames)]
    check(pkg, ctx, types, [0, 1, 2], functions, [0], [1], [0], [rows])
    check(pkg, ctx, types, [0, 1, 2], [Fn(LAST_VALUE, (2,), frame) for frame in frames], [0], [1], [0], [rows], envs=({TILE: "256"},))


def test_bounds_sharing_a_comparison_channel_and_bounds_with_their_own(pkg, ctx):
    """an INTEGER sort key; the start bound is BIGINT against the key cast to BIGINT (channel 3), the end bound DOUBLE against the key cast to DOUBLE (channel 5)"""
    rng = np.random.default_rng(10)
    keys = [None if rng.random() < 0.15 else int(rng.integers(-20, 20)) for _ in range(400)]
    for order in (0, 3):
        asc = X.ascending(order)
        cast = lambda k, f: None if k is None else f(k)
        rows = [(int(rng.integers(3)), k, i, cast(k, int), W.bound_value(B, k, 3, asc), cast(k, float), None if k is None else (float(k) + 1.5 if asc else float(k) - 1.5),
                 W.bound_value(B, k, 1, not asc)) for i, k in enumerate(keys)]
        types = [B, I, B, B, B, DBL, DBL, B]
        own = RangeFrame(PRECEDING, FOLLOWING, 4, 6, 3, 5)
        shared = RangeFrame(PRECEDING, FOLLOWING, 4, 7, 3, 3)
        functions = [Fn(AGGREGATE, (2,), own, SUM_BIGINT), Fn(AGGREGATE, (), shared, COUNT_ALL), Fn(FIRST_VALUE, (2,), own), Fn(LAST_VALUE, (2,), shared), Fn(AGGREGATE, (2,), own, MAX_BIGINT)]
        check(pkg, ctx, types, [0, 1, 2], functions, [0], [1], [order], [rows])


def test_only_a_frames_own_sum_has_to_fit(pkg, ctx):
    big = 2**62
    types, frame = [B, B, B, B], RangeFrame(PRECEDING, CURRENT_ROW, 2, -1, 0, -1)   # 1 PRECEDING: at most two keys' rows
    table = lambda values: [(k, v, k - 1, None) for k, v in enumerate(values)]
    fns = [Fn(AGGREGATE, (1,), frame, SUM_BIGINT)]
    # every prefix from the third row on leaves int64; no frame does
    expected = check(pkg, ctx, types, [0], fns, [], [0], [1], [table([big, big - 1, big - 1, -big, -big, -big])])
    assert [r[1] for r in expected] == [big, 2 * big - 1, 2 * big - 2, -1, -2 * big, -2 * big]
    with pytest.raises(NumericValueOutOfRange):
        X.expected_output(types, [table([5, big, big, 7])], [0], fns, [], [0], [1])
    for env in ENVS:
        with pytest.raises(pkg.TgpuError) as e:
            run(pkg, ctx, types, [0], fns, [], [0], [1], [table([5, big, big, 7])], env)
        assert e.value.code == -2 and e.value.message == "bigint addition overflow"


def test_other_frames_through_the_new_entry_point_give_the_framed_page(pkg, ctx):
    rng = np.random.default_rng(11)
    rows = [r + (int(rng.integers(1, 4)),) for r in key_table(rng, [300, 77], [12, 0], 1)]   # channel 7: ROWS / GROUPS offsets, and nth_value's
    types = TABLE_TYPES + [B]
    frames = [Frame(ROWS, PRECEDING, FOLLOWING, 7, 7), Frame(ROWS, FOLLOWING, UNBOUNDED_FOLLOWING, 7), Frame(GROUPS, PRECEDING, FOLLOWING, 7, 7), Frame(GROUPS, UNBOUNDED_PRECEDING, PRECEDING, -1, 7),
              Frame(RANGE, CURRENT_ROW, UNBOUNDED_FOLLOWING), Frame(RANGE, UNBOUNDED_PRECEDING, CURRENT_ROW), Frame(RANGE, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING), 2]
    functions = [Fn(AGGREGATE, (3,), f, SUM_BIGINT) for f in frames] + [Fn(AGGREGATE, (6,), f, MAX_DOUBLE) for f in frames[:4]] + [Fn(NTH_VALUE, (2, 7), frames[0])]
    framed = run(pkg, ctx, types, [0, 1, 2], functions + [Fn(ROW_NUMBER, (), Frame(RANGE, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING))], [0], [1], [1], [rows])
    ranged = run(pkg, ctx, types, [0, 1, 2], functions + [Fn(ROW_NUMBER, (), RangeFrame(UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING))], [0], [1], [1], [rows])
    assert ranged == framed and len(ranged) == len(rows)
    # their errors too: a negative ROWS offset
    bad = [r[:7] + (-1,) for r in rows]
    for frame in (Frame(RANGE, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING), RangeFrame(UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING)):
        with pytest.raises(pkg.TgpuError) as e:
            run(pkg, ctx, types, [0], functions[:1] + [Fn(ROW_NUMBER, (), frame)], [0], [1], [1], [bad])
        assert e.value.code == -1 and e.value.message == "Window frame offset must not be negative"


# ---- errors and protocol ---------------------------------------------------------------------------------------------------------------------------
def test_null_bounds_and_null_comparison_keys(pkg, ctx):
    """channels: 0 key, 1 / 2 the bounds, 3 the comparison key, 4 values, 5 nth offsets"""
    types, frame = [B, B, B, B, B, B], RangeFrame(PRECEDING, FOLLOWING, 1, 2, 3, 3)
    good = [(k, k - 1, k + 1, k, 2**62, 1) for k in range(1, 300)] + [(None, None, None, None, 1, 1)] * 3   # bounds in null-key rows are never read
    count = [Fn(AGGREGATE, (), frame, COUNT_ALL)]
    check(pkg, ctx, types, [0], count, [], [0], [1], [good])
    overflow, nth = Fn(AGGREGATE, (4,), frame, SUM_BIGINT), Fn(NTH_VALUE, (4, 5), frame)
    start, end, key = "Window frame starting offset must not be null", "Window frame ending offset must not be null", "Window frame comparison key must not be null where the sort key is not null"
    for extra, functions, message in (([(7, None, 8, 7, 1, 1)], count, start), ([(7, 6, None, 7, 1, 1)], count, end), ([(7, 6, 8, None, 1, 1)], count, key),
                                      ([(7, None, None, None, 1, 1)], count, start), ([(7, 6, None, None, 1, 1)], count, end),
                                      ([(7, 6, None, 7, 1, 1)], [overflow], end),                      # before the page's sum overflow
                                      ([(7, 6, 8, None, 1, 0)], [nth, overflow], key)):                # before "Offset must be at least 1" and the overflow
        for env in ENVS:
            with pytest.raises(pkg.TgpuError) as e:
                run(pkg, ctx, types, [0], functions, [], [0], [1], [good[:150], good[150:] + extra], env)
            assert (e.value.code, e.value.message) == (-1, message)
    with pytest.raises(pkg.TgpuError) as e:   # without the null: the overflow
        run(pkg, ctx, types, [0], [overflow], [], [0], [1], [good])
    assert e.value.code == -2


def test_creation_errors(pkg, ctx):
    types = [B, DBL, V, I, DT, B]

    def make(frame, sorts=(0,), orders=(1,)):
        return pkg.WindowOperatorFactory(ctx, 1, types, [0], [window_function(pkg, Fn(AGGREGATE, (), frame, COUNT_ALL))], [], list(sorts), list(orders))
    ok = RangeFrame(PRECEDING, FOLLOWING, 5, 5, 0, 0)
    make(ok).close()
    make(RangeFrame(PRECEDING, CURRENT_ROW, 4, -1, 4, -1), sorts=(4,)).close()
    for frame, sorts, code, text in ((ok, (), -1, "a RANGE frame with an offset needs exactly one sort channel"), (ok, (0, 1), -1, "a RANGE frame with an offset needs exactly one sort channel"),
                                     (RangeFrame(PRECEDING, FOLLOWING, 6, 5, 0, 0), (0,), -1, "frame bound channel out of range"),
                                     (RangeFrame(PRECEDING, FOLLOWING, 5, -1, 0, 0), (0,), -1, "frame bound channel out of range"),
                                     (RangeFrame(PRECEDING, FOLLOWING, 5, 5, 0, 6), (0,), -1, "frame comparison key channel out of range"),
                                     (RangeFrame(PRECEDING, FOLLOWING, 5, 5, -1, 0), (0,), -1, "frame comparison key channel out of range"),
                                     (RangeFrame(PRECEDING, FOLLOWING, 1, 5, 0, 0), (0,), -1, "a frame bound and its comparison key differ in type"),
                                     (RangeFrame(UNBOUNDED_PRECEDING, FOLLOWING, -1, 3, -1, 4), (0,), -1, "a frame bound and its comparison key differ in type"),
                                     (RangeFrame(PRECEDING, CURRENT_ROW, 2, -1, 2, -1), (0,), -1, "a RANGE frame bound must be BIGINT, INTEGER, DATE or DOUBLE"),
                                     (RangeFrame(FOLLOWING, CURRENT_ROW, 5, -1, 0, -1), (0,), -1, "invalid window frame bounds"),
                                     (RangeFrame(CURRENT_ROW, PRECEDING, -1, 5, -1, 0), (0,), -1, "invalid window frame bounds")):
        with pytest.raises(pkg.TgpuError) as e:
            make(frame, sorts, (1,) * len(sorts))
        assert (e.value.code, e.value.message) == (code, text)
    with pytest.raises(pkg.TgpuError) as e:   # the framed entry point keeps refusing the frame
        make(Frame(RANGE, PRECEDING, CURRENT_ROW, 5))
    assert (e.value.code, e.value.message) == (-8, "RANGE frames with an offset are not supported")


def test_memory_bytes_grow_by_the_search_arrays(pkg, ctx):
    """beside a ROWS frame of the same shape (the same frame arrays): 8 bytes per row and distinct comparison channel, one byte per row"""
    n = 1000
    rows = [(k // 3, k // 3 - 1, k // 3 + 1, k // 3, 1) for k in range(n)]
    types = [B, B, B, B, B]

    def memory(frame):
        op = create(pkg, ctx, types, [0], [Fn(AGGREGATE, (), frame, COUNT_ALL)], [], [0], [1])
        drive(op, [page_of(pkg, types, rows)])
        m = op.memoryBytes()
        op.close()
        return m
    base = memory(Frame(ROWS, PRECEDING, FOLLOWING, 4, 4))
    assert memory(RangeFrame(PRECEDING, FOLLOWING, 1, 2, 0, 0)) - base == 8 * n + n
    assert memory(RangeFrame(PRECEDING, FOLLOWING, 1, 2, 0, 3)) - base == 2 * 8 * n + n
    assert memory(RangeFrame(PRECEDING, CURRENT_ROW, 1, -1, 3, -1)) - base == 8 * n + n


# ---- composition ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_a_filter_project_operator_computes_the_bounds(pkg, ctx, order):
    """the planner's shape: offsets in a column, the bound expressions of window_range_bound projected in front of the window"""
    rng = np.random.default_rng(12 + order)
    n = 500
    f = pkg.field
    # a BIGINT key with per-row offsets
    rows = [(None if rng.random() < 0.1 else int(rng.integers(-40, 40)), i, int(rng.integers(0, 6))) for i in range(n)]
    types = [B, B, B]
    projections = [f(0, B), f(1, B), pkg.window_range_bound(f(0, B), f(2, B), pkg.BOUND_PRECEDING, order), pkg.window_range_bound(f(0, B), f(2, B), pkg.BOUND_FOLLOWING, order)]
    project = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, None, projections)
    pages = pkg.to_pages(project.createOperator(), [page_of(pkg, types, rows[:200]), page_of(pkg, types, rows[200:])])
    asc = X.ascending(order)
    projected = [(k, i, W.bound_value(B, k, o, asc), W.bound_value(B, k, o, not asc)) for k, i, o in rows]
    assert tokens([r for p in pages for r in p.rows()]) == tokens(projected)
    frame = RangeFrame(PRECEDING, FOLLOWING, 2, 3, 0, 0)
    fns = [Fn(AGGREGATE, (1,), frame, SUM_BIGINT), Fn(AGGREGATE, (), frame, COUNT_ALL), Fn(FIRST_VALUE, (1,), frame)]
    want = tokens(X.expected_output([B] * 4, [projected], [0, 1], fns, [], [0], [order]))
    op = create(pkg, ctx, [B] * 4, [0, 1], fns, [], [0], [order])
    out = drive(op, pages)
    op.close()
    assert tokens(out.rows()) == want
    # a DATE key with a month interval
    day0 = D.to_days(2001, 1, 1)
    dates = [(None if rng.random() < 0.1 else day0 + int(rng.integers(0, 400)), i) for i in range(n)]
    projections = [f(0, DT), f(1, B), pkg.window_range_bound(f(0, DT), 1, pkg.BOUND_PRECEDING, order, unit="month"), pkg.window_range_bound(f(0, DT), 2, pkg.BOUND_FOLLOWING, order, unit="month")]
    project = pkg.FilterAndProjectOperatorFactory(ctx, 0, [DT, B], None, projections)
    pages = pkg.to_pages(project.createOperator(), [page_of(pkg, [DT, B], dates)])
    sign = -1 if asc else 1
    projected = [(d, i, None if d is None else D.date_add("month", sign * 1, d), None if d is None else D.date_add("month", -sign * 2, d)) for d, i in dates]
    assert tokens([r for p in pages for r in p.rows()]) == tokens(projected)
    fns = [Fn(AGGREGATE, (1,), frame, SUM_BIGINT), Fn(AGGREGATE, (), frame, COUNT_ALL), Fn(LAST_VALUE, (0,), frame)]
    want = tokens(X.expected_output([DT, B, DT, DT], [projected], [0, 1], fns, [], [0], [order]))
    op = create(pkg, ctx, [DT, B, DT, DT], [0, 1], fns, [], [0], [order])
    out = drive(op, pages)
    op.close()
    assert tokens(out.rows()) == want

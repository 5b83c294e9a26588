"""agg.hip agg_ordered_runs_kernel: row-order (ORDERED mode) accumulation straight from the ascending group ids of the group-by's run
route, without the (key, row) lists.  Every case drives HashAggregationOperator over (BIGINT, DATE, INTEGER) keys with the kernel on and
with TGPU_AGG_RUN_ORDERED=0 (the list-based agg_ordered_kernel<false>): the two outputs must have equal bits, and both must equal the
oracle's Java-row-order states, which know neither kernel.

T = 2048 rows per tile (agg.hip kOrdRunTile), 256 lanes x 8 rows; a lane walks at most 4096 rows (agg.h kOrdHandoffRows) before it hands the
rest of its run to the chain kernel; kOrdRunStaged = 3 valued aggregates (every function but the counts) are staged in LDS, an operator with more keeps the lists.
TGPU_ORD_CHAIN_MAX_GROUPS=0 keeps the few-groups chain route out of the way (it has a case of its own), so that every other case meets the
lane-per-run kernel whatever its number of groups."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 2048
HANDOFF = 4096
D, B, M = 3, 4, 5   # channels behind the three keys: DOUBLE input, BIGINT input, BOOLEAN mask


def clustered(rng, n, lo=1, hi=7):
    lens = rng.integers(lo, hi + 1, n)
    return np.repeat(np.arange(n), lens)[:n].astype(np.int64)


def ids_from_heads(n, heads):
    """group index per row: a run starts at row 0 and at every row in `heads`"""
    mark = np.zeros(n, dtype=np.int64)
    mark[[h for h in heads if 0 < h < n]] = 1
    return np.cumsum(mark)


def keys_of(ids):
    return [(ids * 4 + 1).astype(np.int64), (8000 + ids % 2000).astype(np.int32), (ids % 3).astype(np.int32)]


def order_doubles(rng, n):
    """values whose sum shows the order of the additions: 1e16, 1.0, -1e16, 1.0 stretches among values of mixed magnitude"""
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    at = rng.integers(0, max(1, n - 4), max(1, n // 16))
    for a in at:
        v[a:a + 4] = np.array([1e16, 1.0, -1e16, 1.0])[:max(0, min(4, n - a))]
    return v


class Input:
    def __init__(self, ids, rng, nulls=False, mask=False, d=None):
        n = len(ids)
        self.ids = ids
        self.d = order_doubles(rng, n) if d is None else d
        self.b = rng.integers(-(2**50), 2**50, n).astype(np.int64)   # (a run of 5,000 of them stays inside 64 bits: no overflow error)
        self.d_nulls = (rng.random(n) < 0.3).astype(np.uint8) if nulls else None
        self.b_nulls = (rng.random(n) < 0.3).astype(np.uint8) if nulls else None
        self.m = (rng.random(n) < 0.6).astype(np.uint8) if mask else np.ones(n, dtype=np.uint8)
        self.m_nulls = (rng.random(n) < 0.1).astype(np.uint8) if mask else None

    def page(self, pkg, a, z):
        k = keys_of(self.ids[a:z])
        cut = lambda x: None if x is None else x[a:z]
        return pkg.Page(pkg.Block(pkg.BIGINT, k[0]), pkg.Block(pkg.DATE, k[1]), pkg.Block(pkg.INTEGER, k[2]), pkg.Block(pkg.DOUBLE, self.d[a:z], cut(self.d_nulls)),
                        pkg.Block(pkg.BIGINT, self.b[a:z], cut(self.b_nulls)), pkg.Block(pkg.BOOLEAN, self.m[a:z], cut(self.m_nulls)))


def bits(rows):
    return [tuple(None if x is None else (int(np.float64(x).view(np.int64)) if isinstance(x, float) else x) for x in r) for r in rows]


def expected_rows(pkg, oracle, inp, aggs):
    """the rows of a SINGLE aggregation in the reference's row order, every state from the oracle's accumulators"""
    ids, n = inp.ids, len(inp.ids)
    groups = int(ids[-1]) + 1
    k = keys_of(ids)
    _, first = np.unique(ids, return_index=True)
    cols = []
    for a in aggs:
        f, ch = a[0], a[1]
        mask = None
        if len(a) > 2 and a[2] == M:
            mask = (inp.m != 0) & (inp.m_nulls == 0 if inp.m_nulls is not None else True)
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
        nulls = {D: inp.d_nulls, B: inp.b_nulls, -1: None}[ch]
        if f == pkg.COUNT_ALL:
            cols.append([int(c) for c in oracle.agg_count(ids, n, groups, None, mask)])
            continue
        if f == pkg.COUNT_COLUMN:
            cols.append([int(c) for c in oracle.agg_count(ids, n, groups, nulls, mask)])
            continue
        if f == pkg.SUM_DOUBLE:
            cnt, out = oracle.agg_double_sum(ids, inp.d, groups, nulls, mask)
        elif f == pkg.AVG_DOUBLE:
            cnt, s = oracle.agg_double_sum(ids, inp.d, groups, nulls, mask)
            with np.errstate(all="ignore"):
                out = s / np.maximum(cnt, 1)
        elif f == pkg.AVG_BIGINT:
            cnt, s = oracle.agg_long_avg(ids, inp.b, groups, nulls, mask)
            with np.errstate(all="ignore"):
                out = s / np.maximum(cnt, 1)
        elif f == pkg.SUM_BIGINT:
            cnt, out = oracle.agg_long_sum(ids, inp.b, groups, nulls, mask)
        elif f in (pkg.MIN_BIGINT, pkg.MAX_BIGINT):
            cnt, out = oracle.agg_long_minmax(ids, inp.b, groups, f == pkg.MIN_BIGINT, nulls, mask)
        else:
            cnt, out = oracle.agg_double_minmax(ids, inp.d, groups, f == pkg.MIN_DOUBLE, nulls, mask)
        cols.append([None if c == 0 else (float(x) if out.dtype == np.float64 else int(x)) for c, x in zip(cnt, out)])
    return [(int(k[0][r]), int(k[1][r]), int(k[2][r])) + tuple(c[g] for c in cols) for g, r in enumerate(first)]


SUM_COUNT = lambda pkg: [(pkg.SUM_DOUBLE, D), (pkg.COUNT_ALL, -1)]


def check(pkg, oracle, monkeypatch, inp, aggs=None, cuts=None, env=(), scope="agg_accumulate_ordered", also=()):
    """runs the operator with the kernel on and off, compares the two bit for bit and with the oracle; -> the profile with the kernel on"""
    aggs = SUM_COUNT(pkg) if aggs is None else aggs
    n = len(inp.ids)
    cuts = [0, n] if cuts is None else cuts
    monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "16")
    monkeypatch.setenv("TGPU_ORD_CHAIN_MAX_GROUPS", "0")
    for name, value in env:
        monkeypatch.setenv(name, value)
    out = {}
    for setting in ("on", "off"):
        if setting == "off":
            monkeypatch.setenv("TGPU_AGG_RUN_ORDERED", "0")
        else:
            monkeypatch.delenv("TGPU_AGG_RUN_ORDERED", raising=False)
        ctx = pkg.Context(0)
        ctx.profile_enable(True)
        ctx.set_double_sum_order(pkg.SUM_ORDER_JAVA)
        f = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT, pkg.DATE, pkg.INTEGER], [0, 1, 2], aggs, expected_groups=100)
        op = f.createOperator()
        rows = [r for p in pkg.to_pages(op, [inp.page(pkg, a, z) for a, z in zip(cuts[:-1], cuts[1:])]) for r in p.rows()]
        op.close()
        prof = ctx.profile()
        ctx.close()
        assert "gbh_runs" in prof and "gbh_insert" not in prof, sorted(prof)   # the ids came from the run route: ascending, the switch decides
        assert scope in prof, sorted(prof)
        for name in also:
            assert name in prof, sorted(prof)
        out[setting] = (rows, prof)
    assert bits(out["on"][0]) == bits(out["off"][0])
    assert {k for k in out["on"][1] if k.startswith("agg_")} == {k for k in out["off"][1] if k.startswith("agg_")}
    assert bits(out["on"][0]) == bits(expected_rows(pkg, oracle, inp, aggs))
    return out["on"][1]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5])
def test_row_counts(pkg, oracle, monkeypatch, n):
    rng = np.random.default_rng(n)
    check(pkg, oracle, monkeypatch, Input(clustered(rng, n), rng))


@pytest.mark.parametrize("offset", [-2, -1, 0, 1, 2, "all"])
def test_run_boundaries_around_every_wave_workgroup_and_tile_edge(pkg, oracle, monkeypatch, offset):
    """a run starts `offset` rows from every multiple of 64 (so from every wave, workgroup-stride and tile edge) -- "all": at all five
    offsets at once"""
    n = 3 * T + 5
    offsets = [-2, -1, 0, 1, 2] if offset == "all" else [offset]
    ids = ids_from_heads(n, [e + d for e in range(64, n + 64, 64) for d in offsets])
    check(pkg, oracle, monkeypatch, Input(ids, np.random.default_rng(7)))


@pytest.mark.parametrize("shape", ["starts_on_last_row_of_tile", "spans_three_tiles", "all_distinct", "one_group"])
def test_run_shapes(pkg, oracle, monkeypatch, shape):
    n = 3 * T + 5
    if shape == "starts_on_last_row_of_tile":
        ids = ids_from_heads(n, [5, T - 1, T + 3, 2 * T - 1, 3 * T - 1])        # the last one runs into the short last tile
    elif shape == "spans_three_tiles":
        ids = ids_from_heads(n, [100, T - 10, 2 * T + 10, 2 * T + 11])          # rows T - 10 .. 2 T + 9: the whole of tile 1 inside the run
    elif shape == "all_distinct":
        ids = np.arange(n, dtype=np.int64)
    else:
        n = T + 7                                                                # (below the hand-off: one lane walks the page)
        ids = np.zeros(n, dtype=np.int64)
    check(pkg, oracle, monkeypatch, Input(ids, np.random.default_rng(8)))


def test_one_run_of_5000_rows_is_handed_to_the_chain_kernel(pkg, oracle, monkeypatch):
    n = 5000 + 300
    ids = ids_from_heads(n, [37, 37 + 5000] + list(range(37 + 5000, n, 3)))      # the long run starts inside tile 0 and ends inside tile 2
    assert np.bincount(ids).max() == 5000 > HANDOFF
    check(pkg, oracle, monkeypatch, Input(ids, np.random.default_rng(9)), aggs=[(pkg.SUM_DOUBLE, D), (pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, B), (pkg.MAX_BIGINT, B)],
          also=["agg_accumulate_ordered_handoff"])


def test_few_groups_take_the_chain_kernel_without_the_lists(pkg, oracle, monkeypatch):
    """3 groups of 1,000 rows: one workgroup per group (agg_ordered_chain_kernel, stretches form), reading the ids through the same accessor"""
    ids = np.repeat(np.arange(3), 1000).astype(np.int64)
    check(pkg, oracle, monkeypatch, Input(ids, np.random.default_rng(10), nulls=True), env=[("TGPU_ORD_CHAIN_MAX_GROUPS", "65536")], scope="agg_accumulate_ordered_chain")


def test_two_pages_cut_inside_a_run(pkg, oracle, monkeypatch):
    """row 0 of the second page continues the group the first page left: its state is read, added to and written back"""
    rng = np.random.default_rng(11)
    n = 2 * T + 300
    ids = clustered(rng, n, lo=3, hi=9)
    cut = T + 100
    while ids[cut - 1] != ids[cut] or ids[cut] != ids[cut + 1]:
        cut += 1
    check(pkg, oracle, monkeypatch, Input(ids, rng), cuts=[0, cut, n], env=[("TGPU_DISABLE_COALESCE", "1")])


@pytest.mark.parametrize("cap", [1, 2])
def test_workgroup_cap_gives_a_workgroup_several_tiles(pkg, oracle, monkeypatch, cap):
    rng = np.random.default_rng(12)
    n = 5 * T + 5
    check(pkg, oracle, monkeypatch, Input(clustered(rng, n), rng, nulls=True), env=[("TGPU_AGG_RUN_MAX_BLOCKS", str(cap))])


def function_sets(pkg):
    return {
        # three valued aggregates (the LDS holds three) and the two counts
        "sum_count_sumbig_min_countcol": [(pkg.SUM_DOUBLE, D), (pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, B), (pkg.MIN_BIGINT, B), (pkg.COUNT_COLUMN, D)],
        "avg_max_avgbig": [(pkg.AVG_DOUBLE, D), (pkg.MAX_BIGINT, B), (pkg.AVG_BIGINT, B), (pkg.COUNT_ALL, -1)],
        "max_min_double_count": [(pkg.MAX_DOUBLE, D), (pkg.COUNT_COLUMN, B), (pkg.MIN_DOUBLE, D)],
        "masked": [(pkg.SUM_DOUBLE, D, M), (pkg.COUNT_ALL, -1, M), (pkg.SUM_BIGINT, B, M), (pkg.COUNT_COLUMN, B), (pkg.AVG_BIGINT, B, M)],
        "masked_min_max": [(pkg.MIN_DOUBLE, D, M), (pkg.MAX_BIGINT, B, M), (pkg.COUNT_COLUMN, D, M)],
        # four valued aggregates: more than the LDS stages, the operator keeps the lists
        "four_valued_fallback": [(pkg.SUM_DOUBLE, D), (pkg.SUM_BIGINT, B), (pkg.MIN_BIGINT, B), (pkg.AVG_DOUBLE, D, M), (pkg.COUNT_ALL, -1)],
    }


@pytest.mark.parametrize("name", ["sum_count_sumbig_min_countcol", "avg_max_avgbig", "max_min_double_count", "masked", "masked_min_max", "four_valued_fallback"])
def test_functions_nulls_and_masks(pkg, oracle, monkeypatch, name):
    """null input cells, a mask channel (with null mask cells) and groups whose rows are all skipped: groups 5 .. 9 have only null cells,
    groups 20 .. 24 only masked rows; the long run crosses a tile edge, so the walk past the tile reads nulls and masks too"""
    rng = np.random.default_rng(13)
    n = 2 * T + 77
    ids = ids_from_heads(n, list(range(3, T - 40, 3)) + list(range(T + 60, n, 2)))    # rows T - 40 .. T + 59: one run across the edge
    inp = Input(ids, rng, nulls=True, mask=True)
    skipped = (ids >= 5) & (ids <= 9)
    inp.d_nulls[skipped] = 1
    inp.b_nulls[skipped] = 1
    inp.m[(ids >= 20) & (ids <= 24)] = 0
    check(pkg, oracle, monkeypatch, inp, aggs=function_sets(pkg)[name])


def test_doubles_where_the_order_and_the_sign_of_zero_show(pkg, oracle, monkeypatch):
    """per group of four rows a pattern of its own: the 1e16 cancellation in every rotation, -0.0 alone (0.0 + -0.0 = +0.0), -0.0 among
    nulls, +Inf, -Inf and NaN each with finite company.  NaN is compared by its bits."""
    pats = [[1e16, 1.0, -1e16, 1.0], [1.0, 1e16, 1.0, -1e16], [-1e16, 1.0, 1e16, 1.0], [1.0, 1.0, 1e16, -1e16], [-0.0, -0.0, -0.0, -0.0], [-0.0, 0.0, -0.0, 0.0],
            [np.inf, 1.0, 2.0, np.inf], [-np.inf, 1.0, -2.0, 3.0], [np.nan, 1.0, 2.0, 3.0], [1.0, 2.0, np.nan, -0.0], [1e308, 1e308, -1e308, -1e308], [5e-324, -5e-324, 5e-324, 1.0]]
    reps = 180                                           # 8,640 rows: the patterns meet every lane position and the tile edges
    d = np.array(pats * reps, dtype=np.float64).ravel()
    n = len(d)
    ids = (np.arange(n) // 4).astype(np.int64)
    rng = np.random.default_rng(14)
    inp = Input(ids, rng, d=d)
    inp.d_nulls = np.zeros(n, dtype=np.uint8)
    inp.d_nulls[np.arange(n) % 96 == 17] = 1             # row 1 of every second -0.0-only group is null
    check(pkg, oracle, monkeypatch, inp, aggs=[(pkg.SUM_DOUBLE, D), (pkg.COUNT_ALL, -1), (pkg.AVG_DOUBLE, D)])

"""min / max over INTEGER and DATE through the C ABI on every path a grouped aggregation takes (tests/agg_paths.py), compared exactly with
the row-at-a-time model (tests/minmax_expected.py).  One operator holds min and max over an INTEGER and a DATE channel, each with and
without a mask, beside count(*): values at the int32 edges, -1, 0 and nulls; one group whose cells are all NULL and one whose mask
excludes every row.  The kernels run these functions as min / max over BIGINT with a 4-byte load, so what can go wrong is the load
width, the sign extension, the type of the output column and the type checks -- on each path.  The second half of the file is min / max
over VARCHAR, which has kernels and a value store of its own (csrc/minmax_varchar.h)."""
import numpy as np
import pytest

import minmax_expected as M
from agg_paths import (FUSED_GENERAL, ORDERED_GROUPS, ORDERED_PATHS, PARTIAL_FINAL_MANY, PATHS, assert_profile, drive, final_aggs, is_fused, late_group_first_row, page_sizes,
                       run_final, run_partials)

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch's runtime first (test_varchar_input_forms puts tensors on the device): brought up after the library's context it has been
    seen to find no device"""
    import torch

    torch.cuda.init()


INVALID_ARGUMENT = -1
FILTER_BELOW = 0.75
EDGES = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0], dtype=np.int64)
ALL_NULL_GROUP, ALL_MASKED_GROUP, HEAVY_GROUP = 1, 2, 3


def aggs_of(pkg):
    """(function, channel[, mask]): channel 1 INTEGER, 2 DATE, 3 the BOOLEAN mask"""
    return [(pkg.MIN_INTEGER, 1), (pkg.MAX_INTEGER, 1), (pkg.MIN_INTEGER, 1, 3), (pkg.MAX_INTEGER, 1, 3), (pkg.MIN_DATE, 2), (pkg.MAX_DATE, 2), (pkg.MIN_DATE, 2, 3),
            (pkg.MAX_DATE, 2, 3), (pkg.COUNT_ALL, -1)]


def small_aggs_of(pkg):
    """two valued aggregates: few enough for the kernel that walks ascending run ids from LDS (agg.hip kOrdRunStaged)"""
    return [(pkg.MAX_DATE, 2), (pkg.MIN_INTEGER, 1, 3), (pkg.COUNT_ALL, -1)]


def fused_spec(pkg):
    f = pkg.field
    B, I, DT, BO, D = pkg.BIGINT, pkg.INTEGER, pkg.DATE, pkg.BOOLEAN, pkg.DOUBLE
    return [B, I, DT, BO, D], f(4, D) < FILTER_BELOW, [f(0, B), f(1, I), f(2, DT), f(3, BO)]


class Stream:
    """n rows: gids, two int32 value columns with nulls, a mask with nulls, the fused operators' filter column"""

    def __init__(self, rng, ngroups, n, first_row=None, heavy=False, ascending=False):
        g = rng.integers(0, ngroups, n)
        if heavy:                                   # a tenth of the rows: more than a lane walks (agg.h kOrdHandoffRows) in every page
            g = np.where(rng.random(n) < 0.1, HEAVY_GROUP, g)
        if first_row is not None:                   # the last group arrives late (agg_paths.late_group_first_row)
            late = ngroups - 1
            g[:first_row[late]][g[:first_row[late]] == late] = 0
        if ascending:
            g = np.sort(g)
        self.gids = g.astype(np.int64)
        self.n, self.ngroups = n, ngroups
        cols = []
        for _ in range(2):
            v = rng.integers(-2 ** 31, 2 ** 31, n)
            v = np.where(rng.random(n) < 0.2, rng.integers(-3, 4, n), v)            # small values of both signs, ties among them
            v = np.where(rng.random(n) < 0.05, EDGES[rng.integers(0, 4, n)], v)
            nulls = (rng.random(n) < 0.15).astype(np.uint8)
            if ngroups > ALL_NULL_GROUP:
                nulls[g == ALL_NULL_GROUP] = 1
            cols.append((v.astype(np.int32), nulls))
        (self.ints, self.int_nulls), (self.dates, self.date_nulls) = cols
        self.mask = (rng.random(n) < 0.5).astype(np.uint8)
        self.mask_nulls = (rng.random(n) < 0.1).astype(np.uint8)
        if ngroups > ALL_MASKED_GROUP:
            self.mask[g == ALL_MASKED_GROUP] = 0
        self.filt = rng.random(n)
        for want in EDGES:                          # every edge value is there, and not null
            i = int(rng.integers(0, n))
            while ngroups > ALL_NULL_GROUP and g[i] == ALL_NULL_GROUP:
                i = int(rng.integers(0, n))
            self.ints[i] = self.dates[n - 1 - i] = want
            self.int_nulls[i] = 0
            if not (ngroups > ALL_NULL_GROUP and g[n - 1 - i] == ALL_NULL_GROUP):
                self.date_nulls[n - 1 - i] = 0

    def pages(self, pkg, sizes, fused):
        out, at = [], 0
        for m in sizes:
            z = slice(at, at + m)
            cols = [pkg.Block(pkg.BIGINT, self.gids[z]), pkg.Block(pkg.INTEGER, self.ints[z], self.int_nulls[z]), pkg.Block(pkg.DATE, self.dates[z], self.date_nulls[z]),
                    pkg.Block(pkg.BOOLEAN, self.mask[z], self.mask_nulls[z])]
            if fused:
                cols.append(pkg.Block(pkg.DOUBLE, self.filt[z]))
            out.append(pkg.Page(*cols))
            at += m
        assert at == self.n
        return out

    def model_page(self, rows, channel, masked):
        """the rows `rows` (an index array) as a page of the model"""
        v, nulls = (self.ints, self.int_nulls) if channel == 1 else (self.dates, self.date_nulls)
        values = [None if nu else int(x) for x, nu in zip(v[rows], nulls[rows])]
        mask = [None if nu else bool(x) for x, nu in zip(self.mask[rows], self.mask_nulls[rows])] if masked else None
        return values, self.gids[rows].tolist(), mask


def model_states(pkg, s, aggs, rows, fn):
    """per aggregate the model's per-group list over the rows `rows`: fn = M.single or M.partial; count(*): the rows of the group"""
    out = []
    for a in aggs:
        if a[0] == pkg.COUNT_ALL:
            out.append(np.bincount(s.gids[rows], minlength=s.ngroups).tolist())
        else:
            out.append(fn([s.model_page(rows, a[1], len(a) > 2)], a[0], s.ngroups))
    return out


def expected_rows(pkg, s, aggs, rows):
    """{group: (aggregate values...)} of SINGLE over the rows `rows`, for the groups with a row"""
    st = model_states(pkg, s, aggs, rows, M.single)
    present = np.bincount(s.gids[rows], minlength=s.ngroups)
    return {g: tuple(x[g] if isinstance(x[g], int) else x[g][1] for x in st) for g in range(s.ngroups) if present[g]}


def rows_kept(s, fused):
    return np.nonzero(s.filt < FILTER_BELOW)[0] if fused else np.arange(s.n)


def check_edges(want, ngroups):
    """the stream has what the test is about: both int32 edges as results, a group that is all NULL, a group that is all masked out"""
    flat = [v for row in want.values() for v in row[:8]]
    assert -2 ** 31 in flat and 2 ** 31 - 1 in flat
    if ngroups > ALL_MASKED_GROUP:
        assert want[ALL_NULL_GROUP][:8] == (None,) * 8 and want[ALL_NULL_GROUP][8] > 0
        w = want[ALL_MASKED_GROUP]
        assert w[2] is None and w[3] is None and w[6] is None and w[7] is None and w[0] is not None


def cells():
    out = []
    for path in PATHS + (FUSED_GENERAL,):
        out.append((path, 1 if path == "global" else 5))
    for path in ORDERED_PATHS + (PARTIAL_FINAL_MANY,):
        out.append((path, ORDERED_GROUPS[path.rsplit("_", 1)[1]]))
    return [pytest.param(p, g, id="%s-%d" % (p, g)) for p, g in out]


@pytest.mark.parametrize("path,ngroups", cells())
def test_integer_date_extremes(pkg, monkeypatch, path, ngroups):
    sizes = page_sizes(path)
    fused = is_fused(path)
    rng = np.random.default_rng(9100 + len(path) + ngroups % 89)
    s = Stream(rng, ngroups, sum(sizes), first_row=late_group_first_row(path, ngroups), heavy=path.endswith("handoff"))
    pages = s.pages(pkg, sizes, fused)
    aggs = aggs_of(pkg)
    want = expected_rows(pkg, s, aggs, rows_kept(s, fused))
    check_edges(want, ngroups)
    got = drive(pkg, monkeypatch, path, ngroups, pages, aggs, fused_spec, partial_final=lambda ctx: partial_final(pkg, ctx, s, pages, sizes, aggs, path))
    if got.error is not None:
        raise got.error
    assert {r[0]: tuple(r[1:]) for r in got.rows} == want
    assert_profile(path, got.profile, ngroups)


def partial_final(pkg, ctx, s, pages, sizes, aggs, path):
    """two PARTIAL operators over disjoint page sets (many groups: one per page), their intermediate rows -- checked against the model's
    flattened NullableLongState, the value channel BIGINT -- into one FINAL"""
    ends = np.cumsum(sizes)
    if path == PARTIAL_FINAL_MANY:
        sets = [([pg], np.arange(e - m, e)) for pg, m, e in zip(pages, sizes, ends)]
    else:
        sets = [(pages[:1], np.arange(0, sizes[0])), (pages[1:], np.arange(sizes[0], s.n))]
    partials = []
    for pgs, rows in sets:
        out = run_partials(pkg, ctx, [pgs], s.ngroups, aggs)[0]
        st = model_states(pkg, s, aggs, rows, M.partial)
        present = np.bincount(s.gids[rows], minlength=s.ngroups)
        want = {}
        for g in range(s.ngroups):
            if present[g]:
                want[g] = tuple(c for x in st[:-1] for c in x[g]) + (st[-1][g],)
        got = {}
        for p in out:
            assert [b.type for b in p.blocks] == [pkg.BIGINT] * (1 + 2 * 8 + 1)     # key, (count, extreme) x 8, count(*)
            got.update({r[0]: tuple(r[1:]) for r in p.rows()})
        assert got == want
        partials += out
    assert final_aggs(pkg, aggs)[:3] == [(pkg.MIN_INTEGER, 1), (pkg.MAX_INTEGER, 3), (pkg.MIN_INTEGER, 5)]
    rows = run_final(pkg, ctx, partials, s.ngroups, aggs)
    assert ("agg_combine_ordered" if path == PARTIAL_FINAL_MANY else "agg_combine") in ctx.profile(), sorted(ctx.profile())
    return rows


def test_ascending_run_ids(pkg):
    """clustered keys, many groups: the group-by hands ascending run ids over and the accumulators walk them from LDS without the
    (key, row) lists (agg.hip agg_ordered_runs_kernel) -- its 4-byte loads, in the tile and past its end"""
    ngroups, sizes = ORDERED_GROUPS["many"], page_sizes("ordered_many")
    s = Stream(np.random.default_rng(9301), ngroups, sum(sizes), ascending=True)
    aggs = small_aggs_of(pkg)
    want = expected_rows(pkg, s, aggs, np.arange(s.n))
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    try:
        # (two key channels: a single BIGINT key takes the integer table, which has no run route)
        op = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT, pkg.BIGINT], [0, 0], aggs, expected_groups=ngroups).createOperator()
        rows = [r for p in pkg.to_pages(op, s.pages(pkg, sizes, False)) for r in p.rows()]
        op.close()
        prof = ctx.profile()
    finally:
        ctx.close()
    assert {r[0]: tuple(r[2:]) for r in rows} == want and all(r[0] == r[1] for r in rows)
    assert "gbh_runs" in prof and "gbh_insert" not in prof and "agg_accumulate_ordered" in prof, sorted(prof)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def test_output_types(pkg, ctx):
    """SINGLE / FINAL: a channel of the input's own type; PARTIAL: count BIGINT, extreme BIGINT; nulls where no row counted"""
    I, DT, B = pkg.INTEGER, pkg.DATE, pkg.BIGINT
    page = pkg.Page(pkg.Block(B, [0, 0, 1, 1, 2]), pkg.Block(I, [-2 ** 31, 2 ** 31 - 1, -1, 0, None]), pkg.Block(DT, [None, -5, 7, -2 ** 31, None]))
    aggs = [(pkg.MIN_INTEGER, 1), (pkg.MAX_INTEGER, 1), (pkg.MIN_DATE, 2), (pkg.MAX_DATE, 2)]
    single = pkg.to_pages(pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], aggs).createOperator(), [page])
    assert [[b.type for b in p.blocks] for p in single] == [[B, I, I, DT, DT]]
    assert sorted(single[0].rows()) == [(0, -2 ** 31, 2 ** 31 - 1, -5, -5), (1, -1, 0, -2 ** 31, 7), (2, None, None, None, None)]
    partial = pkg.to_pages(pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], aggs, step=pkg.PARTIAL).createOperator(), [page])
    assert [[b.type for b in p.blocks] for p in partial] == [[B] * 9]
    assert sorted(partial[0].rows()) == [(0, 2, -2 ** 31, 2, 2 ** 31 - 1, 1, -5, 1, -5), (1, 2, -1, 2, 0, 2, -2 ** 31, 2, 7), (2, 0, 0, 0, 0, 0, 0, 0, 0)]
    final = pkg.to_pages(pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], final_aggs(pkg, aggs), step=pkg.FINAL).createOperator(), partial + partial)
    assert [[b.type for b in p.blocks] for p in final] == [[B, I, I, DT, DT]]
    assert sorted(final[0].rows()) == sorted(single[0].rows())
    # the global aggregation: no key channel; no row at all gives NULL
    glob = pkg.to_pages(pkg.HashAggregationOperatorFactory(ctx, 0, [], [], aggs).createOperator(), [page])
    assert [b.type for b in glob[0].blocks] == [I, I, DT, DT] and glob[0].rows() == [(-2 ** 31, 2 ** 31 - 1, -2 ** 31, 7)]


STREAM_CUTS = {"one_page": None, "pages_of_1000": 1000, "wave_and_block_edges": [1, 63, 64, 65, 255, 256, 257, 2047, 2049]}


@pytest.mark.parametrize("small", [False, True], ids=["lists", "run_walk"])
@pytest.mark.parametrize("cut", list(STREAM_CUTS))
def test_streaming_aggregation(pkg, ctx, cut, small):
    """the same list through StreamingAggregationOperator on sorted keys under three page cuts; a group spans pages"""
    n, ngroups = 9000, 300
    s = Stream(np.random.default_rng(9400), ngroups, n, ascending=True)
    aggs = small_aggs_of(pkg) if small else aggs_of(pkg)
    c = STREAM_CUTS[cut]
    if c is None:
        sizes = [n]
    elif isinstance(c, int):
        sizes = [c] * (n // c)
    else:
        sizes = c + [n - sum(c)]
    want = expected_rows(pkg, s, aggs, np.arange(n))
    types = [pkg.BIGINT, pkg.INTEGER, pkg.DATE, pkg.BOOLEAN]
    op = pkg.StreamingAggregationOperatorFactory(ctx, 0, types, [0], pkg.SINGLE, aggs).createOperator()
    out = pkg.to_pages(op, s.pages(pkg, sizes, False))
    op.close()
    value_types = {pkg.MIN_INTEGER: pkg.INTEGER, pkg.MAX_INTEGER: pkg.INTEGER, pkg.MIN_DATE: pkg.DATE, pkg.MAX_DATE: pkg.DATE, pkg.COUNT_ALL: pkg.BIGINT}
    for p in out:
        assert [b.type for b in p.blocks] == [pkg.BIGINT] + [value_types[a[0]] for a in aggs]
    rows = [r for p in out for r in p.rows()]
    assert [r[0] for r in rows] == sorted(want)                 # one row per run, in stream order
    assert {r[0]: tuple(r[1:]) for r in rows} == want


def test_streaming_partial_final(pkg, ctx):
    n, ngroups = 6000, 200
    s = Stream(np.random.default_rng(9401), ngroups, n, ascending=True)
    aggs = aggs_of(pkg)
    types = [pkg.BIGINT, pkg.INTEGER, pkg.DATE, pkg.BOOLEAN]
    op = pkg.StreamingAggregationOperatorFactory(ctx, 0, types, [0], pkg.PARTIAL, aggs).createOperator()
    partial = pkg.to_pages(op, s.pages(pkg, [2500, 3500], False))
    op.close()
    for p in partial:
        assert [b.type for b in p.blocks] == [pkg.BIGINT] * 18
    op = pkg.StreamingAggregationOperatorFactory(ctx, 0, [pkg.BIGINT] * 18, [0], pkg.FINAL, final_aggs(pkg, aggs)).createOperator()
    rows = [r for p in pkg.to_pages(op, partial) for r in p.rows()]
    op.close()
    assert {r[0]: tuple(r[1:]) for r in rows} == expected_rows(pkg, s, aggs, np.arange(n))


def test_wrong_input_type(pkg, ctx):
    """the streaming and the fused factory know the types and refuse at creation; the plain factory when the page reaches its accumulators"""
    B, I, DT, D = pkg.BIGINT, pkg.INTEGER, pkg.DATE, pkg.DOUBLE
    f = pkg.field
    for fn, wrong in ((pkg.MIN_INTEGER, DT), (pkg.MAX_INTEGER, B), (pkg.MIN_DATE, I), (pkg.MAX_DATE, D)):
        with pytest.raises(pkg.TgpuError) as e:
            pkg.StreamingAggregationOperatorFactory(ctx, 0, [B, wrong], [0], pkg.SINGLE, [(fn, 1)])
        assert e.value.code == INVALID_ARGUMENT and "type" in str(e.value)
        with pytest.raises(pkg.TgpuError) as e:
            pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [B, wrong], None, [f(0, B), f(1, wrong)], [B], [0], [(fn, 1)])
        assert e.value.code == INVALID_ARGUMENT and "type" in str(e.value)
        op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], [(fn, 1)]).createOperator()
        values = np.zeros(3, dtype=np.float64 if wrong == D else (np.int64 if wrong == B else np.int32))
        with pytest.raises(pkg.TgpuError) as e:              # (a small page waits in the operator's coalescing buffer: the drive raises)
            pkg.to_pages(op, [pkg.Page(pkg.Block(B, [1, 2, 3]), pkg.Block(wrong, values))])
        assert e.value.code == INVALID_ARGUMENT and "type" in str(e.value)
        op.close()


# =====================================================================================================================================
# min / max over VARCHAR: values are `bytes` on both sides -- Python's comparison of bytes is Slice.compareTo's order
# =====================================================================================================================================
NOT_SUPPORTED = -8
VARCHAR_PATHS = ("general", "lowcard", "lowcard_multi", "global", "partial_final", PARTIAL_FINAL_MANY, "ordered_many")
ALPHABET = [0x00, 0x01, 0x61, 0x62, 0x7f, 0x80, 0xff]


def cell(block, i):
    """the cell's bytes (Block.get would decode them), None for NULL"""
    if block.nulls is not None and block.nulls[i]:
        return None
    return bytes(block.values[block.offsets[i]:block.offsets[i + 1]])


def cells_of(block):
    return [cell(block, i) for i in range(block.position_count)]


def random_values(rng, n, null_frac=0.15, prefix=b"https://"):
    """short values over a few bytes (ties, prefixes of each other, '' among them), a third behind a shared 8-byte prefix"""
    lens = rng.integers(0, 13, n)
    raw = rng.integers(0, len(ALPHABET), (n, 12))
    shared = rng.random(n) < 0.33
    nulls = rng.random(n) < null_frac
    return [None if nulls[i] else (prefix if shared[i] else b"") + bytes(ALPHABET[x] for x in raw[i, :lens[i]]) for i in range(n)]


def varchar_aggs(pkg):
    """channels: 0 key, 1 VARCHAR, 2 mask, 3 BIGINT.  sum(bigint) and count(*) beside the extremes keep their usual kernels"""
    return [(pkg.MIN_VARCHAR, 1), (pkg.SUM_BIGINT, 3), (pkg.MAX_VARCHAR, 1), (pkg.MAX_VARCHAR, 1, 2), (pkg.COUNT_ALL, -1)]


class TextStream:
    def __init__(self, rng, ngroups, n, values=None, gids=None):
        self.n, self.ngroups = n, ngroups
        self.gids = rng.integers(0, ngroups, n).astype(np.int64) if gids is None else np.asarray(gids, dtype=np.int64)
        self.values = random_values(rng, n) if values is None else values
        self.mask = [None if x == 2 else bool(x) for x in rng.integers(0, 3, n)]
        self.big = rng.integers(-1000, 1000, n).astype(np.int64)

    def pages(self, pkg, sizes):
        out, at = [], 0
        for m in sizes:
            z = slice(at, at + m)
            mk = self.mask[z]
            out.append(pkg.Page(pkg.Block(pkg.BIGINT, self.gids[z]), pkg.Block(pkg.VARCHAR, self.values[z]),
                                pkg.Block(pkg.BOOLEAN, np.array([bool(x) for x in mk], dtype=np.uint8), np.array([x is None for x in mk], dtype=np.uint8)),
                                pkg.Block(pkg.BIGINT, self.big[z])))
            at += m
        assert at == self.n
        return out

    def want(self, pkg, aggs, rows=None, fn=M.single):
        """{group: one entry per aggregate: (count, value) of the extremes, the sum, the count} over `rows`, for the groups with a row"""
        rows = np.arange(self.n) if rows is None else rows
        g = self.gids[rows].tolist()
        vals = [self.values[i] for i in rows]
        mask = [self.mask[i] for i in rows]
        per = []
        for a in aggs:
            if a[0] == pkg.COUNT_ALL:
                per.append(np.bincount(self.gids[rows], minlength=self.ngroups).tolist())
            elif a[0] == pkg.SUM_BIGINT:
                per.append(np.bincount(self.gids[rows], weights=self.big[rows], minlength=self.ngroups).astype(np.int64).tolist())
            else:
                per.append(fn([(vals, g, mask if len(a) > 2 else None)], a[0], self.ngroups))
        present = np.bincount(self.gids[rows], minlength=self.ngroups)
        return {k: tuple(x[k] for x in per) for k in range(self.ngroups) if present[k]}


def single_rows(pkg, pages, aggs, key=True):
    """host output pages of SINGLE / FINAL -> {key: one entry per aggregate: the value's bytes / the number}"""
    out = {}
    for p in pages:
        cols = [cells_of(b) if b.type == pkg.VARCHAR else b.to_list() for b in p.blocks]
        assert [b.type for b in p.blocks[1 if key else 0:]] == [pkg.VARCHAR if a[0] in (pkg.MIN_VARCHAR, pkg.MAX_VARCHAR) else pkg.BIGINT for a in aggs]
        for i in range(p.position_count):
            row = tuple(c[i] for c in cols)
            out[row[0] if key else 0] = row[1:] if key else row
    return out


def values_only(want):
    """the model's (count, value) -> the value, as a SINGLE / FINAL output row holds it"""
    return {k: tuple(x[1] if isinstance(x, tuple) else x for x in row) for k, row in want.items()}


def run_varchar(pkg, ctx, pages, aggs, ngroups, step=0, global_agg=False):
    if global_agg:
        fac = pkg.HashAggregationOperatorFactory(ctx, 0, [], [], aggs, step=step)
    else:
        fac = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT], [0], aggs, step=step, expected_groups=max(ngroups, 1))
    op = fac.createOperator()
    try:
        return pkg.to_pages(op, pages)
    finally:
        op.close()
        fac.close()


@pytest.mark.parametrize("path", VARCHAR_PATHS)
def test_varchar_paths(pkg, monkeypatch, path):
    from agg_paths import select_path
    ngroups = 1 if path == "global" else (ORDERED_GROUPS["many"] if path in (PARTIAL_FINAL_MANY, "ordered_many") else 5)
    sizes = page_sizes(path)
    s = TextStream(np.random.default_rng(9500 + len(path)), ngroups, sum(sizes))
    aggs = varchar_aggs(pkg)
    pages = s.pages(pkg, sizes)
    select_path(monkeypatch, path)
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    try:
        if path in ("partial_final", PARTIAL_FINAL_MANY):
            ends = np.cumsum(sizes)
            sets = ([([pg], np.arange(e - m, e)) for pg, m, e in zip(pages, sizes, ends)] if path == PARTIAL_FINAL_MANY
                    else [(pages[:1], np.arange(0, sizes[0])), (pages[1:], np.arange(sizes[0], s.n))])
            partials = []
            for pgs, rows in sets:
                out = run_varchar(pkg, ctx, pgs, aggs, ngroups, step=pkg.PARTIAL)
                want = s.want(pkg, aggs, rows, M.partial)
                got = {}
                for p in out:
                    B, V = pkg.BIGINT, pkg.VARCHAR
                    assert [b.type for b in p.blocks] == [B, B, V, B, B, B, V, B, V, B]      # key; count, value | count, sum | ... | count(*)
                    cols = [cells_of(b) if b.type == V else b.to_list() for b in p.blocks]
                    for i in range(p.position_count):
                        r = [c[i] for c in cols]
                        got[r[0]] = ((r[1], r[2]), r[4], (r[5], r[6]), (r[7], r[8]), r[9])
                        assert r[3] == r[9]                                               # sum(bigint)'s count: every row
                assert got == want
                partials += out
            final = run_varchar(pkg, ctx, partials, final_aggs(pkg, aggs), ngroups, step=pkg.FINAL)
            got = single_rows(pkg, final, aggs)
        else:
            got = single_rows(pkg, run_varchar(pkg, ctx, pages, aggs, ngroups, global_agg=path == "global"), aggs, key=path != "global")
        prof = ctx.profile()
    finally:
        ctx.close()
    assert got == values_only(s.want(pkg, aggs))
    assert "agg_varchar_extreme_round" in prof and "agg_varchar_extreme_install" in prof, sorted(prof)
    assert_profile(path, prof, ngroups)                     # the other aggregates of the operator took their usual kernels


def one_page_extremes(pkg, ctx, groups_of_values):
    """every list of values as a group of one page -> [(min, max)] per group"""
    gids = [g for g, vs in enumerate(groups_of_values) for _ in vs]
    vals = [v for vs in groups_of_values for v in vs]
    order = np.random.default_rng(len(vals)).permutation(len(vals))
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array(gids, dtype=np.int64)[order]), pkg.Block(pkg.VARCHAR, [vals[i] for i in order]))
    aggs = [(pkg.MIN_VARCHAR, 1), (pkg.MAX_VARCHAR, 1)]
    got = single_rows(pkg, run_varchar(pkg, ctx, [page], aggs, len(groups_of_values)), aggs)
    return [got[g] for g in range(len(groups_of_values))]


def test_varchar_order_inside_a_group(pkg, ctx):
    base = bytes(range(1, 40))
    groups = [[b"", None], [None, None], [b"a", b"a\x00"], [b"\x7f", b"\x80"], [b"x\x7fz", b"x\x80"]]
    for k in (6, 7, 8, 13, 14, 15):                      # agree for exactly k bytes, differ in the next
        groups.append([base[:k] + b"\x10tail", base[:k] + b"\x11"])
    for k in (7, 14):                                    # one is the other's prefix
        groups.append([base[:k], base[:k] + b"\x00"])
        groups.append([base[:k], base[:k + 1], base[:k + 8]])
    big = bytes(np.random.default_rng(5).integers(0, 256, 100_000).astype(np.uint8))
    groups.append([big, big[:-1] + bytes([big[-1] ^ 1]), big[:-1]])
    got = one_page_extremes(pkg, ctx, groups)
    for vs, g in zip(groups, got):
        live = [v for v in vs if v is not None]
        assert g == ((min(live), max(live)) if live else (None, None)), [v[:20] for v in live]
    assert got[0] == (b"", b"") and got[2] == (b"a", b"a\x00") and got[3] == (b"\x7f", b"\x80")


def test_varchar_contention(pkg, ctx):
    """4 groups x 20,000 rows whose values share 300 bytes and differ in the last 4; 20,000 identical values in a fifth group"""
    rng = np.random.default_rng(9600)
    prefix = bytes(rng.integers(0, 256, 300).astype(np.uint8))
    tails = rng.integers(0, 256, (80_000, 4)).astype(np.uint8)
    vals = [prefix + bytes(t) for t in tails] + [prefix + b"same"] * 20_000
    gids = np.concatenate([rng.integers(0, 4, 80_000), np.full(20_000, 4)]).astype(np.int64)
    order = rng.permutation(len(vals))
    vals, gids = [vals[i] for i in order], gids[order]
    aggs = [(pkg.MIN_VARCHAR, 1), (pkg.MAX_VARCHAR, 1)]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, gids[z]), pkg.Block(pkg.VARCHAR, vals[z])) for z in (slice(0, 60_000), slice(60_000, 100_000))]
    got = single_rows(pkg, run_varchar(pkg, ctx, pages, aggs, 5), aggs)
    for g in range(5):
        mine = [v for v, k in zip(vals, gids) if k == g]
        assert got[g] == (min(mine), max(mine))


def test_varchar_row_counts(pkg, ctx):
    """wave and block edges x group counts, the extreme at the first, the last and a middle row"""
    aggs = [(pkg.MIN_VARCHAR, 1), (pkg.MAX_VARCHAR, 1)]
    rng = np.random.default_rng(9700)
    for n in (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097):
        body = random_values(rng, n, null_frac=0.1, prefix=b"prefix--")
        body = [None if v is None else b"\x02" + v for v in body]          # strictly between the planted extremes
        for ngroups in (1, 2, 64, 65):
            gids = (np.arange(n) % ngroups).astype(np.int64)
            for at in {0, n - 1, n // 2}:
                for planted in (b"\x01", b"\xff\xff\xff\xff\xff\xff\xff\xff\xff"):
                    vals = list(body)
                    vals[at] = planted
                    got = single_rows(pkg, run_varchar(pkg, ctx, [pkg.Page(pkg.Block(pkg.BIGINT, gids), pkg.Block(pkg.VARCHAR, vals))], aggs, ngroups), aggs)
                    want = M.single([(vals, gids.tolist(), None)], pkg.MIN_VARCHAR, ngroups), M.single([(vals, gids.tolist(), None)], pkg.MAX_VARCHAR, ngroups)
                    assert got == {g: (want[0][g][1], want[1][g][1]) for g in range(min(ngroups, n))}, (n, ngroups, at)
                    assert planted in got[int(gids[at])]


def test_varchar_across_pages(pkg, ctx):
    """group 0: the extreme of the first page survives ten more; 1: every page replaces it; 2: a later page ties it; 3: first seen in
    page 5; 4: absent from page 3"""
    pages_model = []
    for p in range(11):
        vals, gids = [], []
        for i in range(50):
            vals += [b"zzzzzzzzzz-first" if p == 0 and i == 7 else b"m%03d" % i, b"page-%02d-%02d" % (p, i), b"tie-tie-tie" if p in (2, 9) and i == 3 else b"sss%d" % i]
            gids += [0, 1, 2]
            if p >= 5:
                vals.append(b"late%02d" % ((p * 7 + i) % 50))
                gids.append(3)
            if p != 3:
                vals.append(b"w%02d" % ((p * 11 + i * 3) % 97))
                gids.append(4)
        pages_model.append((vals, gids, None))
    aggs = [(pkg.MAX_VARCHAR, 1), (pkg.MIN_VARCHAR, 1)]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.array(g, dtype=np.int64)), pkg.Block(pkg.VARCHAR, v)) for v, g, _ in pages_model]
    got = single_rows(pkg, run_varchar(pkg, ctx, pages, aggs, 5), aggs)
    want = M.single(pages_model, pkg.MAX_VARCHAR, 5), M.single(pages_model, pkg.MIN_VARCHAR, 5)
    assert got == {g: (want[0][g][1], want[1][g][1]) for g in range(5)}
    assert got[0][0] == b"zzzzzzzzzz-first" and got[1][0] == b"page-10-49" and got[2][0] == b"tie-tie-tie"


def test_varchar_state_growth(pkg, ctx):
    """the group count grows from 10 to 50,000 during the stream"""
    rng = np.random.default_rng(9800)
    pages_model = []
    for ngroups, n in ((10, 500), (300, 3000), (5000, 20_000), (50_000, 120_000), (50_000, 30_000)):
        gids = rng.integers(0, ngroups, n)
        gids[:min(n, ngroups)] = np.arange(min(n, ngroups))                  # ids are first-seen ranks: every group up to the page's bound appears in order
        pages_model.append((random_values(rng, n), gids.tolist(), None))
    seen, remap = {}, []
    for vals, gids, _ in pages_model:                                        # key -> first-seen rank, what the operator numbers its groups by
        remap.append([seen.setdefault(k, len(seen)) for k in gids])
    aggs = [(pkg.MAX_VARCHAR, 1), (pkg.MIN_VARCHAR, 1)]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.array(g, dtype=np.int64)), pkg.Block(pkg.VARCHAR, v)) for v, g, _ in pages_model]
    got = single_rows(pkg, run_varchar(pkg, ctx, pages, aggs, 10), aggs)
    want = M.single(pages_model, pkg.MAX_VARCHAR, 50_000), M.single(pages_model, pkg.MIN_VARCHAR, 50_000)
    assert got == {g: (want[0][g][1], want[1][g][1]) for g in seen}


def test_varchar_page_cuts(pkg, ctx):
    """the same stream cut into pages of 1 row, of 7 rows and as one page: identical output"""
    n = 300
    s = TextStream(np.random.default_rng(9900), 6, n)
    aggs = varchar_aggs(pkg)
    outs = []
    for width in (1, 7, n):
        sizes = [width] * (n // width) + ([n % width] if n % width else [])
        outs.append(single_rows(pkg, run_varchar(pkg, ctx, s.pages(pkg, sizes), aggs, 6), aggs))
    assert outs[0] == outs[1] == outs[2] == values_only(s.want(pkg, aggs))


def test_varchar_input_forms(pkg, ctx):
    """DICTIONARY and RLE blocks, a device page, a borrowed device block that is a region of a larger one (offsets[0] != 0), masks"""
    import torch

    aggs = [(pkg.MIN_VARCHAR, 1), (pkg.MAX_VARCHAR, 1), (pkg.MAX_VARCHAR, 1, 2)]
    rng = np.random.default_rng(9950)
    n = 5000
    dictionary = [b"", b"delta", b"alpha", None, b"alph", b"omega\xff", b"omega\x80"]
    ids = rng.integers(0, len(dictionary), n).astype(np.int32)
    gids = rng.integers(0, 9, n).astype(np.int64)
    mask = rng.integers(0, 2, n).astype(np.uint8)
    vals = [dictionary[i] for i in ids]
    want = {g: tuple(M.single([(vals, gids.tolist(), mask.astype(bool).tolist() if len(a) > 2 else None)], a[0], 9)[g][1] for a in aggs) for g in range(9)}
    keys, masks = pkg.Block(pkg.BIGINT, gids), pkg.Block(pkg.BOOLEAN, mask)
    forms = {"flat": pkg.Block(pkg.VARCHAR, vals), "dictionary": pkg.DictionaryBlock(pkg.Block(pkg.VARCHAR, dictionary), ids)}
    for name, block in forms.items():
        assert single_rows(pkg, run_varchar(pkg, ctx, [pkg.Page(keys, block, masks)], aggs, 9), aggs) == want, name
    rle = pkg.Page(keys, pkg.RunLengthEncodedBlock(pkg.Block(pkg.VARCHAR, [b"only"]), n), masks)
    got = single_rows(pkg, run_varchar(pkg, ctx, [rle], aggs, 9), aggs)
    assert got == {g: (b"only", b"only", b"only") for g in range(9)}
    # device memory: the whole pool, then the region [first, n) of it -- its offsets do not start at 0
    flat = forms["flat"]
    d_pool = torch.tensor(flat.values, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.tensor(flat.offsets, dtype=torch.int32, device="cuda:0")
    d_nulls = torch.tensor(flat.nulls, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.tensor(gids, dtype=torch.int64, device="cuda:0")
    d_mask = torch.tensor(mask, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for first in (0, 1234):
        m = n - first
        assert first == 0 or flat.offsets[first] != 0
        page = pkg.Page(pkg.DeviceBlock(pkg.BIGINT, m, d_keys.data_ptr() + 8 * first), pkg.DeviceBlock(pkg.VARCHAR, m, d_pool, d_nulls.data_ptr() + first, d_offs.data_ptr() + 4 * first),
                        pkg.DeviceBlock(pkg.BOOLEAN, m, d_mask.data_ptr() + first))
        sub = vals[first:], gids[first:].tolist(), mask[first:].astype(bool).tolist()
        w = {}
        for g in sorted(set(sub[1])):
            w[g] = tuple(M.single([(sub[0], sub[1], sub[2] if len(a) > 2 else None)], a[0], 9)[g][1] for a in aggs)
        assert single_rows(pkg, run_varchar(pkg, ctx, [page], aggs, 9), aggs) == w, first
    ctx.synchronize()


def test_varchar_refusals(pkg, ctx):
    B, V = pkg.BIGINT, pkg.VARCHAR
    f = pkg.field
    for fn in (pkg.MIN_VARCHAR, pkg.MAX_VARCHAR):
        fac = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], [(fn, 1)])
        with pytest.raises(pkg.TgpuError) as e:
            fac.setSpillEnabled(True)
        assert e.value.code == NOT_SUPPORTED and "min / max over VARCHAR cannot spill" in str(e.value)
        # the factory stays usable unspilled
        page = pkg.Page(pkg.Block(B, [1, 1, 2]), pkg.Block(V, [b"b", b"a", None]))
        op = fac.createOperator()
        out = pkg.to_pages(op, [page])
        op.close()
        fac.close()
        assert single_rows(pkg, out, [(fn, 1)]) == {1: (b"a" if fn == pkg.MIN_VARCHAR else b"b",), 2: (None,)}
        with pytest.raises(pkg.TgpuError) as e:
            pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], [(fn, 1)], spill_enabled=True)
        assert e.value.code == NOT_SUPPORTED
        with pytest.raises(pkg.TgpuError) as e:
            pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, [B, V], None, [f(0, B), f(1, V)], [B], [0], [(fn, 1)])
        assert e.value.code == NOT_SUPPORTED and "VARCHAR" in str(e.value)
        with pytest.raises(pkg.TgpuError) as e:
            pkg.StreamingAggregationOperatorFactory(ctx, 0, [B, V], [0], pkg.SINGLE, [(fn, 1)])
        assert e.value.code == NOT_SUPPORTED and "VARCHAR" in str(e.value)
        # a wrong input type: the plain factory says so when the page reaches its accumulators
        op = pkg.HashAggregationOperatorFactory(ctx, 0, [B], [0], [(fn, 1)]).createOperator()
        with pytest.raises(pkg.TgpuError) as e:
            pkg.to_pages(op, [pkg.Page(pkg.Block(B, [1, 2, 3]), pkg.Block(B, [1, 2, 3]))])
        assert e.value.code == INVALID_ARGUMENT and "type" in str(e.value)
        op.close()
    # window aggregates know none of the new functions
    for fn in range(11, 17):
        with pytest.raises(pkg.TgpuError) as e:
            pkg.WindowOperatorFactory(ctx, 0, [B, pkg.INTEGER], [0, 1], [pkg.WindowFunction(pkg.WINDOW_AGGREGATE, (1,), pkg.FRAME_PARTITION, fn)], [0], [], [])
        assert e.value.code == INVALID_ARGUMENT and "unknown aggregate function" in str(e.value), fn


def test_varchar_store_memory(pkg, ctx):
    """50 pages over the same 1,000 groups whose maximum changes with every page.  The store is an append-only arena, compacted -- into
    one of 2 x (live + the page's winners) bytes -- when its garbage exceeds its live bytes, doubled to 2 x (cursor + winners) when full;
    between pages cursor <= 2 x live + the last page's winners, so arena <= 4 x (live + one page's winners) (+ 4 KiB, the smallest
    arena).  Beside it 40 bytes per group of capacity (count, two words, claim, position, length; capacity: the next power of two), and
    the operator's other memory, measured here as what it holds after the first page minus the first page's own bound."""
    ngroups, width = 1000, 40
    aggs = [(pkg.MAX_VARCHAR, 1)]
    gids = np.arange(ngroups, dtype=np.int64)
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT], [0], aggs, expected_groups=ngroups).createOperator()
    live = one_page = ngroups * width
    bound = 4 * (live + one_page) + 4096
    sizes = []
    for p in range(50):
        vals = [b"%04d-%06d-" % (p, g) + b"x" * (width - 12) for g in range(ngroups)]
        assert len(vals[0]) == width
        op.addInput(pkg.Page(pkg.Block(pkg.BIGINT, gids), pkg.Block(pkg.VARCHAR, vals)))
        sizes.append(op.memoryBytes())
    other = sizes[0]                                                         # table, fixed-width arrays, the first arena (at most `bound`)
    assert max(sizes) <= other + bound, (sizes[0], max(sizes), bound)
    assert max(sizes[25:]) <= max(sizes[:25]), sizes                          # it does not grow page by page
    op.finish()
    out = []
    while not op.isFinished():
        o = op.getOutput()
        if o is not None:
            out.append(o.to_host())
            o.release()
    op.close()
    got = single_rows(pkg, out, aggs)
    assert got == {g: (b"0049-%06d-" % g + b"x" * (width - 12),) for g in range(ngroups)}

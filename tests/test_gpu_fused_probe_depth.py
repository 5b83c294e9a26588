"""Pass 1 of the fused join probe with its row loads two tiles ahead (jit.cpp FJ_DEPTH 2, whole-table launches; TGPU_FJ_DEPTH chooses for
studies and tests): a second set of row registers, one more pipeline stage to fill and to drain.  Every case runs the same join at depth 1
and at depth 2, compares the two row for row (null outputs included) and both with the numpy filter + the oracle's probe, and proves from
the per-depth launch counter which variant ran.  TGPU_FJ_MAX_BLOCKS caps the workgroups of pass 1, so that a few thousand rows give a
workgroup up to ten tiles, chunks of several tiles and tiles past the end of its last chunk; TGPU_DISABLE_PROBE_EPILOGUE keeps such small
pages on the whole-table kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 768          # 3 stripes x 256 rows
ROWS = [1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5, 5 * TILE, 6 * TILE - 1, 9 * TILE + 100]
CUT = 9200          # the filter keeps dates above it
KEYS = 6000         # probe keys are drawn from [0, KEYS)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def build_keys():
    rng = np.random.default_rng(977)
    return np.sort(rng.permutation(KEYS)[: (KEYS * 6) // 10]).astype(np.int64)   # unique and dense: DIRECT, or hash table + exact bitmap


_probe_cache = {}


def probe_columns(n, selectivity="half", nulls=True, stride=1):
    """numpy columns [BIGINT key, key nulls, DATE, date nulls, INTEGER, its nulls]; computed once per shape and never changed"""
    k = (n, selectivity, nulls, stride)
    if k not in _probe_cache:
        rng = np.random.default_rng(5000 + n)
        key = rng.integers(0, KEYS, n).astype(np.int64) * stride
        if selectivity == "none":
            date = rng.integers(9000, CUT + 1, n)
        elif selectivity == "all":
            date = rng.integers(CUT + 1, 9400, n)
        elif selectivity == "tenth":
            date = np.where(rng.random(n) < 0.1, CUT + 1 + rng.integers(0, 30, n), 9000 + rng.integers(0, 200, n))
        else:
            date = rng.integers(9000, 9400, n)
        val = rng.integers(-1000, 1000, n).astype(np.int32)
        kn = (rng.random(n) < 0.05).astype(np.uint8) if nulls else None
        dn = (rng.random(n) < 0.05).astype(np.uint8) if nulls else None
        vn = (rng.random(n) < 0.3).astype(np.uint8) if nulls else None
        _probe_cache[k] = (key, kn, date.astype(np.int32), dn, val, vn)
    return _probe_cache[k]


def pages_of(pkg, cols, page_rows=None):
    key, kn, date, dn, val, vn = cols
    n = len(key)
    out = []
    for a in range(0, n, page_rows or n):
        b = min(n, a + (page_rows or n))
        cut = lambda v: None if v is None else v[a:b].copy()
        out.append(pkg.Page(pkg.Block(pkg.BIGINT, key[a:b].copy(), cut(kn)), pkg.Block(pkg.DATE, date[a:b].copy(), cut(dn)), pkg.Block(pkg.INTEGER, val[a:b].copy(), cut(vn))))
    return out


def join_rows(pkg, ctx, bkeys, pages, join_type=0):
    """probe-side outputs (date, key, value) + the build side's payload column"""
    f, c = pkg.field, pkg.constant
    T = [pkg.BIGINT, pkg.DATE, pkg.INTEGER]
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [pkg.BIGINT, pkg.BIGINT], [1], [0])
    jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, T, f(1, pkg.DATE) > c(CUT, pkg.DATE), [f(0, pkg.BIGINT), f(1, pkg.DATE), f(2, pkg.INTEGER)], [0],
                                                     probe_output_channels=[1, 0, 2], join_type=join_type)
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(pkg.BIGINT, bkeys), pkg.Block(pkg.BIGINT, np.arange(len(bkeys), dtype=np.int64) * 3 + 1)))
    b.finish()
    op = jf.createOperator()
    rows = [r for p in pkg.to_pages(op, pages) for r in p.rows()]
    op.close()
    b.close()
    return rows


_want_cache = {}


def expected_rows(pkg, oracle, bkeys, cols, join_type, tag):
    """numpy filter, then the oracle's probe of the surviving keys"""
    k = (tag, join_type)
    if k not in _want_cache:
        key, kn, date, dn, val, vn = cols
        keep = date > CUT
        if dn is not None:
            keep &= dn == 0
        sel = np.nonzero(keep)[0]
        kcol = oracle.Col(pkg.BIGINT, key[sel], None if kn is None else kn[sel])
        opx, obx = oracle.PagesHash([oracle.Col(pkg.BIGINT, bkeys)]).probe([kcol], probe_outer=bool(join_type))
        want = []
        for i, j in zip(opx, obx):
            r = sel[i]
            want.append((int(date[r]), None if (kn is not None and kn[r]) else int(key[r]), None if (vn is not None and vn[r]) else int(val[r]), int(j) * 3 + 1 if j >= 0 else None))
        _want_cache[k] = want
    return _want_cache[k]


def both_depths(pkg, ctx, monkeypatch, bkeys, pages, join_type=0, whole_table=True):
    """the join at TGPU_FJ_DEPTH 1 and 2; asserts from the launch counter which kernel variant ran, and that the two agree"""
    got = {}
    for depth in (1, 2):
        monkeypatch.setenv("TGPU_FJ_DEPTH", str(depth))
        before = pkg.fused_probe_depth_counts()
        got[depth] = join_rows(pkg, ctx, bkeys, pages, join_type)
        after = pkg.fused_probe_depth_counts()
        ran = (after[0] - before[0], after[1] - before[1])
        assert sum(ran) >= 1, "the fused probe did not run"
        assert ran[2 - depth] == 0 if whole_table else ran[1] == 0, (depth, ran)
    monkeypatch.delenv("TGPU_FJ_DEPTH")
    assert got[1] == got[2]
    return got[2]


@pytest.mark.parametrize("max_blocks", [1, 2, 3])
def test_pipeline_fill_and_drain(pkg, ctx, oracle, build_keys, monkeypatch, max_blocks):
    """0 to 10 tiles per workgroup in both parities of the unrolled body, a partial last tile, tiles past the end of the last chunk; the
    41-tile page is there for chunks of four tiles, which 10 tiles never reach (a launch keeps at least four chunks per workgroup)"""
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    monkeypatch.setenv("TGPU_FJ_MAX_BLOCKS", str(max_blocks))
    for n in ROWS + [40 * TILE + 3]:
        cols = probe_columns(n)
        want = expected_rows(pkg, oracle, build_keys, cols, 0, ("half", n))
        for shift in (0, 1, 2):
            monkeypatch.setenv("TGPU_FJ_CHUNK_SHIFT", str(shift))
            assert both_depths(pkg, ctx, monkeypatch, build_keys, pages_of(pkg, cols)) == want, (max_blocks, n, shift)
    assert any(r[2] is None for r in want)      # null outputs (a null key never matches: none of those in an inner join)


@pytest.mark.parametrize("stripes", [2, 4])
def test_other_tile_sizes(pkg, ctx, oracle, build_keys, monkeypatch, stripes):
    """TGPU_FJ_STRIPES 2 and 4 (512- and 1024-row tiles): the wait count follows the stripes"""
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    monkeypatch.setenv("TGPU_FJ_STRIPES", str(stripes))
    monkeypatch.setenv("TGPU_FJ_MAX_BLOCKS", "2")
    tile = stripes * 256
    for n in (1, tile - 1, tile + 1, 3 * tile + 5, 6 * tile - 1, 9 * TILE + 100):
        cols = probe_columns(n)
        want = expected_rows(pkg, oracle, build_keys, cols, 0, ("half", n))
        for shift in (0, 2):
            monkeypatch.setenv("TGPU_FJ_CHUNK_SHIFT", str(shift))
            assert both_depths(pkg, ctx, monkeypatch, build_keys, pages_of(pkg, cols)) == want, (stripes, n, shift)


@pytest.mark.parametrize("layout", ["direct", "bitmap", "sparse"])
def test_table_layouts_join_types_and_selectivities(pkg, ctx, oracle, build_keys, monkeypatch, layout):
    """DIRECT, exact bitmap + hash table, Bloom filter + hash table (sparse keys); inner and probe-outer joins; the filter keeps no row,
    every row, one row in ten"""
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    monkeypatch.setenv("TGPU_FJ_MAX_BLOCKS", "2")
    if layout == "bitmap":
        monkeypatch.setenv("TGPU_DISABLE_DIRECT", "1")
    stride = 10**12 if layout == "sparse" else 1
    bkeys = build_keys * stride
    n = 6 * TILE - 1
    for selectivity in ("none", "all", "tenth"):
        cols = probe_columns(n, selectivity, True, stride)
        for join_type in (0, pkg.PROBE_OUTER):
            want = expected_rows(pkg, oracle, bkeys, cols, join_type, (selectivity, n, stride))
            assert both_depths(pkg, ctx, monkeypatch, bkeys, pages_of(pkg, cols), join_type) == want, (layout, selectivity, join_type)
            assert (len(want) == 0) == (selectivity == "none")
    assert any(r[3] is None for r in want)     # (the last case is a probe-outer join: unmatched rows)


@pytest.mark.parametrize("carry", ["0", "1", None])
@pytest.mark.parametrize("nulls", [True, False])
def test_carry_modes_and_null_vectors(pkg, ctx, oracle, build_keys, monkeypatch, carry, nulls):
    """TGPU_FJ_CARRY 0, 1 and the default (partial carry), on pages with and without null vectors (the kernel's no-null-vector variant
    issues half the row loads: another wait count)"""
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    monkeypatch.setenv("TGPU_FJ_MAX_BLOCKS", "3")
    if carry is not None:
        monkeypatch.setenv("TGPU_FJ_CARRY", carry)
    for n in (TILE + 1, 9 * TILE + 100):
        cols = probe_columns(n, "half", nulls)
        want = expected_rows(pkg, oracle, build_keys, cols, 0, ("half", n, nulls))
        assert both_depths(pkg, ctx, monkeypatch, build_keys, pages_of(pkg, cols)) == want, (carry, nulls, n)


def test_paged_input_keeps_depth_1(pkg, ctx, oracle, build_keys, monkeypatch):
    """pages of 1 000 rows run the page / multi-page kernels, which have no depth-2 variant, whatever TGPU_FJ_DEPTH says"""
    n = 9 * TILE + 100
    cols = probe_columns(n)
    want = expected_rows(pkg, oracle, build_keys, cols, 0, ("half", n))
    assert both_depths(pkg, ctx, monkeypatch, build_keys, pages_of(pkg, cols, 1000), whole_table=False) == want


def test_steady_state_without_the_cap(pkg, ctx, oracle, monkeypatch):
    """13 000 003 rows, every resident workgroup, chunks of several tiles: the loop's steady state.  Expected = numpy filter + the oracle's probe."""
    n = 13_000_003
    rng = np.random.default_rng(41)
    bkeys = rng.permutation(400_000)[:120_000].astype(np.int64) * 3 + 7
    pkeys = rng.integers(0, 1_300_000, n).astype(np.int64)
    dates = rng.integers(9000, 9400, n).astype(np.int32)
    sel = np.nonzero(dates > CUT)[0]
    op_, ob = oracle.PagesHash([oracle.Col(pkg.BIGINT, bkeys)]).probe([oracle.Col(pkg.BIGINT, pkeys[sel])])
    want_rows = sel[op_]
    f, c = pkg.field, pkg.constant
    page = pkg.Page(pkg.Block(pkg.BIGINT, pkeys), pkg.Block(pkg.DATE, dates))
    for depth in (2, 1):
        monkeypatch.setenv("TGPU_FJ_DEPTH", str(depth))
        before = pkg.fused_probe_depth_counts()
        bf = pkg.HashBuilderOperatorFactory(ctx, 1, [pkg.BIGINT], [0], [0])
        b = bf.createOperator()
        b.addInput(pkg.Page(pkg.Block(pkg.BIGINT, bkeys)))
        b.finish()
        jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [pkg.BIGINT, pkg.DATE], f(1, pkg.DATE) > c(CUT, pkg.DATE),
                                                         [f(0, pkg.BIGINT), f(1, pkg.DATE)], [0], probe_output_channels=[0, 1])
        op = jf.createOperator()
        out = pkg.to_pages(op, [page])
        after = pkg.fused_probe_depth_counts()
        assert after[depth - 1] - before[depth - 1] == 1 and after[2 - depth] == before[2 - depth]
        assert np.array_equal(np.concatenate([p.getBlock(0).values for p in out]), pkeys[want_rows])
        assert np.array_equal(np.concatenate([p.getBlock(1).values for p in out]), dates[want_rows])
        assert np.array_equal(np.concatenate([p.getBlock(2).values for p in out]), bkeys[ob])
        op.close()
        b.close()


def test_the_default_rule(pkg, ctx, build_keys, monkeypatch):
    """without TGPU_FJ_DEPTH the static rule decides (jit.cpp kFjDepthByCarry): a whole-table launch without a carry or with the partial
    carry loads its rows two tiles ahead, one with the opt-in full carry does not, and a page never does"""
    monkeypatch.delenv("TGPU_FJ_DEPTH", raising=False)
    cols = probe_columns(3 * TILE + 5)
    for carry, epilogue_off, want in (("0", True, (0, 1)), (None, True, (0, 1)), ("1", True, (1, 0)), ("0", False, (1, 0))):
        if carry is None:
            monkeypatch.delenv("TGPU_FJ_CARRY")
        else:
            monkeypatch.setenv("TGPU_FJ_CARRY", carry)
        if epilogue_off:
            monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
        else:
            monkeypatch.delenv("TGPU_DISABLE_PROBE_EPILOGUE")
        before = pkg.fused_probe_depth_counts()
        join_rows(pkg, ctx, build_keys, pages_of(pkg, cols))
        after = pkg.fused_probe_depth_counts()
        assert (after[0] - before[0], after[1] - before[1]) == want, (carry, epilogue_off)

"""The fused join's PARTIAL carry (jit.cpp FJ_CARRY 2, the default where a probe-side output is free): outputs that pass 1 already holds
(fixed width, cannot raise, read only columns of the filter / key row) travel with the pair, the others are gathered by pass 2.  Every
case is compared bit for bit, null outputs included, with TGPU_FJ_CARRY=0 (the two-pass gather), on the DIRECT and the exact-bitmap
layouts, at the tile boundaries (768 rows = 3 stripes x 256), fed as one page and as pages of 1 000 rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 768
SIZES = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
CUT = 9360          # the filter keeps dates above it, and null dates
KEYS = 4000         # probe keys are drawn from [0, KEYS)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def build_keys():
    rng = np.random.default_rng(411)
    return np.sort(rng.permutation(KEYS)[: (KEYS * 7) // 10]).astype(np.int64)   # unique and dense: DIRECT, or hash table + exact bitmap


def probe_columns(pkg, n, selectivity):
    """[BIGINT key (nullable), DATE (nullable; the filter's column), DOUBLE, INTEGER (nullable)]"""
    rng = np.random.default_rng(1000 + n)
    key = pkg.Block(pkg.BIGINT, rng.integers(0, KEYS, n).astype(np.int64), (rng.random(n) < 0.05).astype(np.uint8))
    if selectivity == "none":
        date, dnull = rng.integers(9000, CUT + 1, n), np.zeros(n, dtype=np.uint8)
    elif selectivity == "all":
        date, dnull = rng.integers(CUT + 1, 9400, n), (rng.random(n) < 0.2).astype(np.uint8)
    else:   # about one row in ten: 8 % above the cut, 2 % null
        date, dnull = np.where(rng.random(n) < 0.08, CUT + 1 + rng.integers(0, 30, n), 9000 + rng.integers(0, 300, n)), (rng.random(n) < 0.02).astype(np.uint8)
    x = pkg.Block(pkg.DOUBLE, rng.standard_normal(n))
    i = pkg.Block(pkg.INTEGER, rng.integers(-5, 5, n).astype(np.int32), (rng.random(n) < 0.3).astype(np.uint8))
    return [key, pkg.Block(pkg.DATE, date.astype(np.int32), dnull), x, i]


def slices(pkg, cols, rows):
    n = cols[0].position_count
    if rows is None:
        return [pkg.Page(*cols)]
    out = []
    for a in range(0, n, rows):
        b = min(n, a + rows)
        out.append(pkg.Page(*[pkg.Block(c.type, c.values[a:b].copy(), None if c.nulls is None else c.nulls[a:b].copy()) for c in cols]))
    return out


def join_rows(pkg, ctx, build_keys, pages, T, filt, projs, out_channels, join_type=0):
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [pkg.BIGINT, pkg.BIGINT], [1], [0])
    jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, T, filt, projs, [0], probe_output_channels=out_channels, join_type=join_type)
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(pkg.BIGINT, build_keys), pkg.Block(pkg.BIGINT, np.arange(len(build_keys), dtype=np.int64) * 3)))
    b.finish()
    op = jf.createOperator()
    rows = [r for p in pkg.to_pages(op, pages) for r in p.rows()]
    op.close()
    b.close()
    return rows


def program(pkg):
    f, c = pkg.field, pkg.constant
    T = [pkg.BIGINT, pkg.DATE, pkg.DOUBLE, pkg.INTEGER]
    filt = pkg.expressions.or_(f(1, pkg.DATE) > CUT, pkg.expressions.is_null(f(1, pkg.DATE)))
    # channel 0: the key (free by the definition; carried under rule 0 only); 1: the filter's column, nullable (free);
    # 2: an expression over a column the filter does not read;
    # 3: a nullable column the filter does not read
    projs = [f(0, pkg.BIGINT), f(1, pkg.DATE), f(2, pkg.DOUBLE) * (c(1.0, pkg.DOUBLE) - f(2, pkg.DOUBLE)), f(3, pkg.INTEGER)]
    return T, filt, projs


@pytest.mark.parametrize("selectivity", ["none", "all", "tenth"])
@pytest.mark.parametrize("layout", ["direct", "bitmap"])
def test_partial_carry_matches_the_two_pass_gather(pkg, ctx, build_keys, monkeypatch, layout, selectivity):
    if layout == "bitmap":
        monkeypatch.setenv("TGPU_DISABLE_DIRECT", "1")
    T, filt, projs = program(pkg)
    for n in SIZES:
        cols = probe_columns(pkg, n, selectivity)
        for page_rows in (None, 1000):
            pages = slices(pkg, cols, page_rows)
            got = {}
            for mode in ("default", "0"):
                if mode == "0":
                    monkeypatch.setenv("TGPU_FJ_CARRY", "0")
                else:
                    monkeypatch.delenv("TGPU_FJ_CARRY", raising=False)
                before = pkg.fused_probe_launch_counts()
                got[mode] = join_rows(pkg, ctx, build_keys, pages, T, filt, projs, [1, 0, 3, 2])
                after = pkg.fused_probe_launch_counts()
                launches = sum(after) - sum(before)
                assert launches >= 1, "the fused probe did not run"
                if mode == "0":
                    assert after[2] == before[2] and after[1] == before[1]
                elif len(pages) == 1:
                    assert after[2] - before[2] == launches, "one page: every launch takes the partial carry"
            assert got["default"] == got["0"], (layout, selectivity, n, page_rows)
            # and the rows are the right ones (numpy): the filter's rows whose key is in the build side, in input order
            key, date = cols[0], cols[1]
            keep = ((date.values > CUT) | (date.nulls != 0)) & (key.nulls == 0) & np.isin(key.values, build_keys)
            assert len(got["0"]) == int(keep.sum())
            assert [r[1] for r in got["0"]] == [int(v) for v in key.values[keep]]
            if selectivity == "all" and n >= TILE:
                assert any(r[0] is None for r in got["default"]) and any(r[2] is None for r in got["default"])


def test_outer_join_and_raising_projection_keep_the_fallback(pkg, ctx, build_keys, monkeypatch):
    """neither an outer probe nor a projection that can raise takes a carry mode; their results are those of TGPU_FJ_CARRY=0"""
    f = pkg.field
    T, filt, projs = program(pkg)
    cols = probe_columns(pkg, 3 * TILE + 5, "tenth")
    raising = [f(0, pkg.BIGINT), f(1, pkg.DATE), f(2, pkg.DOUBLE), f(3, pkg.INTEGER) + 1]   # checked INTEGER arithmetic: the unfused composition
    for name, p, jt in (("outer", projs, pkg.PROBE_OUTER), ("raising", raising, pkg.INNER)):
        got = {}
        for mode in ("default", "0"):
            if mode == "0":
                monkeypatch.setenv("TGPU_FJ_CARRY", "0")
            else:
                monkeypatch.delenv("TGPU_FJ_CARRY", raising=False)
            before = pkg.fused_probe_launch_counts()
            got[mode] = join_rows(pkg, ctx, build_keys, [pkg.Page(*cols)], T, filt, p, [1, 0, 3, 2], join_type=jt)
            after = pkg.fused_probe_launch_counts()
            assert after[1:] == before[1:], name
        assert got["default"] == got["0"] and len(got["0"]) > 0, name
    keep = (cols[1].values > CUT) | (cols[1].nulls != 0)
    # PROBE_OUTER: every row the filter keeps comes out, matched or not
    assert len(join_rows(pkg, ctx, build_keys, [pkg.Page(*cols)], T, filt, projs, [1, 0, 3, 2], join_type=pkg.PROBE_OUTER)) == int(keep.sum())


def test_a_key_projection_that_can_raise_is_not_carried(pkg, ctx, build_keys, monkeypatch):
    """the join key's own projection may raise (checked BIGINT arithmetic); such a key is evaluated by pass 1 but never a free channel"""
    f = pkg.field
    T, filt, _ = program(pkg)
    projs = [f(0, pkg.BIGINT) + 1, f(1, pkg.DATE), f(2, pkg.DOUBLE), f(3, pkg.INTEGER)]
    cols = probe_columns(pkg, 3 * TILE + 5, "all")
    got = {}
    for mode in ("default", "0"):
        if mode == "0":
            monkeypatch.setenv("TGPU_FJ_CARRY", "0")
        else:
            monkeypatch.delenv("TGPU_FJ_CARRY", raising=False)
        got[mode] = join_rows(pkg, ctx, build_keys, [pkg.Page(*cols)], T, filt, projs, [0, 1, 3])
    assert got["default"] == got["0"] and len(got["0"]) > 1000
    assert any(r[1] is None for r in got["default"])


@pytest.mark.parametrize("rule", ["0", "1"])
def test_both_static_rules_for_the_join_key_channel(pkg, ctx, build_keys, monkeypatch, rule):
    """TGPU_FJ_CARRY_RULE (kernel studies): 0 carries every free channel, the 8-byte join key included; 1 leaves the key's channel to
    pass 2.  Whichever is the default, both generate the rows of the two-pass gather."""
    monkeypatch.setenv("TGPU_FJ_CARRY_RULE", rule)
    T, filt, projs = program(pkg)
    for n in (TILE + 1, 3 * TILE + 5):
        cols = probe_columns(pkg, n, "all")
        got = {}
        for mode in ("default", "0"):
            if mode == "0":
                monkeypatch.setenv("TGPU_FJ_CARRY", "0")
            else:
                monkeypatch.delenv("TGPU_FJ_CARRY", raising=False)
            before = pkg.fused_probe_launch_counts()
            got[mode] = join_rows(pkg, ctx, build_keys, [pkg.Page(*cols)], T, filt, projs, [1, 0, 3, 2])
            after = pkg.fused_probe_launch_counts()
            assert (after[2] > before[2]) == (mode == "default")
        assert got["default"] == got["0"] and len(got["0"]) > n // 2

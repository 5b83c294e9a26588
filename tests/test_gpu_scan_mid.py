"""k::exclusive_scan_i32 between one tile (2 048 elements) and 16 384 elements is one launch of one 1 024-lane workgroup (basic.hip
scan_mid_i32); above that the three-launch route.  FilterAndProjectOperator scans one count per 1 024-row tile of its page, so pages of
1 024 x t rows put t on both sides of both bounds; the rows that come out must be numpy's, value for value -- a wrong offset moves or
loses rows.  Also exact: the page of which the filter keeps nothing, and the one of which it keeps everything."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE_ROWS = 1024
TILES = [2048, 2049, 4097, 8191, 16384, 16385, 40000]
ROWS = sorted([TILE_ROWS * t for t in TILES] + [TILE_ROWS * t + d for t in (2049, 16384) for d in (-1, 1)])


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.profile_enable(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def column():
    return np.random.default_rng(4242).integers(0, 1000, max(ROWS)).astype(np.int64)


def filtered(pkg, ctx, values, cut):
    f, B = pkg.field, pkg.BIGINT
    op = pkg.FilterAndProjectOperatorFactory(ctx, 0, [B], f(0, B) > cut, [f(0, B)]).createOperator()
    out = pkg.to_pages(op, [pkg.Page(pkg.Block(B, values))])
    op.close()
    return np.concatenate([p.getBlock(0).values for p in out]) if out else np.zeros(0, np.int64)


@pytest.mark.parametrize("n", ROWS)
def test_filter_offsets_on_both_sides_of_the_scan_bounds(pkg, ctx, column, n):
    values = column[:n]
    for cut in (499, 2000, -1):          # about half of the rows, none, all
        got = filtered(pkg, ctx, values, cut)
        want = values[values > cut]
        assert len(got) == len(want) and np.array_equal(got, want), (n, cut)
    assert 0.45 * n < np.count_nonzero(values > 499) < 0.55 * n

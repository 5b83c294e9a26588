"""k::compact_positions (basic.hip: out[rank[i]] = i for every flagged i) through its three callers -- RowNumberOperator with a per-partition
limit, the unmatched build rows of a LookupOuterOperator after a FULL OUTER probe, the VALUES domain of a DynamicFilterSourceOperator -- at
n = 257 (a second block) and n = 600 001 (more than one full grid of 256 CUs x 8 blocks x 256 rows = 524 288: the grid-stride loop runs).
The expected results are plain selections, computed with numpy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SIZES = [257, 600_001]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", SIZES)
def test_row_number_with_a_limit(pkg, ctx, n):
    B = pkg.BIGINT
    rng = np.random.default_rng(n)
    groups, max_rows = (7, 3) if n == 257 else (50_000, 5)
    keys = rng.integers(0, groups, n).astype(np.int64)
    rows = np.arange(n, dtype=np.int64)
    # row number = 1 + how many earlier rows have the same key
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]
    run_start = np.flatnonzero(np.r_[True, sorted_keys[1:] != sorted_keys[:-1]])
    run_of = np.cumsum(np.r_[True, sorted_keys[1:] != sorted_keys[:-1]]) - 1
    number = np.empty(n, dtype=np.int64)
    number[order] = np.arange(n) - run_start[run_of] + 1
    kept = number <= max_rows
    assert 0 < kept.sum() < n

    op = pkg.RowNumberOperatorFactory(ctx, 1, [B, B], [1], [0], max_rows).createOperator()
    out = pkg.to_pages(op, [pkg.Page(pkg.Block(B, keys), pkg.Block(B, rows))])
    op.close()
    assert len(out) == 1
    assert np.array_equal(out[0].getBlock(0).values, rows[kept])
    assert np.array_equal(out[0].getBlock(1).values, number[kept])


@pytest.mark.parametrize("n", SIZES)
def test_unmatched_build_rows_after_a_full_outer_probe(pkg, ctx, n):
    B = pkg.BIGINT
    build_keys = np.random.default_rng(n).permutation(n).astype(np.int64)
    payload = np.arange(n, dtype=np.int64) * 3
    matched = build_keys % 3 != 0
    probe_keys = np.sort(build_keys[matched])
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B, B], [0, 1], [0])
    jf = pkg.LookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [B], [0], join_type=pkg.FULL_OUTER)
    of = pkg.LookupOuterOperatorFactory(ctx, 3, bf.lookup_source_factory, [B])
    build, probe, outer = bf.createOperator(), jf.createOperator(), of.createOperator()
    build.addInput(pkg.Page(pkg.Block(B, build_keys), pkg.Block(B, payload)))
    build.finish()
    joined = pkg.to_pages(probe, [pkg.Page(pkg.Block(B, probe_keys))])
    assert sum(p.getPositionCount() for p in joined) == len(probe_keys)
    probe.close()
    jf.noMoreOperators()
    assert not outer.isBlocked()
    o = outer.getOutput()
    page = o.to_host()
    o.release()
    assert outer.isFinished()
    # the build rows nobody matched, in build-position order; the probe channel is null
    assert page.getPositionCount() == int((~matched).sum())
    assert page.getBlock(0).nulls is not None and page.getBlock(0).nulls.all()
    assert np.array_equal(page.getBlock(1).values, build_keys[~matched])
    assert np.array_equal(page.getBlock(2).values, payload[~matched])
    build.close(); outer.close(); jf.close(); of.close(); bf.close()


@pytest.mark.parametrize("n", SIZES)
def test_dynamic_filter_values_domain(pkg, ctx, n):
    """n distinct entries, a null and a NaN among them: the domain is the other n - 2 values, in first-seen order"""
    D = pkg.DOUBLE
    values = np.random.default_rng(n).permutation(n).astype(np.float64)
    nulls = np.zeros(n, dtype=np.uint8)
    nulls[n // 3] = 1
    values[n // 2] = np.nan
    keep = np.ones(n, dtype=bool)
    keep[[n // 3, n // 2]] = False
    op = pkg.DynamicFilterSourceOperatorFactory(ctx, 1, [D], [0], 1 << 20, 1 << 40, 100).createOperator()
    passed = pkg.to_pages(op, [pkg.Page(pkg.Block(D, values, nulls))])
    assert sum(p.getPositionCount() for p in passed) == n
    kind, got = op.domain(0)
    op.close()
    assert kind == "values"
    assert np.array_equal(np.array(got, dtype=np.float64), values[keep])

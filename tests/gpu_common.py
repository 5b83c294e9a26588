"""Shared helpers of the GPU parity tests."""
import numpy as np

from key_cases import special_doubles


def ocol(oracle, block):
    """product Block -> oracle column (same flat arrays)."""
    b = block.flatten()
    return oracle.Col(b.type, b.values, b.nulls, b.offsets)


def rand_block(pkg, rng, type_id, n, null_frac=0.0, domain=None, special=False):
    """special=True: a DOUBLE block comes from key_cases.special_doubles (NaN payloads, both zeros, infinities, denormals as bit patterns at
    fixed positions over the integer-valued draw from `domain`); every other type, and the default, is unchanged"""
    nulls = (rng.random(n) < null_frac).astype(np.uint8) if null_frac > 0 else None
    if type_id == pkg.BIGINT:
        v = rng.integers(-(2**62), 2**62, n) if domain is None else rng.integers(domain[0], domain[1], n)
        return pkg.Block(pkg.BIGINT, v.astype(np.int64), nulls)
    if type_id in (pkg.INTEGER, pkg.DATE):
        lo, hi = domain or (-(2**31), 2**31 - 1)
        return pkg.Block(type_id, rng.integers(lo, hi, n).astype(np.int32), nulls)
    if type_id == pkg.DOUBLE:
        if special:
            return pkg.Block(pkg.DOUBLE, special_doubles(rng, n, domain or (-1000, 1000)), nulls)
        if domain is None:
            v = rng.standard_normal(n) * 10.0 ** rng.integers(-5, 6, n)
        else:
            v = rng.integers(domain[0], domain[1], n).astype(np.float64)
        return pkg.Block(pkg.DOUBLE, v, nulls)
    if type_id == pkg.BOOLEAN:
        return pkg.Block(pkg.BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), nulls)
    if type_id == pkg.VARCHAR:
        lo, hi = domain or (0, 1000)
        ks = rng.integers(lo, hi, n)
        vals = [None if (nulls is not None and nulls[i]) else ("k%d" % k) * (1 + k % 3) for i, k in enumerate(ks)]
        return pkg.Block(pkg.VARCHAR, vals)
    raise ValueError(type_id)


def ulp_diff(a, b):
    """distance in units in the last place between two float64 arrays (0 for identical bits, NaN == NaN)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ia = a.view(np.int64).copy()
    ib = b.view(np.int64).copy()
    ia = np.where(ia < 0, np.int64(-(2**63)) - ia, ia)
    ib = np.where(ib < 0, np.int64(-(2**63)) - ib, ib)
    d = np.abs(ia - ib)
    both_nan = np.isnan(a) & np.isnan(b)
    return np.where(both_nan, 0, d)


def run_agg(pkg, ctx, pages, group_types, group_channels, aggs, step=0, hash_channel=-1, expected=100):
    f = pkg.HashAggregationOperatorFactory(ctx, 0, group_types, group_channels, aggs, step=step, hash_channel=hash_channel, expected_groups=expected)
    op = f.createOperator()
    out = pkg.to_pages(op, pages)
    op.close()
    rows = []
    for p in out:
        rows.extend(p.rows())
    return rows


def drive_with_revokes(op, pages, revoke, as_pages=False):
    """T/operator/OperatorAssertion.java:84-156 (toPagesPartial + finishOperator with revokeMemory): before every addInput and after
    every getOutput the driver revokes whatever the operator holds as revocable memory.  -> the output rows (as_pages=True: host pages)"""
    out = []

    def revoke_all():
        if revoke and op.revocableMemoryBytes() > 0:
            op.startMemoryRevoke()
            op.finishMemoryRevoke()
    for pg in pages:
        revoke_all()
        assert op.needsInput()
        op.addInput(pg)
        o = op.getOutput()
        assert o is None
    op.finish()
    for _ in range(1000):
        if op.isFinished():
            break
        o = op.getOutput()
        if o is not None:
            out.append(o.to_host())
            o.release()
        revoke_all()
    assert op.isFinished() and not op.needsInput()
    if as_pages:
        return out
    return [r for p in out for r in p.rows()]


def run_join(pkg, ctx, build_pages, probe_pages, types_b, types_p, key_b, key_p, hash_b=-1, hash_p=-1, join_type=0, out_b=None, out_p=None, as_pages=False):
    """-> (output rows, lookup source stats); as_pages=True: the host pages instead of their rows (large outputs, bit-exact comparisons)"""
    out_b = list(range(len(types_b))) if out_b is None else out_b
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, types_b, out_b, key_b, precomputed_hash_channel=hash_b)
    jf = pkg.LookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, types_p, key_p, probe_hash_channel=hash_p, probe_output_channels=out_p, join_type=join_type)
    build = bf.createOperator()
    probe = jf.createOperator()
    assert probe.isBlocked() and not probe.needsInput()  # waits on the lookup source future (LookupJoinOperator.java:235-243)
    for p in build_pages:
        assert build.needsInput()
        build.addInput(p)
    build.finish()
    assert not probe.isBlocked()
    out = pkg.to_pages(probe, probe_pages)
    stats = bf.lookup_source_factory.stats()
    probe.close()
    jf.noMoreOperators()
    assert build.isFinished()
    build.close()
    if as_pages:
        return out, stats
    rows = []
    for p in out:
        rows.extend(p.rows())
    return rows, stats


def outer_join(pkg, ctx, build_pages, probe_page_lists, types_b, types_p, key_b, key_p, join_type, out_b, out_p, fused=None, as_pages=False):
    """several probe operators over one lookup source, then the outer operator; returns (probe rows per operator, outer rows) -- with
    as_pages=True (the host pages per operator, the outer operator's host page or None, the lookup source stats)"""
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, types_b, out_b, key_b)
    if fused is None:
        jf = pkg.LookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, types_p, key_p, probe_output_channels=out_p, join_type=join_type)
    else:
        jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, types_p, fused[0], fused[1], key_p, probe_output_channels=out_p, join_type=join_type)
    of = pkg.LookupOuterOperatorFactory(ctx, 3, bf.lookup_source_factory, [types_p[c] for c in out_p] if fused is None else fused[2])
    build = bf.createOperator()
    probes = [jf.createOperator() for _ in probe_page_lists]
    outer = of.createOperator()
    assert outer.isBlocked() and not outer.needsInput() and outer.getOutput() is None
    for p in build_pages:
        build.addInput(p)
    build.finish()
    stats = bf.lookup_source_factory.stats()
    assert outer.isBlocked()   # the probes are not done yet (PartitionedLookupSourceFactory.java:259-297)
    probe_rows = []
    for op, pages in zip(probes, probe_page_lists):
        host = pkg.to_pages(op, pages)
        if as_pages:
            probe_rows.append(host)
        else:
            rows = []
            for pg in host:
                rows.extend(pg.rows())
            probe_rows.append(rows)
        op.close()
        assert outer.isBlocked()   # ... and the factory may still create more probe operators
    jf.noMoreOperators()
    assert not outer.isBlocked() and not build.isFinished()   # the table stays alive for the outer operator
    o = outer.getOutput()
    if as_pages:
        outer_rows = o.to_host() if o is not None else None
    else:
        outer_rows = o.to_host().rows() if o is not None else []
    if o is not None:
        o.release()
    assert outer.isFinished() and outer.getOutput() is None
    assert build.isFinished()
    build.close(); outer.close(); jf.close(); of.close(); bf.close()
    if as_pages:
        return probe_rows, outer_rows, stats
    return probe_rows, outer_rows

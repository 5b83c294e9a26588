"""Inputs and the join runner shared by test_gpu_direct_rank_heads.py and test_gpu_key_range_wide.py: build sides of the DIRECT
layout (join.hip build_direct) as (key, BIGINT payload = row number) with the payload as the build output, so that every match
needs the key's rank; a probe side that asks for every value around the key range; the join through LookupJoinOperator and through
FilterProjectLookupJoinOperator; the oracle's PagesHash probe as the expectation.  Arrays are computed once per case and never changed."""
import numpy as np

SHAPES = ("consecutive", "stride2", "tpch", "stride64", "clusters")


def np_type(pkg, key_type):
    return np.int64 if key_type == pkg.BIGINT else np.int32


def key_mins(pkg, key_type):
    """not a multiple of 64; negative; next to the type's minimum"""
    lowest = -2**63 if key_type == pkg.BIGINT else -2**31
    return (1000003, -1000, lowest + 5)


_offsets = {}


def offsets(shape, n):
    """strictly ascending int64 distances from the smallest key (the first is 0: bitmap words count from the smallest key);
    largest distance / 64 <= n, the DIRECT layout's density rule"""
    if (shape, n) not in _offsets:
        i = np.arange(n, dtype=np.int64)
        if shape == "consecutive":
            # one key, then consecutive keys from bit 60 of word 0 on: every word's run of 64 rows starts at row 5 mod 64, so the
            # runs straddle every wave, workgroup and grid-stride boundary (all multiples of 64 rows)
            o = np.where(i == 0, 0, i + 59)
        elif shape == "stride2":
            o = 2 * i
        elif shape == "tpch":
            o = (i // 8) * 32 + i % 8          # order keys: 8 present, 24 absent; the smallest is key_min itself
        elif shape == "stride64":
            o = 64 * i                          # one key per word: every row is a run head
        elif shape == "clusters":
            rng = np.random.default_rng(7100 + n)
            step = np.where(rng.random(n) < 1 / 40, 64 * rng.integers(3, 7, n) + rng.integers(0, 64, n), 1)   # gaps of 3-6 empty words
            step[0] = 0
            o = np.cumsum(step)
        else:
            raise ValueError(shape)
        assert n == 1 or (np.all(np.diff(o) > 0) and o[-1] // 64 <= n)
        _offsets[(shape, n)] = o.astype(np.int64)
    return _offsets[(shape, n)]


def probe_side(pkg, key_type, bkeys, seed):
    """every value in [key_min - 2, key_max + 2] once, plus rows with a null key, shuffled; a 0/1 flag column for the fused
    operator's filter (one row in eight is filtered out)"""
    rng = np.random.default_rng(seed)
    lo, hi = int(bkeys.min()) - 2, int(bkeys.max()) + 2
    vals = np.arange(lo, hi + 1, dtype=np.int64)
    n_null = 3 + len(vals) // 16
    keys = np.concatenate([vals, rng.choice(vals, n_null)])
    nulls = np.concatenate([np.zeros(len(vals), np.uint8), np.ones(n_null, np.uint8)])
    perm = rng.permutation(len(keys))
    flags = (rng.integers(0, 8, len(keys)) > 0).astype(np.int64)
    return keys[perm].astype(np_type(pkg, key_type)), nulls[perm], flags


def expected(pkg, oracle, key_type, bkeys, bnulls, probe):
    """(probe key, build position) of every match, in the reference's output order: for the plain join and for the fused
    operator (filter first: the same pairs without the rows the filter drops)"""
    pkeys, pnulls, flags = probe
    op, ob = oracle.PagesHash([oracle.Col(key_type, bkeys, bnulls)]).probe([oracle.Col(key_type, pkeys, pnulls)])
    kept = flags[op] > 0
    return (pkeys[op], ob.astype(np.int64)), (pkeys[op][kept], ob[kept].astype(np.int64))


def run_join(pkg, ctx, key_type, build_page, probe, fused):
    """-> (probe key column, build payload column) of the join's output, and the profile scopes of the build and the probe"""
    pkeys, pnulls, flags = probe
    f, c, B = pkg.field, pkg.constant, pkg.BIGINT
    ctx.profile_reset()
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [key_type, B], [1], [0])
    if fused:
        jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [key_type, B], f(1, B) > c(0, B), [f(0, key_type)], [0])
        page = pkg.Page(pkg.Block(key_type, pkeys, pnulls), pkg.Block(B, flags))
    else:
        jf = pkg.LookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [key_type], [0])
        page = pkg.Page(pkg.Block(key_type, pkeys, pnulls))
    b = bf.createOperator()
    b.addInput(build_page)
    b.finish()
    op = jf.createOperator()
    out = pkg.to_pages(op, [page])
    prof = ctx.profile()
    op.close()
    b.close()
    if not out:
        return (np.zeros(0, pkeys.dtype), np.zeros(0, np.int64)), prof
    for p in out:
        assert p.getBlock(0).nulls is None or not np.any(p.getBlock(0).nulls)
        assert p.getBlock(1).nulls is None or not np.any(p.getBlock(1).nulls)
    return (np.concatenate([p.getBlock(0).values for p in out]), np.concatenate([p.getBlock(1).values for p in out])), prof


def host_build_page(pkg, key_type, bkeys, bnulls=None):
    return pkg.Page(pkg.Block(key_type, bkeys, bnulls), pkg.Block(pkg.BIGINT, np.arange(len(bkeys), dtype=np.int64)))


def same(got, want):
    return len(got[0]) == len(want[0]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

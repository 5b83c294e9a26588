"""The range pass of the DIRECT build (join.hip key_range_kernel) reads a BIGINT key column without a null vector as 16-byte pairs of rows
when its base is 16-byte aligned, several loads per lane, and every other column with the scalar loop.  Its descent flag decides whether the
build side counts as strictly ascending (no direct[] array, rank_base from the run heads), so a missed pair would keep that path for a table
that is not ascending and give wrong payloads or lose a repeated key's second row: the check is the join against the oracle, for tables with
rows p and p + 1 swapped, with row p + 1 equal to row p, and untouched, with p at every kind of boundary -- the halves of a load, neighbouring
lanes, waves, workgroups, the loads of one lane and grid-stride iterations.  The key column is a DeviceBlock over a torch tensor (the
builder adopts it: the kernel sees the tensor's own address) and over that tensor sliced by [1:], whose base is 8 mod 16."""
import numpy as np
import pytest

import direct_build_cases as D

pytestmark = pytest.mark.gpu

# with 256 workgroups (one per CU) the loads of one lane are 65 536 pairs = 131 072 rows apart on the 16-byte route and 65 536 rows apart on
# the scalar route, whose second grid-stride iteration starts at row 4 x 65 536; the 16-byte route's starts at row 8 x 131 072
LOAD_EDGES = [65_535, 65_536, 131_071, 131_072, 262_143, 262_144]
ITERATION_EDGE = 8 * 131_072


def positions(n):
    ps = [0, 1, 2, 63, 64, 127, 255, 256, 1023, 1024, n - 2] + LOAD_EDGES + [ITERATION_EDGE - 1, ITERATION_EDGE]
    return [p for p in ps if p + 1 < n]


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch

    torch.cuda.init()   # torch's runtime first: brought up after the library's context it has been seen to find no device
    c = pkg.Context(0)
    c.profile_enable(True)
    yield c
    c.close()


def ascending_keys(n):
    return 1000003 + D.offsets("tpch" if n < ITERATION_EDGE else "consecutive", n)   # (the large table: a key range, and a probe side, of n values)


def variants(asc, p):
    swapped, equal = asc.copy(), asc.copy()
    swapped[[p, p + 1]] = swapped[[p + 1, p]]
    equal[p + 1] = equal[p]
    return (("swapped", swapped), ("equal", equal))


def device_build_page(pkg, bkeys, skew):
    """the key column at a 16-byte aligned address (skew 0) or 8 bytes past one (skew 1); -> page, tensors to keep alive"""
    import torch

    n = len(bkeys)
    store = torch.from_numpy(np.concatenate([np.zeros(skew, np.int64), bkeys])).to("cuda:0")
    keys = store[skew:]
    assert keys.data_ptr() % 16 == 8 * skew
    payload = torch.arange(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return pkg.Page(pkg.DeviceBlock(pkg.BIGINT, n, keys), pkg.DeviceBlock(pkg.BIGINT, n, payload)), (store, keys, payload)


def check(pkg, ctx, oracle, key_type, bkeys, bnulls, probe, page, ascending, tag):
    want = D.expected(pkg, oracle, key_type, bkeys, bnulls, probe)
    for fused in (False, True):
        got, prof = D.run_join(pkg, ctx, key_type, page, probe, fused)
        assert D.same(got, want[fused]), (tag, fused)
        if ascending is not None:
            assert ("join_build_rank" not in prof and "join_build_prefilter" not in prof) == ascending, (tag, sorted(prof))


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("n", [4099, 300_001, ITERATION_EDGE + 4099])
def test_every_adjacent_pair_is_compared(pkg, ctx, oracle, monkeypatch, n, skew):
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    asc = ascending_keys(n)
    probe = D.probe_side(pkg, pkg.BIGINT, asc, 900 + n)
    page, keep = device_build_page(pkg, asc, skew)
    check(pkg, ctx, oracle, pkg.BIGINT, asc, None, probe, page, True, "ascending")
    # the largest size is there for the iteration edge alone (the smaller two cover every other position)
    for p in (positions(n) if n < ITERATION_EDGE else [ITERATION_EDGE - 1, ITERATION_EDGE]):
        for name, bkeys in variants(asc, p):
            page, keep = device_build_page(pkg, bkeys, skew)
            check(pkg, ctx, oracle, pkg.BIGINT, bkeys, None, probe, page, False, (name, p))


@pytest.mark.parametrize("n", [4099, 300_001])
def test_integer_keys_and_null_vectors_take_the_scalar_loop(pkg, ctx, oracle, monkeypatch, n):
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    asc = ascending_keys(n)
    ints = asc.astype(np.int32)
    probe = D.probe_side(pkg, pkg.INTEGER, ints, 901 + n)
    check(pkg, ctx, oracle, pkg.INTEGER, ints, None, probe, D.host_build_page(pkg, pkg.INTEGER, ints), True, "ascending")
    for p in positions(n):
        for name, bkeys in variants(ints, p):
            check(pkg, ctx, oracle, pkg.INTEGER, bkeys, None, probe, D.host_build_page(pkg, pkg.INTEGER, bkeys), False, (name, p))
    # BIGINT with a null vector: never the ascending path, whatever the order; null build rows are not indexed
    probe = D.probe_side(pkg, pkg.BIGINT, asc, 902 + n)
    bnulls = (np.random.default_rng(903 + n).random(n) < 0.02).astype(np.uint8)
    check(pkg, ctx, oracle, pkg.BIGINT, asc, bnulls, probe, D.host_build_page(pkg, pkg.BIGINT, asc, bnulls), False, "nulls")
    for p in positions(n)[::3]:
        for name, bkeys in variants(asc, p):
            check(pkg, ctx, oracle, pkg.BIGINT, bkeys, bnulls, probe, D.host_build_page(pkg, pkg.BIGINT, bkeys, bnulls), None, (name, p, "nulls"))

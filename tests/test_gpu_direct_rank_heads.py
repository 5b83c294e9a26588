"""DIRECT layout, build side in strictly ascending key order: rank_base comes out of the build pass (join.hip build_direct_kernel<true>:
the first row of every run of rows that share a bitmap word stores its row number) instead of a popcount + scan over the bitmap.  The
build output is the row number, so every match reads rank_base; the probe side asks for every value in [key_min - 2, key_max + 2] (every
empty word, every absent key of a present word) and for nulls.  Rows must equal the oracle's PagesHash probe, through LookupJoinOperator
and through FilterProjectLookupJoinOperator (the fused DIRECT kernels), and the same join with TGPU_DIRECT_RANK_FROM_HEADS=0 (popcount +
scan) and with TGPU_DISABLE_ASCENDING_BUILD=1 (direct[] as well); the profile scopes prove which path built the table."""
import numpy as np
import pytest

import direct_build_cases as D

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]
MANY = 600_000      # above cu_count x 8 x 256 = 524 288 rows: a workgroup of the build pass runs a second grid-stride iteration
VARIANTS = ((None, None), ("TGPU_DIRECT_RANK_FROM_HEADS", "0"), ("TGPU_DISABLE_ASCENDING_BUILD", "1"))


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.profile_enable(True)
    yield c
    c.close()


def key_types(pkg):
    return {"BIGINT": pkg.BIGINT, "INTEGER": pkg.INTEGER, "DATE": pkg.DATE}


def check_ascending(pkg, ctx, oracle, monkeypatch, key_type, shape, n, key_min):
    bkeys = (key_min + D.offsets(shape, n)).astype(D.np_type(pkg, key_type))
    probe = D.probe_side(pkg, key_type, bkeys, 31 + n)
    want = D.expected(pkg, oracle, key_type, bkeys, None, probe)
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")      # the whole-table fused kernels, as a table-at-a-time plan runs them
    for env, value in VARIANTS:
        if env:
            monkeypatch.setenv(env, value)
        for fused in (False, True):
            got, prof = D.run_join(pkg, ctx, key_type, D.host_build_page(pkg, key_type, bkeys), probe, fused)
            assert D.same(got, want[fused]), (shape, n, key_min, env, fused)
            assert "join_build_range" in prof and "join_build_insert" in prof and "join_build_prefilter" not in prof, sorted(prof)   # DIRECT
            assert ("join_build_rank" in prof) == (env is not None), (env, sorted(prof))
            assert ("fused_filter_probe" in prof) == fused, sorted(prof)
        if env:
            monkeypatch.delenv(env)
    assert len(want[0][0]) == n                                  # every build key is asked for exactly once


@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE"])
@pytest.mark.parametrize("n", ROWS)
def test_rank_from_run_heads(pkg, ctx, oracle, monkeypatch, n, type_name):
    key_type = key_types(pkg)[type_name]
    for shape in D.SHAPES:
        for key_min in D.key_mins(pkg, key_type):
            check_ascending(pkg, ctx, oracle, monkeypatch, key_type, shape, n, key_min)


@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE"])
@pytest.mark.parametrize("shape", D.SHAPES)
def test_several_grid_stride_iterations(pkg, ctx, oracle, monkeypatch, shape, type_name):
    key_type = key_types(pkg)[type_name]
    key_min = D.key_mins(pkg, key_type)[D.SHAPES.index(shape) % 3]
    check_ascending(pkg, ctx, oracle, monkeypatch, key_type, shape, MANY, key_min)


@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE"])
def test_not_ascending_keeps_the_scan_and_repeats_leave_the_layout(pkg, ctx, oracle, monkeypatch, type_name):
    key_type = key_types(pkg)[type_name]
    monkeypatch.setenv("TGPU_DISABLE_PROBE_EPILOGUE", "1")
    n = 1025
    for shape in ("tpch", "consecutive"):
        asc = (-1000 + D.offsets(shape, n)).astype(D.np_type(pkg, key_type))
        probe = D.probe_side(pkg, key_type, asc, 77)
        for p in (0, 63, 511, n - 2):
            swapped = asc.copy()
            swapped[[p, p + 1]] = swapped[[p + 1, p]]
            want = D.expected(pkg, oracle, key_type, swapped, None, probe)
            for fused in (False, True):
                got, prof = D.run_join(pkg, ctx, key_type, D.host_build_page(pkg, key_type, swapped), probe, fused)
                assert D.same(got, want[fused]), (shape, p, fused)
                assert "join_build_rank" in prof and "join_build_prefilter" not in prof, sorted(prof)    # DIRECT with direct[]
            repeated = asc.copy()
            repeated[p + 1] = repeated[p]
            want = D.expected(pkg, oracle, key_type, repeated, None, probe)
            assert len(want[0][0]) == n                         # one key is missing, another matches twice
            for fused in (False, True):
                got, prof = D.run_join(pkg, ctx, key_type, D.host_build_page(pkg, key_type, repeated), probe, fused)
                assert D.same(got, want[fused]), (shape, p, fused)
                assert "join_build_rank" not in prof and "join_build_prefilter" in prof, sorted(prof)    # the hash table

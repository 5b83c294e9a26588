"""fj_pair -- pass 2 of an earlier page and pass 1 of a new page in one launch -- on every table layout of the fused probe: DIRECT, exact
bitmap + hash table, Bloom filter + hash table, and the hash table without a pre-filter.  Five probe pages of about one tile, one launch each
(TGPU_DISABLE_PROBE_BATCHING), so that the third page's pass 1 shares its launch with the first page's pass 2; the pairs are the oracle's.
The layout without a pre-filter needs a Bloom budget of zero, which the library reads once per process: that case runs in a fresh one.

Why these cases: every extern "C" entry point of the generated sources is launched by a test that compares with the oracle --
  fp_count, fp_emit                          test_gpu_bench_programs.py::test_cfg2_filter_project_program_vs_oracle
  fp_vwrite                                  test_gpu_string_functions.py::test_boundary_page_every_op_every_row_count
  fj_probe_ / fj_emit_ direct, bitmap, bloom test_gpu_fused_probe_depth.py::test_table_layouts_join_types_and_selectivities
  fj_pair_direct                             test_gpu_parity.py::test_fused_join_keeps_two_small_pages_in_flight
  fa_accumulate_lowcard, fg_probe            test_gpu_parity.py::test_fused_filter_project_aggregation_matches_unfused_and_oracle (4 and 30 groups:
                                             byte ids, 3000: int32 ids)
  fa_accumulate_global                       test_gpu_bigint_sums.py::test_bigint_sums (path fused_general)
  fa_accumulate_ordered, fa_ordered_chain    test_gpu_parity.py::test_aggregation_java_order_chained_few_groups (fused)
  fq_onepass, fq_onepass_multi               test_gpu_double_sums_exact.py::test_double_sums_exact (paths fused_onepass_batch1, fused_onepass)
  nlj_pair_count, nlj_pair_emit              test_gpu_nested_loop_filter.py::test_fused_programs_over_the_shapes
-- except fj_pair_bitmap, fj_pair_bloom and fj_probe_plain / fj_emit_plain / fj_pair_plain, which this file adds.  (fa_mask has no caller in the
library: FusedAggGpu::filter_mask is not used by any operator.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE, CUT = 768, 9200
SIZES = [TILE, TILE + 1, 700, 1, TILE]
# layout -> (stride of the key domain, environment): dense unique keys take DIRECT, without it the exact bitmap; sparse keys the Bloom filter
LAYOUTS = {"direct": (1, {}), "bitmap": (1, {"TGPU_DISABLE_DIRECT": "1"}), "bloom": (10**12, {}), "plain": (10**12, {"TGPU_BLOOM_MAX_BYTES": "0"})}


def paired_probe_equals_the_oracle(pkg, oracle, stride):
    rng = np.random.default_rng(77)
    bkeys = rng.permutation(3000)[:1800].astype(np.int64) * stride
    keys = [rng.integers(0, 3000, n).astype(np.int64) * stride for n in SIZES]
    dates = [rng.integers(9000, 9400, n).astype(np.int32) for n in SIZES]
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    f, c = pkg.field, pkg.constant
    bf = pkg.HashBuilderOperatorFactory(ctx, 1, [pkg.BIGINT], [0], [0])
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(pkg.BIGINT, bkeys)))
    b.finish()
    jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, [pkg.BIGINT, pkg.DATE], f(1, pkg.DATE) > c(CUT, pkg.DATE),
                                                     [f(0, pkg.BIGINT), f(1, pkg.DATE)], [0], probe_output_channels=[0, 1])
    op = jf.createOperator()
    out = pkg.to_pages(op, [pkg.Page(pkg.Block(pkg.BIGINT, k), pkg.Block(pkg.DATE, d)) for k, d in zip(keys, dates)])
    prof = ctx.profile()
    assert "fused_filter_probe" in prof and "fused_probe_pair" in prof and "fused_probe_emit" in prof, sorted(prof)
    key, date = np.concatenate(keys), np.concatenate(dates)
    sel = np.nonzero(date > CUT)[0]
    op_, ob = oracle.PagesHash([oracle.Col(oracle.BIGINT, bkeys)]).probe([oracle.Col(oracle.BIGINT, key[sel])])
    rows = sel[op_]
    assert 0 < len(rows) < len(sel)
    assert np.array_equal(np.concatenate([p.getBlock(0).values for p in out]), key[rows])
    assert np.array_equal(np.concatenate([p.getBlock(1).values for p in out]), date[rows])
    assert np.array_equal(np.concatenate([p.getBlock(2).values for p in out]), bkeys[ob])
    op.close()
    b.close()
    ctx.close()


@pytest.mark.parametrize("layout", ["direct", "bitmap", "bloom"])
def test_paired_launch_on_the_layout(pkg, oracle, monkeypatch, layout):
    stride, env = LAYOUTS[layout]
    monkeypatch.setenv("TGPU_DISABLE_PROBE_BATCHING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    paired_probe_equals_the_oracle(pkg, oracle, stride)


def test_paired_launch_without_a_prefilter_in_a_fresh_process():
    stride, env = LAYOUTS["plain"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, TGPU_DISABLE_PROBE_BATCHING="1", **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "plain child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    import importlib

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    from oracle import oracle as o

    o.build()
    paired_probe_equals_the_oracle(importlib.import_module("presto-1_amd"), o, LAYOUTS["plain"][0])
    print("plain child ok")

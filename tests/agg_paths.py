"""Every path a grouped aggregation takes, reached on purpose: the page sizes, the environment switches, the drivers and the profile scopes
that prove which kernels ran.  Shared by the GPU tests that feed adversarial values down every path (test_gpu_double_sums_exact.py,
test_gpu_bigint_sums.py); each brings its aggregate list, its pages and its expected values.  Importing this file needs no GPU."""
from typing import NamedTuple

from gpu_common import drive_with_revokes

# a few groups: the global-atomics kernel, the lane-private LDS kernels (plain and fused, one launch per page), pages of mixed size into
# one state, global aggregation, PARTIAL -> FINAL, spilled runs, and the Java order
PATHS = ("general", "lowcard", "lowcard_multi", "global", "fused", "fused_onepass", "fused_onepass_batch1", "partial_final", "spilled",
         "java_order", "java_order_fused")
# row-order kernels that differ for BIGINT sums only: many groups, one lane per group (__int128 per lane); the same with one group of more
# than agg.h kOrdHandoffRows rows, whose tail goes to the chained kernel; few groups in Java order, one workgroup per group (split halves)
ORDERED_PATHS = ("ordered_many", "ordered_handoff", "ordered_chain", "fused_ordered_many", "fused_ordered_handoff", "fused_ordered_chain")
# the fused operator's per-row global atomics (the generated "global" body), which a few groups reach only with the LDS path switched off
FUSED_GENERAL = "fused_general"
# PARTIAL -> FINAL over many groups, one PARTIAL per page: every step sums in row order, FINAL through agg_ordered_kernel<INTERMEDIATE>
# (agg_combine_ordered) where a few groups go through agg_combine
PARTIAL_FINAL_MANY = "partial_final_many"
ORDERED_GROUPS = {"many": 20_000, "handoff": 20_000, "chain": 4}
LDS_BYTES = 160 * 1024


def is_fused(path):
    return path.startswith("fused") or path == "java_order_fused"


def page_sizes(path):
    if path == "lowcard_multi":
        return [20_000, 1_000, 3_000, 9_000, 4095, 4096]            # both kernels into one state (asserted for the global aggregation)
    if path.startswith("fused_onepass"):
        return [9_000] * 8
    if path in ("partial_final", "spilled"):
        return [12_000, 3_000, 16_000]
    if path == PARTIAL_FINAL_MANY:
        return [15_000] * 8
    if path.endswith(("ordered_many", "ordered_handoff")):
        return [70_000, 50_000]
    if path.endswith("ordered_chain"):
        return [40_000, 30_000]
    return [40_000]


def late_group_first_row(path, ngroups):
    """fused_onepass: the last group arrives in the 6th page -- that one-pass launch is dirty and re-run; else None"""
    if not (path.startswith("fused_onepass") and ngroups > 1):
        return None
    return [0] * (ngroups - 1) + [sum(page_sizes(path)[:5]) + 4000]


def max_lowcard_groups_plain(n_wide, n_aggs):
    """the most groups that still take the lane-private path of the plain operator (agg.hip lowcard_bytes_per_group): per group one
    (hi, lo) pair of 8-byte words per sum and lane, one 4-byte count per aggregate and lane, 256 lanes, against 160 KiB of LDS"""
    return LDS_BYTES // (n_wide * 2 * 256 * 8 + n_aggs * 256 * 4)


def max_lowcard_groups_fused(n_wide, n_counts):
    """... of the fused operator (jit.cpp): aggregates over the same (input, mask) share a count, sums of the same kind over the same
    (input, mask) share a pair; one more count for the group's rows; 64 bytes of headroom"""
    return (LDS_BYTES - 64) // (n_wide * 2 * 256 * 8 + (n_counts + 1) * 256 * 4)


def select_path(monkeypatch, path):
    if path == "general":
        monkeypatch.setenv("TGPU_DISABLE_LOWCARD", "1")
    if path == "lowcard_multi":                # (the mode is decided by the first page: the later pages are accumulated one by one)
        monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "5000")
    if path in ("fused", FUSED_GENERAL):
        monkeypatch.setenv("TGPU_DISABLE_ONEPASS", "1")
    if path == FUSED_GENERAL:
        monkeypatch.setenv("TGPU_DISABLE_LOWCARD", "1")
    if path.startswith("fused_onepass"):
        monkeypatch.setenv("TGPU_MODE_PREFIX_ROWS", "5000")
        if path == "fused_onepass_batch1":
            monkeypatch.setenv("TGPU_ONEPASS_BATCH_ROWS", "1")


def _rows_of(pkg, op, pages):
    try:
        return [r for p in pkg.to_pages(op, pages) for r in p.rows()]
    finally:
        op.close()


def run_plain(pkg, ctx, pages, ngroups, aggs, global_agg=False, step=0):
    if global_agg:
        op = pkg.HashAggregationOperatorFactory(ctx, 0, [], [], aggs, step=step).createOperator()
        return [(0,) + tuple(r) for r in _rows_of(pkg, op, pages)]
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT], [0], aggs, step=step, hash_channel=-1, expected_groups=ngroups).createOperator()
    return _rows_of(pkg, op, pages)


def run_fused(pkg, ctx, pages, aggs, fused_spec):
    """fused_spec: (input types, filter, projections); the group-by key is projection 0, a BIGINT"""
    types, filt, projs = fused_spec(pkg)
    fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, types, filt, projs, [pkg.BIGINT], [0], aggs)
    return _rows_of(pkg, fac.createOperator(), pages)


def run_spilled(pkg, ctx, pages, ngroups, aggs):
    op = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT], [0], aggs, expected_groups=ngroups, spill_enabled=True).createOperator()
    try:
        rows = drive_with_revokes(op, pages, True)
        assert op.spillStats()[0] >= 1
        return rows
    finally:
        op.close()


def run_partials(pkg, ctx, page_sets, ngroups, aggs):
    """one PARTIAL operator per page set -> its intermediate pages (host), per set"""
    out = []
    for pages in page_sets:
        op = pkg.HashAggregationOperatorFactory(ctx, 0, [pkg.BIGINT], [0], aggs, step=pkg.PARTIAL, expected_groups=ngroups).createOperator()
        try:
            out.append(pkg.to_pages(op, pages))
        finally:
            op.close()
    return out


def final_aggs(pkg, aggs):
    """the FINAL step's aggregates over the intermediate layout: key, then per aggregate count | (count, sum)"""
    out, ch = [], 1
    for a in aggs:
        out.append((a[0], ch))
        ch += 1 if a[0] in (pkg.COUNT_ALL, pkg.COUNT_COLUMN) else 2
    return out


def run_final(pkg, ctx, partial_pages, ngroups, aggs):
    return run_plain(pkg, ctx, partial_pages, ngroups, final_aggs(pkg, aggs), step=pkg.FINAL)


class Outcome(NamedTuple):
    rows: list              # None when the drive raised
    error: object           # the TgpuError the drive raised, or None
    profile: dict


def drive(pkg, monkeypatch, path, ngroups, pages, aggs, fused_spec, partial_final=None):
    """the whole drive of one path in a context of its own -- every page in, finish, every output page out -- with the profile of what
    ran.  A TgpuError is part of the outcome (the profile is still taken); partial_final(ctx) -> rows runs that path's operators."""
    select_path(monkeypatch, path)
    ctx = pkg.Context(0)
    ctx.profile_enable(True)
    rows = error = None
    try:
        try:
            if path in ("general", "lowcard", "lowcard_multi", "global"):
                # (one group through lowcard_multi: a global aggregation, whose pages are accumulated one by one as they come)
                rows = run_plain(pkg, ctx, pages, ngroups, aggs, global_agg=path == "global" or (path == "lowcard_multi" and ngroups == 1))
            elif path in ("fused", "fused_onepass", "fused_onepass_batch1", FUSED_GENERAL):
                rows = run_fused(pkg, ctx, pages, aggs, fused_spec)
            elif path == "spilled":
                rows = run_spilled(pkg, ctx, pages, ngroups, aggs)
            elif path in ("partial_final", PARTIAL_FINAL_MANY):
                rows = partial_final(ctx)
            else:
                if path.startswith("java_order") or path.endswith("ordered_chain"):   # (many groups take the row order by themselves)
                    ctx.set_double_sum_order(pkg.SUM_ORDER_JAVA)
                rows = run_fused(pkg, ctx, pages, aggs, fused_spec) if is_fused(path) else run_plain(pkg, ctx, pages, ngroups, aggs)
        except pkg.TgpuError as e:
            error = e
        prof = ctx.profile()
    finally:
        ctx.close()
    return Outcome(rows, error, prof)


def assert_profile(path, prof, ngroups):
    """the kernels of `path` ran, and not the ones it is meant to avoid"""
    lowcard = "agg_accumulate_lowcard" in prof
    if path == "general":
        assert "agg_accumulate" in prof and not lowcard
    if path in ("lowcard", "global", "spilled", "partial_final"):
        assert lowcard
    if path == "lowcard_multi":
        assert lowcard and ("agg_accumulate" in prof or ngroups > 1), sorted(prof)
    if path == "spilled":
        assert "agg_merge_states" in prof
    if path == "fused":
        assert "fused_project_accumulate_lowcard" in prof and "fused_filter_group_accumulate_onepass" not in prof
    if path.startswith("fused_onepass"):
        assert "fused_filter_group_accumulate_onepass" in prof
    if path == FUSED_GENERAL:
        assert "fused_project_accumulate" in prof and "fused_project_accumulate_lowcard" not in prof and "fused_filter_group_accumulate_onepass" not in prof, sorted(prof)
    if path == PARTIAL_FINAL_MANY:
        assert "agg_accumulate_ordered" in prof and not lowcard, sorted(prof)
    if path in ORDERED_PATHS:
        stem = "fused_project_accumulate_ordered" if is_fused(path) else "agg_accumulate_ordered"
        if path.endswith("chain"):
            assert stem + "_chain" in prof and stem not in prof, sorted(prof)
        else:
            assert stem in prof and stem + "_chain" not in prof, sorted(prof)
        if path.endswith("handoff"):
            assert stem + "_handoff" in prof, sorted(prof)


def assert_folded(path, prof):
    """the lane-private partials of the path's launches were folded into the global state"""
    if path in ("lowcard", "lowcard_multi", "global", "spilled", "partial_final", "fused", "fused_onepass", "fused_onepass_batch1"):
        assert "agg_fold_flush" in prof, sorted(prof)

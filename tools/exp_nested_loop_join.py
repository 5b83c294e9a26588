"""Nested loop join study (DESIGN.md section 5 "Nested loop join").

  product   a 2^20-row probe page x a {1, 16, 1024}-row build page, two BIGINT + one DOUBLE channel on each side, all six channels out:
            output bytes / kernel time of the materialisation (profile scope nlj_product), against the float4-copy rate of the chip
            (6.29 TB/s) -- the kernels only write -- and the library's own join_gather rate.
  band      2^20 probe rows x 4096 intervals (2^32 pairs, about 0.1 % surviving): pairs/s of the fused route (nlj_pair_count + nlj_pair_emit
            over the virtual product) and of the unfused composition (NestedLoopJoinOperator -> FilterAndProjectOperator), in the same run.

Prints one JSON line per measurement.  Registers and occupancy of the generated kernels come from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/exp_nested_loop_join.py --only band), counters from a run of their own.

  python tools/exp_nested_loop_join.py [--only product|band] [--probe-rows 1048576] [--intervals 4096]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBPS = 6.29   # float4 copy, MI355X_MICROARCH.md


def dev_page(p, types, tensors):
    n = tensors[0].numel()
    return p.Page(*[p.DeviceBlock(t, n, x) for t, x in zip(types, tensors)], position_count=n)


def build_side(p, ctx, types, tensors):
    bf = p.NestedLoopBuildOperatorFactory(ctx, 1, types)
    bop = bf.createOperator()
    bop.addInput(dev_page(p, types, tensors))
    bop.finish()
    return bf, bop


def drive(op, page):
    """one probe page through the operator, output released as it comes: -> (rows out, output pages)"""
    op.addInput(page)
    rows = pages = 0
    while not op.needsInput():
        o = op.getOutput()
        if o is not None:
            rows += o.position_count
            pages += 1
            o.release()
    return rows, pages


def product(p, ctx, dev, probe_rows, max_output_rows):
    B, D = p.BIGINT, p.DOUBLE
    types = [B, B, D]
    g = torch.Generator(device=dev).manual_seed(7)
    side = lambda n: [torch.randint(0, 1 << 40, (n,), device=dev, generator=g), torch.randint(0, 1 << 40, (n,), device=dev, generator=g),
                      torch.rand(n, device=dev, generator=g, dtype=torch.float64)]
    probe = side(probe_rows)
    for build_rows in (1, 16, 1024):
        bf, bop = build_side(p, ctx, types, side(build_rows))
        jf = p.NestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, types, [0, 1, 2], [0, 1, 2], max_output_rows=max_output_rows)
        op = jf.createOperator()
        for rep in range(2):   # the first pass warms up the allocator
            ctx.profile_enable(rep == 1)
            ctx.profile_reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            rows, pages = drive(op, dev_page(p, types, probe))
            ctx.synchronize()
            wall_ms = (time.perf_counter() - t0) * 1e3
        prof = ctx.profile()
        ctx.profile_enable(False)
        kms = prof["nlj_product"]["total_ms"]
        out_bytes = rows * 48
        tbps = out_bytes / (kms * 1e-3) / 1e12
        print(json.dumps({"study": "product", "probe_rows": probe_rows, "build_rows": build_rows, "rows_out": rows, "output_pages": pages, "max_output_rows": max_output_rows,
                          "output_bytes": out_bytes, "kernel_ms": round(kms, 3), "wall_ms": round(wall_ms, 2), "write_TBps": round(tbps, 3),
                          "frac_of_float4_copy_6.29TBps": round(tbps / COPY_TBPS, 3)}), flush=True)
        op.close()
        jf.noMoreOperators()
        bop.close()
        for h in (jf, bf.bridge, bf):
            h.close()


def band(p, ctx, dev, probe_rows, intervals):
    B = p.BIGINT
    f = p.field
    g = torch.Generator(device=dev).manual_seed(11)
    domain = 1 << 30
    width = domain // 1000   # an interval holds about 0.1 % of the probe values
    x = torch.randint(0, domain, (probe_rows,), device=dev, generator=g)
    lo = torch.randint(0, domain - width, (intervals,), device=dev, generator=g)
    hi = lo + width
    pairs = probe_rows * intervals
    filt = p.and_(f(1, B) <= f(0, B), f(0, B) < f(2, B))   # b.lo <= a.x AND a.x < b.hi
    projs = [f(0, B), f(1, B)]
    bf, bop = build_side(p, ctx, [B, B], [lo, hi])
    results = {}
    # fused: the predicate over the virtual product
    ff = p.FilterProjectNestedLoopJoinOperatorFactory(ctx, 2, bf.bridge, [B], filt, projs)
    # unfused: the product materialised (x, lo, hi), then the page processor
    jf = p.NestedLoopJoinOperatorFactory(ctx, 3, bf.bridge, [B], [0], [0, 1], max_output_rows=1 << 26)
    pf = p.FilterAndProjectOperatorFactory(ctx, 4, [B, B, B], filt, projs)
    fop, jop, pop = ff.createOperator(), jf.createOperator(), pf.createOperator()
    probe = dev_page(p, [B], [x])
    for rep in range(2):
        ctx.profile_enable(rep == 1)
        ctx.profile_reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        survivors, pages = drive(fop, probe)
        ctx.synchronize()
        results["fused"] = (time.perf_counter() - t0, survivors, pages, ctx.profile() if rep == 1 else None)
    for rep in range(2):
        ctx.profile_enable(rep == 1)
        ctx.profile_reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        jop.addInput(probe)
        survivors = pages = 0
        while not jop.needsInput():
            o = jop.getOutput()
            if o is None:
                continue
            pop.addInput(o)
            o.release()
            q = pop.getOutput()
            if q is not None:
                survivors += q.position_count
                pages += 1
                q.release()
        ctx.synchronize()
        results["unfused"] = (time.perf_counter() - t0, survivors, pages, ctx.profile() if rep == 1 else None)
    ctx.profile_enable(False)
    assert results["fused"][1] == results["unfused"][1], (results["fused"][1], results["unfused"][1])
    for route, (wall, survivors, pages, prof) in results.items():
        names = ["nlj_pair_count", "nlj_pair_emit", "nlj_gather"] if route == "fused" else ["nlj_product", "filter_count", "filter_project_emit"]
        kms = {n: round(prof[n]["total_ms"], 3) for n in names if n in prof}
        total = sum(kms.values())
        print(json.dumps({"study": "band", "route": route, "probe_rows": probe_rows, "intervals": intervals, "pairs": pairs, "survivors": survivors,
                          "surviving_fraction": survivors / pairs, "output_pages": pages, "kernel_ms": kms, "kernel_ms_total": round(total, 3), "wall_ms": round(wall * 1e3, 2),
                          "pairs_per_s_kernel": pairs / (total * 1e-3), "pairs_per_s_wall": pairs / wall}), flush=True)
    for op in (fop, jop, pop):
        op.close()
    ff.noMoreOperators()
    jf.noMoreOperators()
    bop.close()
    for h in (ff, jf, pf, bf.bridge, bf):
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["product", "band"])
    ap.add_argument("--probe-rows", type=int, default=1 << 20)
    ap.add_argument("--intervals", type=int, default=4096)
    ap.add_argument("--max-output-rows", type=int, default=0)
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    if args.only in (None, "product"):
        for rows in ([args.max_output_rows] if args.max_output_rows else [1 << 20, 0, 1 << 24]):   # 0 = the operator's default (2^22)
            product(p, ctx, dev, args.probe_rows, rows)
    if args.only in (None, "band"):
        band(p, ctx, dev, args.probe_rows, args.intervals)
    ctx.close()


if __name__ == "__main__":
    main()

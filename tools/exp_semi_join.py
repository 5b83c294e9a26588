"""Semi join study: SqlSemiJoinInPredicateBenchmark's shape (orderkey IN (SELECT orderkey FROM orders WHERE orderkey % 2 = 0)) on bench.gen_q3
data.  Set = o_orderkey with orderkey % 2 = 0; probe = l_orderkey.  Three variants:
  (a) the probe keys as generated (key order) -> bitmap layout,
  (b) the same keys shuffled                  -> bitmap layout, random word loads,
  (c) set and probe keys spread by an odd 64-bit multiplier (a bijection: the same memberships) -> hash layout.
Per variant: build ms (wall, add_input .. finish), probe kernel time (per-kernel HIP events), rows/s, the byte roofline (8 B key + 1 B out per
row against 8 TB/s peak and the 6.1 TB/s measured streaming read of DESIGN.md section 4) and, for (b) / (c), bench.request_roofline with section
4a's random-load rates.  Prints one JSON line per variant.

  python tools/exp_semi_join.py [--sf 100] [--page-rows 67108864]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SPREAD = 0x9E3779B97F4A7C15 - (1 << 64)   # odd: multiplication modulo 2^64 is a bijection


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--page-rows", type=int, default=1 << 26)
    ap.add_argument("--variants", default="abc")
    args = ap.parse_args()
    import importlib
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    t = bench.gen_q3(dev, args.sf)
    okey = t["o_orderkey"]
    lkey = t["l_orderkey"]
    for k in list(t):
        if k not in ("o_orderkey", "l_orderkey"):
            del t[k]
    set_keys = okey[okey % 2 == 0].contiguous()
    torch.cuda.synchronize()
    ctx = p.Context(0)
    B = p.BIGINT
    n = lkey.numel()
    for v in args.variants:
        if v == "a":
            probe_keys, build_keys = lkey, set_keys
        elif v == "b":
            probe_keys, build_keys = lkey[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(5))], set_keys
        else:
            probe_keys, build_keys = lkey * SPREAD, set_keys * SPREAD
        torch.cuda.synchronize()
        bf = p.SetBuilderOperatorFactory(ctx, 1, [B], 0)
        b = bf.createOperator()
        t0 = time.perf_counter()
        b.addInput(p.Page(p.DeviceBlock(B, build_keys.numel(), build_keys), position_count=build_keys.numel()))
        b.finish()
        ctx.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        st = bf.set_supplier.stats()
        jf = p.HashSemiJoinOperatorFactory(ctx, 2, bf.set_supplier, [B], 0)
        op = jf.createOperator()
        kernel = {0: "semi_probe_bitmap", 1: "semi_probe_hash", 2: "semi_probe_generic"}[st["layout"]]
        hits = 0
        for rep in range(2):   # the first pass warms up (allocator, code objects); the second is measured
            ctx.profile_enable(rep == 1)
            ctx.profile_reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            for a in range(0, n, args.page_rows):
                z = min(n, a + args.page_rows)
                op.addInput(p.Page(p.DeviceBlock(B, z - a, probe_keys[a:z]), position_count=z - a))
                o = op.getOutput()
                if rep == 1 and a == 0:
                    hits = int(o.to_host().getBlock(1).values[: 1 << 20].sum())
                o.release()
            ctx.synchronize()
            wall_ms = (time.perf_counter() - t0) * 1e3
        prof = ctx.profile()
        ctx.profile_enable(False)
        kms = prof[kernel]["total_ms"]
        rows_s = n / (kms * 1e-3)
        gbs = 9.0 * n / (kms * 1e-3) / 1e9
        res = {"variant": v, "layout": st["layout"], "set_keys": st["size"], "set_bytes": st["bytes"], "probe_rows": n, "build_ms": round(build_ms, 2),
               "probe_kernel_ms": round(kms, 3), "probe_launches": prof[kernel]["count"], "probe_wall_ms": round(wall_ms, 2), "rows_per_s": rows_s,
               "byte_roofline": {"bytes_per_row": 9, "achieved_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / 8000, 3), "frac_of_6.1TBps": round(gbs / 6100, 3)},
               "hits_in_first_2^20_rows": hits}
        if v in "bc":
            prof1 = {kernel: prof[kernel]}
            res["request_roofline"] = bench.request_roofline(prof1, 1, kernel, n, 1.0, 0.0, st["bytes"],
                                                             "one dependent random load per probe row (the bitmap word / the first slot)")
        print(json.dumps(res), flush=True)
        op.close()
        del op, jf, bf, b
    ctx.close()


if __name__ == "__main__":
    main()

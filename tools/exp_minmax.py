"""min / max over INTEGER, DATE and VARCHAR (DESIGN.md section 5 "min / max over INTEGER, DATE, VARCHAR"): HashAggregationOperator over one
device-resident page of 2^24 rows, BIGINT key, 4 / 65,536 / 4 M groups.

  fixed    max(integer) and max(date) against max(bigint) -- the yardstick -- on the same operator, same keys
  varchar  max(varchar) over values of 10 - 40 bytes, and once more with a shared 8-byte prefix ("https://"), against count(varchar_col)
           beside max(bigint) on the same operator -- the yardstick -- and against the bytes the rounds must touch (offsets, the 7 window
           bytes and the group ids, read by the round and by the select launch) over 8 TB/s; from a profiled drive: the time per round,
           the survivors of round 0, the read-backs per page
  timing   one process, the variants of a shape ALTERNATE drive by drive (measuring guide, section 5): --warmup untimed and --steps timed
           drives each, wall clock around the whole drive with the context synchronised; median, min and spread.  Every drive runs under
           its own time limit (--step-limit seconds, SIGALRM): a drive that exceeds it ends the tool, nothing is started after it.

Prints one JSON line per shape.

  python tools/exp_minmax.py [--only fixed|varchar] [--rows 16777216] [--steps 10] [--warmup 3] [--step-limit 60]
"""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12
GROUPS = (4, 65_536, 4_000_000)


class StepTimeout(Exception):
    pass


def limited(seconds, fn):
    def on_alarm(signum, frame):
        raise StepTimeout()
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(seconds))
    try:
        return fn()
    finally:
        signal.alarm(0)


def drive(fac, page):
    op = fac.createOperator()
    rows = 0
    op.addInput(page)
    op.finish()
    while not op.isFinished():
        o = op.getOutput()
        if o is not None:
            rows += o.position_count
            o.release()
    op.close()
    return rows


def alternate(ctx, variants, page, args):
    """variants: {name: factory}.  -> {name: {median_ms, min_ms, max_ms, groups, kernel_ms, readbacks}}"""
    def one(fac):
        ctx.synchronize()
        t0 = time.perf_counter()
        rows = drive(fac, page)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, rows
    times = {k: [] for k in variants}
    rows = {}
    for step in range(args.warmup + args.steps):
        for name, fac in variants.items():
            t, rows[name] = limited(args.step_limit, lambda: one(fac))
            if step >= args.warmup:
                times[name].append(t)
    out = {}
    for name, fac in variants.items():
        ctx.profile_enable(True)
        ctx.profile_reset()
        limited(args.step_limit, lambda: one(fac))
        prof = ctx.profile()
        ctx.profile_enable(False)
        out[name] = {"median_ms": round(statistics.median(times[name]), 3), "min_ms": round(min(times[name]), 3), "max_ms": round(max(times[name]), 3), "groups": rows[name],
                     "kernel_ms": {k: round(v["total_ms"], 3) for k, v in sorted(prof.items()) if isinstance(v, dict) and v.get("total_ms", 0) > 0},
                     "launches": {k: v["count"] for k, v in sorted(prof.items()) if isinstance(v, dict) and k.startswith("agg_varchar")},
                     "readbacks": prof.get("__readbacks", {}).get("count")}
    return out


def fixed(p, ctx, dev, groups, args):
    rng = np.random.default_rng(11)
    n = args.rows
    keys = torch.from_numpy(rng.integers(0, groups, n)).to(dev)
    big = torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, n)).to(dev)
    i32 = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    page = p.Page(p.DeviceBlock(p.BIGINT, n, keys), p.DeviceBlock(p.BIGINT, n, big), p.DeviceBlock(p.INTEGER, n, i32), p.DeviceBlock(p.DATE, n, i32), position_count=n)
    facs = {name: p.HashAggregationOperatorFactory(ctx, 1, [p.BIGINT], [0], [agg], expected_groups=groups)
            for name, agg in (("max_bigint", (p.MAX_BIGINT, 1)), ("max_integer", (p.MAX_INTEGER, 2)), ("max_date", (p.MAX_DATE, 3)))}
    res = alternate(ctx, facs, page, args)
    for f in facs.values():
        f.close()
    print(json.dumps({"study": "minmax", "shape": "fixed", "rows": n, "groups": groups, **res}), flush=True)


def varchar(p, ctx, dev, groups, prefix, args):
    rng = np.random.default_rng(12)
    n = args.rows
    lens = rng.integers(10, 41, n).astype(np.int32)
    offs = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    pool = rng.integers(97, 123, int(offs[-1])).astype(np.uint8)
    if prefix:
        at = offs[:-1].astype(np.int64)[:, None] + np.arange(len(prefix))
        pool[at] = np.frombuffer(prefix, dtype=np.uint8)
    keys = torch.from_numpy(rng.integers(0, groups, n)).to(dev)
    big = torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, n)).to(dev)
    d_pool, d_offs = torch.from_numpy(pool).to(dev), torch.from_numpy(offs).to(dev)
    torch.cuda.synchronize()
    page = p.Page(p.DeviceBlock(p.BIGINT, n, keys), p.DeviceBlock(p.VARCHAR, n, d_pool, None, d_offs), p.DeviceBlock(p.BIGINT, n, big), position_count=n)
    facs = {"max_varchar": p.HashAggregationOperatorFactory(ctx, 1, [p.BIGINT], [0], [(p.MAX_VARCHAR, 1)], expected_groups=groups),
            "count_varchar_max_bigint": p.HashAggregationOperatorFactory(ctx, 1, [p.BIGINT], [0], [(p.COUNT_COLUMN, 1), (p.MAX_BIGINT, 2)], expected_groups=groups)}
    res = alternate(ctx, facs, page, args)
    for f in facs.values():
        f.close()
    v = res["max_varchar"]
    rounds = v["launches"].get("agg_varchar_extreme_round", 0)
    survivors = v["launches"].get("agg_varchar_extreme_survivors", 0)
    # per candidate row and launch (round, select): two offsets (8 B, neighbours share one), 7 window bytes, the group id (4 B), the group's word (8 B)
    touched = 2 * (4 + 7 + 4) * (n + survivors)
    line = {"study": "minmax", "shape": "varchar", "rows": n, "groups": groups, "prefix": prefix.decode(), "value_bytes": int(offs[-1]), **res, "rounds": rounds,
            "round_ms_each": round(v["kernel_ms"].get("agg_varchar_extreme_round", 0) / max(rounds, 1), 3), "survivors_after_round_0": survivors,
            "round_bytes_touched": touched, "round_floor_ms_at_8TBps": round(touched / HBM_BYTES_PER_S * 1e3, 4)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["fixed", "varchar"])
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=60)
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    torch.cuda.init()
    ctx = p.Context(0)
    try:
        for groups in GROUPS:
            if args.only in (None, "fixed"):
                fixed(p, ctx, dev, groups, args)
            if args.only in (None, "varchar"):
                varchar(p, ctx, dev, groups, b"", args)
        if args.only in (None, "varchar"):
            varchar(p, ctx, dev, GROUPS[1], b"https://", args)
    except StepTimeout:
        print(json.dumps({"study": "minmax", "error": "a drive exceeded its time limit; nothing was started after it"}), flush=True)
        os._exit(3)   # (no clean-up: it would be more work for a device that does not answer)
    ctx.close()


if __name__ == "__main__":
    main()

"""Streaming aggregation study (DESIGN.md section 5 "Streaming aggregation"): StreamingAggregationOperator against HashAggregationOperator on
identical device-resident pages whose rows are grouped on the keys.

  shapes  (a) the reference's BenchmarkHashAndStreamingAggregationOperators: 140 pages x 10 000 rows, rows per group 1 / 10 / 1000, keys
              bigint / varchar / mixed (bigint, varchar, double), count(*) and sum(bigint); key = row / rowsPerGroup
          (b) one page of 2^24 rows, BIGINT key, rows per group 4 and 1000, sum(double)
  timing  one process; --warmup (>= 5) untimed and --steps (>= 20) timed drives per operator and shape, wall clock around the whole drive
          (addInput of every page, every getOutput, finish) with the context synchronised; median and min.  Every drive runs under its own
          time limit (--step-limit seconds, SIGALRM): a drive that exceeds it ends the tool, nothing is started after it.
  profile one more drive per operator with the kernel timer on: the scopes' total ms (the kernel-stat table), and for the streaming
          operator the detection launches' (sagg_heads + sagg_publish) achieved bytes/s against their algorithmic bytes per row
          (2 x key bytes + 4: streaming_agg.hip) and the fraction of 8 TB/s that is.

Prints one JSON line per shape.

  python tools/exp_streaming_agg.py [--only a|b] [--steps 20] [--warmup 5] [--step-limit 60]
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


def varchar_tensors(dev, ids):
    """String.valueOf(id) per row as (byte pool, int32 offsets) on the device"""
    strs = [str(int(i)).encode() for i in ids]
    lens = np.fromiter((len(s) for s in strs), dtype=np.int32, count=len(strs))
    offs = np.zeros(len(strs) + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    pool = np.frombuffer(b"".join(strs), dtype=np.uint8).copy()
    return torch.from_numpy(pool).to(dev), torch.from_numpy(offs).to(dev)


def make_pages(p, dev, key_kinds, rows_per_page, pages, rows_per_group, value_kind, keep):
    """-> (types, pages): key channels first, then one value channel; keys = row / rows_per_group over the whole stream"""
    n = rows_per_page * pages
    ids = np.arange(n, dtype=np.int64) // rows_per_group
    cols = []
    for kind in key_kinds:
        if kind == "bigint":
            cols.append((p.BIGINT, torch.from_numpy(ids).to(dev), None))
        elif kind == "double":
            cols.append((p.DOUBLE, torch.from_numpy(ids.astype(np.float64)).to(dev), None))
        else:
            cols.append((p.VARCHAR,) + varchar_tensors(dev, ids))
    rng = np.random.default_rng(1)
    if value_kind == "bigint":
        cols.append((p.BIGINT, torch.from_numpy(rng.integers(0, 1000, n)).to(dev), None))
    else:
        cols.append((p.DOUBLE, torch.from_numpy(rng.standard_normal(n)).to(dev), None))
    keep.append(cols)
    out = []
    for a in range(0, n, rows_per_page):
        b = a + rows_per_page
        blocks = []
        for t, values, offsets in cols:
            if t == p.VARCHAR:
                blocks.append(p.DeviceBlock(t, b - a, values, None, offsets[a:b + 1]))
            else:
                blocks.append(p.DeviceBlock(t, b - a, values[a:b]))
        out.append(p.Page(*blocks, position_count=b - a))
    return [c[0] for c in cols], out


def drive(op_factory, pages):
    op = op_factory.createOperator()
    rows = 0

    def pull():
        nonlocal rows
        o = op.getOutput()
        if o is None:
            return False
        rows += o.position_count
        o.release()
        return True

    for pg in pages:
        op.addInput(pg)
        while pull():
            pass
    op.finish()
    while not op.isFinished():
        pull()
    op.close()
    return rows


def timed(ctx, fac, pages, warmup, steps, limit):
    def one():
        ctx.synchronize()
        t0 = time.perf_counter()
        rows = drive(fac, pages)
        ctx.synchronize()
        return time.perf_counter() - t0, rows
    for _ in range(warmup):
        limited(limit, one)
    times, rows = [], 0
    for _ in range(steps):
        t, rows = limited(limit, one)
        times.append(t * 1e3)
    ctx.profile_enable(True)
    ctx.profile_reset()
    limited(limit, one)
    prof = ctx.profile()
    ctx.profile_enable(False)
    table = {k: round(v["total_ms"], 3) for k, v in sorted(prof.items()) if isinstance(v, dict) and v.get("total_ms", 0) > 0}
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "groups": rows, "kernel_ms": table}


def shape(p, ctx, dev, name, key_kinds, rows_per_page, pages, rows_per_group, aggs_of, value_kind, args):
    keep = []
    types, pgs = make_pages(p, dev, key_kinds, rows_per_page, pages, rows_per_group, value_kind, keep)
    torch.cuda.synchronize()
    nk = len(key_kinds)
    aggs = aggs_of(nk)
    sf = p.StreamingAggregationOperatorFactory(ctx, 1, types, list(range(nk)), p.SINGLE, aggs)
    hf = p.HashAggregationOperatorFactory(ctx, 2, types[:nk], list(range(nk)), aggs, expected_groups=max(16, rows_per_page * pages // rows_per_group))
    streaming = timed(ctx, sf, pgs, args.warmup, args.steps, args.step_limit)
    hashed = timed(ctx, hf, pgs, args.warmup, args.steps, args.step_limit)
    assert streaming["groups"] == hashed["groups"]
    n = rows_per_page * pages
    key_bytes = sum({"bigint": 8, "double": 8}.get(k, 0) for k in key_kinds)
    line = {"study": "streaming_agg", "shape": name, "keys": key_kinds, "rows": n, "pages": pages, "rows_per_group": rows_per_group, "streaming": streaming, "hash": hashed,
            "hash_over_streaming_median": round(hashed["median_ms"] / streaming["median_ms"], 3)}
    detect_ms = streaming["kernel_ms"].get("sagg_heads", 0) + streaming["kernel_ms"].get("sagg_publish", 0)
    if "varchar" not in key_kinds and detect_ms > 0:
        per_row = 2 * key_bytes + 4
        line["detect_bytes_per_row"] = per_row
        line["detect_ms"] = round(detect_ms, 3)
        line["detect_TBps"] = round(per_row * n / (detect_ms * 1e-3) / 1e12, 3)
        line["detect_fraction_of_8TBps"] = round(per_row * n / (detect_ms * 1e-3) / HBM_BYTES_PER_S, 3)
    print(json.dumps(line), flush=True)
    sf.close()
    hf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["a", "b"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=60)
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    try:
        if args.only in (None, "a"):
            for keys in (["bigint"], ["varchar"], ["bigint", "varchar", "double"]):
                for rpg in (1, 10, 1000):
                    shape(p, ctx, dev, "a_%s_%d" % ("mixed" if len(keys) > 1 else keys[0], rpg), keys, 10_000, 140, rpg,
                          lambda nk: [(p.COUNT_ALL, -1), (p.SUM_BIGINT, nk)], "bigint", args)
        if args.only in (None, "b"):
            for rpg in (4, 1000):
                shape(p, ctx, dev, "b_bigint_%d" % rpg, ["bigint"], 1 << 24, 1, rpg, lambda nk: [(p.SUM_DOUBLE, nk)], "double", args)
    except StepTimeout:
        print(json.dumps({"study": "streaming_agg", "error": "a drive exceeded its time limit; nothing was started after it"}), flush=True)
        os._exit(3)   # (no clean-up: it would be more work for a device that does not answer)
    ctx.close()


if __name__ == "__main__":
    main()

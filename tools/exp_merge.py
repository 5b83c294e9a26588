"""Merge study (DESIGN.md section 5 "Merge"): the k-way merge of sorted streams against what a user had to do before -- feed the same
streams, concatenated, to OrderByOperator and sort them again.

  shapes    k = 8 streams of 2^21 rows (one BIGINT key, two BIGINT payload channels), k = 2 and k = 64 at the same total, and a two-key shape
            (k = 8) whose first key has 16 distinct values.  Every stream is device resident and handed over in pages of --page-rows rows.
  per shape rows/s of the merge and of the re-sort (wall clock around the whole drive, second of two passes), their ratio, the kernel time of
            the profile scopes merge_bound / merge_path / merge_gather, and the merge_path passes' achieved bytes/s against their algorithmic
            bytes: 2 x 16 B per row and pass, ceil(log2 k) passes a round (the scope also holds the kernel that writes the pairs).

Prints one JSON line per shape.

  python tools/exp_merge.py [--total-rows 16777216] [--page-rows 262144] [--only k8|k2|k64|lowcard]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_streams(dev, k, rows, lowcard, seed):
    """k sorted streams as tensors: (sort key tensors..., two payload tensors)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    streams = []
    for s in range(k):
        key = torch.randint(-(1 << 62), 1 << 62, (rows,), device=dev, generator=g)
        if lowcard:
            first = torch.randint(0, 16, (rows,), device=dev, generator=g)
            second = torch.randint(0, 1 << 40, (rows,), device=dev, generator=g)
            order = torch.argsort(first * (1 << 40) + second, stable=True)   # by (first, second)
            keys = [first[order].contiguous(), second[order].contiguous()]
        else:
            keys = [torch.sort(key).values]
        payload = [torch.arange(rows, device=dev) + s * rows, torch.randint(0, 1 << 40, (rows,), device=dev, generator=g)]
        streams.append(keys + payload)
    return streams


def pages_of(p, stream, page_rows):
    n = stream[0].numel()
    out = []
    for a in range(0, n, page_rows):
        b = min(n, a + page_rows)
        out.append(p.Page(*[p.DeviceBlock(p.BIGINT, b - a, t[a:b]) for t in stream], position_count=b - a))
    return out


def drive_merge(p, ctx, fac, streams, page_rows):
    op = fac.createOperator()
    for st in streams:
        op.addSplit(p.PageSource(pages_of(p, st, page_rows)))
    op.noMoreSplits()
    rows = pages = 0
    while not op.isFinished():
        o = op.getOutput()
        if o is not None:
            rows += o.position_count
            pages += 1
            o.release()
    op.close()
    return rows, pages


def drive_sort(p, ctx, fac, streams, page_rows):
    op = fac.createOperator()
    for st in streams:
        for pg in pages_of(p, st, page_rows):
            op.addInput(pg)
    op.finish()
    rows = 0
    while not op.isFinished():
        o = op.getOutput()
        if o is not None:
            rows += o.position_count
            o.release()
    op.close()
    return rows


def shape(p, ctx, dev, name, k, total_rows, page_rows, lowcard):
    rows = total_rows // k
    streams = make_streams(dev, k, rows, lowcard, 5)
    nkeys = 2 if lowcard else 1
    types = [p.BIGINT] * (nkeys + 2)
    sort_channels, orders, out = list(range(nkeys)), [p.ASC_NULLS_FIRST] * nkeys, list(range(nkeys + 2))
    torch.cuda.synchronize()
    mf = p.MergeOperatorFactory(ctx, 1, types, out, sort_channels, orders)
    sf = p.OrderByOperatorFactory(ctx, 2, types, out, 10, sort_channels, orders)
    res = {}
    for rep in range(2):   # the first pass warms up the allocator
        ctx.profile_enable(rep == 1)
        ctx.profile_reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        n, pages = drive_merge(p, ctx, mf, streams, page_rows)
        ctx.synchronize()
        res["merge"] = (time.perf_counter() - t0, n, pages)
    prof = ctx.profile()
    ctx.profile_enable(False)
    for rep in range(2):
        ctx.synchronize()
        t0 = time.perf_counter()
        n = drive_sort(p, ctx, sf, streams, page_rows)
        ctx.synchronize()
        res["sort"] = (time.perf_counter() - t0, n)
    assert res["merge"][1] == res["sort"][1] == rows * k
    kms = {s: round(prof[s]["total_ms"], 3) for s in ("merge_bound", "merge_path", "merge_gather") if s in prof}
    rounds = prof.get("merge_bound", {}).get("count", 0)
    passes = max(1, math.ceil(math.log2(k))) if k > 1 else 0
    path_bytes = 2 * 16 * rows * k * passes
    line = {"study": "merge", "shape": name, "k": k, "rows_per_stream": rows, "rows": rows * k, "page_rows": page_rows, "sort_keys": nkeys, "rounds": rounds,
            "output_pages": res["merge"][2], "merge_wall_ms": round(res["merge"][0] * 1e3, 2), "resort_wall_ms": round(res["sort"][0] * 1e3, 2),
            "merge_rows_per_s": rows * k / res["merge"][0], "resort_rows_per_s": rows * k / res["sort"][0], "merge_over_resort": res["sort"][0] / res["merge"][0],
            "kernel_ms": kms, "merge_path_passes": passes, "merge_path_algorithmic_bytes": path_bytes}
    if "merge_path" in kms and kms["merge_path"] > 0:
        line["merge_path_TBps"] = round(path_bytes / (kms["merge_path"] * 1e-3) / 1e12, 3)
    print(json.dumps(line), flush=True)
    for h in (mf, sf):
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-rows", type=int, default=1 << 24)
    ap.add_argument("--page-rows", type=int, default=1 << 18)
    ap.add_argument("--only", choices=["k8", "k2", "k64", "lowcard"])
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    for name, k, lowcard in (("k8", 8, False), ("k2", 2, False), ("k64", 64, False), ("lowcard", 8, True)):
        if args.only in (None, name):
            shape(p, ctx, dev, name, k, args.total_rows, args.page_rows, lowcard)
    ctx.close()


if __name__ == "__main__":
    main()

"""RowNumberOperator study: the partitioned operator over device-resident, library-owned pages (one BIGINT partition key drawn uniformly from G
values, the key as the only output channel), with and without maxRowsPerPartition, at
  page sizes  2^20 and 2^24 rows,
  G           4, 1000, kLdsGroups (read from csrc/rownumber.h) and 10^6,
and, for G <= kLdsGroups, the same input forced down the sort path (TGPU_ROW_NUMBER_PATH=sort, read when the operator is created): the sort
path is the baseline of the LDS path.  Per configuration: a fresh operator takes one untimed page (the hash learns the keys, scratch is
allocated), then --pages timed pages; wall time per row (median / min / max over --runs), the HIP-event time of the ranking scopes
(row_number_lds or row_number_sort, + row_number_compact with a limit) against everything else (= get_group_ids and the gathers), and the
ranking step's bytes per second for the LDS path's traffic model (4 B id read twice + 8 B row number written, + 4 B keep flag with a
limit).  Prints one JSON line per configuration.

  python tools/exp_row_number.py [--sizes 20,24] [--groups 4,1000,2048,1000000] [--pages 2] [--runs 3] [--max 3]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))



def lds_groups():
    """RowNumbererGpu::kLdsGroups, read from csrc/rownumber.h: the tool's choice of the group counts it also forces down the sort path and
    its `path` label follow the library's threshold"""
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "presto-1_amd", "csrc", "rownumber.h")
    return int(re.search(r"kLdsGroups\s*=\s*(\d+)", open(header).read()).group(1))


K_LDS_GROUPS = lds_groups()
RANK_SCOPES = ("row_number_lds", "row_number_sort", "row_number_compact")


def owned_pages(p, ctx, dev, rows, groups, count):
    """`count` library-owned device pages of one BIGINT channel (an identity projection copies the borrowed blocks once)"""
    g = torch.Generator(device=dev).manual_seed(11)
    head = p.FilterAndProjectOperatorFactory(ctx, 90, [p.BIGINT], None, [p.field(0, p.BIGINT)]).createOperator()
    out = []
    for _ in range(count):
        k = torch.randint(0, groups, (rows,), dtype=torch.int64, device=dev, generator=g)
        torch.cuda.synchronize()
        head.addInput(p.Page(p.DeviceBlock(p.BIGINT, rows, k), position_count=rows))
        out.append(head.getOutput())
        ctx.synchronize()
    head.close()
    return out


def one_run(p, ctx, pages, max_rows, path):
    if path:
        os.environ["TGPU_ROW_NUMBER_PATH"] = path
    else:
        os.environ.pop("TGPU_ROW_NUMBER_PATH", None)
    op = p.RowNumberOperatorFactory(ctx, 1, [p.BIGINT], [0], [0], max_rows, -1, 10_000).createOperator()
    os.environ.pop("TGPU_ROW_NUMBER_PATH", None)
    op.addInput(pages[0])
    o = op.getOutput()
    if o is not None:
        o.release()
    ctx.synchronize()
    kept = 0
    t0 = time.perf_counter()
    for pg in pages[1:]:
        op.addInput(pg)
        o = op.getOutput()
        if o is not None:
            kept += o.position_count
            o.release()
    ctx.synchronize()
    wall = time.perf_counter() - t0
    op.close()
    return wall, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--groups", default="4,1000,%d,1000000" % K_LDS_GROUPS)
    ap.add_argument("--pages", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max", type=int, default=3)
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    for log_rows in [int(s) for s in args.sizes.split(",")]:
        rows = 1 << log_rows
        for groups in [int(s) for s in args.groups.split(",")]:
            pages = owned_pages(p, ctx, dev, rows, groups, args.pages + 1)
            timed_rows = rows * args.pages
            for max_rows in (None, args.max):
                for path in ([None, "sort"] if groups <= K_LDS_GROUPS else [None]):
                    one_run(p, ctx, pages, max_rows, path)   # warm-up: allocator, code objects
                    walls = [one_run(p, ctx, pages, max_rows, path)[0] for _ in range(args.runs)]
                    ctx.profile_enable(True)
                    ctx.profile_reset()
                    _, kept = one_run(p, ctx, pages, max_rows, path)
                    prof = ctx.profile()
                    ctx.profile_enable(False)
                    scopes = {k: v for k, v in prof.items() if not k.startswith("__")}
                    # the profile covers the untimed first page too: pages + 1 pages of the same size
                    rank_ms = sum(v["total_ms"] for k, v in scopes.items() if k in RANK_SCOPES) * args.pages / (args.pages + 1)
                    other_ms = sum(v["total_ms"] for k, v in scopes.items() if k not in RANK_SCOPES) * args.pages / (args.pages + 1)
                    med = statistics.median(walls)
                    bytes_per_row = 16 + (4 if max_rows is not None else 0)
                    gbs = bytes_per_row * timed_rows / (rank_ms * 1e-3) / 1e9 if rank_ms > 0 else 0.0
                    print(json.dumps({
                        "rows_per_page": rows, "groups": groups, "max_rows_per_partition": max_rows,
                        "path": path or ("lds" if groups <= K_LDS_GROUPS else "sort"), "forced": path is not None,
                        "timed_pages": args.pages, "kept_rows": kept,
                        "wall_ms": {"median": round(med * 1e3, 3), "min": round(min(walls) * 1e3, 3), "max": round(max(walls) * 1e3, 3), "runs": args.runs},
                        "ns_per_row": round(med / timed_rows * 1e9, 4),
                        "ranking_ms": round(rank_ms, 3), "ranking_ns_per_row": round(rank_ms * 1e6 / timed_rows, 4), "other_ms": round(other_ms, 3),
                        "ranking_GBps": round(gbs, 1), "ranking_bytes_per_row_model": bytes_per_row,
                        "readbacks": prof["__readbacks"]["count"],
                        "scopes_ms": {k: round(v["total_ms"], 3) for k, v in sorted(scopes.items())},
                    }), flush=True)
            for o in pages:
                o.release()
    ctx.close()


if __name__ == "__main__":
    main()

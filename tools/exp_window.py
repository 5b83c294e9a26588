"""WindowOperator study: window functions OVER (PARTITION BY k ORDER BY x) over one device-resident, library-owned page (one BIGINT partition key
drawn uniformly from G values, one BIGINT sort key from 2^20 values, one BIGINT value), at
  rows  2^20 and 2^24,
  G     1, 1000, 10^6.
Two operators over the same rows and keys, in the same run:
  window    WindowOperator with --functions: `few` = row_number, rank, sum(v) RANGE .. CURRENT ROW; `many` = those plus dense_rank, cume_dist, lag(v),
            count(*), min(v), max(v) over the partition, sum(v) ROWS .. CURRENT ROW (5 running aggregates: two runs of the scan)
  order_by  OrderByOperator over (k, x): the sort is common to both, so the difference is what heads, scan, evaluate and the gathers of the function
            channels cost
Per shape and operator: the wall time of addInput + finish() + getOutput() as median / min / max over --runs, per row, and the HIP-event time of every
profile scope of one further run (window_heads, window_scan, window_evaluate; the sort shows under TopN's scopes, the gathers under `gather`).  For the
scan the line carries the bytes it must move (launch 1: the head byte, the position and the 8-byte argument per aggregate in, count and word out;
launch 3: count and word in and out, the head byte in, four index arrays and the head scatter out) and bytes / scope time = the achieved rate.  The
window operator's row_number is compared with the order of OrderByOperator before anything is timed.  Prints one JSON line per shape and operator.

  python tools/exp_window.py [--sizes 20,24] [--groups 1,1000,1000000] [--functions few,many] [--runs 5]
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



def owned_page(p, ctx, dev, rows, groups):
    """one library-owned device page (BIGINT k, BIGINT x, BIGINT v): an identity projection copies the borrowed blocks once"""
    g = torch.Generator(device=dev).manual_seed(13)
    head = p.FilterAndProjectOperatorFactory(ctx, 90, [p.BIGINT] * 3, None, [p.field(c, p.BIGINT) for c in range(3)]).createOperator()
    k = torch.randint(0, groups, (rows,), dtype=torch.int64, device=dev, generator=g)
    x = torch.randint(0, 1 << 20, (rows,), dtype=torch.int64, device=dev, generator=g)
    v = torch.randint(-1000, 1000, (rows,), dtype=torch.int64, device=dev, generator=g)
    torch.cuda.synchronize()
    head.addInput(p.Page(*[p.DeviceBlock(p.BIGINT, rows, t) for t in (k, x, v)], position_count=rows))
    out = head.getOutput()
    ctx.synchronize()
    head.close()
    return out


def functions(p, which):
    f = [p.WindowFunction(p.WINDOW_ROW_NUMBER), p.WindowFunction(p.WINDOW_RANK), p.WindowFunction(p.WINDOW_AGGREGATE, (2,), p.FRAME_RANGE_TO_CURRENT, p.SUM_BIGINT)]
    if which == "many":
        f += [p.WindowFunction(p.WINDOW_DENSE_RANK), p.WindowFunction(p.WINDOW_CUME_DIST), p.WindowFunction(p.WINDOW_LAG, (2,)),
              p.WindowFunction(p.WINDOW_AGGREGATE, (), p.FRAME_PARTITION, p.COUNT_ALL), p.WindowFunction(p.WINDOW_AGGREGATE, (2,), p.FRAME_PARTITION, p.MIN_BIGINT),
              p.WindowFunction(p.WINDOW_AGGREGATE, (2,), p.FRAME_PARTITION, p.MAX_BIGINT), p.WindowFunction(p.WINDOW_AGGREGATE, (2,), p.FRAME_ROWS_TO_CURRENT, p.SUM_BIGINT)]
    return f


def scan_bytes(rows, fns, p):
    """what launches 1 and 3 must read and write (launch 2 moves one summary per tile: nothing beside these)"""
    aggs = [f for f in fns if f.function == p.WINDOW_AGGREGATE]
    counts = sum(f.agg_function in (p.COUNT_ALL, p.COUNT_COLUMN) for f in aggs)
    values = len(aggs) - counts
    runs = max(1, -(-len(aggs) // 4))
    launch1 = runs * (1 + 4) + values * (8 + 16) + counts * 8
    launch3 = runs * 1 + values * 32 + counts * 16 + 6 * 4
    return rows * (launch1 + launch3)


def run(p, ctx, page, way, fns, keep=False):
    if way == "window":
        op = p.WindowOperatorFactory(ctx, 1, [p.BIGINT] * 3, [0, 1, 2], fns, [0], [1], [p.ASC_NULLS_LAST], 10_000).createOperator()
    else:
        op = p.OrderByOperatorFactory(ctx, 2, [p.BIGINT] * 3, [0, 1, 2], 10_000, [0, 1], [p.ASC_NULLS_LAST, p.ASC_NULLS_LAST]).createOperator()
    ctx.synchronize()
    t0 = time.perf_counter()
    op.addInput(page)
    op.finish()
    o = op.getOutput()
    ctx.synchronize()
    t1 = time.perf_counter()
    result = o.to_host() if keep else None
    o.release()
    op.close()
    return t1 - t0, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--groups", default="1,1000,1000000")
    ap.add_argument("--functions", default="few,many")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--verify-rows", type=int, default=1 << 20, help="compare the two outputs row for row up to this many rows")
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    for log_rows in [int(s) for s in args.sizes.split(",")]:
        rows = 1 << log_rows
        for groups in [int(s) for s in args.groups.split(",")]:
            page = owned_page(p, ctx, dev, rows, groups)
            ways = [("order_by", None)] + [("window", w) for w in args.functions.split(",")]
            if rows <= args.verify_rows:   # the warm-up doubles as the comparison: same rows in the same order, row_number restarts with the key
                ordered = run(p, ctx, page, "order_by", None, True)[1]
                windowed = run(p, ctx, page, "window", functions(p, "few"), True)[1]
                k = ordered.getBlock(0).values
                assert all((ordered.getBlock(c).values == windowed.getBlock(c).values).all() for c in range(3)), "the window operator's row order differs from OrderBy's"
                heads = [0] + [i for i in range(1, rows) if k[i] != k[i - 1]] if groups <= 1000 else None
                if heads is not None:
                    assert all(windowed.getBlock(3).values[h] == 1 for h in heads)
            for way, which in ways:
                fns = functions(p, which) if which else None
                run(p, ctx, page, way, fns)
                walls = [run(p, ctx, page, way, fns)[0] for _ in range(args.runs)]
                line = {"rows": rows, "groups": groups, "way": way if not which else "window_" + which,
                        "wall_ms": {"median": round(statistics.median(walls) * 1e3, 3), "min": round(min(walls) * 1e3, 3), "max": round(max(walls) * 1e3, 3), "runs": args.runs},
                        "ns_per_row": round(statistics.median(walls) / rows * 1e9, 4)}
                ctx.profile_enable(True)
                ctx.profile_reset()
                run(p, ctx, page, way, fns)
                prof = ctx.profile()
                ctx.profile_enable(False)
                line["readbacks"] = prof["__readbacks"]["count"]
                line["scopes_ms"] = {k: round(v["total_ms"], 3) for k, v in sorted(prof.items()) if not k.startswith("__") and v["total_ms"] > 0}
                if which and prof.get("window_scan", {}).get("total_ms", 0) > 0:
                    line["scan_bytes"] = scan_bytes(rows, fns, p)
                    line["scan_gb_per_s"] = round(line["scan_bytes"] / (prof["window_scan"]["total_ms"] * 1e-3) / 1e9, 1)
                print(json.dumps(line), flush=True)
            page.release()
    ctx.close()


if __name__ == "__main__":
    main()

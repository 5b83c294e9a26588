"""TopNRankingOperator study: row_number() OVER (PARTITION BY k ORDER BY x) <= n over device-resident, library-owned pages (one BIGINT partition
key drawn uniformly from G values, one DOUBLE sort key, both as output), at
  page sizes  2^20 and 2^24 rows,
  G           4, 1000, 10^6,
  n           1, 10, 100,
one untimed page plus --pages further pages per stream.  Three ways to the same rows, on the same data in the same run:
  operator     TopNRankingOperator
  no_prefilter the same with TGPU_TOP_N_RANKING_PREFILTER=off (read when the operator is created)
  composition  OrderByOperator (partition key, sort key) -> RowNumberOperator(max = n): how the rows were obtained before the operator existed
Per shape and way: the wall time of the WHOLE stream (every page, finish(), the output page -- the composition does all of its work at finish(),
so only the whole stream compares) as median / min / max over --runs, per input row; for the two operator runs also the wall time of the pages
after the first alone (the steady state of a long stream), the HIP-event time of the prefilter / select / gather / compact scopes, the share of
rows the prefilter dropped and the candidate store's peak size against G x n.  The three outputs are compared row for row before anything is
timed.  Prints one JSON line per shape and way.

  python tools/exp_top_n_ranking.py [--sizes 20,24] [--groups 4,1000,1000000] [--n 1,10,100] [--pages 8] [--runs 3] [--ways operator,no_prefilter,composition]
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

SCOPES = ("top_n_ranking_prefilter", "top_n_ranking_select", "top_n_ranking_gather", "top_n_ranking_compact")
PREFILTER = "TGPU_TOP_N_RANKING_PREFILTER"


def owned_pages(p, ctx, dev, rows, groups, count):
    """`count` library-owned device pages (BIGINT key, DOUBLE sort key): an identity projection copies the borrowed blocks once"""
    g = torch.Generator(device=dev).manual_seed(11)
    head = p.FilterAndProjectOperatorFactory(ctx, 90, [p.BIGINT, p.DOUBLE], None, [p.field(0, p.BIGINT), p.field(1, p.DOUBLE)]).createOperator()
    out = []
    for _ in range(count):
        k = torch.randint(0, groups, (rows,), dtype=torch.int64, device=dev, generator=g)
        x = torch.rand((rows,), dtype=torch.float64, device=dev, generator=g)
        torch.cuda.synchronize()
        head.addInput(p.Page(p.DeviceBlock(p.BIGINT, rows, k), p.DeviceBlock(p.DOUBLE, rows, x), position_count=rows))
        out.append(head.getOutput())
        ctx.synchronize()
    head.close()
    return out


def run_operator(p, ctx, pages, n, prefilter, keep_output=False):
    """(whole-stream wall, wall of the pages after the first, output rows or their count)"""
    if not prefilter:
        os.environ[PREFILTER] = "off"
    try:
        op = p.TopNRankingOperatorFactory(ctx, 1, p.ROW_NUMBER, [p.BIGINT, p.DOUBLE], [0, 1], [0], [1], [p.ASC_NULLS_LAST], n, False, -1, 10_000).createOperator()
    finally:
        os.environ.pop(PREFILTER, None)
    ctx.synchronize()
    t0 = time.perf_counter()
    op.addInput(pages[0])
    ctx.synchronize()
    t1 = time.perf_counter()
    for pg in pages[1:]:
        op.addInput(pg)
    ctx.synchronize()
    t2 = time.perf_counter()
    op.finish()
    o = op.getOutput()
    ctx.synchronize()
    t3 = time.perf_counter()
    result = o.to_host().rows() if keep_output else o.position_count
    o.release()
    op.close()
    return t3 - t0, t2 - t1, result


def run_composition(p, ctx, pages, n, keep_output=False):
    types = [p.BIGINT, p.DOUBLE]
    order_by = p.OrderByOperatorFactory(ctx, 2, types, [0, 1], 10_000, [0, 1], [p.ASC_NULLS_LAST, p.ASC_NULLS_LAST]).createOperator()
    numberer = p.RowNumberOperatorFactory(ctx, 3, types, [0, 1], [0], n, -1, 10_000).createOperator()
    ctx.synchronize()
    t0 = time.perf_counter()
    for pg in pages:
        order_by.addInput(pg)
    order_by.finish()
    ordered = order_by.getOutput()
    numberer.addInput(ordered)
    o = numberer.getOutput()
    ctx.synchronize()
    t1 = time.perf_counter()
    result = o.to_host().rows() if keep_output else o.position_count
    o.release()
    ordered.release()
    order_by.close()
    numberer.close()
    return t1 - t0, None, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--groups", default="4,1000,1000000")
    ap.add_argument("--n", default="1,10,100")
    ap.add_argument("--pages", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ways", default="operator,no_prefilter,composition")
    ap.add_argument("--verify-rows", type=int, default=1 << 21, help="compare the three outputs row for row up to this many output rows")
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    ways = args.ways.split(",")
    runners = {"operator": lambda pages, n, keep=False: run_operator(p, ctx, pages, n, True, keep),
               "no_prefilter": lambda pages, n, keep=False: run_operator(p, ctx, pages, n, False, keep),
               "composition": lambda pages, n, keep=False: run_composition(p, ctx, pages, n, keep)}
    for log_rows in [int(s) for s in args.sizes.split(",")]:
        rows = 1 << log_rows
        for groups in [int(s) for s in args.groups.split(",")]:
            pages = owned_pages(p, ctx, dev, rows, groups, args.pages + 1)
            total_rows = rows * (args.pages + 1)
            for n in [int(s) for s in args.n.split(",")]:
                # the warm-up run of every way doubles as the comparison of their outputs (per partition: the composition emits the partitions
                # in key order, the operator in arrival order; uniform DOUBLE sort keys make ties improbable)
                outputs = {}
                small = min(groups, total_rows) * n <= args.verify_rows
                for way in ways:
                    outputs[way] = runners[way](pages, n, small)[2]
                counts = {w: (len(v) if small else v) for w, v in outputs.items()}
                assert len(set(counts.values())) == 1, counts
                if small and "composition" in outputs:
                    want = sorted(outputs["composition"])
                    for w in ways:
                        assert sorted(outputs[w]) == want, "the output of %s differs from the composition's" % w
                for way in ways:
                    measured = [runners[way](pages, n) for _ in range(args.runs)]
                    walls, steady = [m[0] for m in measured], [m[1] for m in measured if m[1] is not None]
                    line = {"rows_per_page": rows, "groups": groups, "n": n, "way": way, "pages": args.pages + 1, "output_rows": counts[way], "verified_rows": bool(small),
                            "wall_ms": {"median": round(statistics.median(walls) * 1e3, 3), "min": round(min(walls) * 1e3, 3), "max": round(max(walls) * 1e3, 3), "runs": args.runs},
                            "ns_per_row": round(statistics.median(walls) / total_rows * 1e9, 4)}
                    if steady:
                        line["steady_ms"] = {"median": round(statistics.median(steady) * 1e3, 3), "min": round(min(steady) * 1e3, 3), "max": round(max(steady) * 1e3, 3)}
                        line["steady_ns_per_row"] = round(statistics.median(steady) / (rows * args.pages) * 1e9, 4)
                    ctx.profile_enable(True)
                    ctx.profile_reset()
                    runners[way](pages, n)
                    prof = ctx.profile()
                    ctx.profile_enable(False)
                    line["readbacks"] = prof["__readbacks"]["count"]
                    if way != "composition":
                        line["scopes_ms"] = {k: round(prof[k]["total_ms"], 3) for k in SCOPES if k in prof}
                        line["compactions"] = prof.get("top_n_ranking_compact", {}).get("count", 0)
                        seen, dropped = prof["top_n_ranking_rows_seen"]["count"], prof["top_n_ranking_rows_dropped"]["count"]
                        line["prefilter_dropped_share"] = round(dropped / seen, 6)
                        line["store_peak_rows"] = int(prof["top_n_ranking_store_rows"]["max_ms"])
                        line["groups_x_n"] = min(groups, total_rows) * n
                    else:
                        line["scopes_ms"] = {k: round(v["total_ms"], 3) for k, v in sorted(prof.items()) if not k.startswith("__") and v["total_ms"] > 0}
                    print(json.dumps(line), flush=True)
            for o in pages:
                o.release()
    ctx.close()


if __name__ == "__main__":
    main()

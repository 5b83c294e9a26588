"""WindowOperator study, RANGE frames with value bounds beside the ROWS frames of tools/exp_window_frames.py: sum(v) and min(v) OVER (PARTITION BY k ORDER BY x
<frame>) over one device-resident, library-owned page (BIGINT k drawn uniformly from G values, BIGINT x from 2^20 values, BIGINT v, three constant ROWS
offsets and the six bound channels x -/+ offset), at 2^24 rows and G = 1000, under
  rows_narrow / rows_wide / rows_whole      ROWS BETWEEN w PRECEDING AND w FOLLOWING, w = 3 / 2000 / 2^30 rows: the yardstick (the path of the parent commit)
  range_narrow / range_wide / range_whole   RANGE BETWEEN d PRECEDING AND d FOLLOWING through tgpu_window_factory_create_ranged, d chosen so that the value
                                            window holds as many rows on average as the ROWS frame beside it: d = w * 2^20 * G / rows (whole: 2^20)
The frames alternate inside every repetition.  Per frame: the wall time of addInput + finish() + getOutput() and the HIP-event time of the profile scopes;
window_frames is the bound pass -- window_ends plus window_frame_bounds for ROWS, window_ends plus window_range_keys and window_range_bounds for RANGE -- as
median / min / max over --runs profiled repetitions.  Before anything is timed, at 2^16 rows, every result is compared with numpy.  One JSON line per frame.

  python tools/exp_window_range.py [--rows 24] [--groups 1000] [--runs 7] [--frames rows_narrow,range_narrow,...]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

WIDTHS = {"narrow": 3, "wide": 2000, "whole": 1 << 30}
SCOPES = ("window_heads", "window_scan", "window_frames", "window_extremes", "window_evaluate")
FRAMES = ["rows_narrow", "range_narrow", "rows_wide", "range_wide", "rows_whole", "range_whole"]
KINDS = ("narrow", "wide", "whole")


def distances(rows, groups):
    """the value distance whose window holds about 2 w + 1 rows of a partition"""
    spacing = max(1, ((1 << 20) * groups) // rows)
    return {"narrow": WIDTHS["narrow"] * spacing, "wide": min(WIDTHS["wide"] * spacing, 1 << 20), "whole": 1 << 20}


def owned_page(p, ctx, dev, rows, groups):
    """one library-owned device page: k, x, v, the three ROWS offsets (3 - 5), x - d and x + d per kind (6 - 11)"""
    g = torch.Generator(device=dev).manual_seed(13)
    head = p.FilterAndProjectOperatorFactory(ctx, 90, [p.BIGINT] * 12, None, [p.field(c, p.BIGINT) for c in range(12)]).createOperator()
    k = torch.randint(0, groups, (rows,), dtype=torch.int64, device=dev, generator=g)
    x = torch.randint(0, 1 << 20, (rows,), dtype=torch.int64, device=dev, generator=g)
    v = torch.randint(-1000, 1000, (rows,), dtype=torch.int64, device=dev, generator=g)
    consts = [torch.full((rows,), WIDTHS[kind], dtype=torch.int64, device=dev) for kind in KINDS]
    d = distances(rows, groups)
    bounds = [t for kind in KINDS for t in (x - d[kind], x + d[kind])]
    torch.cuda.synchronize()
    head.addInput(p.Page(*[p.DeviceBlock(p.BIGINT, rows, t) for t in [k, x, v] + consts + bounds], position_count=rows))
    out = head.getOutput()
    ctx.synchronize()
    head.close()
    return out


def functions(p, frame):
    family, kind = frame.split("_")
    at = KINDS.index(kind)
    if family == "rows":
        f = p.WindowFrame(p.FRAME_TYPE_ROWS, p.BOUND_PRECEDING, p.BOUND_FOLLOWING, 3 + at, 3 + at)
    else:
        f = p.WindowRangeFrame(p.BOUND_PRECEDING, p.BOUND_FOLLOWING, 6 + 2 * at, 7 + 2 * at, 1, 1)
    return [p.WindowFunction(p.WINDOW_AGGREGATE, (2,), f, p.SUM_BIGINT), p.WindowFunction(p.WINDOW_AGGREGATE, (2,), f, p.MIN_BIGINT)]


def run(p, ctx, page, frame, keep=False):
    op = p.WindowOperatorFactory(ctx, 1, [p.BIGINT] * 12, [0, 1, 2], functions(p, frame), [0], [1], [p.ASC_NULLS_LAST], 10_000).createOperator()
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


def verify(p, ctx, dev, groups, frames):
    """2^16 rows: every frame's sum and min against numpy over the operator's own output order"""
    rows = 1 << 16
    page = owned_page(p, ctx, dev, rows, groups)
    d = distances(rows, groups)
    widths = {}
    for frame in frames:
        family, kind = frame.split("_")
        out = run(p, ctx, page, frame, True)[1]
        k, x, v = out.getBlock(0).values, out.getBlock(1).values, out.getBlock(2).values
        n = len(k)
        first = np.maximum.accumulate(np.where(np.r_[True, k[1:] != k[:-1]], np.arange(n), 0))
        last = n - 1 - np.maximum.accumulate(np.where(np.r_[True, k[::-1][1:] != k[::-1][:-1]], np.arange(n), 0))[::-1]
        if family == "rows":
            lo, hi = np.maximum(np.arange(n) - WIDTHS[kind], first), np.minimum(np.arange(n) + WIDTHS[kind], last)
        else:
            combined = k * (1 << 23) + x   # a partition's values stay 2^22 and more away from the next one's
            lo, hi = np.searchsorted(combined, combined - d[kind], "left"), np.searchsorted(combined, combined + d[kind], "right") - 1
            assert (lo >= first).all() and (hi <= last).all()
        prefix = np.r_[0, np.cumsum(v)]
        assert np.array_equal(out.getBlock(3).values, prefix[hi + 1] - prefix[lo]), frame
        sample = np.random.default_rng(1).integers(0, n, 2000)
        assert all(out.getBlock(4).values[i] == v[lo[i]:hi[i] + 1].min() for i in sample), frame
        widths[frame] = float((hi - lo + 1).mean())
    page.release()
    return widths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", default=",".join(FRAMES))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p = importlib.import_module("presto-1_amd")
    frames = args.frames.split(",")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    widths = verify(p, ctx, dev, args.groups, frames)
    print(json.dumps({"verified_rows": 1 << 16, "mean_frame_rows": {f: round(w, 1) for f, w in widths.items()}}), flush=True)
    rows = 1 << args.rows
    page = owned_page(p, ctx, dev, rows, args.groups)
    for frame in frames:
        run(p, ctx, page, frame)   # warm-up
    walls = {f: [] for f in frames}
    scopes = {f: {s: [] for s in SCOPES} for f in frames}
    ctx.profile_enable(True)
    for _ in range(args.runs):
        for frame in frames:
            ctx.profile_reset()
            walls[frame].append(run(p, ctx, page, frame)[0])
            prof = ctx.profile()
            for s in SCOPES:
                scopes[frame][s].append(prof.get(s, {}).get("total_ms", 0.0))
    ctx.profile_enable(False)
    three = lambda xs: {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    for frame in frames:
        line = {"rows": rows, "groups": args.groups, "frame": frame, "distance": distances(rows, args.groups)[frame.split("_")[1]] if frame.startswith("range") else None,
                "runs": args.runs, "wall_ms": three([w * 1e3 for w in walls[frame]]), "bound_pass_ms": three(scopes[frame]["window_frames"]),
                "scopes_ms": {s: three(v) for s, v in scopes[frame].items() if max(v) > 0}}
        line["all_window_scopes_ms"] = three([sum(scopes[frame][s][i] for s in SCOPES) for i in range(args.runs)])
        print(json.dumps(line), flush=True)
    page.release()
    ctx.close()


if __name__ == "__main__":
    main()

"""WindowOperator study, frames with offsets: sum(v) and min(v) OVER (PARTITION BY k ORDER BY x <frame>) over one device-resident, library-owned page
(BIGINT k drawn uniformly from G values, BIGINT x from 2^20 values, BIGINT v, and two constant BIGINT offset channels), at 2^24 rows and G = 1000, under
  to_current   ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW through tgpu_window_factory_create (FRAME_ROWS_TO_CURRENT): the yardstick; with --root it
               runs on another checkout of the library, e.g. the parent commit
  narrow       ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING
  wide         ROWS BETWEEN 2000 PRECEDING AND 2000 FOLLOWING
The frames alternate inside every repetition.  Per frame: the wall time of addInput + finish() + getOutput() and the HIP-event time of the profile scopes
window_scan, window_frames, window_extremes and window_evaluate, as median / min / max over --runs profiled repetitions.  A wide frame that costs more
than a narrow one beyond the spread means something walks the frame.  Before anything is timed, at 2^16 rows, the three results are compared with numpy.
Prints one JSON line per frame.

  python tools/exp_window_frames.py [--rows 24] [--groups 1000] [--runs 7] [--frames to_current,narrow,wide] [--root DIR]
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

NARROW, WIDE = 3, 2000
SCOPES = ("window_heads", "window_scan", "window_frames", "window_extremes", "window_evaluate")


def owned_page(p, ctx, dev, rows, groups):
    """one library-owned device page (k, x, v, 3, 2000): an identity projection copies the borrowed blocks once"""
    g = torch.Generator(device=dev).manual_seed(13)
    head = p.FilterAndProjectOperatorFactory(ctx, 90, [p.BIGINT] * 5, None, [p.field(c, p.BIGINT) for c in range(5)]).createOperator()
    k = torch.randint(0, groups, (rows,), dtype=torch.int64, device=dev, generator=g)
    x = torch.randint(0, 1 << 20, (rows,), dtype=torch.int64, device=dev, generator=g)
    v = torch.randint(-1000, 1000, (rows,), dtype=torch.int64, device=dev, generator=g)
    consts = [torch.full((rows,), c, dtype=torch.int64, device=dev) for c in (NARROW, WIDE)]
    torch.cuda.synchronize()
    head.addInput(p.Page(*[p.DeviceBlock(p.BIGINT, rows, t) for t in [k, x, v] + consts], position_count=rows))
    out = head.getOutput()
    ctx.synchronize()
    head.close()
    return out


def functions(p, frame):
    if frame == "to_current":
        f = p.FRAME_ROWS_TO_CURRENT
    else:
        channel = 3 if frame == "narrow" else 4
        f = p.WindowFrame(p.FRAME_TYPE_ROWS, p.BOUND_PRECEDING, p.BOUND_FOLLOWING, channel, channel)
    return [p.WindowFunction(p.WINDOW_AGGREGATE, (2,), f, p.SUM_BIGINT), p.WindowFunction(p.WINDOW_AGGREGATE, (2,), f, p.MIN_BIGINT)]


def run(p, ctx, page, frame, keep=False):
    op = p.WindowOperatorFactory(ctx, 1, [p.BIGINT] * 5, [0, 1, 2], functions(p, frame), [0], [1], [p.ASC_NULLS_LAST], 10_000).createOperator()
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
    page = owned_page(p, ctx, dev, 1 << 16, groups)
    for frame in frames:
        out = run(p, ctx, page, frame, True)[1]
        k, v = out.getBlock(0).values, out.getBlock(2).values
        n = len(k)
        first = np.maximum.accumulate(np.where(np.r_[True, k[1:] != k[:-1]], np.arange(n), 0))
        last = n - 1 - np.maximum.accumulate(np.where(np.r_[True, k[::-1][1:] != k[::-1][:-1]], np.arange(n), 0))[::-1]
        width = {"to_current": None, "narrow": NARROW, "wide": WIDE}[frame]
        lo = first if width is None else np.maximum(np.arange(n) - width, first)
        hi = np.arange(n) if width is None else np.minimum(np.arange(n) + width, last)
        prefix = np.r_[0, np.cumsum(v)]
        assert np.array_equal(out.getBlock(3).values, prefix[hi + 1] - prefix[lo]), frame
        sample = np.random.default_rng(1).integers(0, n, 2000)
        assert all(out.getBlock(4).values[i] == v[lo[i]:hi[i] + 1].min() for i in sample), frame
    page.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", default="to_current,narrow,wide")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose presto-1_amd package runs")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    p = importlib.import_module("presto-1_amd")
    frames = args.frames.split(",")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    verify(p, ctx, dev, args.groups, frames)
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
        line = {"root": args.root, "rows": rows, "groups": args.groups, "frame": frame, "runs": args.runs, "wall_ms": three([w * 1e3 for w in walls[frame]]),
                "scopes_ms": {s: three(v) for s, v in scopes[frame].items() if max(v) > 0}}
        line["scan_plus_evaluate_ms"] = three([a + b for a, b in zip(scopes[frame]["window_scan"], scopes[frame]["window_evaluate"])])
        line["all_window_scopes_ms"] = three([sum(scopes[frame][s][i] for s in SCOPES) for i in range(args.runs)])
        print(json.dumps(line), flush=True)
    page.release()
    ctx.close()


if __name__ == "__main__":
    main()

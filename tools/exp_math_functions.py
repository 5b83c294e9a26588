"""Math-function study: which generated kernels stay memory-bound?

2^24 rows: two DOUBLE columns (a price-like x in [1, 100000), a discount-like y in [0, 0.1]) resident on the device.  Each case is one
FilterAndProjectOperator whose output stays on the device; times are per-kernel HIP-event times (tgpu_profile_*) of the kernel that evaluates
the expression -- the minimum over the repeats after the warm-up runs.

    baseline   x * (1 - y)                     16 B in, 8 B out per row: a program the library always had (TPC-H's discounted price)
    round(x * (1 - y), 2)   abs(x - y)         the same bytes
    floor(x)   ln(x)   power(x, 2.0)   power(x, 1.5)     8 B in, 8 B out (x ^ 2 is one product; 1.5 takes the library's pow)

The baseline runs first and last.  Each case is reported as the ratio of its minimum to the baseline's minimum, beside the ratio of the bytes
it moves: a case keeps the memory-bound pace when the two agree within the baseline's run-to-run spread.  No ratio is a pass / fail condition.

    python tools/exp_math_functions.py [--rows 16777216] [--repeats 7] [--warmup 3]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases(p):
    """-> (input types, [(name, projections, bytes per row)])"""
    f, D = p.field, p.DOUBLE
    x, y, one = f(0, D), f(1, D), p.constant(1.0, D)
    return [D, D], [
        ("baseline x * (1 - y)", [x * (one - y)], 24),
        ("round(x * (1 - y), 2)", [p.round_(x * (one - y), 2)], 24),
        ("abs(x - y)", [p.abs_(x - y)], 24),
        ("floor(x)", [p.floor(x)], 16),
        ("ln(x)", [p.ln(x)], 16),
        ("power(x, 2.0)", [p.power(x, 2.0)], 16),
        ("power(x, 1.5)", [p.power(x, 1.5)], 16),
        ("baseline x * (1 - y) again", [x * (one - y)], 24),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    import torch

    torch.cuda.init()
    rng = np.random.default_rng(7)
    n = args.rows
    host = [np.round(rng.uniform(1.0, 100000.0, n), 2), np.round(rng.uniform(0.0, 0.1, n), 2)]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    torch.cuda.synchronize()
    types, items = cases(p)
    page = p.Page(*[p.DeviceBlock(t, n, a.data_ptr()) for t, a in zip(types, dev)])
    ctx = p.Context(0)

    def run(fac):
        for o in p.to_pages(fac.createOperator(), [page], to_host=False):
            o.release()

    results = []
    for name, projs, bytes_per_row in items:
        fac = p.FilterAndProjectOperatorFactory(ctx, 0, types, None, projs)
        for _ in range(args.warmup):
            run(fac)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            run(fac)
        prof = ctx.profile()
        ctx.profile_enable(False)
        prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
        kernel = max(prof, key=lambda name_: prof[name_]["total_ms"])
        k1 = prof[kernel]
        results.append({"case": name, "kernel": kernel, "rows": n, "ms_min": round(k1["min_ms"], 4), "ms_max": round(k1["max_ms"], 4), "ms_mean": round(k1["total_ms"] / k1["count"], 4),
                        "bytes_per_row": bytes_per_row, "GB_per_s": round(bytes_per_row * n / (k1["min_ms"] * 1e-3) / 1e9, 1)})
        print(json.dumps(results[-1]), flush=True)
        fac.close()
    ctx.close()
    base = [r for r in results if r["case"].startswith("baseline")]
    base_min, spread = min(r["ms_min"] for r in base), max(r["ms_max"] for r in base) - min(r["ms_min"] for r in base)
    print(json.dumps({"baseline_ms_min": base_min, "baseline_spread_ms": round(spread, 4), "baseline_spread_ratio": round(spread / base_min, 3)}))
    for r in results:
        if not r["case"].startswith("baseline"):
            print(json.dumps({"case": r["case"], "ratio_to_baseline": round(r["ms_min"] / base_min, 3), "bytes_ratio": round(r["bytes_per_row"] / 24, 3)}))


if __name__ == "__main__":
    main()

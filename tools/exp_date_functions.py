"""DATE-function study: do the generated kernels of year / week / date_trunc / date_add / date_diff stay memory-bound?

2^24 rows: a DATE column spread over 1992-1998, a second DATE column, a BIGINT amount and an INTEGER column, all resident on the device.
Each case is one FilterAndProjectOperator whose output stays on the device; times are per-kernel HIP-event times (tgpu_profile_*) of the
kernel that evaluates the expression -- the minimum over the repeats after the warm-up runs.

    baseline   CAST(i AS BIGINT)               4 B in, 8 B out per row: the bytes of an extraction, a program the library always had
    year(d)  week(d)  date_trunc('month', d)  date_add('month', k, d)  date_diff('month', d, e)
    filter year(d) = 1995   beside   filter d BETWEEN DATE '1995-01-01' AND DATE '1995-12-31'

The baseline runs first and last; its run-to-run spread (max - min over all its runs) is the margin: a case "keeps the baseline's pace" when
its minimum is within the baseline's minimum plus that spread -- for cases that move more bytes, after scaling the baseline by the bytes.
The last line is the device-to-device copy bandwidth of tools/exp_hbm_calibration.py, run as a child process.

    python tools/exp_date_functions.py [--rows 16777216] [--repeats 5] [--warmup 2] [--no-calibration]
    python tools/exp_date_functions.py --rehearse DIR     # no GPU: writes each program's source to DIR, compiles it for gfx950 with hipcc and
                                                          # prints registers, scratch and occupancy (-Rpass-analysis=kernel-resource-usage)
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DAY_1992, DAY_1995, DAY_1996, DAY_1999 = 8035, 9131, 9496, 10592     # January 1 of those years


def cases(p):
    """-> (input types, [(name, filter, projections, bytes per row)])"""
    f, D, B, I = p.field, p.DATE, p.BIGINT, p.INTEGER
    d, e, k, i, row = f(0, D), f(1, D), f(2, B), f(3, I), f(4, B)
    return [D, D, B, I, B], [
        ("baseline CAST(i AS BIGINT)", None, [p.cast(i, B)], 12),
        ("year(d)", None, [p.year(d)], 12),
        ("week(d)", None, [p.week(d)], 12),
        ("date_trunc('month', d)", None, [p.date_trunc("month", d)], 8),
        ("date_add('month', k, d)", None, [p.date_add("month", k, d)], 16),
        ("date_diff('month', d, e)", None, [p.date_diff("month", d, e)], 16),
        ("filter year(d) = 1995", p.year(d).eq(1995), [row], 4),
        ("filter d BETWEEN 1995-01-01 AND 1995-12-31", p.between(d, DAY_1995, DAY_1996 - 1), [row], 4),
        ("baseline CAST(i AS BIGINT) again", None, [p.cast(i, B)], 12),
    ]


def rehearse(p, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    types, items = cases(p)
    for n, (name, filt, projs, _) in enumerate(items[:-1]):
        path = os.path.join(out_dir, "date_case_%d.hip" % n)
        with open(path, "w") as fh:
            fh.write("#include <hip/hip_runtime.h>\n" + p.page_processor_source(types, filt, projs))   # (hiprtc has the runtime header built in)
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", path, "-o", path[:-4] + ".co",
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        if r.returncode != 0:
            print(name, "does not compile:", r.stderr[-2000:])
            continue
        kernel = None
        for line in r.stderr.splitlines():
            m = re.search(r"remark: (?:Function Name: (\w+)|\s*(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+))", line)
            if m and m.group(1):
                kernel = {"case": name, "kernel": m.group(1)}
            elif m and kernel is not None:
                kernel[m.group(2).split(" ")[0]] = int(m.group(3))
                if m.group(2).startswith("Occupancy"):
                    print(json.dumps(kernel), flush=True)
                    kernel = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--rehearse", metavar="DIR")
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    if args.rehearse:
        return rehearse(p, args.rehearse)
    import torch

    torch.cuda.init()
    D, B, I = p.DATE, p.BIGINT, p.INTEGER
    rng = np.random.default_rng(7)
    n = args.rows
    host = [rng.integers(DAY_1992, DAY_1999, n).astype(np.int32), rng.integers(DAY_1992, DAY_1999, n).astype(np.int32), rng.integers(-60, 61, n).astype(np.int64),
            rng.integers(-2**31, 2**31, n).astype(np.int32), np.arange(n, dtype=np.int64)]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    torch.cuda.synchronize()
    types, items = cases(p)
    page = p.Page(*[p.DeviceBlock(t, n, a.data_ptr()) for t, a in zip(types, dev)])
    ctx = p.Context(0)

    def run(fac):
        rows = 0
        for o in p.to_pages(fac.createOperator(), [page], to_host=False):
            rows += o.position_count
            o.release()
        return rows

    results = []
    for name, filt, projs, bytes_per_row in items:
        fac = p.FilterAndProjectOperatorFactory(ctx, 0, types, filt, projs)
        for _ in range(args.warmup):
            selected = run(fac)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            run(fac)
        prof = ctx.profile()
        ctx.profile_enable(False)
        prof = json.loads(prof) if isinstance(prof, (str, bytes)) else prof
        kernel = "filter_count" if filt is not None and "filter_count" in prof else max(prof, key=lambda name_: prof[name_]["total_ms"])
        k1 = prof[kernel]
        results.append({"case": name, "kernel": kernel, "rows": n, "selected": selected, "ms_min": round(k1["min_ms"], 4), "ms_max": round(k1["max_ms"], 4),
                        "ms_mean": round(k1["total_ms"] / k1["count"], 4), "bytes_per_row": bytes_per_row,
                        "GB_per_s": round(bytes_per_row * n / (k1["min_ms"] * 1e-3) / 1e9, 1),
                        "all_kernels_ms_per_page": round(sum(v["total_ms"] for v in prof.values()) / args.repeats, 4)})
        print(json.dumps(results[-1]), flush=True)
        fac.close()
    ctx.close()
    base = [r for r in results if r["case"].startswith("baseline")]
    base_min, spread = min(r["ms_min"] for r in base), max(r["ms_max"] for r in base) - min(r["ms_min"] for r in base)
    print(json.dumps({"baseline_ms_min": base_min, "baseline_spread_ms": round(spread, 4), "margin": "baseline min x bytes / 12 + spread"}))
    for r in results:
        if not r["case"].startswith("baseline") and not r["case"].startswith("filter"):
            limit = base_min * max(1.0, r["bytes_per_row"] / 12) + spread
            print(json.dumps({"case": r["case"], "ms_min": r["ms_min"], "limit_ms": round(limit, 4), "within_margin": r["ms_min"] <= limit}))
    a, b = [r for r in results if r["case"].startswith("filter")]
    print(json.dumps({"filter year(d) = 1995 over the range filter": round(a["ms_min"] / b["ms_min"], 3), "same_rows": a["selected"] == b["selected"]}))
    if not args.no_calibration:
        try:   # a fresh child process: the calibration brings the device up itself
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "exp_hbm_calibration.py")], capture_output=True, text=True, timeout=300)
            lines = [l for l in out.stdout.splitlines() if "copy" in l]
            print(lines[-1] if lines else "device-to-device copy: not available (" + (out.stderr.strip().splitlines() or ["no output"])[-1] + ")")
        except subprocess.TimeoutExpired:
            print("device-to-device copy: not available (timed out)")


if __name__ == "__main__":
    main()

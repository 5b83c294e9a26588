"""Computed VARCHAR projections: what the variable-width write pass (fp_vwrite, profile scope `project_varchar_write`) gets out of the GPU.

Two shapes, each a VARCHAR column x of random lower-case bytes plus a BIGINT column k (the row number):

    phone    2^24 rows of 13 to 17 bytes (about 15: the c_phone shape)
    comment  2^22 rows of 40 to 200 bytes

Timed, each as a projection of a FilterAndProjectOperator without a filter, per kernel with the HIP-event profile, after warm-up runs:

    substr(x, 1)                              the whole value through the new path
    substr(x, 1, 2)
    concat('Customer#', CAST(k AS varchar))

and next to them the only other VARCHAR writer on the same bytes: the identity projection of x under a filter that drops just the last
row (scope `gather`: k::gather_column's length kernel, scan, host read of the total and byte-copy kernel together; the kernel-exact split
needs a kernel trace, e.g. `rocprofv3 --kernel-trace --stats -- python tools/exp_varchar_project.py --no-sweep`).

Per kernel: milliseconds (minimum over the repeats), bytes per second on the algorithmic bytes (source bytes and offsets read, output
offsets read, pool bytes written) and the fraction of 8 TB/s.  Then the sweep of TGPU_VW_COOP_MIN (read when the kernel is generated) on
substr(x, 1) of both shapes.

    python tools/exp_varchar_project.py [--repeats 5] [--warmup 2] [--scale 1] [--no-sweep]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12   # bytes per second


def make_column(rng, rows, lo, hi):
    lens = rng.integers(lo, hi + 1, rows).astype(np.int64)
    offs = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    assert offs[-1] < 2**31
    pool = rng.integers(97, 123, int(offs[-1]), dtype=np.uint8)
    return pool, offs.astype(np.int32)


def timed(p, ctx, types, filt, projs, page, warmup, repeats):
    fac = p.FilterAndProjectOperatorFactory(ctx, 0, types, filt, projs)

    def once():
        rows = 0
        for o in p.to_pages(fac.createOperator(), [page], to_host=False):
            rows += o.position_count
            o.release()
        return rows
    for _ in range(warmup):
        rows = once()
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(repeats):
        once()
    prof = ctx.profile()
    ctx.profile_enable(False)
    return rows, (json.loads(prof) if isinstance(prof, (str, bytes)) else prof)


def report(shape, name, kernel, stat, nbytes, extra=None):
    ms = stat["min_ms"]
    rate = nbytes / (ms * 1e-3)
    line = {"shape": shape, "projection": name, "kernel": kernel, "ms_min": round(ms, 4), "ms_mean": round(stat["total_ms"] / stat["count"], 4), "bytes": int(nbytes),
            "GB_per_s": round(rate / 1e9, 1), "fraction_of_8TBps": round(rate / PEAK, 4)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the row counts")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    os.environ.pop("TGPU_VW_COOP_MIN", None)
    p = importlib.import_module("presto-1_amd")
    V, B, f = p.VARCHAR, p.BIGINT, p.field
    rng = np.random.default_rng(7)
    ctx = p.Context(0)
    T = [V, B]
    x, k = f(0, V), f(1, B)
    shapes = [("phone", int((1 << 24) * args.scale), 13, 17), ("comment", int((1 << 22) * args.scale), 40, 200)]
    pages = {}
    for shape, n, lo, hi in shapes:
        pool, offs = make_column(rng, n, lo, hi)
        page = p.Page(p.Block(V, pool, offsets=offs), p.Block(B, np.arange(n, dtype=np.int64)))
        src = int(offs[-1])
        pages[shape] = (page, n, src)
        digits = sum(len(str(i)) * (min(n, 10 ** len(str(i))) - i) for i in [0] + [10 ** e for e in range(1, 9)] if i < n)   # bytes of str(0 .. n - 1)
        cases = [("substr(x, 1)", p.substr(x, 1), 4 * (n + 1) + src, src), ("substr(x, 1, 2)", p.substr(x, 1, 2), 4 * (n + 1) + 2 * n, 2 * n),
                 ("concat('Customer#', CAST(k AS varchar))", p.concat("Customer#", p.cast(k, V)), 8 * n, 9 * n + digits)]
        write_ms = None
        for name, expr, read, written in cases:
            rows, prof = timed(p, ctx, T, None, [expr], page, args.warmup, args.repeats)
            assert rows == n
            report(shape, name, "project_emit", prof["project_emit"], read + 5 * n)                      # the source, then a length and a null byte per row
            ms = report(shape, name, "project_varchar_write", prof["project_varchar_write"], read + 4 * n + written)
            write_ms = ms if write_ms is None else write_ms
        rows, prof = timed(p, ctx, T, k < n - 1, [x], page, args.warmup, args.repeats)
        assert rows == n - 1
        gather_ms = report(shape, "x under a filter dropping the last row", "gather", prof["gather"], 4 * n + 2 * 4 * (n + 1) + 4 * n + 2 * src,
                           {"note": "the whole scope: length kernel, scan, host read, byte-copy kernel"})
        print(json.dumps({"shape": shape, "project_varchar_write_ms": round(write_ms, 4), "gather_scope_ms": round(gather_ms, 4),
                          "write_over_gather": round(write_ms / gather_ms, 3)}), flush=True)
    if not args.no_sweep:
        for shape, n, lo, hi in shapes:
            page, n, src = pages[shape]
            for value in ("0", "16", "32", "64", "128", "256", "512", str(2**40)):
                os.environ["TGPU_VW_COOP_MIN"] = value
                rows, prof = timed(p, ctx, T, None, [p.substr(x, 1)], page, args.warmup, args.repeats)
                report(shape, "substr(x, 1)", "project_varchar_write", prof["project_varchar_write"], 4 * (n + 1) + 4 * n + 2 * src, {"TGPU_VW_COOP_MIN": int(value)})
        os.environ.pop("TGPU_VW_COOP_MIN", None)
    ctx.close()


if __name__ == "__main__":
    main()

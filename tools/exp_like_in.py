"""LIKE / IN study: what the generated filter kernels get out of the GPU on comment-like strings.

2^24 rows of strings of 19 to 78 bytes cut out of a text of random words (the shape of TPC-H comment columns), plus a BIGINT key column.
Timed, each as the filter of a FilterAndProjectOperator that projects the BIGINT row number:

    c LIKE '%special%requests%'   c LIKE 'PROMO%'   c LIKE '%BRASS'   c IN (8 strings)   k IN (8 bigints)   k IN (1,000 bigints)

and next to them `c = 'constant'` on the same column (the floor: it reads the offsets and, for strings of the constant's length, their
first bytes).  Times are per-kernel HIP-event times of pass 1 (`filter_count`: the kernel that evaluates the predicate) -- the minimum
and the mean over the repeats after the warm-up runs, so neither the upload of the page nor the compaction is in them.  Bytes moved =
the offsets plus every value byte (strings), 8 bytes per row (keys).  The last line is the device-to-device copy bandwidth of
tools/exp_hbm_calibration.py, run as a child process.

    python tools/exp_like_in.py [--rows 16777216] [--repeats 5] [--warmup 2] [--no-calibration]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ("special requests packages deposits accounts foxes ideas theodolites pinto beans instructions dependencies excuses platelets asymptotes "
         "courts dolphins multipliers sauternes warthogs frets dinos attainments somas Tiresias patterns forges braids hockey players frays warhorses "
         "dugouts notornis epitaphs pearls tithes waters orbits gifts sheaves depths sentiments decoys realms pains grouches escapades PROMO BRASS "
         "furiously slyly carefully blithely quickly fluffily final ironic regular express bold pending unusual even silent").split()


def make_strings(rng, rows):
    """(pool, offsets): string i = a random cut of 19..78 bytes out of a 16 MiB text of random words; built a million rows at a time"""
    text = np.frombuffer(" ".join(rng.choice(WORDS, 3_000_000)).encode()[:1 << 24], dtype=np.uint8)
    lens = rng.integers(19, 79, rows).astype(np.int64)
    offs = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    assert offs[-1] < 2**31
    pool = np.empty(int(offs[-1]), dtype=np.uint8)
    starts = rng.integers(0, len(text) - 80, rows)
    step = 1 << 20
    for a in range(0, rows, step):
        b = min(rows, a + step)
        idx = np.repeat(starts[a:b] - offs[a:b], lens[a:b]) + np.arange(offs[a], offs[b])
        pool[offs[a]:offs[b]] = text[idx]
    return pool, offs.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    V, B, f = p.VARCHAR, p.BIGINT, p.field
    rng = np.random.default_rng(7)
    n = args.rows
    pool, offs = make_strings(rng, n)
    keys = rng.integers(0, 1_000_000, n).astype(np.int64)
    page = p.Page(p.Block(V, pool, offsets=offs), p.Block(B, keys), p.Block(B, np.arange(n, dtype=np.int64)))
    string_bytes = 4 * (n + 1) + int(offs[-1])
    first = bytes(pool[offs[5]:offs[6]]).decode()
    c, k = f(0, V), f(1, B)
    eight = [bytes(pool[offs[i]:offs[i + 1]]).decode() for i in range(10, 18)]
    cases = [
        ("c = 'constant' (floor)", c.eq(first), string_bytes),
        ("c LIKE '%special%requests%'", p.like(c, "%special%requests%"), string_bytes),
        ("c LIKE 'PROMO%'", p.like(c, "PROMO%"), string_bytes),
        ("c LIKE '%BRASS'", p.like(c, "%BRASS"), string_bytes),
        ("c IN (8 strings)", p.in_(c, eight), string_bytes),
        ("k IN (8 bigints)", p.in_(k, [int(x) for x in keys[:8]]), 8 * n),
        ("k IN (1,000 bigints)", p.in_(k, [int(x) for x in np.unique(keys[:1200])[:1000]]), 8 * n),
    ]
    ctx = p.Context(0)
    T = [V, B, B]
    for name, filt, nbytes in cases:
        fac = p.FilterAndProjectOperatorFactory(ctx, 0, T, filt, [f(2, B)])
        selected = 0
        for _ in range(args.warmup):
            selected = sum(o.position_count for o in p.to_pages(fac.createOperator(), [page]))
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            p.to_pages(fac.createOperator(), [page])
        prof = ctx.profile()
        ctx.profile_enable(False)
        k1 = prof["filter_count"]
        ms_min, ms_mean = k1["min_ms"], k1["total_ms"] / k1["count"]
        print(json.dumps({"predicate": name, "rows": n, "selected": selected, "ms_per_page_min": round(ms_min, 4), "ms_per_page_mean": round(ms_mean, 4),
                          "rows_per_s": round(n / (ms_min * 1e-3)), "GB_per_s": round(nbytes / (ms_min * 1e-3) / 1e9, 1), "bytes": nbytes,
                          "all_kernels_ms_per_page": round(sum(v["total_ms"] for v in prof.values()) / args.repeats, 4)}), flush=True)
    ctx.close()
    if not args.no_calibration:
        try:   # a fresh child process: the calibration needs torch to see the device
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "exp_hbm_calibration.py")], capture_output=True, text=True, timeout=300)
            lines = [l for l in out.stdout.splitlines() if "copy" in l]
            print(lines[-1] if lines else "device-to-device copy: not available (" + (out.stderr.strip().splitlines() or ["no output"])[-1] + ")")
        except subprocess.TimeoutExpired:
            print("device-to-device copy: not available (timed out)")


if __name__ == "__main__":
    main()

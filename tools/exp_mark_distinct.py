"""MarkDistinctOperator study: the operator over device-resident, library-owned pages of 2^22 rows, two shapes:
  bigint  one BIGINT key, 80 M rows, 10 M distinct values drawn uniformly;
  q16     TPC-H Q16's count(DISTINCT ps_suppkey) GROUP BY p_brand, p_type, p_size: keys (VARCHAR, VARCHAR, INTEGER, INTEGER), about 19 k
          distinct (brand, type, size) triples times 1 M values of the last key, 80 M rows.
Per shape: the operator's wall time per row (a fresh operator per run, one warm-up run, then --runs timed runs: median, min, max), the
per-scope HIP-event times of one more run split into the marking step (distinct_first_row, distinct_mark) and everything else
(= get_group_ids), and the marking kernels' bytes per second (4 B id read + 1 B mark written per row) against 8 TB/s peak and the
6.1 TB/s measured streaming read of DESIGN.md section 4.  Prints one JSON line per shape.

  python tools/exp_mark_distinct.py [--rows 80000000] [--page-rows 4194304] [--runs 5] [--shapes bigint,q16]
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

MARK_SCOPES = ("distinct_first_row", "distinct_mark")
BRANDS = ["Brand#%d%d" % (a, b) for a in range(1, 6) for b in range(1, 6)]
TYPES = ["%s %s %s" % (a, b, c) for a in ("STANDARD", "SMALL", "MEDIUM", "LARGE", "ECONOMY", "PROMO")
         for b in ("ANODIZED", "BURNISHED", "PLATED", "POLISHED", "BRUSHED") for c in ("TIN", "NICKEL", "BRASS", "STEEL", "COPPER")]
TRIPLES = 19_000


def varchar_blocks(p, dev, strings, picks):
    """a VARCHAR DeviceBlock with strings[picks[i]] in row i: (block, tensors to keep alive)"""
    width = max(len(s) for s in strings)
    table = torch.tensor([list(s.encode().ljust(width, b" ")) for s in strings], dtype=torch.uint8, device=dev)
    lens = torch.tensor([len(s) for s in strings], dtype=torch.int32, device=dev)[picks]
    offsets = torch.zeros(picks.numel() + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    keep = torch.arange(width, device=dev)[None, :] < lens[:, None]
    pool = table[picks][keep].contiguous()
    return p.DeviceBlock(p.VARCHAR, picks.numel(), pool, None, offsets), (pool, offsets)


def make_pages(p, dev, shape, rows, page_rows):
    """(source types, mark channels, borrowed device pages, tensors to keep alive, distinct keys of the stream)"""
    g = torch.Generator(device=dev).manual_seed(7)
    pages, keep, ident = [], [], []
    for a in range(0, rows, page_rows):
        n = min(rows, a + page_rows) - a
        if shape == "bigint":
            k = torch.randint(0, 10_000_000, (n,), dtype=torch.int64, device=dev, generator=g)
            keep.append(k)
            ident.append(k)
            pages.append(p.Page(p.DeviceBlock(p.BIGINT, n, k), position_count=n))
            continue
        triple = torch.randint(0, TRIPLES, (n,), dtype=torch.int64, device=dev, generator=g)
        brand, kb = varchar_blocks(p, dev, BRANDS, triple % 25)
        ptype, kt = varchar_blocks(p, dev, TYPES, (triple // 25) % 150)
        size = (triple // 3750).to(torch.int32) * 9 + 3
        supp = torch.randint(1, 1_000_001, (n,), dtype=torch.int32, device=dev, generator=g)
        keep.extend([kb, kt, size, supp])
        ident.append(triple * (1 << 20) + supp)
        pages.append(p.Page(brand, ptype, p.DeviceBlock(p.INTEGER, n, size), p.DeviceBlock(p.INTEGER, n, supp), position_count=n))
    distinct = int(torch.unique(torch.cat(ident)).numel())
    if shape == "bigint":
        return [p.BIGINT], [0], pages, keep, distinct
    return [p.VARCHAR, p.VARCHAR, p.INTEGER, p.INTEGER], [0, 1, 2, 3], pages, keep, distinct


def owned(p, ctx, types, pages):
    """the pages as library-owned OutputPages (an identity projection copies the borrowed blocks once): the operator then forwards them
    without copying, as inside a device-resident operator chain"""
    head = p.FilterAndProjectOperatorFactory(ctx, 90, types, None, [p.field(i, t) for i, t in enumerate(types)]).createOperator()
    out = []
    for pg in pages:
        head.addInput(pg)
        out.append(head.getOutput())
    head.close()
    return out


def one_run(p, ctx, types, channels, pages):
    op = p.MarkDistinctOperatorFactory(ctx, 1, types, channels).createOperator()
    ctx.synchronize()
    t0 = time.perf_counter()
    for pg in pages:
        op.addInput(pg)
        op.getOutput().release()
    ctx.synchronize()
    wall = time.perf_counter() - t0
    op.close()
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80_000_000)
    ap.add_argument("--page-rows", type=int, default=1 << 22)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="bigint,q16")
    args = ap.parse_args()
    p = importlib.import_module("presto-1_amd")
    dev = torch.device("cuda:0")
    ctx = p.Context(0)
    for shape in args.shapes.split(","):
        types, channels, borrowed, keep, distinct = make_pages(p, dev, shape, args.rows, args.page_rows)
        torch.cuda.synchronize()
        pages = owned(p, ctx, types, borrowed)
        ctx.synchronize()
        del borrowed, keep
        one_run(p, ctx, types, channels, pages)   # warm-up: allocator, code objects
        walls = [one_run(p, ctx, types, channels, pages) for _ in range(args.runs)]
        ctx.profile_enable(True)
        ctx.profile_reset()
        one_run(p, ctx, types, channels, pages)
        prof = ctx.profile()
        ctx.profile_enable(False)
        scopes = {k: v for k, v in prof.items() if not k.startswith("__")}
        mark_ms = sum(v["total_ms"] for k, v in scopes.items() if k in MARK_SCOPES)
        other_ms = sum(v["total_ms"] for k, v in scopes.items() if k not in MARK_SCOPES)
        med = statistics.median(walls)
        gbs = 5.0 * args.rows / (mark_ms * 1e-3) / 1e9 if mark_ms > 0 else 0.0
        print(json.dumps({
            "shape": shape, "rows": args.rows, "pages": len(pages), "page_rows": args.page_rows, "distinct_keys": distinct,
            "wall_ms": {"median": round(med * 1e3, 2), "min": round(min(walls) * 1e3, 2), "max": round(max(walls) * 1e3, 2), "runs": args.runs},
            "ns_per_row": round(med / args.rows * 1e9, 4),
            "marking_ms": round(mark_ms, 3), "group_ids_ms": round(other_ms, 3),
            "marking_share_of_kernel_time": round(mark_ms / (mark_ms + other_ms), 4) if mark_ms + other_ms > 0 else None,
            "readbacks": prof["__readbacks"]["count"],
            "scopes_ms": {k: round(v["total_ms"], 3) for k, v in sorted(scopes.items())},
            "marking_byte_roofline": {"bytes_per_row": 5, "achieved_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / 8000, 3), "frac_of_6.1TBps": round(gbs / 6100, 3)},
        }), flush=True)
        for o in pages:
            o.release()
    ctx.close()


if __name__ == "__main__":
    main()

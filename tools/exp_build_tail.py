"""Kernel study: HashBuilder.finish on Q3's two build sides at SF100 -- 3.0 M customer keys (one in five of 15 M consecutive keys) and 14.6 M
order keys (one in ten of 150 M TPCH order keys, range 600 M), both strictly ascending without a null vector.  Prints the range pass
(join_build_range) under TGPU_KEY_RANGE_LOADS x TGPU_KEY_RANGE_BLOCKS, then the build pass and the rank passes with the rank from the run
heads and with TGPU_DIRECT_RANK_FROM_HEADS=0 (popcount + scan).  Event times per scope, averaged over the repetitions."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("presto-1_amd")
dev = torch.device("cuda", 0)
B = pkg.BIGINT
torch.manual_seed(3)


def subset(n_all, n):
    return torch.sort(torch.randperm(n_all, device=dev)[:n]).values


customer = subset(15_000_000, 3_000_000).to(torch.int64) + 1
o = subset(150_000_000, 14_600_000).to(torch.int64)
orders = (o // 8) * 32 + o % 8 + 1
sides = {"customer 3.0M": customer, "orders 14.6M": orders}


def build_times(keys, reps=10):
    n = keys.numel()
    payload = torch.arange(n, dtype=torch.int64, device=dev)
    page = pkg.Page(pkg.DeviceBlock(B, n, keys), pkg.DeviceBlock(B, n, payload))
    ctx = pkg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.profile_enable(True)
    for it in range(reps + 2):
        if it == 2:
            ctx.profile_reset()
        bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B, B], [1], [0])
        b = bf.createOperator()
        b.addInput(page)
        b.finish()
        b.close()
    torch.cuda.synchronize()
    prof = ctx.profile()
    ctx.close()
    return {k: round(v["total_ms"] * 1e3 / reps, 1) for k, v in prof.items() if k.startswith("join_build")}


for rnd in range(2):
    for name, keys in sides.items():
        for blocks in ("1", "2", "4"):
            for loads in ("2", "4", "8", "16"):
                os.environ["TGPU_KEY_RANGE_LOADS"], os.environ["TGPU_KEY_RANGE_BLOCKS"] = loads, blocks
                print("round", rnd, name, "loads", loads, "blocks/CU", blocks, "range_us", build_times(keys)["join_build_range"], flush=True)
        del os.environ["TGPU_KEY_RANGE_LOADS"], os.environ["TGPU_KEY_RANGE_BLOCKS"]
        for heads in ("1", "0"):
            os.environ["TGPU_DIRECT_RANK_FROM_HEADS"] = heads
            print("round", rnd, name, "TGPU_DIRECT_RANK_FROM_HEADS=" + heads, "us per build", build_times(keys), flush=True)
        del os.environ["TGPU_DIRECT_RANK_FROM_HEADS"]

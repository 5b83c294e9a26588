"""Kernel study: the generic group-by on the Q3 aggregation's key shape -- clustered, shuffled and distinct rows, each by the run route
(gbh_runs; TGPU_GBH_RUNS unset) and by the table route (gbh_insert ...; TGPU_GBH_RUNS=0).  The shuffled layout with the run route on shows
what a failed attempt costs on top of the table route.  Prints the per-launch kernel times, the read-backs and the wall time per page."""
import importlib, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("presto-1_amd")
dev = torch.device("cuda", 0)
B, DT, I, D = pkg.BIGINT, pkg.DATE, pkg.INTEGER, pkg.DOUBLE
g = 1_131_128
torch.manual_seed(1)
cnt = torch.randint(1, 5, (g,), device=dev)
oi = torch.repeat_interleave(torch.arange(g, device=dev), cnt)
n = oi.numel()
for label in ("clustered", "shuffled", "distinct"):
    idx = oi if label != "shuffled" else oi[torch.randperm(n, device=dev)]
    if label == "distinct":
        idx = torch.arange(n, device=dev)
    key = (idx * 4 + 1).to(torch.int64)
    date = (8000 + idx % 2000).to(torch.int32)
    prio = torch.zeros(n, dtype=torch.int32, device=dev)
    val = torch.rand(n, dtype=torch.float64, device=dev)
    page = pkg.Page(pkg.DeviceBlock(B, n, key), pkg.DeviceBlock(DT, n, date), pkg.DeviceBlock(I, n, prio), pkg.DeviceBlock(D, n, val))
    for runs in ("1", "0"):
        os.environ["TGPU_GBH_RUNS"] = runs   # read by the library at call time
        ctx = pkg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        ctx.profile_enable(True)
        fac = pkg.HashAggregationOperatorFactory(ctx, 14, [B, DT, I], [0, 1, 2], [(pkg.SUM_DOUBLE, 3)], expected_groups=1 << 20)
        reps = 5
        for it in range(reps + 1):
            if it == 1:
                ctx.profile_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            op = fac.createOperator()
            op.addInput(page)
            op.finish()
            o = op.getOutput()
            groups = o.position_count
            o.release()
            op.close()
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3 / reps
        prof = ctx.profile()
        readbacks = prof.pop("__readbacks", {"count": 0})["count"] / reps
        print(label, "TGPU_GBH_RUNS=" + runs, n, groups, "wall_ms", round(wall_ms, 3), "readbacks", readbacks,
              {k: round(x["total_ms"] / reps, 3) for k, x in prof.items()}, flush=True)
        ctx.close()

"""Kernel study: pass 1 of the fused probe with its row loads one or two tiles ahead (jit.cpp FJ_DEPTH), on the two Q3 shapes.

    python tools/exp_fj_depth.py [SF=100] [lineitem|orders|both] [repeats=6] [stripes:shift,... [rounds=1]]

For every TGPU_FJ_DEPTH x TGPU_FJ_STRIPES x TGPU_FJ_CHUNK_SHIFT it prints the average launch time of pass 1, the scan and pass 2 (the
library's profile scopes), all from one process over one set of tables, so the lines of one run compare; lines of different runs do not
(box-to-box spread is larger than the effect).  The lineitem sweep is stripes {2, 3, 4} x shift 0..6, the orders sweep stripes 3 x shift {0, 3, 6};
a list of stripes:shift pairs replaces the sweep and is run `rounds` times over, which shows the spread of one configuration."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

sf = float(sys.argv[1]) if len(sys.argv) > 1 else 100.0
which = sys.argv[2] if len(sys.argv) > 2 else "both"
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 6
pkg = importlib.import_module("presto-1_amd")
entry = importlib.import_module("__graft_entry__")
dev = torch.device("cuda", 0)
t = bench.gen_q3(dev, sf)
B, D, DT, I = pkg.BIGINT, pkg.DOUBLE, pkg.DATE, pkg.INTEGER
pp = entry.bench_page_processors(pkg)
seg = t["c_seg_bytes"][t["c_seg_off"][:-1].to(torch.int64)]
ckeys = t["c_custkey"][seg == ord("B")].contiguous()
cust_ok = torch.zeros(t["c_custkey"].numel() + 2, dtype=torch.bool, device=dev)
cust_ok[t["c_custkey"]] = seg == ord("B")
okeys = t["o_orderkey"][(t["o_orderdate"] < 9204) & cust_ok[t["o_custkey"]]].contiguous()
n_l, n_o = t["l_orderkey"].numel(), t["o_orderkey"].numel()
shapes = {
    "lineitem": (okeys, pp["q3_lineitem"], [0], [0, 1],
                 lambda: pkg.Page(pkg.DeviceBlock(B, n_l, t["l_orderkey"]), pkg.DeviceBlock(D, n_l, t["l_extendedprice"]), pkg.DeviceBlock(D, n_l, t["l_discount"]),
                                  pkg.DeviceBlock(DT, n_l, t["l_shipdate"]))),
    "orders": (ckeys, pp["q3_orders"], [1], [0, 2, 3],
               lambda: pkg.Page(pkg.DeviceBlock(B, n_o, t["o_orderkey"]), pkg.DeviceBlock(B, n_o, t["o_custkey"]), pkg.DeviceBlock(DT, n_o, t["o_orderdate"]),
                                pkg.DeviceBlock(I, n_o, t["o_shippriority"]))),
}
sweeps = {"lineitem": [(s, c) for s in (3, 2, 4) for c in range(7)], "orders": [(3, c) for c in (6, 3, 0)]}
if len(sys.argv) > 4:   # "stripes:shift,..." for every shape named, the whole list `rounds` times over: the spread of one configuration next to the differences
    sweeps = {k: [tuple(int(x) for x in p.split(":")) for p in sys.argv[4].split(",")] * (int(sys.argv[5]) if len(sys.argv) > 5 else 1) for k in sweeps}
print("shape depth stripes chunk_shift rows probe_ms scan_ms emit_ms sum_ms", flush=True)
for name in (["lineitem", "orders"] if which == "both" else [which]):
    bkeys, proc, join_ch, out_ch, make_page = shapes[name]
    page = make_page()
    for stripes, shift in sweeps[name]:
        for depth in (1, 2):
            os.environ.update(TGPU_FJ_DEPTH=str(depth), TGPU_FJ_STRIPES=str(stripes), TGPU_FJ_CHUNK_SHIFT=str(shift))
            ctx = pkg.Context(0, stream=torch.cuda.current_stream().cuda_stream)
            ctx.profile_enable(True)
            bf = pkg.HashBuilderOperatorFactory(ctx, 1, [B], [], [0])
            b = bf.createOperator()
            b.addInput(pkg.Page(pkg.DeviceBlock(B, bkeys.numel(), bkeys)))
            b.finish()
            jf = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 2, bf.lookup_source_factory, *proc, join_ch, probe_output_channels=out_ch)
            rows = 0
            for it in range(repeats + 1):
                op = jf.createOperator()
                op.addInput(page)
                o = op.getOutput()
                rows = o.position_count if o is not None else 0
                if o is not None:
                    o.release()
                op.close()
                if it == 0:
                    ctx.profile_reset()
            prof = ctx.profile()
            ms = [prof[k]["total_ms"] / prof[k]["count"] if k in prof else 0.0 for k in ("fused_filter_probe", "fused_probe_scan", "fused_probe_emit")]
            print(name, depth, stripes, shift, rows, *("%.3f" % v for v in ms), "%.3f" % sum(ms), flush=True)
            b.close()
            ctx.close()

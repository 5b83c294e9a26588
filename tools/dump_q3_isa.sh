#!/bin/bash
# kernel study: dump the generated fused probe source of Q3 (lineitem by default) and compile its whole-table variant to ISA under /tmp
# usage: dump_q3_isa.sh [FJ_PF=1] [FJ_NO_NULLS=1] [FJ_CARRY=0] [q3_lineitem|q3_orders] [FJ_DEPTH=1]
# (TGPU_FJ_DEPTH / TGPU_FJ_STRIPES in the environment choose what precompile generates)
cd "$(dirname "$0")/.."
find presto-1_amd/_kcache -name '*.hip' -delete
TGPU_JIT_DUMP=1 python - ${4:-q3_lineitem} <<'PY' 2>&1 | tail -3
import importlib, os, sys
sys.path.insert(0, os.getcwd())
pkg = importlib.import_module("presto-1_amd")
e = importlib.import_module("__graft_entry__")
pp = e.bench_page_processors(pkg)
pkg.precompile_fused_probe(*pp[sys.argv[1] if len(sys.argv) > 1 else "q3_lineitem"], *((1, [0, 2, 3]) if len(sys.argv) > 1 and sys.argv[1] == "q3_orders" else (0, [0, 1])))
PY
for f in presto-1_amd/_kcache/*.hip; do if head -5 $f | tr "\n" " " | grep -q "FJ_PF ${1:-1} #define FJ_NO_NULLS ${2:-1} #define FJ_CARRY ${3:-0} #define FJ_DEPTH ${5:-1} #define FJ_EPILOGUE 0"; then (echo '#include <hip/hip_runtime.h>'; cat $f) > /tmp/fj.hip; fi; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S /tmp/fj.hip -o /tmp/fj.s -Rpass-analysis=kernel-resource-usage 2>&1 | grep -A12 "Function Name: fj_" | grep -E "Name|VGPRs:|Scratch|Occupancy"
awk '/^fj_probe[a-z_]*:/,/s_endpgm/' /tmp/fj.s > /tmp/fj_p.s
wc -l /tmp/fj_p.s

"""The argument blocks of the generated kernels have one definition each: a header under csrc/ that the host includes and every generated
source embeds verbatim.  Checked on the sources themselves, without a GPU: each source carries exactly the headers of its kernels, once."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "presto-1_amd")
CSRC = os.path.join(PKG_DIR, "csrc")
# header -> the blocks it declares
BLOCKS = {
    "device_fp_args.h": ["FpArgs"],
    "device_fv_args.h": ["FvArgs"],
    "device_fj_args.h": ["FjArgs", "FjPairArgs"],
    "device_fa_args.h": ["FaArgs"],
    "device_fq_args.h": ["FqArgs"],
    "device_fg_args.h": ["FgArgs"],
    "device_nl_args.h": ["NlArgs"],
}
BLOCK_DECL = re.compile(r"struct\s+((?:F[a-z]|Nl)\w*Args)\s*\{")


def header_text(name):
    text = open(os.path.join(CSRC, name)).read()
    assert text.count("#pragma once") == 1
    return text.replace("#pragma once", "", 1)


def check_source(src, headers, what):
    assert set(headers) <= set(BLOCKS)
    for name, blocks in BLOCKS.items():
        text = header_text(name)
        assert sorted(BLOCK_DECL.findall(text)) == sorted(blocks), name
        assert src.count(text) == (1 if name in headers else 0), (what, name)
    # ... and nobody else declares a block: every block of the source's headers once, and no other
    assert sorted(BLOCK_DECL.findall(src)) == sorted(b for name in headers for b in BLOCKS[name]), what


def test_the_host_and_the_generator_hold_no_second_definition():
    for name in ("jit.cpp", "jit.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert re.search(r"struct\s+\w*Args\w*\s*\{", text) is None, name
        for header in BLOCKS:
            assert header in text, (name, header)   # included by jit.h, embedded by jit.cpp


def test_page_processor_and_nested_loop_sources(pkg):
    f, B, V = pkg.field, pkg.BIGINT, pkg.VARCHAR
    check_source(pkg.page_processor_source([B, B, B], f(0, B) > 899, [f(1, B) * f(2, B)]), ["device_fp_args.h"], "filter + project")
    check_source(pkg.page_processor_source([V, B], f(1, B) > 3, [pkg.concat(f(0, V), "-"), f(1, B)]), ["device_fp_args.h", "device_fv_args.h"], "VARCHAR projection")
    band = pkg.and_(f(2, B) <= f(0, B), f(0, B) < f(3, B))
    src = pkg.nested_loop_filter_source([B, B], [B, B], band)
    check_source(src, ["device_fp_args.h", "device_nl_args.h"], "nested-loop filter")
    assert src.index("tg_pair_filter(const FpArgs& A, const NlRow& R)") < src.index("#define NL_STRIP")


# The fused probe and the fused aggregation have no source getter: a fresh process compiles them with TGPU_JIT_DUMP=1 into a resource
# directory of its own (csrc = the real one), which keeps every variant's source next to its code object.  The code objects the package's
# own cache already holds (build() pre-compiles the bench programs) are linked into the new cache first, so that those are not compiled again.
CHILD = r"""
import os, sys
root, tmp = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
import __graft_entry__ as g
pkg = g._pkg()
def resources(name):
    d = os.path.join(tmp, name)
    os.makedirs(os.path.join(d, "_kcache"))
    os.symlink(os.path.join(root, "presto-1_amd", "csrc"), os.path.join(d, "csrc"))
    for co in os.listdir(os.path.join(root, "presto-1_amd", "_kcache")) if os.path.isdir(os.path.join(root, "presto-1_amd", "_kcache")) else []:
        if co.endswith(".hsaco"):
            os.symlink(os.path.join(root, "presto-1_amd", "_kcache", co), os.path.join(d, "_kcache", co))
    pkg._lib.check(pkg._lib.lib().tgpu_set_resource_dir(d.encode()))
pps = g.bench_page_processors(pkg)
resources("agg_keys")
pkg.precompile_fused_aggregation(*pps["q1"], g.q1_aggregates(pkg), [0, 1])
resources("agg_global")
pkg.precompile_fused_aggregation(*pps["cfg2"], [(pkg.SUM_BIGINT, 0), (pkg.COUNT_ALL, -1)])
resources("probe")
pkg.precompile_fused_probe(*pps["q3_lineitem"], 0, [0, 1])
"""


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("jit_dump"))
    env = dict(os.environ, TGPU_JIT_DUMP="1")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, tmp], env=env, check=True, timeout=600)
    return {name: [open(p).read() for p in sorted(glob.glob(os.path.join(tmp, name, "_kcache", "*.hip")))] for name in ("agg_keys", "agg_global", "probe")}


@pytest.mark.parametrize("program,variants,headers", [
    ("agg_keys", 3, ["device_fp_args.h", "device_fa_args.h", "device_fq_args.h", "device_fg_args.h"]),
    ("agg_global", 3, ["device_fp_args.h", "device_fa_args.h"]),
    ("probe", 24, ["device_fp_args.h", "device_fj_args.h"]),
])
def test_fused_sources(dumped, program, variants, headers):
    sources = dumped[program]
    assert len(sources) >= variants and len(set(sources)) == len(sources)   # (the probe adds its partial-carry variants)
    for i, src in enumerate(sources):
        check_source(src, headers, (program, i))
    kernels = {"agg_keys": ["fa_mask", "fa_accumulate_lowcard", "fa_ordered_chain", "fq_onepass", "fq_onepass_multi", "fg_probe"],
               "agg_global": ["fa_mask", "fa_accumulate_global"], "probe": ["fj_probe", "fj_emit", "fj_pair"]}[program]
    for k in kernels:
        assert all(re.search(r'extern "C" __global__ void __launch_bounds__\(\w+( \* 64)?\) ' + k + r"\(", src) for src in sources), (program, k)

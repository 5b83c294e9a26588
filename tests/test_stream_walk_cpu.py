"""The host walks of csrc/stream_walk.h -- the whole bounds check of the ORC / Parquet decode kernels -- fuzzed on the CPU under AddressSanitizer
and UndefinedBehaviorSanitizer: tests/stream_walk/walk_main.cpp is built here (like tests/jni_harness.py builds its library: at test time, into an
ignored directory) and run as an ordinary child process, once per walker, over the corpus of tests/decode_cases.py.  Nothing is preloaded and
nothing is loaded into Python.

Exit status 0 means no sanitizer report, and that includes signed overflow: before the block-shape checks were fixed, the two DELTA_BINARY_PACKED
headers `delta/block_size_2^61_width_8` and `delta/block_size_2^63` of decode_cases.malformed() failed this assertion with
"runtime error: signed integer overflow: 8 * 2305843009213693952 cannot be represented in type 'long int'" (and 8 * -9223372036854775808) at
the walk's `at + mini * width / 8 <= len` (checked once by hand with that commit's two expressions put back; oracle/parquet_oracle.c held the same
two, and the process ends at the first report).

Mutant counts per walker (ok / reject), printed by test_walkers_keep_the_kernels_contract: see DESIGN.md section 2."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as dc   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "stream_walk", "walk_main.cpp")
OUT = os.path.join(ROOT, "tests", "stream_walk", "build")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# walker `ok` <=> oracle `ok` holds for the streams the library decodes in full (the RLE streams) and for PLAIN BYTE_ARRAY sections; for the
# `want`-limited walkers (hybrid, delta) `ok` implies `oracle_ok`.  Exceptions to either, by mutant name -> reason: none.
EXCEPTIONS = {}
BOTH_WAYS = ("rle_v2", "rle_v1", "byte_rle", "byte_arrays")


@pytest.fixture(scope="module")
def walk_main():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "walk_main")
    deps = [SRC, os.path.join(ROOT, "presto-1_amd", "csrc", "stream_walk.h"), os.path.join(ROOT, "oracle", "orc_oracle.c"), os.path.join(ROOT, "oracle", "parquet_oracle.c")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    objs = []
    for c in deps[2:]:
        o = os.path.join(OUT, os.path.basename(c)[:-2] + ".o")
        subprocess.check_call(["gcc", "-std=c11"] + SANITIZE + ["-c", c, "-o", o])
        objs.append(o)
    subprocess.check_call(["g++", "-std=c++17"] + SANITIZE + ["-Wall", "-Wextra", "-Werror", SRC] + objs + ["-o", exe])
    return exe


def run(exe, streams, tmp_path, tag):
    """one process over `streams`: [(walker result words, oracle result words)] in their order"""
    path = os.path.join(str(tmp_path), tag + ".cases")
    with open(path, "w") as f:
        for s in streams:
            f.write(s.case_line() + "\n")
    # (the time limit only catches a walk that does not end: the corpus takes seconds)
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    done = p.stdout.decode().splitlines()
    at = streams[len(done) - 1].name if 0 < len(done) <= len(streams) else "?"
    assert p.returncode == 0, "sanitizer report or crash (exit %d) at or behind case %d %s:\n%s" % (p.returncode, len(done), at, p.stderr.decode()[-3000:])
    assert len(done) == len(streams)
    out = []
    for i, line in enumerate(done):
        w = line.split()
        assert int(w[0]) == i + 1
        k = next(j for j, x in enumerate(w) if x.startswith("oracle_"))
        out.append((w[1:k], w[k:]))
    return out


@pytest.mark.parametrize("walker", dc.WALKERS)
def test_walkers_keep_the_kernels_contract(walk_main, tmp_path, walker):
    base, mutants = dc.corpus(walker)
    results = run(walk_main, base + mutants, tmp_path, walker)
    violations = [(s.name, r[0]) for s, r in zip(base + mutants, results) if r[0][0] == "VIOLATION"]
    assert not violations, violations[:10]
    # every well-formed base stream is walked, with the number of values its encoder wrote
    for s, (mine, theirs) in zip(base, results):
        assert mine[0] == "ok" and int(mine[2]) == s.total, (s.name, mine, s.total)
        assert theirs[0] == "oracle_ok", (s.name, theirs)
    # the walker and the oracle agree on what is a stream
    ok = rejected = 0
    for s, (mine, theirs) in zip(mutants, results[len(base):]):
        ok += mine[0] == "ok"
        rejected += mine[0] == "reject"
        if s.name in EXCEPTIONS:
            continue
        if mine[0] == "ok":
            assert theirs[0] == "oracle_ok", (s.name, mine, theirs)
        elif walker in BOTH_WAYS:
            assert theirs[0] == "oracle_reject", (s.name, mine, theirs)
    print("%s: %d mutants, %d ok, %d reject" % (walker, len(mutants), ok, rejected))
    # the fuzz is not vacuous: both outcomes, each at least one twentieth of the mutants
    assert ok + rejected == len(mutants)
    assert ok * 20 >= len(mutants) and rejected * 20 >= len(mutants), (walker, ok, rejected)


def test_malformed_streams_are_refused_before_anything_is_uploaded(walk_main, tmp_path):
    bad = dc.malformed()
    for s, (mine, theirs) in zip(bad, run(walk_main, bad, tmp_path, "malformed")):
        assert mine == ["reject"], (s.name, mine)
        assert theirs == ["oracle_reject"], (s.name, theirs)


def test_odd_but_legal_streams_are_walked(walk_main, tmp_path):
    odd = dc.odd_but_legal()
    for s, (mine, theirs) in zip(odd, run(walk_main, odd, tmp_path, "odd")):
        assert mine[0] == "ok" and int(mine[2]) == s.total == len(s.meta["values"]), (s.name, mine)
        assert theirs[0] == "oracle_ok", (s.name, theirs)


def test_coverage_streams_are_walked(walk_main, tmp_path):
    """the well-formed streams the GPU tests decode on top of the base streams: walked, with the number of values their encoders wrote"""
    cover = [s for w in dc.WALKERS for s in dc.coverage(w)]
    for s, (mine, theirs) in zip(cover, run(walk_main, cover, tmp_path, "coverage")):
        assert mine[0] == "ok" and int(mine[2]) == s.total, (s.name, mine, s.total)
        assert theirs[0] == "oracle_ok", (s.name, theirs)

"""The math functions without a GPU: the expected-value model (tests/math_fn_expected.py) against exact rational arithmetic and the reference's
pinned cases; the correctly rounded corpus of the bounded functions, regenerated when mpmath imports, with the host's libm held to the same
bound the device is; the kernels' arithmetic (presto-1_amd/csrc/device_math.h) compiled for the host under AddressSanitizer and
UndefinedBehaviorSanitizer -- tests/math_fn/math_main.cpp, built here at test time into an ignored directory and run as an ordinary child
process, nothing preloaded, nothing loaded into Python -- against the model; the generated programs compiled for gfx950; the errors raised
when a program is created; the IR's layout and the Java glue's names."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import pytest

import math_fn_cases as C
import math_fn_expected as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "math_function_vectors.json")))
CORPUS_PATH = os.path.join(ROOT, "tests", "golden", "math_function_ulp_corpus.json")
CORPUS = json.load(open(CORPUS_PATH))
SRC = os.path.join(ROOT, "tests", "math_fn", "math_main.cpp")
OUT = os.path.join(ROOT, "tests", "math_fn", "build")
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = ["ABS", "SIGN", "FLOOR", "CEILING", "TRUNCATE", "ROUND", "SQRT", "CBRT", "EXP", "LN", "LOG2", "LOG10", "LOG", "POWER", "IS_NAN", "IS_FINITE", "IS_INFINITE",
         "DEGREES", "RADIANS"]
BUILDERS = ["abs_", "sign", "floor", "ceiling", "truncate", "round_", "sqrt", "cbrt", "exp", "ln", "log2", "log10", "log", "power", "is_nan", "is_finite", "is_infinite",
            "degrees", "radians"]


def hexbits(x):
    return "%016x" % X.bits(x)


# ---- (a) the model ------------------------------------------------------------------------------------------------------------------------
def test_jround_against_exact_rational_arithmetic():
    values = C.edge_doubles() + C.random_doubles(3000, 3)
    assert 0.49999999999999994 in values and 2.0**52 + 1 in values and -(2.0**52) - 1 in values and 2.0**63 in values and -(2.0**63) in values
    for x in values:
        if x != x:
            assert X.jround(x) == 0
        elif math.isinf(x):
            assert X.jround(x) == (X.INT64_MAX if x > 0 else X.INT64_MIN)
        else:
            q = Fraction(x) + Fraction(1, 2)
            floor = q.numerator // q.denominator
            assert X.jround(x) == max(X.INT64_MIN, min(X.INT64_MAX, floor)), x
    assert X.jround(0.49999999999999994) == 0 and X.jround(0.5) == 1 and X.jround(-0.5) == 0 and X.jround(-1.5) == -1 and X.jround(2.5) == 3
    assert X.jround(2.0**52 + 1) == 2**52 + 1 and X.jround(-(2.0**52) - 1) == -2**52 - 1 and X.jround(2.0**63) == 2**63 - 1 and X.jround(-(2.0**63)) == -2**63
    assert X.jround(4503599627370495.5) == 2**52 and X.jround(-4503599627370495.5) == -2**52 + 1


def test_model_edges():
    assert X.same(X.ceiling(-0.5), -0.0) and X.same(X.truncate(-0.5), -0.0) and X.same(X.floor(-0.0), -0.0) and X.same(X.sign(-0.0), -0.0) and X.sign(C.NAN) != X.sign(C.NAN)
    assert X.same(X.abs_(-0.0), 0.0) and X.abs_(-5) == 5 and X.abs_(-2**63 + 1) == 2**63 - 1 and X.abs_(-2**31 + 1, "integer") == 2**31 - 1
    for v, kind, text in ((-2**63, "bigint", "Value -9223372036854775808 is out of range for abs(bigint)"), (-2**31, "integer", "Value -2147483648 is out of range for abs(integer)")):
        with pytest.raises(X.OutOfRange) as e:
            X.abs_(v, kind)
        assert str(e.value) == text
    assert X.abs_(-2**31, "bigint") == 2**31
    # round over integers: half away from zero, checked
    assert [X.round_(v, -1) for v in (14, 15, -14, -15, 25, -25)] == [10, 20, -10, -20, 30, -30] and X.round_(12345, 3) == 12345 and X.round_(149, -2) == 100
    assert X.round_(9223372036854775804, -1) == 9223372036854775800 and X.round_(-2**63, -18) == -9 * 10**18 and X.round_(2**63 - 1, -18) == 9 * 10**18
    for v, d, kind in ((2**63 - 1, -1, "bigint"), (-2**63, -1, "bigint"), (2**63 - 1, -14, "bigint"), (0, -19, "bigint"), (7, -2147483648, "integer"), (2**31 - 1, -1, "integer"),
                       (2147450000, -5, "integer"), (-2**31, -3, "integer")):
        with pytest.raises(X.OutOfRange) as e:
            X.round_(v, d, kind)
        assert str(e.value) == "numerical overflow: %d" % v
    # round over DOUBLE
    assert X.round_(2.5) == 3.0 and X.round_(-2.5) == -3.0 and X.round_(0.49999999999999994) == 0.0 and X.same(X.round_(-0.3), -0.0) and X.same(X.round_(-0.0), 0.0)
    assert X.round_(2.675, 2) == 2.68 and X.round_(1.005, 2) == 1.0 and X.round_(1e300, 2) == 9.223372036854776e16 and X.round_(123.456, -1) == 120.0 and X.round_(5e-324, 2) == 0.0
    assert X.same(X.round_(-3.5, 309), -0.0) and X.same(X.round_(3.5, 400), 0.0) and X.round_(3.5, -324) != X.round_(3.5, -324) and X.round_(C.INF, -324) == C.INF
    assert [X.decimal_power(d) == 10.0**d for d in range(0, 23)] == [True] * 23 and X.decimal_power(309) == C.INF and X.decimal_power(-324) == 0.0 and X.decimal_power(-323) == 1e-323
    assert X.round_(None, 2) is None and X.round_(2.5, None) is None and X.power(None, 2.0) is None and X.log(2.0, None) is None
    # Math.pow's list
    assert X.power(1.0, C.NAN) != X.power(1.0, C.NAN) and X.power(-1.0, C.INF) != X.power(-1.0, C.INF) and X.power(1.0, -C.INF) != X.power(1.0, -C.INF)
    assert X.power(C.NAN, 0.0) == 1.0 and X.power(C.NAN, -0.0) == 1.0 and X.power(2.0, 10.0) == 1024.0 and X.power(10.0, 22.0) == 1e22 and X.power(-3.0, 3.0) == -27.0
    assert X.same(X.power(-0.0, 3.0), -0.0) and X.power(-0.0, -3.0) == -C.INF and X.power(-0.0, -2.0) == C.INF and X.power(-C.INF, 3.0) == -C.INF and X.same(X.power(-C.INF, -3.0), -0.0)
    assert X.power(-8.0, 1.0 / 3.0) != X.power(-8.0, 1.0 / 3.0) and X.power(0.5, C.INF) == 0.0 and X.power(0.5, -C.INF) == C.INF
    assert X.ln(-1.0) != X.ln(-1.0) and X.ln(-0.0) == -C.INF and X.exp(1000.0) == C.INF and X.log(1.0, 1.0) != X.log(1.0, 1.0) and X.log2(8.0) == 3.0
    assert X.ulp_distance(1.0, math.nextafter(1.0, 2.0)) == 1 and X.ulp_distance(-5e-324, 5e-324) == 2 and X.ulp_distance(0.0, -0.0) == C.INF and X.ulp_distance(C.NAN, C.NAN) == 0
    assert X.ulp_distance(C.INF, 1.7976931348623157e308) == C.INF and X.ulp_distance(2.0, math.nextafter(2.0, 0.0)) == 1


def golden_argument(a):
    return None if a["value"] is None else X.from_bits(int(a["value"]["bits"], 16)) if a["type"] == "double" else a["value"]


def model_call(g):
    name = {"ceil": "ceiling", "pow": "power"}.get(g["function"], g["function"])
    args = [golden_argument(a) for a in g["arguments"]]
    kind = g["arguments"][0]["type"]
    if name == "abs":
        return X.abs_(args[0], kind)
    if name == "round":
        return X.round_(args[0], args[1] if len(args) == 2 else 0, kind)
    return (X.UNARY.get(name) or X.BINARY[name])(*args)


def test_model_against_the_golden_cases():
    cases = GOLD["cases"]
    counts = {}
    for g in cases:
        counts[g["function"]] = counts.get(g["function"], 0) + 1
    assert set(counts) == {"abs", "ceil", "ceiling", "floor", "truncate", "round", "sign", "sqrt", "cbrt", "exp", "ln", "log2", "log10", "log", "power", "pow", "is_nan", "is_finite",
                           "is_infinite", "degrees", "radians"}
    assert len(cases) > 350 and counts["round"] > 70 and counts["power"] > 100 and isinstance(GOLD["skipped_lines"], dict) and sum(GOLD["skipped_lines"].values()) > 100
    worst = {}
    for g in cases:
        if "error" in g:
            with pytest.raises(X.OutOfRange):
                model_call(g)
            continue
        got, want = model_call(g), g["expected"]
        want = None if want is None else X.from_bits(int(want["bits"], 16)) if isinstance(want, dict) else want
        name = {"pow": "power"}.get(g["function"], g["function"])
        if name in X.BOUNDED and want is not None:
            d = X.ulp_distance(got, want)
            worst[name] = max(worst.get(name, 0), d)
            assert d <= CORPUS["bounds"][name], (g, got)
        else:
            assert X.same(got, want), (g, got)
    assert len([g for g in cases if "error" in g]) == 8 and set(worst) == set(X.BOUNDED)
    # the file holds data only: numbers, bit patterns, names
    text = open(os.path.join(ROOT, "tests", "golden", "math_function_vectors.json")).read()
    assert "assertFunction" not in text and "Math." not in text and ";" not in text


# ---- (b) the correctly rounded corpus ------------------------------------------------------------------------------------------------------------
def test_ulp_corpus_layout_and_host_libm_within_the_bound():
    assert os.path.getsize(CORPUS_PATH) < 256 * 1024 and set(CORPUS["functions"]) == set(X.BOUNDED) == set(CORPUS["bounds"])
    assert {k: CORPUS["bounds"][k] for k in ("cbrt", "exp", "ln", "log10", "power")} == dict(cbrt=1, exp=1, ln=1, log10=1, power=1)
    assert 1 <= CORPUS["bounds"]["log2"] <= 4 and 1 <= CORPUS["bounds"]["log"] <= 5      # two logarithms one ulp off each, and the division
    for name, rows in CORPUS["functions"].items():
        assert 200 <= len(rows) <= 512, name
        fn = X.UNARY.get(name) or X.BINARY[name]
        worst = 0
        for row in rows:
            args, want = [X.from_bits(int(h, 16)) for h in row[:-2]], X.from_bits(int(row[-2], 16))
            d = X.ulp_distance(fn(*args), want)
            worst = max(worst, d)
            if name == "cbrt":
                # this host's cbrt is no yardstick: glibc's lies two doubles from the correctly rounded result for some arguments.  The cube
                # root is checked exactly instead: x lies between the cubes of the stored result's two rounding boundaries
                if want == want and not math.isinf(want) and want != 0.0:
                    lo, hi = (Fraction(want) + Fraction(math.nextafter(want, -C.INF))) / 2, (Fraction(want) + Fraction(math.nextafter(want, C.INF))) / 2
                    assert lo**3 <= Fraction(args[0]) <= hi**3, row
                else:
                    assert d == 0, row
                continue
            assert d <= (0 if row[-1] else CORPUS["bounds"][name]), (name, row, fn(*args))
        print("host libm, %s: at most %d doubles from the correctly rounded result" % (name, worst))
    rows = CORPUS["functions"]["power"]
    flagged = {(X.from_bits(int(r[0], 16)), X.from_bits(int(r[1], 16))) for r in rows if r[3]}
    assert {(2.0, 10.0), (10.0, 22.0), (-3.0, 3.0), (2.0, -1074.0), (1.5, 2.0)} <= flagged and (10.0, 23.0) not in flagged and len(flagged) > 60
    specials = [r for r in rows if r[2] in (hexbits(C.NAN), hexbits(C.INF), hexbits(-C.INF), hexbits(0.0), hexbits(-0.0))]
    assert len(specials) > 80 and [hexbits(1.0), hexbits(C.NAN), hexbits(C.NAN), 0] in rows and [hexbits(-1.0), hexbits(C.INF), hexbits(C.NAN), 0] in rows
    assert [hexbits(C.NAN), hexbits(-0.0), hexbits(1.0), 0] in rows
    exp_args = {X.from_bits(int(r[0], 16)) for r in CORPUS["functions"]["exp"]}
    assert {709.782712893384, 709.7827128933841, -745.0, -750.0, 5e-324} <= exp_args
    assert any(0 < X.from_bits(int(r[1], 16)) < 2.2250738585072014e-308 for r in CORPUS["functions"]["exp"])           # a subnormal result


def test_ulp_corpus_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_math_function_ulp_corpus as G
    finally:
        sys.path.pop(0)
    assert G.text(G.build()) == open(CORPUS_PATH).read()


# ---- (c) the kernels' arithmetic on the host, under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def math_main():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "math_main")
    deps = [SRC, os.path.join(ROOT, "presto-1_amd", "csrc", "device_math.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-std=c++17"] + SANITIZE + ["-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def run(exe, lines, tmp_path, name):
    path = str(tmp_path / (name + ".cases"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    # (the time limit only catches a program that does not end: the cases take well under a second)
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    done = p.stdout.decode().splitlines()
    assert p.returncode == 0, "sanitizer report or crash (exit %d) behind case %d:\n%s" % (p.returncode, len(done), p.stderr.decode()[-3000:])
    assert len(done) == len(lines)
    return done


def same_bits(got_hex, want):
    got = X.from_bits(int(got_hex, 16))
    return X.same(got, want)


def test_host_jround_signum_truncate_and_round_double(math_main, tmp_path):
    values = C.edge_doubles() + C.random_doubles(6000, 5)
    lines = ["jround " + hexbits(x) for x in values] + ["signum " + hexbits(x) for x in values] + ["trunc " + hexbits(x) for x in values]
    want = [str(X.jround(x)) for x in values]
    got = run(math_main, lines, tmp_path, "unary")
    n = len(values)
    assert got[:n] == want
    for x, s, t in zip(values, got[n:2 * n], got[2 * n:]):
        assert same_bits(s, X.sign(x)) and same_bits(t, X.truncate(x)), x
    lines, want = [], []
    for d in C.DECIMALS + [1, 3, -2, 15, 16, 17, 300, -300]:
        factor = X.decimal_power(d)
        for x in values:
            lines.append("round %s %s" % (hexbits(x), hexbits(factor)))
            want.append(X.round_(x, d))
    got = run(math_main, lines, tmp_path, "round")
    bad = [(l, g, hexbits(w)) for l, g, w in zip(lines, got, want) if not same_bits(g, w)]
    assert not bad, bad[:10]


def test_host_integer_round_at_the_edges(math_main, tmp_path):
    lines, want = [], []
    for kind, values in (("bigint", C.edge_bigints()), ("integer", C.edge_integers())):
        values = values + [v + k for v in values for k in (-1, 1) if (X.INT64_MIN if kind == "bigint" else X.INT32_MIN) <= v + k <= (X.INT64_MAX if kind == "bigint" else X.INT32_MAX)]
        for d in range(-1, -20, -1):
            for v in values:
                lines.append("iround %d %d %d" % (v, d, kind == "integer"))
                try:
                    want.append(str(X.round_(v, d, kind)))
                except X.OutOfRange:
                    want.append("OVERFLOW")
    got = run(math_main, lines, tmp_path, "iround")
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:10]
    assert 300 < want.count("OVERFLOW") < len(want) // 2 and len(want) > 3000


def test_host_power_patch(math_main, tmp_path):
    """tg_pow over the corpus: Math.pow's special cases exactly, the `exact` entries exactly, everything else within the bound"""
    rows = CORPUS["functions"]["power"]
    got = run(math_main, ["pow %s %s" % (r[0], r[1]) for r in rows], tmp_path, "pow")
    for r, g in zip(rows, got):
        d = X.ulp_distance(X.from_bits(int(g, 16)), X.from_bits(int(r[2], 16)))
        assert d <= (0 if r[3] else 1), (r, g)


# ---- (d) the generated programs compile for gfx950 -----------------------------------------------------------------------------------------------
def all_exprs(pkg, x, y, b, i):
    return [pkg.abs_(x), pkg.sign(x), pkg.floor(x), pkg.ceil(x), pkg.truncate(x), pkg.round_(x), pkg.round_(x, 2), pkg.sqrt(x), pkg.cbrt(x), pkg.exp(x), pkg.ln(x), pkg.log2(x),
            pkg.log10(x), pkg.log(x, y), pkg.power(x, y), pkg.pow_(x, 2), pkg.is_nan(x), pkg.is_finite(x), pkg.is_infinite(x), pkg.degrees(x), pkg.radians(x), pkg.abs_(b), pkg.abs_(i),
            pkg.sign(b), pkg.sign(i), pkg.floor(b), pkg.ceiling(i), pkg.round_(b), pkg.round_(i, 2), pkg.round_(b, -2), pkg.round_(i, -3), pkg.round_(b, -19)]


def test_every_op_compiles(pkg):
    f, D, B, I = pkg.field, pkg.DOUBLE, pkg.BIGINT, pkg.INTEGER
    x, y, b, i = f(0, D), f(1, D), f(2, B), f(3, I)
    types = [D, D, B, I]
    exprs = all_exprs(pkg, x, y, b, i)
    for at in range(0, len(exprs), 16):
        pkg.precompile_page_processor(types, pkg.and_(pkg.is_finite(x), pkg.abs_(x - y) < 1.0), exprs[at:at + 16])
    src = pkg.page_processor_source(types, pkg.abs_(x - y) < 1.0, [pkg.round_(x * (pkg.constant(1.0, D) - y), 2), pkg.power(x, 2.0), pkg.round_(b, -2)])
    header = open(os.path.join(ROOT, "presto-1_amd", "csrc", "device_math.h")).read()
    assert src.count("#define TG_MATH_HELPERS") == 1 and header in src and not re.search(r"^\s*#\s*include", header, re.M)
    assert "static __device__ __forceinline__" in header and "static inline" in header and "#ifndef TG_MATH_HELPERS" in header
    # round(x, 2): the factor 100 is a hex-float literal in the source, no table
    assert "tg_round_double(" in src and ", 0x1.9p+6)" in src and float.fromhex("0x1.9p+6") == 100.0 and "tg_pow(" in src and "tg_round_long((long long)" in src and ", 100LL, &o_)" in src
    assert "TG_RAISE_OPERAND(TG_E_ROUND" in src
    # only a program that needs the helpers gets them: abs, floor, sqrt, ln, the predicates and the integer identities are single expressions
    src = pkg.page_processor_source(types, pkg.is_nan(x), [pkg.abs_(x), pkg.floor(x), pkg.ceiling(x), pkg.sqrt(x), pkg.ln(x), pkg.log2(x), pkg.log(x, y), pkg.exp(x), pkg.cbrt(x), pkg.log10(x),
                                                            pkg.degrees(x), pkg.abs_(b), pkg.sign(i), pkg.round_(b, 3), pkg.round_(i)])
    assert "TG_MATH_HELPERS" not in src and "tg_" + "pow" not in src and "fabs(" in src and "TG_RAISE(TG_E_ABS_BIGINT)" in src and "TG_RAISE_OPERAND" not in src
    assert "tg_round_double" not in pkg.page_processor_source(types, x < y, [b + 1]) and "TG_MATH" not in pkg.page_processor_source(types, x < y, [b + 1])
    # a null number of decimals evaluates nothing
    src = pkg.page_processor_source(types, None, [pkg.round_(x, pkg.constant(None, I)), pkg.round_(b, pkg.constant(None, I))])
    assert "tg_round_double" not in src and "tg_round_long" not in src and "TG_MATH_HELPERS" not in src and "c0[row]" not in src and "c2[row]" not in src
    # decimals beyond the double range: the factor is +inf (its bit pattern), resp. zero
    src = pkg.page_processor_source(types, None, [pkg.round_(x, 309), pkg.round_(x, -324), pkg.round_(x, 22), pkg.round_(x, -323)])
    assert "0x7ff0000000000000ULL" in src and ", 0x0p+0)" in src and (", %s)" % re.sub(r"0+p", "p", (1e22).hex())) in src and ", 0x0.0000000000002p-1022)" in src


def test_fused_generators_take_math_functions(pkg):
    """in the filter and as an aggregate's input the functions are fused; a computed group key keeps the unfused composition; sign(k) is a fused
    probe key; a program whose round over integers can fail is left to the page processor, which fetches the message's operand"""
    f, D, B = pkg.field, pkg.DOUBLE, pkg.BIGINT
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_DOUBLE, 1)]
    filt = pkg.abs_(f(0, D)) < 900.0
    pkg.precompile_fused_aggregation([D, B], filt, [f(1, B), pkg.round_(f(0, D) * (pkg.constant(1.0, D) - f(0, D)), 2)], aggs, [0])
    pkg.precompile_fused_aggregation([D, B], filt, [pkg.sign(f(1, B)), pkg.power(f(0, D), 2.0)], aggs, [0])
    pkg.precompile_fused_aggregation([D, B], None, [f(1, B), pkg.ln(f(0, D))], aggs, [0])
    pkg.precompile_fused_probe([D, B], filt, [pkg.sign(f(1, B)), pkg.round_(f(0, D), 1)], 0, [0, 1])
    pkg.precompile_fused_probe([D, B], None, [pkg.abs_(f(1, B)), pkg.floor(f(0, D))], 0, [0, 1])


# ---- (e) errors when the program is created ----------------------------------------------------------------------------------------------------------
def raw_status(pkg, types, prog):
    spec, keep = prog.to_c()
    arr = (ctypes.c_int32 * len(types))(*types)
    return pkg._lib.lib().tgpu_precompile_page_processor(len(types), arr, ctypes.byref(spec))


def test_ir_errors(pkg):
    f, c, D, B, V, I, BO, DT, E = pkg.field, pkg.constant, pkg.DOUBLE, pkg.BIGINT, pkg.VARCHAR, pkg.INTEGER, pkg.BOOLEAN, pkg.DATE, pkg.expressions
    types = [D, B, V, I, DT]
    x, b, v, i, dt = f(0, D), f(1, B), f(2, V), f(3, I), f(4, DT)

    def status(expr):
        return raw_status(pkg, types, E.FlatProgram(None, [expr]))

    COMPILER, NOT_SUPPORTED = -4, -8
    integers_too = {"ABS", "SIGN", "FLOOR", "CEILING", "ROUND"}
    predicates = {"IS_NAN", "IS_FINITE", "IS_INFINITE"}
    for name in NAMES:
        two = name in ("LOG", "POWER")
        result = BO if name in predicates else D
        good = [x, x] if two else [x]
        assert status(E.call(name, result, *good)) == 0, name
        # wrong argument count
        assert status(E.call(name, result, *(good + [x]))) == COMPILER or name == "ROUND", name
        assert status(E.call(name, result, x, x, x)) == COMPILER, name
        if two:
            assert status(E.call(name, result, x)) == COMPILER, name
        # wrong argument type
        for bad in (v, dt, f(0, BO) if False else c(True, BO)):
            assert status(E.call(name, result, *([bad] + good[1:]))) == COMPILER, name
        if two:
            assert status(E.call(name, result, x, b)) == COMPILER and status(E.call(name, result, i, x)) == COMPILER, name
        if name in integers_too:
            assert status(E.call(name, B, b)) == 0 and status(E.call(name, I, i)) == 0, name
            assert status(E.call(name, D, b)) == COMPILER and status(E.call(name, B, i)) == COMPILER and status(E.call(name, I, x)) == COMPILER, name     # the result keeps the argument's type
        else:
            assert status(E.call(name, result, b)) == COMPILER and status(E.call(name, result, i)) == COMPILER, name
        # wrong result type
        assert status(E.call(name, BO if result == D else D, *good)) == COMPILER and status(E.call(name, B, *good)) == COMPILER, name
    # round's decimals: an INTEGER constant
    assert status(E.call("ROUND", D, x, c(2, I))) == 0 and status(E.call("ROUND", B, b, c(-2, I))) == 0 and status(E.call("ROUND", I, i, c(None, I))) == 0
    assert status(E.call("ROUND", D, x, c(2, B))) == COMPILER and status(E.call("ROUND", D, x, c(2.0, D))) == COMPILER and status(E.call("ROUND", B, x, c(2, I))) == COMPILER
    for expr in (pkg.round_(x, i), pkg.round_(b, i), pkg.round_(x, pkg.abs_(i)), pkg.round_(i, pkg.coalesce(i, c(1, I)))):
        assert status(expr) == NOT_SUPPORTED
        with pytest.raises(pkg.TgpuError) as e:
            pkg.precompile_page_processor(types, None, [expr])
        assert e.value.code == NOT_SUPPORTED and "the number of decimals must be an INTEGER constant" in str(e.value)


# ---- (f) the IR's layout, the header, the Java glue ----------------------------------------------------------------------------------------------------
def test_flat_program_layout_builders_and_header(pkg):
    f, c, D, B, I, BO, E = pkg.field, pkg.constant, pkg.DOUBLE, pkg.BIGINT, pkg.INTEGER, pkg.BOOLEAN, pkg.expressions
    assert [E.OPS[n] for n in NAMES] == list(range(33, 52))
    assert all(hasattr(pkg, n) for n in BUILDERS + ["ceil", "pow_"]) and pkg.ceil is pkg.ceiling and pkg.pow_ is pkg.power
    # the builders infer the result type from the argument and wrap Python numbers
    assert pkg.abs_(f(0, B)).type == B and pkg.abs_(f(0, I)).type == I and pkg.abs_(f(0, D)).type == D and pkg.abs_(-5).type == B and pkg.abs_(-5.0).type == D
    assert pkg.round_(f(0, I), -1).type == I and pkg.round_(f(0, D)).type == D and pkg.floor(7).type == B and pkg.sqrt(4).type == D and pkg.sqrt(4).arguments[0].type == D
    assert pkg.is_nan(f(0, D)).type == BO and pkg.log(2, f(0, D)).arguments[0].type == D and pkg.power(f(0, D), 2).arguments[1].value == 2
    prog = E.FlatProgram(None, [pkg.round_(f(0, D), 2), pkg.log(2.0, f(0, D)), pkg.round_(f(0, D)), pkg.round_(f(1, B), c(None, I))])
    rnd = prog.nodes[prog.projection_roots[0]]
    assert rnd["kind"] == 2 and rnd["op"] == 38 and rnd["type"] == D and [prog.nodes[a]["type"] for a in rnd["args"]] == [D, I]
    assert prog.nodes[rnd["args"][1]]["kind"] == 1 and prog.nodes[rnd["args"][1]]["ival"] == 2
    log = prog.nodes[prog.projection_roots[1]]
    assert log["op"] == 45 and prog.nodes[log["args"][0]]["dval"] == 2.0 and prog.nodes[log["args"][1]]["kind"] == 0
    assert len(prog.nodes[prog.projection_roots[2]]["args"]) == 1 and prog.nodes[prog.nodes[prog.projection_roots[3]]["args"][1]]["is_null"] == 1
    header = open(os.path.join(ROOT, "include/tgpu.h")).read()
    for name, value in zip(NAMES, range(33, 52)):
        assert "TGPU_OP_%s = %d" % (name, value) in header
    for rule in ("Value -9223372036854775808 is out of range for\n     *                     abs(bigint)", "Math.signum", "ceiling(-0.5) is -0.0", "signum(x) * floor(abs(x))",
                 "the number of decimals must be an INTEGER constant", "RoundingMode.HALF_UP", "numerical overflow: ", "checkedPow overflows before num is looked at",
                 "toIntExact there throws an ArithmeticException that escapes its own catch", "the exact floor(x + 1/2) as a\n     *                     long",
                 "JVM parity unpinned", "d > 308 (factor +inf) gives +-0.0 and d < -323 (factor 0)", "correctly rounded IEEE square root", "57.29577951308232", "0.017453292519943295",
                 "since JDK 9", "the reference needs Java 11", "within 1 ulp of the exact result", "pow(1, NaN) is NaN and pow(+-1, +-inf) is NaN", "pow(x, +-0) is 1 even for a NaN x",
                 "ln(x) / ln(base), the base first", "Out of the IR: the trigonometric and hyperbolic functions", "mod(a, b) is TGPU_OP_MODULUS"):
        assert rule in header, rule


def test_java_glue_maps_the_math_functions():
    """GpuRowExpressions against the reference's sources as text (no JDK here)"""
    glue = open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuRowExpressions.java")).read()
    for name, value in zip(NAMES, range(33, 52)):
        assert re.search(r"\bOP_%s = %d[,;]" % (name, value), glue), name
    table = glue[glue.index("private static int mathFunction("):glue.index("private static boolean overNumbers(")]
    labels = set(re.findall(r'case "(\w+)":', table))
    want = {"abs", "sign", "floor", "ceiling", "ceil", "truncate", "round", "sqrt", "cbrt", "exp", "ln", "log2", "log10", "log", "power", "pow", "is_nan", "is_finite", "is_infinite",
            "degrees", "radians"}
    assert labels == want | {"mod"} and 'case "mod": return arguments == 2 ? OP_MODULUS : 0;' in table and "OP_MODULUS = 5," in glue
    assert "DIVISION_BY_ZERO here" in glue and "instanceof DoubleType" in glue and "instanceof BigintType" in glue and "instanceof IntegerType" in glue
    for constant in ('"pi"', '"e"', '"nan"', '"infinity"'):
        assert constant in glue, constant
    # the lines the earlier tests read are as they were
    assert "OP_CAST = 14, OP_LENGTH = 16, OP_SUBSTR = 17, OP_CONCAT = 18, OP_STRPOS = 19, OP_STARTS_WITH = 20;" in glue and "private static int dateFunction(" in glue
    ref = "/root/reference/core/trino-main/src/main/java/io/trino/operator/scalar/MathFunctions.java"
    if not os.path.isfile(ref):
        pytest.skip("needs a checkout of the reference sources")
    source = open(ref).read()
    names = set()
    for m in re.finditer(r"@ScalarFunction(\(([^)]*)\))?", source):
        found = re.findall(r'"(\w+)"', m.group(2) or "")
        if not re.search(r'"\w+"', (m.group(2) or "").split("alias")[0]):           # no name given: the method's (or the class's) name in snake case
            after = source[m.end():m.end() + 600]
            method = re.search(r"public static (?:final class )?(?:\w+ )?(\w+)[\s({]", after)
            found.append(re.sub(r"(?<!^)([A-Z])", r"_\1", method.group(1)).lower())
        names.update(found)
    assert labels <= names, labels - names

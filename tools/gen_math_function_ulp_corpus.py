#!/usr/bin/env python3
"""Writes tests/golden/math_function_ulp_corpus.json: arguments of the bounded math functions (cbrt, exp, ln, log10, log2, log, power) with the
correctly rounded result of each, computed with mpmath at 256 bits and rounded to a double through an exact Fraction.

  python tools/gen_math_function_ulp_corpus.py [--check]

Layout: {"functions": {name: [[argument bits ..., result bits, exact], ...]}, "bounds": {name: ulps}}, bits as 16 hex digits.
exact = 1: the mathematical result is the double stored, and the function's contract promises it (power over integral arguments, log10 of a
power of ten, exp(0), ln(1)): 0 ulp is required.  Special cases (NaN, infinities, zeros) are stored as the rule gives them.

bounds: 1 for the functions java.lang.Math specifies to within 1 ulp of the exact result (an answer within 1 ulp of the exact result is at
most one double away from the correctly rounded one).  log2 = ln(x) / ln(2) and log(b, x) = ln(x) / ln(b) are quotients of two such
logarithms and one division: for every argument the quotient is evaluated with each logarithm moved by one ulp either way from its exact
value, the extreme quotients are rounded to nearest (the division's half ulp), and the bound is the largest distance in doubles from the
correctly rounded result over the corpus.

The GPU test reads only the JSON; the CPU test runs this generator again when mpmath imports and compares."""
import json
import math
import os
import struct
import sys
from fractions import Fraction

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import math_fn_expected as X   # noqa: E402  (special cases and bit helpers only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "math_function_ulp_corpus.json")
NAN, INF = float("nan"), float("inf")
SPECIALS = [NAN, INF, -INF, 0.0, -0.0, 5e-324, -5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0]


def hexbits(x):
    return "%016x" % X.bits(x)


def rounded(v):
    """an mpmath value -> the nearest double, through the exact rational it holds"""
    import mpmath
    v = mpmath.mpf(v)
    sign, man, exp, _ = v._mpf_
    if int(man) == 0:
        return 0.0
    top = int(exp) + int(man).bit_length()             # the value lies in [2^(top - 1), 2^top)
    if top > 1100 or top < -1200:
        return (-1.0 if sign else 1.0) * (INF if top > 0 else 0.0)
    q = Fraction(int(man)) * (Fraction(2) ** int(exp))
    q = -q if sign else q
    try:
        return float(q)
    except OverflowError:
        return -INF if sign else INF


def spread(seed, n, lo_exp, hi_exp, negative=False):
    """n doubles with exponents spread evenly over [2^lo_exp, 2^hi_exp) and pseudo-random mantissas (a fixed multiplicative sequence)"""
    out, state = [], seed
    for i in range(n):
        state = (state * 6364136223846793005 + 1442695040888963407) % 2**64
        e = lo_exp + (hi_exp - lo_exp) * i // n
        v = math.ldexp(1.0 + (state >> 12) / 2.0**52, e)
        out.append(-v if negative and i % 2 else v)
    return out


def near(x, k=3):
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = math.nextafter(lo, -INF), math.nextafter(hi, INF)
        out += [lo, hi]
    return out


def unary_arguments(name):
    args = list(SPECIALS)
    if name == "exp":
        args += [709.782712893384, 709.7827128933841, 709.0, 710.0, 1000.0, -708.3964185322641, -708.4, -740.0, -745.0, -750.0, -1000.0, 1e-300, -1e-300, 1e-17, -1e-17]
        args += near(1.0) + near(-1.0) + near(0.5) + [float(k) for k in range(-20, 21)] + [k + 0.5 for k in range(-10, 10)]
        args += spread(1, 120, -30, 9, negative=True)
    else:
        if name == "cbrt":
            args += [float(k**3) for k in range(2, 30)] + [-27.0, -8.0, 1e300, 1e-300, 3e-320, 0.001, 1e-9, 2.0**-1074 * 27]
            args += spread(2, 200, -1074, 1023, negative=True)
        else:   # the logarithms: around 1, the subnormals, powers of the base, negatives
            args += near(1.0, 8) + [1.0 + k * 2.0**-30 for k in range(-6, 7)] + [1.0 + k * 1e-3 for k in range(-5, 6)]
            args += [10.0**k for k in range(0, 23)] + [2.0**k for k in (-1074, -1073, -1023, -1022, -100, -3, -1, 1, 2, 3, 10, 52, 100, 1023)]
            args += [0.1, 0.01, 1e-5, 1e-300, 1e300, 3e-320, 1e-310, math.e, -2.0, -1e-300, 2.5, 3.0, 7.0, 9.999999999999998, 1000.0000000000001]
            args += spread(3, 160, -1074, 1023)
    return args


POWER_PAIRS = ([(x, y) for x in (NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5) for y in (NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, 2.0, 3.0, -3.0, 0.5, -0.5, 1e300, -1e300)]
               + [(2.0, 10.0), (10.0, 22.0), (-3.0, 3.0), (10.0, 23.0), (10.0, -1.0), (10.0, -2.0), (2.0, -1074.0), (2.0, 1023.0), (2.0, 1024.0), (2.0, -1080.0), (3.0, 33.0), (3.0, 34.0),
                  (3.0, 40.0), (5.0, 22.0), (5.0, 23.0), (7.0, 18.0), (7.0, 19.0), (-7.0, 19.0), (1.5, 2.0), (1.5, 30.0), (1.5, 31.0), (0.75, 26.0), (0.75, 27.0), (-2.5, 5.0), (-2.5, 4.0),
                  (4.0, 0.5), (2.25, 0.5), (2.0, 0.5), (8.0, 1.0 / 3.0), (27.0, -0.5), (100.0, 1.5), (-8.0, 1.0 / 3.0), (-2.0, 0.5), (-2.0, 1e300), (-2.0, 2.0**53 + 2), (-2.0, 1025.0),
                  (1.0000000000000002, 1e16), (0.9999999999999999, 1e16), (1.0000000000000002, 4e18), (1e-300, 2.0), (1e300, 2.0), (1e154, 2.0), (1e-160, 2.0), (5e-324, 0.5),
                  (5e-324, 2.0), (1e-310, 0.25), (1.7976931348623157e308, 0.5), (1.7976931348623157e308, 1.0), (5e-324, 1.0), (5e-324, -1.0), (2.0, -1022.0), (2.0, -1023.0), (3.0, -2.0),
                  (0.1, 3.0), (1.1, 2.0), (123456.789, 2.0), (math.pi, 2.0), (math.e, 3.0), (10.0, 308.0), (10.0, 309.0), (10.0, -323.0), (10.0, -324.0), (10.0, -330.0), (12.0, 14.0), (12.0, 15.0)]
               + [(float(b), float(e)) for b in (2, 3, 5, 6, 10, -2, -3, -10) for e in (2, 3, 7, 15, 20)]
               + [(b + 0.5, e) for b in (0, 1, 2, 7, -1, -4) for e in (2.0, 3.0, 0.5, -1.0, 2.5, -2.5)])


def power_pairs():
    xs, ys = spread(5, 150, -40, 40), spread(6, 150, -6, 6, negative=True)
    return POWER_PAIRS + list(zip(xs, ys)) + [(x, float(k % 9 - 4)) for k, x in enumerate(spread(7, 60, -100, 100, negative=True))]


LOG_PAIRS = ([(b, x) for b in (NAN, INF, 0.0, -0.0, 1.0, -2.0, 2.0, 10.0, 0.5) for x in (NAN, INF, 0.0, -0.0, 1.0, -1.0, 8.0, 0.001)]
             + [(2.0, 2.0**k) for k in (-1074, -10, -1, 1, 3, 10, 100, 1023)] + [(10.0, 10.0**k) for k in (1, 2, 3, 15, 22)] + [(3.0, 81.0), (7.0, 49.0), (0.5, 8.0), (math.e, math.e)])


def log_pairs():
    bases = [2.0, 10.0, 0.5, math.e, 1.0000001, 0.9999999, 7.0, 1e300, 1e-300, 3.0, 1.5, 16.0]
    return LOG_PAIRS + [(bases[k % len(bases)], x) for k, x in enumerate(near(1.0, 4) + spread(8, 220, -1074, 1023))]


def truth(name, *args):
    """-> (the correctly rounded result as a double, exact); the special cases as tests/math_fn_expected.py states Java's rules"""
    import mpmath
    mpmath.mp.prec = 256
    mp = mpmath.mp
    if name == "power":
        x, y = args
        want = X.power_special(x, y)
        if want is not None:
            return want, 0
        q = X.exact_power(x, y)
        if q is None:
            return rounded(mp.power(mp.mpf(x), mp.mpf(y))), 0
        want = X.as_exact_double(q)
        if want is not None:
            return want, 1
        try:
            return float(q), 0                                   # Fraction -> float rounds correctly
        except OverflowError:
            return (-INF if q < 0 else INF), 0
    if name in ("log2", "log"):
        b, x = (2.0, args[0]) if name == "log2" else args
        if not (x == x and b == b and 0.0 < x < INF and 0.0 < b < INF and b != 1.0 and x != 1.0):
            return X.log(b, x), 0                                # the IEEE quotient of the special logarithms
        return rounded(mp.log(mp.mpf(x)) / mp.log(mp.mpf(b))), 0
    fn = {"cbrt": lambda v: mp.cbrt(v) if v > 0 else -mp.cbrt(-v), "exp": mp.exp, "ln": mp.log, "log10": mp.log10}[name]
    (x,) = args
    special = X.UNARY[name](x)
    if special != special or math.isinf(special) or special == 0.0 or x != x or math.isinf(x):
        if name in ("exp", "cbrt") and special == 0.0 and x != 0.0 and not math.isinf(x):
            return rounded(fn(mp.mpf(x))), 0                     # an underflowing exp: the correctly rounded result, which may be a subnormal
        return special, int((name == "exp" and x == 0.0) or (name in ("ln", "log10") and x == 1.0))
    return rounded(fn(mp.mpf(x))), int((name == "log10" and x in [10.0**k for k in range(23)]) or (name == "exp" and x == 0.0))


def quotient_bound(b, x, want):
    """the largest distance from `want` of ln(x) / ln(b) with each logarithm one ulp off its exact value and the quotient rounded to nearest"""
    import mpmath
    mp = mpmath.mp
    fr = lambda v: Fraction(int(v._mpf_[1]) * (-1 if v._mpf_[0] else 1)) * Fraction(2) ** int(v._mpf_[2])
    num, den = mp.log(mp.mpf(x)), mp.log(mp.mpf(b))
    n0, d0 = fr(num), fr(den)
    un, ud = Fraction(math.ulp(rounded(num))), Fraction(math.ulp(rounded(den)))
    return max(X.ulp_distance(float(n / d), want) for n in (n0 - un, n0 + un) for d in (d0 - ud, d0 + ud) if d != 0)


def build():
    out, bounds = {}, {}
    plans = [(n, [(x,) for x in unary_arguments(n)]) for n in ("cbrt", "exp", "ln", "log10")]
    plans += [("power", power_pairs()), ("log2", [(x,) for x in unary_arguments("ln")]), ("log", log_pairs())]
    for name, arguments in plans:
        rows, seen, worst = [], set(), 1
        for a in arguments:
            key = tuple(hexbits(v) for v in a)
            if key in seen:
                continue
            seen.add(key)
            want, exact = truth(name, *a)
            if name in ("log2", "log"):
                b, x = (2.0, a[0]) if name == "log2" else a
                if x == x and b == b and 0.0 < x < INF and 0.0 < b < INF and b != 1.0 and x != 1.0:
                    worst = max(worst, quotient_bound(b, x, want))
            rows.append(list(key) + [hexbits(want), exact])
        out[name], bounds[name] = rows, worst
    return {"precision_bits": 256, "bounds": bounds, "functions": out}


def text(corpus):
    lines = ['{"precision_bits": %d,' % corpus["precision_bits"], ' "bounds": %s,' % json.dumps(corpus["bounds"], sort_keys=True), ' "functions": {']
    names = sorted(corpus["functions"])
    for k, name in enumerate(names):
        lines.append('  "%s": [' % name)
        rows = corpus["functions"][name]
        lines += ["   %s%s" % (json.dumps(r), "," if i + 1 < len(rows) else "") for i, r in enumerate(rows)]
        lines.append("  ]" + ("," if k + 1 < len(names) else ""))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    new = text(build())
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == new else "the committed corpus differs from what this generator writes")
    with open(OUT, "w") as f:
        f.write(new)
    c = json.loads(new)
    print({k: len(v) for k, v in c["functions"].items()}, c["bounds"], len(new), "bytes")

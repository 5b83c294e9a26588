"""Seeded inputs of the math-function tests: the edge doubles and integers, the decimals and the row counts.  Values come from the
floating-point format and the integer ranges, never from the product."""
import math
import struct

import numpy as np

ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]          # wave and block edges.  No op has cross-row state.
DECIMALS = [-324, -323, -19, -18, -1, 0, 2, 22, 23, 308, 309]
INTEGER_DECIMALS = [-19, -18, -10, -9, -2, -1, 0, 2]
NAN, INF = float("nan"), float("inf")
MIN_SUBNORMAL, MAX_SUBNORMAL, MIN_NORMAL, MAX_DOUBLE = 5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _neighbours(x):
    return [math.nextafter(x, -INF), x, math.nextafter(x, INF)]


def edge_doubles():
    """specials, subnormals, halves up to 2^53, the doubles around 1/2, around the int64 ends and around 2^52; each with its negative"""
    pos = [0.0, MIN_SUBNORMAL, 3 * MIN_SUBNORMAL, MAX_SUBNORMAL, MIN_NORMAL, MAX_DOUBLE, INF, 1.0, 2.0, 10.0, 100.0, 0.1, 0.3, 0.7, 1e-5, 1e22, 1e23, 1e300, 1e-300,
           2.675, 1.005, 0.125, 0.285, 1.45, 2.5e-3, 123456.789, 1e15 + 0.3, math.pi, math.e]
    pos += _neighbours(0.5) + _neighbours(1.5) + _neighbours(2.5) + [0.49999999999999994]
    pos += [k + 0.5 for k in (0, 1, 2, 3, 4, 7, 8, 99, 100, 1023, 2**20, 2**31 - 1, 2**31, 2**32, 2**40 + 1, 2**51 - 1, 2**51, 2**52 - 1)]
    for p in (52, 53, 62, 63, 64):
        pos += _neighbours(2.0**p)
    pos += [2.0**52 + 1, 2.0**52 - 1, 2.0**53 - 1, 2.0**53 + 2, 9.2e18, 9.3e18, 4.6e18]
    out = []
    for v in pos:
        out += [v, -v]
    return out + [NAN, _from_bits(0xFFF8000000000001), _from_bits(0x7FF0000000000001)]


def random_doubles(n, seed):
    """a third uniform bit patterns, a third within +-1000 with two or three decimals, a third near halves"""
    rng = np.random.default_rng(seed)
    a = [_from_bits(int(b)) for b in rng.integers(0, 2**64, n // 3, dtype=np.uint64)]
    b = [round(float(v), int(k)) for v, k in zip(rng.uniform(-1000, 1000, n // 3), rng.integers(0, 4, n // 3))]
    c = [float(int(v)) + 0.5 * int(s) for v, s in zip(rng.integers(-2**40, 2**40, n - 2 * (n // 3)), rng.integers(-1, 2, n - 2 * (n // 3)))]
    return a + b + c


def edge_bigints():
    ends = [-2**63, -2**63 + 1, 2**63 - 1, 2**63 - 2]
    mids = [0, 1, -1, 4, 5, 6, -4, -5, -6, 14, 15, 16, 49, 50, 51, -50, 149, 150, 151, 499, 500, 501, 10**18, -10**18, 5 * 10**18, -5 * 10**18, 4 * 10**18 + 999, 9 * 10**18,
            -9 * 10**18, 9223372036854775800, 9223372036854775805, -9223372036854775805, 4999999999, 5000000000, -5000000000, 123456789012345678, 2**31, -2**31 - 1]
    return ends + mids


def edge_integers():
    return [-2**31, -2**31 + 1, 2**31 - 1, 2**31 - 2, 0, 1, -1, 4, 5, 6, -4, -5, -6, 14, 15, 49, 50, 51, -50, 149, 150, 2147483640, 2147483645, -2147483645,
            1500000000, 2100000000, -2100000000, 499999999, 500000000, 1000000000, -1000000000, 123456789]


def with_nulls(values):
    """every fourth row NULL: a None put in after every three values, so that no value is lost"""
    out = []
    for i, v in enumerate(values):
        out.append(v)
        if i % 3 == 2:
            out.append(None)
    return out


def cycle(values, n, start=0):
    return [values[(start + i) % len(values)] for i in range(n)]

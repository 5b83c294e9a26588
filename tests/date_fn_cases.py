"""Seeded inputs of the DATE-function tests: the edge days, the add amounts and the row counts.  Day numbers come from the expected-value
evaluator's calendar (tests/date_fn_expected.py), never from the product."""
import numpy as np

import date_fn_expected as X

ROW_COUNTS = [1, 63, 64, 65, 257]          # wave and block tails; the full edge list is the sixth count.  No op has cross-row state.
AMOUNTS = [0, 1, -1, 11, -11, 12, -12, 13, -13, 1200, -1200, 2**31 - 1, -(2**31 - 1), 2**31, -2**31 - 1, 2**62, -2**62]
UNIT_CODES = {u: i for i, u in enumerate(X.UNITS)}
YEARS_53 = (2004, 2009, 2015, 2020)         # ISO years of 53 weeks
YEARS_52 = (2005, 2010, 2017, 2021)


def _centres():
    d = X.to_days
    out = [X.INT32_MIN, X.INT32_MAX, 0]
    out += [k * 146097 for k in range(-3, 4)]
    for y in (1996, 2000, 2400, 1999, 2001, 1900, 2100, 0, -1, -4, -100, -400):           # leap, century-leap, non-leap, century, around year 0
        out += [d(y, 2, 28), d(y, 3, 1)] + ([d(y, 2, 29)] if X.is_leap(y) else [])
    for y in (1999, 2000):
        out += [d(y, m, X.month_length(y, m)) for m in range(1, 13)]
    for y in YEARS_53 + YEARS_52:
        out += list(range(d(y, 12, 28), d(y + 1, 1, 4) + 1))
    for y in (0, -1):
        out += [d(y, 1, 1), d(y, 6, 30), d(y, 12, 31)]
    return out


def edge_days():
    """each centre and its two neighbours inside int32, ascending, distinct"""
    days = {c + k for c in _centres() for k in (-1, 0, 1) if X.INT32_MIN <= c + k <= X.INT32_MAX}
    return sorted(days)


def with_nulls(values):
    """every fourth row NULL: a None put in after every three values, so that no value is lost"""
    out = []
    for i, v in enumerate(values):
        out.append(v)
        if i % 3 == 2:
            out.append(None)
    return out


def edge_rows():
    return with_nulls(edge_days())


def cycle(values, n, start=0):
    return [values[(start + i) % len(values)] for i in range(n)]


def random_days(n=100_000, seed=20):
    """int32 days: half over the whole range, half within +-400 years of the epoch"""
    rng = np.random.default_rng(seed)
    wide = rng.integers(X.INT32_MIN, X.INT32_MAX, n // 2, endpoint=True)
    near = rng.integers(-146097, 146097, n - n // 2, endpoint=True)
    return [int(v) for v in np.concatenate([wide, near])]


def diff_pairs():
    """edge-day pairs: every edge day against a spread of edge days, in both orders"""
    days = edge_days()
    partners = days[::7] + [days[0], days[-1]]
    return [(a, b) for a in days for b in partners]

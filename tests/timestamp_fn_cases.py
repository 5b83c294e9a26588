"""Seeded inputs of the TIMESTAMP-function tests: the edge instants, the add amounts, the precisions and the row counts.  Every number comes
from the expected-value evaluators' calendar (tests/date_fn_expected.py, tests/timestamp_fn_expected.py), never from the product."""
import numpy as np

import date_fn_cases as DC
import date_fn_expected as D
import timestamp_fn_expected as X

ROW_COUNTS = [1, 63, 64, 65, 4097]         # wave and block tails, more than one block.  No op has cross-row state.
UNIT_CODES = {u: i for i, u in enumerate(X.UNITS)}
PRECISIONS = list(range(7))
AMOUNTS = [0, 1, -1, 11, -13, 1200, 2**31 - 1, -2**31, 2**31, -2**31 - 1, 2**62, -2**62]        # the int32 edges and past them
DATE_CAST_DAYS = [0, 1, -1, 106751991, 106751992, -106751991, -106751992, 106751990, -106751990, D.INT32_MIN, D.INT32_MAX, 19000, -19000]
US = 1
MS = 1000
DAY_US = X.US_PER_DAY
MAX_DAY, MIN_DAY = X.INT64_MAX // 1000 // X.MS_PER_DAY, X.INT64_MIN // 1000 // X.MS_PER_DAY        # 106751991, -106751992


def at(y, m, d, h=0, mi=0, s=0, us=0):
    return D.to_days(y, m, d) * DAY_US + ((h * 60 + mi) * 60 + s) * 1_000_000 + us


def _centres():
    out = [0, -1, 999, 1000, -1000, 1, -999, -1001, 500, -500, 499, -499, 501, -501]                  # where floor and truncation differ; rounding ties
    out += [X.INT64_MIN, X.INT64_MIN + 1, X.INT64_MAX, X.INT64_MAX - 1]
    # the first / last whole millisecond, second, minute, hour, day of the range: date_trunc's and date_add's overflow edges
    for unit_us in (1000, 1_000_000, 60_000_000, 3_600_000_000, DAY_US, 7 * DAY_US):
        out += [X.INT64_MIN // unit_us * unit_us, (X.INT64_MIN // unit_us + 1) * unit_us, X.INT64_MAX // unit_us * unit_us, (X.INT64_MAX // unit_us - 1) * unit_us]
    # the first and last Monday, month, quarter and year that begin inside the range
    for day in (MIN_DAY, MIN_DAY + 1, MAX_DAY, MAX_DAY - 1):
        for u in ("week", "month", "quarter", "year"):
            for t in (D.date_trunc(u, day), D.date_trunc(u, day) + {"week": 7, "month": 31, "quarter": 92, "year": 366}[u]):
                out.append(t * DAY_US)
    # unit boundaries near the epoch and at the calendar's edge days: leap days, year 0, the ISO week-year edges
    for y in (1996, 2000, 1900, 2100, 0, -1, -4, 1970, 1969):
        out += [at(y, 2, 28), at(y, 3, 1), at(y, 12, 31, 23, 59, 59, 999_999), at(y, 1, 1)] + ([at(y, 2, 29, 12)] if D.is_leap(y) else [])
    for y in DC.YEARS_53[:2] + DC.YEARS_52[:2]:
        out += [at(y, 12, 28) + k * DAY_US for k in range(0, 8)]
    out += [at(2001, 8, 22, 3, 4, 5, 321_987), at(2020, 5, 10, 12, 34, 56, 123_456), at(1960, 1, 22, 3, 4, 5, 678_000), at(2020, 1, 31, 23, 59, 59, 999_000),
            at(1999, 12, 31, 23, 59, 59, 999_999), at(2000, 2, 29, 0, 0, 0, 1)]
    out += [at(2020, 5, 10, h, 0, 0) for h in (0, 1, 12, 23)] + [at(2020, 5, 10, 12, mi, 0) for mi in (1, 59)] + [at(2020, 5, 10, 12, 34, s) for s in (1, 59)]
    return out


def edge_instants():
    """each centre and its two neighbours inside int64, ascending, distinct"""
    return sorted({c + k for c in _centres() for k in (-1, 0, 1) if X.INT64_MIN <= c + k <= X.INT64_MAX})


def random_instants(n=2000, seed=31):
    """a third over the whole int64 range, a third within years 1..9999, a third within a few days of the epoch"""
    rng = np.random.default_rng(seed)
    k = n // 3
    wide = rng.integers(X.INT64_MIN, X.INT64_MAX, k, endpoint=True)
    civil = rng.integers(at(1, 1, 1), at(9999, 12, 31, 23, 59, 59, 999_999), k, endpoint=True)
    near = rng.integers(-5 * DAY_US, 5 * DAY_US, n - 2 * k, endpoint=True)
    return [int(v) for v in np.concatenate([wide, civil, near])]


def instants():
    """the corpus of the host program and of the device tests"""
    return edge_instants() + random_instants()


with_nulls, cycle = DC.with_nulls, DC.cycle


def diff_pairs():
    """every edge instant against a spread of instants, in both orders"""
    xs = edge_instants()
    partners = xs[::17] + [xs[0], xs[-1], 0, at(2000, 2, 29), at(2001, 1, 31, 12)]
    return [(a, b) for a in xs for b in partners]

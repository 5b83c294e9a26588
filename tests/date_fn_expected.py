"""The twelve DATE functions of the expression IR (include/tgpu.h TGPU_OP_YEAR .. TGPU_OP_DATE_DIFF) restated in Python integers: the expected
value of every DATE-function test.  Written from the calendar's definition -- a year's first day from the leap-year count, months from a
table of lengths, date_diff by searching with date_add -- not from the product's era arithmetic, and it imports nothing of the product.
A day is the count of days since 1970-01-01 in the proleptic Gregorian calendar with a year 0; None is NULL.  Cross-checked against
datetime over datetime's whole range by tests/test_date_functions_cpu.py."""

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
UNITS = ("day", "week", "month", "quarter", "year")
_LENGTHS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


class OutOfRange(Exception):
    """TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE (-2): an amount outside int32 or a DATE result outside int32 days"""


def unit_of(unit):
    """the unit as the library matches it: ASCII lower-cased; ValueError with the reference's message otherwise"""
    u = "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in unit)
    if u not in UNITS:
        raise ValueError("'%s' is not a valid DATE field" % u)
    return u


def is_leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def _leaps_before(y):
    """leap years among the years ... , y - 1, up to a constant"""
    return (y - 1) // 4 - (y - 1) // 100 + (y - 1) // 400


def year_start(y):
    return 365 * (y - 1970) + _leaps_before(y) - _leaps_before(1970)


def month_length(y, m):
    return 29 if m == 2 and is_leap(y) else _LENGTHS[m - 1]


def to_days(y, m, d):
    return year_start(y) + sum(month_length(y, k) for k in range(1, m)) + d - 1


def civil(days):
    """-> (year, month, day, day of year)"""
    y = 1970 + days * 400 // 146097      # an estimate, then the definition decides
    while year_start(y) > days:
        y -= 1
    while year_start(y + 1) <= days:
        y += 1
    doy = days - year_start(y) + 1
    m, rest = 1, doy
    while rest > month_length(y, m):
        rest -= month_length(y, m)
        m += 1
    return y, m, rest, doy


def _checked(days):
    if not INT32_MIN <= days <= INT32_MAX:
        raise OutOfRange(days)
    return days


def year(d): return None if d is None else civil(d)[0]
def month(d): return None if d is None else civil(d)[1]
def quarter(d): return None if d is None else (civil(d)[1] - 1) // 3 + 1
def day(d): return None if d is None else civil(d)[2]
def day_of_year(d): return None if d is None else civil(d)[3]
def day_of_week(d): return None if d is None else (d + 3) % 7 + 1


def _thursday(d):
    return d - (day_of_week(d) - 1) + 3


def year_of_week(d): return None if d is None else civil(_thursday(d))[0]
def week(d): return None if d is None else (civil(_thursday(d))[3] - 1) // 7 + 1


def last_day_of_month(d):
    if d is None:
        return None
    y, m, _, _ = civil(d)
    return _checked(to_days(y, m, month_length(y, m)))


def date_trunc(unit, d):
    if unit is None or d is None:
        return None
    u = unit_of(unit)
    y, m, _, _ = civil(d)
    if u == "day":
        return d
    if u == "week":
        return _checked(d - (day_of_week(d) - 1))
    if u == "month":
        return _checked(to_days(y, m, 1))
    if u == "quarter":
        return _checked(to_days(y, (m - 1) // 3 * 3 + 1, 1))
    return _checked(to_days(y, 1, 1))


def _add_months(d, n):
    y, m, dd, _ = civil(d)
    k = y * 12 + (m - 1) + n
    y, m = k // 12, k % 12 + 1
    return to_days(y, m, min(dd, month_length(y, m)))


def _add(u, v, d):
    """unbounded"""
    if u == "day":
        return d + v
    if u == "week":
        return d + 7 * v
    return _add_months(d, v * {"month": 1, "quarter": 3, "year": 12}[u])


def date_add(unit, v, d):
    if unit is None:
        return None
    u = unit_of(unit)
    if v is None or d is None:
        return None
    if not INT32_MIN <= v <= INT32_MAX:
        raise OutOfRange(v)
    return _checked(_add(u, v, d))


def date_diff(unit, d1, d2):
    if unit is None:
        return None
    u = unit_of(unit)
    if d1 is None or d2 is None:
        return None
    if d2 < d1:
        return -date_diff(u, d2, d1)
    # the largest n >= 0 with d1 + n units <= d2: bisected between a count that is certainly reached and one that certainly is not
    # (d1 + n units grows with n)
    longest, shortest = {"day": (1, 1), "week": (7, 7), "month": (31, 28), "quarter": (92, 89), "year": (366, 365)}[u]
    lo, hi = (d2 - d1) // longest, (d2 - d1) // shortest + 2
    assert _add(u, lo, d1) <= d2 < _add(u, hi, d1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _add(u, mid, d1) <= d2:
            lo = mid
        else:
            hi = mid
    return lo


UNARY_NAMES = ("year", "quarter", "month", "week", "day", "day_of_week", "day_of_year", "year_of_week", "last_day_of_month")


def unary_row(d):
    """the nine unary results of one day in the order of UNARY_NAMES, the calendar walked twice instead of nine times; last_day_of_month
    is None where it overflows"""
    y, m, dd, doy = civil(d)
    ty, _, _, tdoy = civil(_thursday(d))
    last = d + month_length(y, m) - dd
    return (y, (m - 1) // 3 + 1, m, (tdoy - 1) // 7 + 1, dd, (d + 3) % 7 + 1, doy, ty, last if last <= INT32_MAX else None)


UNARY = {"year": year, "quarter": quarter, "month": month, "week": week, "day": day, "day_of_week": day_of_week, "day_of_year": day_of_year,
         "year_of_week": year_of_week, "last_day_of_month": last_day_of_month}

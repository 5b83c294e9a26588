"""The TIMESTAMP functions of the expression IR (include/tgpu.h "TIMESTAMP functions") restated in Python integers: the expected value of every
TIMESTAMP-function test.  A timestamp is the count of microseconds since 1970-01-01 00:00:00 UTC; None is NULL.  The calendar is
tests/date_fn_expected.py's (its year starts, month table and add-months search); the arithmetic here is plain unbounded integers with the
64-bit behaviour written out where the reference has it (Java's wrapping long in DateTimes.roundDiv, its multiplyExact / toIntExact
elsewhere).  It imports nothing of the product.  Cross-checked against datetime + timedelta for years 1..9999 by
tests/test_timestamp_functions_cpu.py."""
import struct

import date_fn_expected as D

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
INT32_MIN, INT32_MAX = D.INT32_MIN, D.INT32_MAX
UNITS = ("millisecond", "second", "minute", "hour", "day", "week", "month", "quarter", "year")
UNIT_MS = {"millisecond": 1, "second": 1000, "minute": 60_000, "hour": 3_600_000, "day": 86_400_000, "week": 7 * 86_400_000}
MS_PER_DAY = 86_400_000
US_PER_DAY = 86_400_000_000
OutOfRange = D.OutOfRange


def unit_of(unit):
    """the unit as the library matches it: ASCII lower-cased; ValueError with the reference's message otherwise"""
    u = "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in unit)
    if u not in UNITS:
        raise ValueError("'%s' is not a valid Timestamp field" % u)
    return u


def wrap64(x):
    """x as Java's long holds it"""
    return (x + 2**63) % 2**64 - 2**63


def _tdiv(a, b):
    """Java's / on longs: truncated toward zero (b > 0)"""
    return a // b if a >= 0 else -((-a) // b)


def millis(us): return us // 1000
def split(us):
    """-> (day, tod in ms, micros of the millisecond)"""
    ms = us // 1000
    return ms // MS_PER_DAY, ms % MS_PER_DAY, us % 1000


def _checked_us(us):
    if not INT64_MIN <= us <= INT64_MAX:
        raise OutOfRange(us)
    return us


# ---- extraction --------------------------------------------------------------------------------------------------------------------------
def _of_day(fn):
    return lambda us: None if us is None else fn(split(us)[0])


year, quarter, month, week, day = _of_day(D.year), _of_day(D.quarter), _of_day(D.month), _of_day(D.week), _of_day(D.day)
day_of_week, day_of_year, year_of_week = _of_day(D.day_of_week), _of_day(D.day_of_year), _of_day(D.year_of_week)
last_day_of_month = _of_day(D.last_day_of_month)


def hour(us): return None if us is None else split(us)[1] // 3_600_000
def minute(us): return None if us is None else split(us)[1] // 60_000 % 60
def second(us): return None if us is None else split(us)[1] // 1000 % 60
def millisecond(us): return None if us is None else split(us)[1] % 1000


def to_unixtime(us):
    """(double) us / 1000000.0: Python's int -> float conversion and its float division are the IEEE ones"""
    return None if us is None else float(us) / 1000000.0


def double_bits(x):
    return None if x is None else struct.unpack("<q", struct.pack("<d", x))[0]


UNARY_NAMES = ("year", "quarter", "month", "week", "day", "day_of_week", "day_of_year", "year_of_week", "last_day_of_month", "hour", "minute", "second",
               "millisecond")
UNARY = {n: globals()[n] for n in UNARY_NAMES}


def unary_row(us):
    """the thirteen integer-valued unary results of one timestamp, in the order of UNARY_NAMES"""
    d, tod, _ = split(us)
    return D.unary_row(d) + (tod // 3_600_000, tod // 60_000 % 60, tod // 1000 % 60, tod % 1000)


# ---- rounding (M/type/DateTimes.java:104-117, :169-177) -------------------------------------------------------------------------------------
def round_div(value, factor):
    """roundDiv as the reference writes it, every intermediate a Java long"""
    if factor == 1:
        return value
    if value >= 0:
        return _tdiv(wrap64(value + factor // 2), factor)
    return _tdiv(wrap64(value + 1 - factor // 2), factor)


def round_to(value, factor):
    return wrap64(round_div(value, factor) * factor)


# ---- casts ---------------------------------------------------------------------------------------------------------------------------------
def cast_precision(us, q):
    """CAST(timestamp AS timestamp(q))"""
    assert 0 <= q <= 6
    return None if us is None else (us if q == 6 else round_to(us, 10 ** (6 - q)))


def from_date(days):
    """CAST(date AS timestamp): TimeUnit.DAYS.toMicros saturates"""
    return None if days is None else max(INT64_MIN, min(INT64_MAX, days * US_PER_DAY))


def to_date(us):
    """CAST(timestamp AS date)"""
    return None if us is None else us // US_PER_DAY


# ---- date_trunc / date_add / date_diff ------------------------------------------------------------------------------------------------------
def date_trunc(unit, us):
    if unit is None:
        return None
    u = unit_of(unit)
    if us is None:
        return None
    ms = us // 1000
    if u in ("millisecond", "second", "minute", "hour", "day"):
        ms = ms // UNIT_MS[u] * UNIT_MS[u]
    else:
        ms = D.date_trunc(u, ms // MS_PER_DAY) * MS_PER_DAY
    return _checked_us(ms * 1000)


def _add_ms(u, v, ms):
    """unbounded: the millisecond count v units later"""
    if u in UNIT_MS:
        return ms + v * UNIT_MS[u]
    d, tod = ms // MS_PER_DAY, ms % MS_PER_DAY
    return D._add_months(d, v * {"month": 1, "quarter": 3, "year": 12}[u]) * MS_PER_DAY + tod


def date_add(unit, v, us, p=6):
    assert 0 <= p <= 6
    if unit is None:
        return None
    u = unit_of(unit)
    if v is None or us is None:
        return None
    if not INT32_MIN <= v <= INT32_MAX:
        raise OutOfRange(v)
    ms = _add_ms(u, v, us // 1000)
    if p <= 3:
        ms = round_to(ms, 10 ** (3 - p))      # (|ms| < 2^62 here: nothing wraps)
    return _checked_us(ms * 1000 + us % 1000)


def date_diff(unit, us1, us2):
    if unit is None:
        return None
    u = unit_of(unit)
    if us1 is None or us2 is None:
        return None
    ms1, ms2 = us1 // 1000, us2 // 1000
    if u in UNIT_MS:
        return _tdiv(ms2 - ms1, UNIT_MS[u])
    per = {"month": 1, "quarter": 3, "year": 12}[u]      # quarters and years: whole multiples of months, truncated toward zero
    if ms2 < ms1:
        return -(_diff_months(ms2, ms1) // per)
    return _diff_months(ms1, ms2) // per


def _diff_months(ms1, ms2):
    """ms1 <= ms2: the largest n >= 0 with ms1 + n months <= ms2, bisected (ms1 + n months grows with n)"""
    span = (ms2 - ms1) // MS_PER_DAY
    lo, hi = span // 31, span // 28 + 2
    assert _add_ms("month", lo, ms1) <= ms2 < _add_ms("month", hi, ms1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _add_ms("month", mid, ms1) <= ms2:
            lo = mid
        else:
            hi = mid
    return lo

// Time-of-day and precision arithmetic of the TIMESTAMP functions (include/tgpu.h, "TIMESTAMP functions"): a timestamp(p), p <= 6, is an int64
// count of microseconds since 1970-01-01 00:00:00 UTC.  The calendar is device_date.h's, whose text must stand in front of this one: with
// ms = floordiv(us, 1000), day = floordiv(ms, 86 400 000) and tod = ms - day * 86 400 000, |day| <= 106 751 992 always fits int32.
//
// Like device_date.h this text has no #include and uses plain integer types only: it is embedded as it stands into the JIT sources (jit.cpp
// device_header("device_timestamp.h")) and compiled as it stands by a host program (tests/timestamp_math/ts_main.cpp) that checks it on
// the CPU.  Every function is declared through TG_DATE_FN.
//
// Nothing overflows a signed type: what the reference computes with Java's wrapping long arithmetic (DateTimes.roundDiv) is computed in
// unsigned 64 bits here, and everything else is range-checked before it is formed.
#ifndef TG_TIMESTAMP_HELPERS
#define TG_TIMESTAMP_HELPERS

#define TG_TS_UNIT_MILLISECOND 0
#define TG_TS_UNIT_SECOND 1
#define TG_TS_UNIT_MINUTE 2
#define TG_TS_UNIT_HOUR 3
#define TG_TS_UNIT_DAY 4
#define TG_TS_UNIT_WEEK 5
#define TG_TS_UNIT_MONTH 6
#define TG_TS_UNIT_QUARTER 7
#define TG_TS_UNIT_YEAR 8

#define TG_TS_MS_PER_DAY 86400000LL
#define TG_TS_INT64_MIN (-9223372036854775807LL - 1)
#define TG_TS_INT64_MAX 9223372036854775807LL

// Math.floorDiv by a positive constant
TG_DATE_FN long long tg_ts_floordiv(long long a, long long b)
{
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// scaleEpochMicrosToMillis / getMicrosOfMilli (M/type/DateTimes.java:119-122, :159-162)
TG_DATE_FN long long tg_ts_millis(long long us) { return tg_ts_floordiv(us, 1000LL); }
TG_DATE_FN int tg_ts_micros_of_milli(long long us)
{
  const int r = (int)(us % 1000LL);   // (not us - ms * 1000: that product lies below INT64_MIN for the first 808 microseconds of the range)
  return r < 0 ? r + 1000 : r;
}
TG_DATE_FN int tg_ts_day(long long ms) { return (int)tg_ts_floordiv(ms, TG_TS_MS_PER_DAY); }
// 0 .. 86 399 999
TG_DATE_FN int tg_ts_tod(long long ms) { return (int)(ms - (long long)tg_ts_day(ms) * TG_TS_MS_PER_DAY); }

TG_DATE_FN long long tg_ts_unit_millis(int unit)
{
  return unit == TG_TS_UNIT_MILLISECOND ? 1LL : unit == TG_TS_UNIT_SECOND ? 1000LL : unit == TG_TS_UNIT_MINUTE ? 60000LL
       : unit == TG_TS_UNIT_HOUR ? 3600000LL : unit == TG_TS_UNIT_DAY ? TG_TS_MS_PER_DAY : 7LL * TG_TS_MS_PER_DAY;
}

// the DATE unit code of month / quarter / year
TG_DATE_FN int tg_ts_date_unit(int unit) { return unit - TG_TS_UNIT_MONTH + TG_DATE_UNIT_MONTH; }

// extraction (operator/scalar/timestamp/Extract*.java: the Joda field of scaleEpochMicrosToMillis)
TG_DATE_FN int tg_ts_date(long long us) { return tg_ts_day(tg_ts_millis(us)); }
TG_DATE_FN long long tg_ts_hour(long long us) { return tg_ts_tod(tg_ts_millis(us)) / 3600000; }
TG_DATE_FN long long tg_ts_minute(long long us) { return tg_ts_tod(tg_ts_millis(us)) / 60000 % 60; }
TG_DATE_FN long long tg_ts_second(long long us) { return tg_ts_tod(tg_ts_millis(us)) / 1000 % 60; }
TG_DATE_FN long long tg_ts_millisecond(long long us) { return tg_ts_tod(tg_ts_millis(us)) % 1000; }

// scaleEpochMillisToMicros(ms) + micros (DateTimes.java:139-142), micros in 0 .. 999: *overflow is set when the sum is no int64
TG_DATE_FN long long tg_ts_from_millis(long long ms, int micros, int *overflow)
{
  // 9223372036854775 * 1000 + 807 = INT64_MAX, -9223372036854775 * 1000 - 808 = INT64_MIN
  const int bad = ms > 9223372036854775LL || ms < -9223372036854776LL || (ms == 9223372036854775LL && micros > 807) ||
                  (ms == -9223372036854776LL && micros < 192);
  *overflow |= bad;
  return bad ? 0 : (long long)((unsigned long long)ms * 1000ULL + (unsigned long long)micros);   // (the product alone may lie below INT64_MIN)
}

// DateTimes.roundDiv :104-117 followed by the multiplication of roundToNearest :174-177, in Java's wrapping 64-bit arithmetic
TG_DATE_FN long long tg_ts_round_to(long long value, long long factor)
{
  if (factor == 1) return value;
  const unsigned long long half = (unsigned long long)(factor / 2);
  const long long t = value >= 0 ? (long long)((unsigned long long)value + half) : (long long)((unsigned long long)value + 1ULL - half);
  return (long long)((unsigned long long)(t / factor) * (unsigned long long)factor);
}

TG_DATE_FN long long tg_ts_pow10(int n)
{
  long long f = 1;
  for (int i = 0; i < n; i++) f *= 10;
  return f;
}

// CAST(timestamp AS timestamp(q)), 0 <= q <= 6 (TimestampToTimestampCast.java: round(value, 6 - q))
TG_DATE_FN long long tg_ts_cast_precision(long long us, int q) { return q >= 6 ? us : tg_ts_round_to(us, tg_ts_pow10(6 - q)); }

// CAST(date AS timestamp): TimeUnit.DAYS.toMicros saturates (DateToTimestampCast.java)
TG_DATE_FN long long tg_ts_from_date(int days)
{
  if (days > 106751991) return TG_TS_INT64_MAX;
  if (days < -106751991) return TG_TS_INT64_MIN;
  return (long long)days * 86400000000LL;
}

// CAST(timestamp AS date): floordiv(us, 86 400 000 000) (TimestampToDateCast.java)
TG_DATE_FN int tg_ts_to_date(long long us) { return (int)tg_ts_floordiv(us, 86400000000LL); }

// date_trunc (DateTrunc.java): the millisecond count floored to the unit, the sub-millisecond part dropped.  A floor in front of the first
// representable microsecond sets *overflow.
TG_DATE_FN long long tg_ts_trunc(int unit, long long us, int *overflow)
{
  const long long ms = tg_ts_millis(us);
  long long r;
  if (unit <= TG_TS_UNIT_DAY) {
    const long long u = tg_ts_unit_millis(unit);
    r = tg_ts_floordiv(ms, u) * u;   // |ms| < 2^54: nothing to check
  }
  else {
    int o = 0;   // (never set: a timestamp's day lies deep inside the int32 range)
    const int day = tg_ts_day(ms);
    const int d = tg_date_trunc(unit == TG_TS_UNIT_WEEK ? TG_DATE_UNIT_WEEK : tg_ts_date_unit(unit), day, &o);
    r = (long long)d * TG_TS_MS_PER_DAY;
  }
  return tg_ts_from_millis(r, 0, overflow);
}

// date_add (DateAdd.java:41-57) on a timestamp(p).  A value outside int32 and a result that is no int64 count of microseconds set *overflow.
TG_DATE_FN long long tg_ts_add(int unit, long long value, long long us, int p, int *overflow)
{
  const int bad = value < -2147483648LL || value > 2147483647LL;
  *overflow |= bad;
  const long long v = bad ? 0 : value;
  long long ms = tg_ts_millis(us);
  const int micros = tg_ts_micros_of_milli(us);
  if (unit <= TG_TS_UNIT_WEEK) ms += v * tg_ts_unit_millis(unit);   // |v * unit| < 2^61, |ms| < 2^54
  else {
    const int day = tg_ts_day(ms), tod = tg_ts_tod(ms);
    int o = 0;
    // the months index in 64 bits; a result day outside int32 lies far outside the microsecond range as well
    const int d = tg_date_add_months(day, unit == TG_TS_UNIT_MONTH ? v : unit == TG_TS_UNIT_QUARTER ? 3 * v : 12 * v, &o);
    *overflow |= o;
    ms = o ? 0 : (long long)d * TG_TS_MS_PER_DAY + tod;
  }
  if (p <= 3) ms = tg_ts_round_to(ms, tg_ts_pow10(3 - p));   // |ms| < 2^62: no wrap here
  const long long r = tg_ts_from_millis(ms, micros, overflow);
  return *overflow ? 0 : r;
}

// The whole months from ms1 to ms2: for ms2 >= ms1 the largest n >= 0 with add_months(ms1, n) <= ms2, else the negated count the other way.
// Closed form as in tg_date_diff_months, the time of day breaking the tie of equal days.
TG_DATE_FN long long tg_ts_diff_months(long long ms1, long long ms2)
{
  const int swap = ms2 < ms1;
  const long long lo = swap ? ms2 : ms1, hi = swap ? ms1 : ms2;
  const int tod_a = tg_ts_tod(lo), tod_b = tg_ts_tod(hi);
  const tg_civil a = tg_date_civil(tg_ts_day(lo)), b = tg_date_civil(tg_ts_day(hi));
  const int len = tg_date_month_length(b.leap, b.month);
  const int day_a = a.day < len ? a.day : len;
  const int past = day_a > b.day || (day_a == b.day && tod_a > tod_b);
  const int n = (b.year - a.year) * 12 + (b.month - a.month) - past;
  return swap ? -(long long)n : (long long)n;
}

// date_diff (DateDiff.java) on the millisecond counts; the precise units truncate toward zero
TG_DATE_FN long long tg_ts_diff(int unit, long long us1, long long us2)
{
  const long long ms1 = tg_ts_millis(us1), ms2 = tg_ts_millis(us2);
  if (unit <= TG_TS_UNIT_WEEK) return (ms2 - ms1) / tg_ts_unit_millis(unit);
  const long long n = tg_ts_diff_months(ms1, ms2);
  return unit == TG_TS_UNIT_MONTH ? n : unit == TG_TS_UNIT_QUARTER ? n / 3 : n / 12;
}
#endif

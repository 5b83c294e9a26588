// Calendar arithmetic of the DATE functions (TGPU_OP_YEAR .. TGPU_OP_DATE_DIFF, include/tgpu.h): the proleptic Gregorian (ISO) calendar in UTC
// with astronomical year numbering, for every int32 count of days since 1970-01-01 (-5877641-06-23 .. 5881580-07-11).
//
// This text has no #include and uses plain int / unsigned / long long only: it is embedded as it stands into the JIT sources
// (jit.cpp device_header("device_date.h"), where hiprtc has no libc headers) and compiled as it stands by a host program
// (tests/date_math/date_main.cpp) that checks it on the CPU.  Every function is declared through TG_DATE_FN.
//
// No table in memory, no division by a run-time divisor (constant divisors become a multiply-high), and 32-bit arithmetic wherever the
// int32 day range fits: a day count becomes unsigned by adding 2^31, so that the era split is one unsigned division.  64 bits are used for
// what can leave int32: the months index of an addition and a DATE result that is range-checked.  Nothing overflows a signed type.
#ifndef TG_DATE_HELPERS
#define TG_DATE_HELPERS
#if defined(__HIPCC_RTC__) || defined(__HIP_DEVICE_COMPILE__)
#define TG_DATE_FN static __device__ __forceinline__
#else
#define TG_DATE_FN static inline
#endif

#define TG_DATE_UNIT_DAY 0
#define TG_DATE_UNIT_WEEK 1
#define TG_DATE_UNIT_MONTH 2
#define TG_DATE_UNIT_QUARTER 3
#define TG_DATE_UNIT_YEAR 4

struct tg_civil {
  int year, month, day;   // month and day from 1
  int doy;                // day of the year from 1
  int leap;               // 1 in a leap year
};

TG_DATE_FN int tg_date_is_leap(int year) { return (year & 3) == 0 && ((year % 25) != 0 || (year & 15) == 0); }

// 28..31; m + (m >> 3) is odd exactly for the months of 31 days
TG_DATE_FN int tg_date_month_length(int leap, int month) { return month == 2 ? 28 + leap : 30 + ((month + (month >> 3)) & 1); }

// days -> (year, month, day, day of year).  With u = days + 2^31 and 2^31 = 14699 * 146097 + 3845, the day count from 0000-03-01 is
// days + 719468 = u + 131235 - 14695 * 146097: eras of 400 years (146097 days) counted from era -14695, all of it in unsigned 32 bits.
TG_DATE_FN tg_civil tg_date_civil(int days)
{
  const unsigned u = (unsigned)days ^ 0x80000000u;
  unsigned era = u / 146097u, doe = u % 146097u + 131235u;   // doe < 2 * 146097
  if (doe >= 146097u) { doe -= 146097u; era += 1u; }
  const unsigned yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;   // 0 .. 399
  const unsigned doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                  // 0 .. 365, from March 1
  const unsigned mp = (5u * doy + 2u) / 153u;                                       // 0 .. 11, March = 0
  tg_civil c;
  c.day = (int)(doy - (153u * mp + 2u) / 5u) + 1;
  c.month = mp < 10u ? (int)mp + 3 : (int)mp - 9;
  c.year = (int)yoe + ((int)era - 14695) * 400 + (mp >= 10u);
  c.leap = tg_date_is_leap(c.year);
  c.doy = mp < 10u ? (int)doy + 60 + c.leap : (int)doy - 305;
  return c;
}

// (year, month, day) -> days, for -5880000 < year < 5880000; the result may lie outside int32, hence 64 bits
TG_DATE_FN long long tg_date_days(int year, int month, int day)
{
  const unsigned yy = (unsigned)(year - (month <= 2) + 5880000);   // 14700 eras: never negative
  const unsigned era = yy / 400u, yoe = yy % 400u;
  const unsigned mp = month > 2 ? (unsigned)month - 3u : (unsigned)month + 9u;
  const unsigned doy = (153u * mp + 2u) / 5u + (unsigned)day - 1u;
  const unsigned doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
  return ((long long)era - 14700LL) * 146097LL + (long long)doe - 719468LL;
}

// 0 = Monday .. 6 = Sunday: floormod(days + 3, 7), and 2^31 mod 7 = 2
TG_DATE_FN int tg_date_dow0(int days)
{
  const unsigned r = ((unsigned)days ^ 0x80000000u) % 7u + 1u;
  return r == 7u ? 0 : (int)r;
}

TG_DATE_FN long long tg_date_year(int days) { return tg_date_civil(days).year; }
TG_DATE_FN long long tg_date_month(int days) { return tg_date_civil(days).month; }
TG_DATE_FN long long tg_date_quarter(int days) { return (tg_date_civil(days).month + 2) / 3; }
TG_DATE_FN long long tg_date_day(int days) { return tg_date_civil(days).day; }
TG_DATE_FN long long tg_date_day_of_year(int days) { return tg_date_civil(days).doy; }
TG_DATE_FN long long tg_date_day_of_week(int days) { return tg_date_dow0(days) + 1; }

// The Thursday of the ISO week of `days`.  It stays inside int32: day -2^31 is a Tuesday and day 2^31 - 1 a Friday, so the first week's
// Thursday is day -2^31 + 2 and the last week's is day 2^31 - 2.
TG_DATE_FN int tg_date_iso_thursday(int days) { return days + (3 - tg_date_dow0(days)); }
TG_DATE_FN long long tg_date_year_of_week(int days) { return tg_date_civil(tg_date_iso_thursday(days)).year; }
TG_DATE_FN long long tg_date_week(int days) { return (unsigned)(tg_date_civil(tg_date_iso_thursday(days)).doy - 1) / 7u + 1; }

// A DATE result computed in 64 bits: *overflow is set when it is no int32 day count (the value returned is then 0)
TG_DATE_FN int tg_date_checked(long long days, int *overflow)
{
  const int bad = days < -2147483648LL || days > 2147483647LL;
  *overflow |= bad;
  return bad ? 0 : (int)days;
}

TG_DATE_FN int tg_date_last_day_of_month(int days, int *overflow)
{
  const tg_civil c = tg_date_civil(days);
  return tg_date_checked((long long)days + (tg_date_month_length(c.leap, c.month) - c.day), overflow);
}

// day: the value; week: the Monday on or before it; month, quarter, year: the first day of the period.  In the first year of the
// int32 range that Monday / first day can lie before day -2^31: overflow.
TG_DATE_FN int tg_date_trunc(int unit, int days, int *overflow)
{
  if (unit == TG_DATE_UNIT_DAY) return days;
  if (unit == TG_DATE_UNIT_WEEK) return tg_date_checked((long long)days - tg_date_dow0(days), overflow);
  const tg_civil c = tg_date_civil(days);
  if (unit == TG_DATE_UNIT_MONTH) return tg_date_checked((long long)days - (c.day - 1), overflow);
  if (unit == TG_DATE_UNIT_YEAR) return tg_date_checked((long long)days - (c.doy - 1), overflow);
  return tg_date_checked(tg_date_days(c.year, (c.month - 1) / 3 * 3 + 1, 1), overflow);
}

// days + months: the (year, month) moves, the day of the month is clamped to the target month's length.  |months| <= 12 * 2^31.
// The months index year * 12 + month - 1 of a DATE lies in [-70531687, 70578966]; an index outside it is an overflow before any
// narrowing, an index inside it fits 32 bits.
TG_DATE_FN int tg_date_add_months(int days, long long months, int *overflow)
{
  const tg_civil c = tg_date_civil(days);
  const long long idx = (long long)(c.year * 12 + (c.month - 1)) + months;
  const int bad = idx < -70531687LL || idx > 70578966LL;
  *overflow |= bad;
  const unsigned ui = (unsigned)((bad ? 0 : (int)idx) + 70560000);   // 12 * 5880000: never negative
  const int year = (int)(ui / 12u) - 5880000, month = (int)(ui % 12u) + 1;
  const int len = tg_date_month_length(tg_date_is_leap(year), month);
  const int r = tg_date_checked(tg_date_days(year, month, c.day < len ? c.day : len), overflow);
  return bad ? 0 : r;
}

// date_add(unit, value, days).  A value outside int32 and a result outside int32 days set *overflow.
TG_DATE_FN int tg_date_add(int unit, long long value, int days, int *overflow)
{
  const int bad = value < -2147483648LL || value > 2147483647LL;
  *overflow |= bad;
  const long long v = bad ? 0 : value;
  int r;
  if (unit == TG_DATE_UNIT_DAY) r = tg_date_checked((long long)days + v, overflow);
  else if (unit == TG_DATE_UNIT_WEEK) r = tg_date_checked((long long)days + 7 * v, overflow);
  else r = tg_date_add_months(days, unit == TG_DATE_UNIT_MONTH ? v : unit == TG_DATE_UNIT_QUARTER ? 3 * v : 12 * v, overflow);
  return bad ? 0 : r;
}

// The whole months from d1 to d2: for d2 >= d1 the largest n >= 0 with tg_date_add_months(d1, n) <= d2, for d2 < d1 the negated count from
// d2 to d1.  Closed form: the months-index difference, less one when the clamped day of the earlier date is past the later date's day.
TG_DATE_FN int tg_date_diff_months(int d1, int d2)
{
  const int swap = d2 < d1;
  const tg_civil a = tg_date_civil(swap ? d2 : d1), b = tg_date_civil(swap ? d1 : d2);
  const int len = tg_date_month_length(b.leap, b.month);
  const int n = (b.year - a.year) * 12 + (b.month - a.month) - ((a.day < len ? a.day : len) > b.day);
  return swap ? -n : n;
}

// date_diff(unit, d1, d2); quarters and years are whole multiples of months (adding months is monotone in their number)
TG_DATE_FN long long tg_date_diff(int unit, int d1, int d2)
{
  if (unit == TG_DATE_UNIT_DAY) return (long long)d2 - (long long)d1;
  if (unit == TG_DATE_UNIT_WEEK) {
    const int swap = d2 < d1;
    const unsigned w = (swap ? (unsigned)d1 - (unsigned)d2 : (unsigned)d2 - (unsigned)d1) / 7u;
    return swap ? -(long long)w : (long long)w;
  }
  const int n = tg_date_diff_months(d1, d2);
  return unit == TG_DATE_UNIT_MONTH ? n : unit == TG_DATE_UNIT_QUARTER ? n / 3 : n / 12;
}
#endif

// Arithmetic of the math functions (TGPU_OP_ABS .. TGPU_OP_RADIANS, include/tgpu.h) that is more than one expression: Java's Math.round, the
// two-argument round over DOUBLE and over integers, signum, truncate and the Math.pow special cases that C's pow answers differently.
//
// This text has no #include: it is embedded as it stands into the JIT sources (jit.cpp device_header("device_math.h"), where hiprtc has no libc
// headers) and compiled as it stands by a host program (tests/math_fn/math_main.cpp) that checks it on the CPU under ASan and UBSan.  floor, fabs,
// pow and fma are the device library's double functions under hiprtc and <math.h>'s on the host, which includes that first.  Every function is
// declared through TG_MATH_FN.  No table in memory; nothing overflows a signed type, and no double outside the target's range is converted to
// an integer.
#ifndef TG_MATH_HELPERS
#define TG_MATH_HELPERS
#if defined(__HIPCC_RTC__) || defined(__HIP_DEVICE_COMPILE__)
#define TG_MATH_FN static __device__ __forceinline__
#else
#define TG_MATH_FN static inline
#endif

#define TG_I64_MIN (-9223372036854775807LL - 1)
#define TG_I64_MAX 9223372036854775807LL

// Math.round(double): floor(x + 1/2) computed exactly, as a long; saturates at the int64 ends, NaN gives 0.  x + 0.5 is never formed in
// floating point (0.49999999999999994 + 0.5 rounds to 1.0): below 2^52 x - floor(x) is exact, from 2^52 on x is integral.
TG_MATH_FN long long tg_jround(double x)
{
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return TG_I64_MAX;
  if (x <= -9223372036854775808.0) return TG_I64_MIN;
  if (fabs(x) >= 4503599627370496.0) return (long long)x;
  const double f = floor(x);
  return (long long)f + (x - f >= 0.5 ? 1 : 0);
}

// round(x, d) over DOUBLE (MathFunctions.java:821-833) with factor = 10^d: NaN and the infinities as they are; the magnitude is rounded and
// the sign put back, so halves go away from zero and -0.3 gives -0.0 while -0.0 gives +0.0 (it is not < 0).
TG_MATH_FN double tg_round_double(double x, double factor)
{
  if (x != x || x - x != 0.0) return x;
  if (x < 0) return -((double)tg_jround(-x * factor) / factor);
  return (double)tg_jround(x * factor) / factor;
}

// roundLong :787-800 for -18 <= d < 0 with factor = 10^-d: num / factor rounded half away from zero (RoundingMode.HALF_UP), times factor.
// *overflow = 1 when the product leaves int64 (the reference's multiplyExact).  |remainder| < 10^18, so doubling it stays inside int64.
TG_MATH_FN long long tg_round_long(long long num, long long factor, int *overflow)
{
  long long q = num / factor;
  const long long r = num % factor;
  const long long twice = r < 0 ? -2 * r : 2 * r;
  if (twice >= factor) q += num < 0 ? -1 : 1;
  long long out = 0;
  if (__builtin_mul_overflow(q, factor, &out)) *overflow = 1;
  return out;
}

// Math.signum: NaN gives NaN, a zero keeps its sign
TG_MATH_FN double tg_signum(double x) { return (x != x || x == 0.0) ? x : (x < 0 ? -1.0 : 1.0); }

// truncate :315-320: signum(x) * floor(abs(x)); -0.5 gives -0.0, NaN and the infinities pass through
TG_MATH_FN double tg_truncate(double x) { return tg_signum(x) * floor(fabs(x)); }

// Math.pow.  Where it differs from C's pow: a NaN exponent gives NaN also for base 1, and (+-1) ^ (+-inf) is NaN.  x ^ (+-0) is 1 in both.
// An integral exponent up to 2^10 in magnitude is first tried by squaring, each product tested for exactness with an fma residual: when
// every product is exact the power is (for y > 0) the mathematical value, which Math.pow promises where it is representable, and for y < 0
// the one correctly rounded reciprocal of it.  A product below 2^-960 is not trusted (its residual could underflow to zero); anything
// inexact falls through to the library's pow.  x ^ 2 is the single correctly rounded product.
TG_MATH_FN double tg_pow(double x, double y)
{
  if (y == 0.0) return 1.0;
  if (y != y || x != x) return x + y;
  const bool y_inf = y - y != 0.0;
  if (y_inf && fabs(x) == 1.0) return y - y;
  if (y == 2.0) return x * x;   // one product: correctly rounded
  if (!y_inf && fabs(y) <= 1024.0 && floor(y) == y && x - x == 0.0 && x != 0.0) {
    int e = (int)fabs(y);
    double b = x, r = 1.0;
    bool exact = true;
    while (true) {
      if (e & 1) {
        const double p = r * b;
        exact = fabs(p) >= 1e-289 && fma(r, b, -p) == 0.0;
        r = p;
      }
      e >>= 1;
      if (!exact || e == 0) break;
      const double s = b * b;
      exact = fabs(s) >= 1e-289 && fma(b, b, -s) == 0.0;
      b = s;
      if (!exact) break;
    }
    if (exact) return y < 0 ? 1.0 / r : r;
  }
  return pow(x, y);
}

#endif

"""Expected values of the math functions (TGPU_OP_ABS .. TGPU_OP_RADIANS): a plain Python model of the rules in include/tgpu.h, written from
M/operator/scalar/MathFunctions.java and the java.lang.Math contract with Python ints, math, struct and fractions.  It shares no code with the
product; the tests compare the product with it, never the other way round.

None is NULL; the first NULL argument gives NULL.  A row that fails raises OutOfRange with the reference's message."""
import math
import struct
from fractions import Fraction

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
NAN, INF = float("nan"), float("inf")
TO_DEGREES, TO_RADIANS = 57.29577951308232, 0.017453292519943295   # JDK 9+: Math.toDegrees / toRadians are one multiplication
LN2 = math.log(2.0)
BOUNDED = ("cbrt", "exp", "ln", "log10", "power", "log2", "log")
EXACT_UNARY_DOUBLE = ("abs", "sign", "floor", "ceiling", "truncate", "round", "sqrt", "degrees", "radians")


class OutOfRange(Exception):
    """NUMERIC_VALUE_OUT_OF_RANGE; str(e) is the reference's message"""


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def same(a, b):
    """bit for bit, except that any NaN equals any NaN; None equals None"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or bits(a) == bits(b)
    return type(a) is type(b) and a == b


def ordinal(x):
    """a monotone integer over the doubles: neighbours differ by 1, -0.0 and +0.0 are both 0"""
    b = bits(x)
    return -(b & (2**63 - 1)) if b >> 63 else b


def ulp_distance(got, truth):
    """how many doubles lie between `got` and `truth`, in steps: 0 = the same double.  NaN matches NaN only; an infinity or a zero matches
    only itself with the same sign (-> 0, else infinity)"""
    if truth != truth or got != got:
        return 0 if (truth != truth and got != got) else INF
    if math.isinf(truth) or math.isinf(got) or truth == 0.0:
        return 0 if bits(got) == bits(truth) else INF
    return abs(ordinal(got) - ordinal(truth))


# ---- Math.round and the exact group --------------------------------------------------------------------------------------------------------
def jround(x):
    """Math.round(double): floor(x + 1/2) exactly, as a long; saturates; NaN -> 0"""
    if x != x:
        return 0
    if math.isinf(x):
        return INT64_MAX if x > 0 else INT64_MIN
    return max(INT64_MIN, min(INT64_MAX, math.floor(Fraction(x) + Fraction(1, 2))))


def decimal_power(d):
    """the correctly rounded double of the decimal 1e<d> (Python's float() rounds correctly); +inf above 308, 0 below -323"""
    return float("1e%d" % d)


def abs_(x, integer_type=None):
    if x is None:
        return None
    if isinstance(x, float):
        return from_bits(bits(x) & (2**63 - 1))
    if integer_type == "integer" and x == INT32_MIN:
        raise OutOfRange("Value -2147483648 is out of range for abs(integer)")
    if integer_type != "integer" and x == INT64_MIN:
        raise OutOfRange("Value -9223372036854775808 is out of range for abs(bigint)")
    return -x if x < 0 else x


def sign(x):
    if x is None:
        return None
    if isinstance(x, float):
        return x if (x != x or x == 0.0) else math.copysign(1.0, x)
    return (x > 0) - (x < 0)


def _float_integral(x, fn):
    """Math.floor / Math.ceil: NaN, the infinities and zeros as they are; a result of zero keeps the argument's sign"""
    if x != x or math.isinf(x) or x == 0.0:
        return x
    return math.copysign(float(fn(Fraction(x))), x)


def floor(x):
    if x is None:
        return None
    return _float_integral(x, math.floor) if isinstance(x, float) else x


def ceiling(x):
    if x is None:
        return None
    return _float_integral(x, math.ceil) if isinstance(x, float) else x


def truncate(x):
    """signum(x) * floor(abs(x))"""
    if x is None:
        return None
    if x != x or math.isinf(x) or x == 0.0:
        return x
    return math.copysign(float(math.floor(abs(Fraction(x)))), x)


def round_long(num, d, integer_type=None):
    """roundLong: the identity for d >= 0; else num / 10^-d rounded half away from zero, times 10^-d, checked"""
    if d >= 0:
        return num
    overflow = OutOfRange("numerical overflow: %d" % num)
    if -d > 18:                                     # LongMath.checkedPow(10, -d) overflows: whatever num is
        raise overflow
    factor = 10 ** -d
    q, r = divmod(abs(num), factor)
    if 2 * r >= factor:
        q += 1
    out = (-q if num < 0 else q) * factor
    lo, hi = (INT32_MIN, INT32_MAX) if integer_type == "integer" else (INT64_MIN, INT64_MAX)
    if not lo <= out <= hi:
        raise overflow
    return out


def _div(a, b):
    """IEEE double division"""
    if a != a or b != b:
        return NAN
    if b == 0.0:
        return NAN if a == 0.0 else math.copysign(INF, a) * math.copysign(1.0, b)
    if math.isinf(a):
        return NAN if math.isinf(b) else a * math.copysign(1.0, b)
    return a / b


def _mul(a, b):
    return a * b          # Python's float product is the IEEE one, NaN and infinities included


def round_double(x, d=0):
    if x != x or math.isinf(x):
        return x
    factor = decimal_power(d)
    if x < 0:
        return -_div(float(jround(_mul(-x, factor))), factor)
    return _div(float(jround(_mul(x, factor))), factor)


def round_(x, d=0, integer_type=None):
    if x is None or d is None:
        return None
    return round_double(x, d) if isinstance(x, float) else round_long(x, d, integer_type)


def sqrt(x):
    if x is None:
        return None
    if x != x or x < 0:
        return NAN
    return x if (x == 0.0 or math.isinf(x)) else math.sqrt(x)      # IEEE: correctly rounded


def is_nan(x): return None if x is None else x != x
def is_finite(x): return None if x is None else not (x != x or math.isinf(x))
def is_infinite(x): return None if x is None else math.isinf(x)
def degrees(x): return None if x is None else x * TO_DEGREES
def radians(x): return None if x is None else x * TO_RADIANS


# ---- the bounded group: special cases exactly, finite results from the host's libm (the tests bound its error by the corpus) -------------------
def _log_with(fn, x):
    if x != x or x < 0:
        return NAN
    if x == 0.0:
        return -INF
    return INF if math.isinf(x) else fn(x)


def ln(x): return None if x is None else _log_with(math.log, x)
def log10(x): return None if x is None else _log_with(math.log10, x)
def log2(x): return None if x is None else _div(ln(x), LN2)


def log(b, x):
    """log(b, x) = ln(x) / ln(b): the base comes first"""
    if b is None or x is None:
        return None
    return _div(ln(x), ln(b))


def exp(x):
    if x is None:
        return None
    if x != x:
        return NAN
    if math.isinf(x):
        return INF if x > 0 else 0.0
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def cbrt(x):
    if x is None:
        return None
    if x != x or math.isinf(x) or x == 0.0:
        return x
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.cbrt.restype, libm.cbrt.argtypes = ctypes.c_double, [ctypes.c_double]
    return libm.cbrt(x)


def is_odd_integer(y):
    return not math.isinf(y) and y == math.floor(y) and abs(y) < 2.0**53 and int(y) % 2 == 1


def power_special(x, y):
    """Math.pow's list of special cases -> the result, or None when (x, y) is an ordinary case"""
    if y == 0.0:
        return 1.0
    if y != y or x != x:
        return NAN
    ax = abs(x)
    if math.isinf(y):
        if ax == 1.0:
            return NAN
        return INF if (ax > 1.0) == (y > 0) else 0.0
    if x == 0.0 or math.isinf(x):
        grows = (x == 0.0) == (y < 0)                          # 0 ^ negative and inf ^ positive are infinite
        negative = math.copysign(1.0, x) < 0 and is_odd_integer(y)
        return math.copysign(INF if grows else 0.0, -1.0 if negative else 1.0)
    if x < 0 and y != math.floor(y):
        return NAN
    return None


def exact_power(x, y):
    """x ^ y as a Fraction when y is integral, else None"""
    if math.isinf(y) or math.isinf(x) or x != x or y != y or y != math.floor(y) or x == 0.0 or abs(y) > 4096:
        return None
    return Fraction(x) ** int(y)


def as_exact_double(q):
    """the double that equals the Fraction q, or None"""
    try:
        f = float(q)
    except OverflowError:
        return None
    return f if (not math.isinf(f) and Fraction(f) == q) else None


def power(x, y):
    if x is None or y is None:
        return None
    s = power_special(x, y)
    if s is not None:
        return s
    q = exact_power(x, y)
    if q is not None:
        f = as_exact_double(q)
        if f is not None:
            return f
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.copysign(INF, -1.0 if (x < 0 and is_odd_integer(y)) else 1.0)


UNARY = {"abs": abs_, "sign": sign, "floor": floor, "ceiling": ceiling, "truncate": truncate, "round": round_, "sqrt": sqrt, "cbrt": cbrt, "exp": exp,
         "ln": ln, "log2": log2, "log10": log10, "is_nan": is_nan, "is_finite": is_finite, "is_infinite": is_infinite, "degrees": degrees, "radians": radians}
BINARY = {"log": log, "power": power}

"""The string functions and the casts to VARCHAR restated in plain Python over `bytes`, following the reference line by line
(M/operator/scalar/StringFunctions.java: length :94-100, stringPosition :205-247, substring :274-309 and :321-367, startsWith :909-915;
ConcatFunction.java; M/type/BigintOperators.java:198-205, IntegerOperators.java:170, BooleanOperators.java:82).  None is SQL NULL.

Code points follow the rule of include/tgpu.h: one starts at every byte b with (b & 0xC0) != 0x80.  On well-formed UTF-8 that is airlift's
SliceUtf8; on malformed bytes the reference's answer is not pinned by anything under its tree.  Python's ints do not overflow, so the
negative-start branch of substring gives the suffix where the reference's int addition (:359) overflows: the deviation the header states."""

INT_MAX, INT_MIN = 2**31 - 1, -2**31
TOO_LARGE = "Concatenated string is too large"


class StringFunctionError(Exception):
    pass


def saturated_cast(x):   # Ints.saturatedCast
    return INT_MAX if x > INT_MAX else INT_MIN if x < INT_MIN else x


def is_start(b):
    return (b & 0xC0) != 0x80


def count_code_points(v, lo=0, hi=None):   # SliceUtf8.countCodePoints
    return sum(1 for b in v[lo:len(v) if hi is None else hi] if is_start(b))


def offset_of_code_point(v, position, count):
    """SliceUtf8.offsetOfCodePoint: the offset of code point `count` (from 0) among those that start at or after `position`, -1 if there
    are no more than `count` of them"""
    for i in range(position, len(v)):
        if is_start(v[i]):
            if count == 0:
                return i
            count -= 1
    return -1


def length(v):
    return None if v is None else count_code_points(v)


def substring(v, start, length=None, has_length=False):
    if v is None or start is None or (has_length and length is None):
        return None
    if start == 0 or (has_length and length <= 0) or len(v) == 0:
        return b""
    start_cp = saturated_cast(start)
    length_cp = saturated_cast(length) if has_length else None
    if start_cp > 0:
        index_start = offset_of_code_point(v, 0, start_cp - 1)
        if index_start < 0:
            return b""          # before beginning of string (the reference's comment; it is past the end)
        index_end = len(v)
        if has_length:
            index_end = offset_of_code_point(v, index_start, length_cp)
            if index_end < 0:
                index_end = len(v)   # after end of string
        return v[index_start:index_end]
    code_points = count_code_points(v)
    start_cp += code_points
    if start_cp < 0:
        return b""
    index_start = offset_of_code_point(v, 0, start_cp)
    if has_length and start_cp + length_cp < code_points:
        index_end = offset_of_code_point(v, index_start, length_cp)
    else:
        index_end = len(v)
    return v[index_start:index_end]


def concat(a, b):
    if a is None or b is None:
        return None
    if len(a) + len(b) > INT_MAX:
        raise StringFunctionError(TOO_LARGE)
    return a + b


def strpos(v, sub):
    if v is None or sub is None:
        return None
    if len(sub) == 0:
        return 1
    index = v.find(sub)          # Slice.indexOf: a byte search
    if index < 0:
        return 0
    return count_code_points(v, 0, index) + 1


def starts_with(v, prefix):
    if v is None or prefix is None:
        return None
    return len(prefix) <= len(v) and v[:len(prefix)] == prefix


def cast_integer(x):     # String.valueOf(long / int)
    return None if x is None else str(int(x)).encode()


def cast_boolean(x):
    return None if x is None else (b"true" if x else b"false")


def column(fn, *cols):
    """fn over rows; an argument that is no list is a constant"""
    n = max(len(c) for c in cols if isinstance(c, list))
    return [fn(*[c[i] if isinstance(c, list) else c for c in cols]) for i in range(n)]


def substr_column(values, start, length=None, has_length=False):
    return column(lambda v, s, l: substring(v, s, l, has_length), values, start, length)

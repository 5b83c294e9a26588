"""What LIKE and IN must give: an independent restatement of the reference in plain Python, shared by the LIKE / IN tests.

LIKE restates LikeFunctions.likePattern (M/type/LikeFunctions.java:198-241): the pattern is walked one UTF-16 unit at a time with the
`escaped` flag, the checkEscape points and the empty-escape rule of getEscapeChar (:244-255), and written out as a regular expression
that Python's `re` runs with DOTALL and fullmatch over the decoded value ('_' = `.` = one code point; the whole value must match).
IN restates InCodeGenerator (M/sql/gen/InCodeGenerator.java:92-121) with the type's EQUAL operator."""
import math
import re

ESCAPE_LENGTH = "Escape string must be a single character"
ESCAPE_FOLLOW = "Escape character must be followed by '%', '_' or the escape character itself"


class LikeError(ValueError):
    pass


def _utf16_units(s):
    b = s.encode("utf-16-le", "surrogatepass")
    return [int.from_bytes(b[i:i + 2], "little") for i in range(0, len(b), 2)]


def _units_to_str(units):
    return b"".join(u.to_bytes(2, "little") for u in units).decode("utf-16-le", "surrogatepass")


def like_regex(pattern, escape=None):
    """the compiled expression of `pattern` [ESCAPE `escape`]; raises LikeError with the reference's message"""
    should_escape = escape is not None
    escape_unit = ord("0")
    if should_escape:
        units = _utf16_units(escape)
        if len(units) == 0:
            escape_unit = 0xFFFF   # (char) -1: escaping disabled
        elif len(units) == 1:
            escape_unit = units[0]
        else:
            raise LikeError(ESCAPE_LENGTH)
    out = []
    literal = []   # UTF-16 units of the literal run being collected (a surrogate pair must be re-joined before re.escape)

    def flush():
        if literal:
            out.append(re.escape(_units_to_str(literal)))
            literal.clear()

    escaped = False
    for cur in _utf16_units(pattern):
        if escaped and cur not in (ord("%"), ord("_"), escape_unit):
            raise LikeError(ESCAPE_FOLLOW)
        if should_escape and not escaped and cur == escape_unit:
            escaped = True
            continue
        if cur == ord("%") and not escaped:
            flush()
            out.append(".*")
        elif cur == ord("_") and not escaped:
            flush()
            out.append(".")
        else:
            literal.append(cur)
        escaped = False
    if escaped:
        raise LikeError(ESCAPE_FOLLOW)
    flush()
    return re.compile("".join(out), re.DOTALL)


def like(value, pattern, escape=None, has_escape=None):
    """three-valued `value LIKE pattern [ESCAPE escape]`; value: str, bytes (valid UTF-8) or None.  A null escape needs
    has_escape=True (escape=None alone means: no ESCAPE clause)"""
    if has_escape is None:
        has_escape = escape is not None
    if pattern is None or (has_escape and escape is None):
        return None
    rx = like_regex(pattern, escape if has_escape else None)   # the pattern is compiled (and may raise) before any value is seen
    if value is None:
        return None
    if isinstance(value, (bytes, bytearray)):
        value = bytes(value).decode("utf-8")
    return rx.fullmatch(value) is not None


def like_column(values, pattern, escape=None, has_escape=None):
    return [like(v, pattern, escape, has_escape) for v in values]


def _equal(a, b):
    if isinstance(a, float) or isinstance(b, float):
        a, b = float(a), float(b)
        if math.isnan(a) or math.isnan(b):
            return False
        return a == b   # -0.0 == +0.0
    if isinstance(a, str):
        a = a.encode("utf-8")
    if isinstance(b, str):
        b = b.encode("utf-8")
    return a == b


def in_list(value, items):
    """three-valued `value IN (items)`"""
    if value is None:
        return None
    if any(i is not None and _equal(value, i) for i in items):
        return True
    return None if any(i is None for i in items) else False


def in_column(values, items):
    return [in_list(v, items) for v in values]


# ---- the helpers of LikeFunctions the optimizer uses (:120-190): restated so that every case of TestLikeFunctions has a counterpart ----
def _escape_character(escape):
    """getEscapeCharacter :181-190 (escape None = Optional.empty())"""
    if escape is None:
        return -1
    if len(_utf16_units(escape)) != 1:
        raise LikeError(ESCAPE_LENGTH)
    return ord(escape)


def pattern_constant_prefix_bytes(pattern, escape=None):
    esc = _escape_character(escape)
    escaped, position = False, 0
    for ch in pattern:
        cur = ord(ch)
        if not escaped and cur == esc:
            escaped = True
        elif escaped:
            if cur not in (ord("%"), ord("_"), esc):
                raise LikeError(ESCAPE_FOLLOW)
            escaped = False
        elif ch in "%_":
            return position
        position += len(ch.encode("utf-8"))
    if escaped:
        raise LikeError(ESCAPE_FOLLOW)
    return position


def is_like_pattern(pattern, escape=None):
    return pattern_constant_prefix_bytes(pattern, escape) < len(pattern.encode("utf-8"))


def unescape_literal_like_pattern(pattern, escape=None):
    if escape is None:
        return pattern
    esc = _escape_character(escape)
    out, escaped = [], False
    for ch in pattern:
        if not escaped and ord(ch) == esc:
            escaped = True
        else:
            out.append(ch)
            escaped = False
    if escaped:
        raise LikeError(ESCAPE_FOLLOW)
    return "".join(out)

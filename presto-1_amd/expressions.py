"""RowExpression IR: the input language of the GPU page-processor compiler.

Mirrors io.trino.sql.relational.{InputReferenceExpression, ConstantExpression, CallExpression, SpecialForm}
(M/sql/relational/*.java; forms: SpecialForm.java:137-152).  `a > b` is kept as GREATER_THAN here; the reference's
translator rewrites it to `b < a` (SqlToRowExpressionTranslator.java:317-320), which is equivalent for the types supported.
"""
import ctypes as C

from . import _lib
from .spi import BIGINT, BOOLEAN, DATE, DOUBLE, INTEGER, TIMESTAMP, VARCHAR

EX_INPUT, EX_CONST, EX_CALL, EX_SPECIAL = 0, 1, 2, 3
OPS = {"ADD": 1, "SUBTRACT": 2, "MULTIPLY": 3, "DIVIDE": 4, "MODULUS": 5, "NEGATE": 6, "EQUAL": 7, "NOT_EQUAL": 8,
       "LESS_THAN": 9, "LESS_THAN_OR_EQUAL": 10, "GREATER_THAN": 11, "GREATER_THAN_OR_EQUAL": 12, "NOT": 13, "CAST": 14, "LIKE": 15,
       "LENGTH": 16, "SUBSTR": 17, "CONCAT": 18, "STRPOS": 19, "STARTS_WITH": 20,
       "YEAR": 21, "QUARTER": 22, "MONTH": 23, "WEEK": 24, "DAY": 25, "DAY_OF_WEEK": 26, "DAY_OF_YEAR": 27, "YEAR_OF_WEEK": 28,
       "LAST_DAY_OF_MONTH": 29, "DATE_TRUNC": 30, "DATE_ADD": 31, "DATE_DIFF": 32,
       "ABS": 33, "SIGN": 34, "FLOOR": 35, "CEILING": 36, "TRUNCATE": 37, "ROUND": 38, "SQRT": 39, "CBRT": 40, "EXP": 41, "LN": 42, "LOG2": 43,
       "LOG10": 44, "LOG": 45, "POWER": 46, "IS_NAN": 47, "IS_FINITE": 48, "IS_INFINITE": 49, "DEGREES": 50, "RADIANS": 51,
       "HOUR": 52, "MINUTE": 53, "SECOND": 54, "MILLISECOND": 55, "TO_UNIXTIME": 56}
FORMS = {"AND": 1, "OR": 2, "IF": 3, "IS_NULL": 4, "COALESCE": 5, "BETWEEN": 6, "IN": 7}
_CMP = {"EQUAL", "NOT_EQUAL", "LESS_THAN", "LESS_THAN_OR_EQUAL", "GREATER_THAN", "GREATER_THAN_OR_EQUAL"}


class RowExpression:
    type = None

    # small builder sugar so tests read like SQL
    def __add__(self, o): return call("ADD", self.type, self, _wrap(o, self.type))
    def __sub__(self, o): return call("SUBTRACT", self.type, self, _wrap(o, self.type))
    def __mul__(self, o): return call("MULTIPLY", self.type, self, _wrap(o, self.type))
    def __truediv__(self, o): return call("DIVIDE", self.type, self, _wrap(o, self.type))
    def __mod__(self, o): return call("MODULUS", self.type, self, _wrap(o, self.type))
    def __neg__(self): return call("NEGATE", self.type, self)
    def __lt__(self, o): return call("LESS_THAN", BOOLEAN, self, _wrap(o, self.type))
    def __le__(self, o): return call("LESS_THAN_OR_EQUAL", BOOLEAN, self, _wrap(o, self.type))
    def __gt__(self, o): return call("GREATER_THAN", BOOLEAN, self, _wrap(o, self.type))
    def __ge__(self, o): return call("GREATER_THAN_OR_EQUAL", BOOLEAN, self, _wrap(o, self.type))
    def eq(self, o): return call("EQUAL", BOOLEAN, self, _wrap(o, self.type))
    def ne(self, o): return call("NOT_EQUAL", BOOLEAN, self, _wrap(o, self.type))


class InputReferenceExpression(RowExpression):
    def __init__(self, field, type_id):
        self.field, self.type = field, type_id


class ConstantExpression(RowExpression):
    def __init__(self, value, type_id):
        self.value, self.type = value, type_id


class CallExpression(RowExpression):
    def __init__(self, name, type_id, arguments, ival=0):
        assert name in OPS, name
        self.name, self.type, self.arguments = name, type_id, list(arguments)
        self.ival = ival   # the node's ival: the precision of a TIMESTAMP date_add / cast, unused otherwise


class SpecialForm(RowExpression):
    def __init__(self, form, type_id, arguments, items=None):
        assert form in FORMS, form
        self.form, self.type, self.arguments = form, type_id, list(arguments)
        self.items = None if items is None else list(items)   # IN: the list, constants of the value's type


def _wrap(v, type_id):
    return v if isinstance(v, RowExpression) else ConstantExpression(v, type_id)


def field(channel, type_id):
    return InputReferenceExpression(channel, type_id)


def constant(value, type_id):
    return ConstantExpression(value, type_id)


def call(name, type_id, *args):
    return CallExpression(name, type_id, args)


def and_(a, b): return SpecialForm("AND", BOOLEAN, [a, b])
def or_(a, b): return SpecialForm("OR", BOOLEAN, [a, b])
def not_(a): return call("NOT", BOOLEAN, a)
def is_null(a): return SpecialForm("IS_NULL", BOOLEAN, [a])
def if_(c, t, f): return SpecialForm("IF", t.type, [c, t, f])
def coalesce(*args): return SpecialForm("COALESCE", args[0].type, [_wrap(a, args[0].type) for a in args])
def between(v, lo, hi): return SpecialForm("BETWEEN", BOOLEAN, [v, _wrap(lo, v.type), _wrap(hi, v.type)])


def cast(a, type_id, precision=6):
    """CAST(a AS type); precision: the target's p of a CAST(timestamp AS timestamp(p)), 0..6 (the value is rounded to it)"""
    return CallExpression("CAST", type_id, [a], ival=precision if type_id == TIMESTAMP and a.type == TIMESTAMP else 0)


def like(value, pattern, escape=None):
    """value LIKE pattern [ESCAPE escape]; pattern / escape: a str (None = the null literal) or a VARCHAR expression, which must be a constant"""
    args = [value, _wrap(pattern, VARCHAR)]
    if escape is not None:
        args.append(_wrap(escape, VARCHAR))
    return call("LIKE", BOOLEAN, *args)


def in_(value, items):
    """value IN (items); an item is a Python value (None = the null literal) or a constant of the value's type"""
    return SpecialForm("IN", BOOLEAN, [value], [_wrap(i, value.type) for i in items])


def length(x):
    """length(x): the code points of a VARCHAR value"""
    return call("LENGTH", BIGINT, _wrap(x, VARCHAR))


def substr(x, start, length=None):
    """substr(x, start[, length]): positions in code points from 1, a negative start counts from the end"""
    args = [_wrap(x, VARCHAR), _wrap(start, BIGINT)]
    if length is not None:
        args.append(_wrap(length, BIGINT))
    return call("SUBSTR", VARCHAR, *args)


def concat(*args):
    """concat(a, b, ...): two or more VARCHAR arguments, nested to the left as the IR's CONCAT takes two"""
    if len(args) < 2:
        raise ValueError("There must be two or more concatenation arguments")
    r = _wrap(args[0], VARCHAR)
    for a in args[1:]:
        r = call("CONCAT", VARCHAR, r, _wrap(a, VARCHAR))
    return r


def strpos(x, sub):
    """strpos(x, sub): the code-point index from 1 of the first occurrence of sub, 0 if there is none"""
    return call("STRPOS", BIGINT, _wrap(x, VARCHAR), _wrap(sub, VARCHAR))


def starts_with(x, prefix):
    return call("STARTS_WITH", BOOLEAN, _wrap(x, VARCHAR), _wrap(prefix, VARCHAR))


# DATE functions: extraction gives BIGINT; a Python int stands for a DATE constant (days since 1970-01-01), None for the null literal.
# Every one of them takes a TIMESTAMP expression (field(ch, TIMESTAMP), constant(us, TIMESTAMP)) in the DATE argument's place as well.
def _date_like(d):
    """the DATE / TIMESTAMP argument, and its type"""
    d = _wrap(d, DATE)
    return d, (TIMESTAMP if d.type == TIMESTAMP else DATE)


def year(d): return call("YEAR", BIGINT, _date_like(d)[0])
def quarter(d): return call("QUARTER", BIGINT, _date_like(d)[0])
def month(d): return call("MONTH", BIGINT, _date_like(d)[0])
def week(d): return call("WEEK", BIGINT, _date_like(d)[0])
def day(d): return call("DAY", BIGINT, _date_like(d)[0])
def day_of_week(d): return call("DAY_OF_WEEK", BIGINT, _date_like(d)[0])
def day_of_year(d): return call("DAY_OF_YEAR", BIGINT, _date_like(d)[0])
def year_of_week(d): return call("YEAR_OF_WEEK", BIGINT, _date_like(d)[0])
def last_day_of_month(d): return call("LAST_DAY_OF_MONTH", DATE, _date_like(d)[0])


def date_trunc(unit, d):
    """date_trunc(unit, d); unit: 'day', 'week', 'month', 'quarter' or 'year' -- for a TIMESTAMP also 'millisecond', 'second', 'minute' and
    'hour' -- in any case (a str, None = the null literal), a constant.  The result has d's type"""
    d, t = _date_like(d)
    return call("DATE_TRUNC", t, _wrap(unit, VARCHAR), d)


def date_add(unit, value, d, precision=6):
    """date_add(unit, value, d): value a BIGINT expression or a Python int; months clamp the day of the month to the target month.
    precision: the p of a timestamp(p) argument, 0..6 (for p <= 3 the reference rounds the millisecond result to it)"""
    d, t = _date_like(d)
    return CallExpression("DATE_ADD", t, [_wrap(unit, VARCHAR), _wrap(value, BIGINT), d], ival=precision if t == TIMESTAMP else 0)


def date_diff(unit, d1, d2):
    """date_diff(unit, d1, d2): the whole units from d1 to d2, negative when d2 < d1; two DATEs or two TIMESTAMPs"""
    d1, t = _date_like(d1)
    return call("DATE_DIFF", BIGINT, _wrap(unit, VARCHAR), d1, _wrap(d2, t))


# TIMESTAMP functions: int64 microseconds since 1970-01-01 00:00:00 UTC; a Python int stands for a TIMESTAMP constant
def hour(t): return call("HOUR", BIGINT, _wrap(t, TIMESTAMP))
def minute(t): return call("MINUTE", BIGINT, _wrap(t, TIMESTAMP))
def second(t): return call("SECOND", BIGINT, _wrap(t, TIMESTAMP))
def millisecond(t): return call("MILLISECOND", BIGINT, _wrap(t, TIMESTAMP))
def to_unixtime(t): return call("TO_UNIXTIME", DOUBLE, _wrap(t, TIMESTAMP))


# Math functions.  abs_ / sign / floor / ceiling / round_ keep the argument's type (BIGINT, INTEGER or DOUBLE); a Python float stands for a DOUBLE
# constant, a Python int for a BIGINT one; every other function is over DOUBLE, where Python ints and floats both become DOUBLE constants.
def _numeric(x):
    if isinstance(x, RowExpression):
        return x
    return ConstantExpression(x, BIGINT if isinstance(x, int) and not isinstance(x, bool) else DOUBLE)


def _same(name, x):
    x = _numeric(x)
    return call(name, x.type, x)


def _double(name, *args):
    return call(name, DOUBLE, *[_wrap(a, DOUBLE) for a in args])


def abs_(x): return _same("ABS", x)
def sign(x): return _same("SIGN", x)
def floor(x): return _same("FLOOR", x)
def ceiling(x): return _same("CEILING", x)
def truncate(x): return _double("TRUNCATE", x)


def round_(x, decimals=None):
    """round(x) or round(x, decimals); decimals: a Python int or an INTEGER constant (the null literal: constant(None, INTEGER))"""
    x = _numeric(x)
    return call("ROUND", x.type, x) if decimals is None else call("ROUND", x.type, x, _wrap(decimals, INTEGER))


def sqrt(x): return _double("SQRT", x)
def cbrt(x): return _double("CBRT", x)
def exp(x): return _double("EXP", x)
def ln(x): return _double("LN", x)
def log2(x): return _double("LOG2", x)
def log10(x): return _double("LOG10", x)


def log(b, x):
    """log(b, x): the logarithm of x to the base b, ln(x) / ln(b)"""
    return _double("LOG", b, x)


def power(x, y): return _double("POWER", x, y)
def is_nan(x): return call("IS_NAN", BOOLEAN, _wrap(x, DOUBLE))
def is_finite(x): return call("IS_FINITE", BOOLEAN, _wrap(x, DOUBLE))
def is_infinite(x): return call("IS_INFINITE", BOOLEAN, _wrap(x, DOUBLE))
def degrees(x): return _double("DEGREES", x)
def radians(x): return _double("RADIANS", x)


ceil = ceiling
pow_ = power


class FlatProgram:
    """A filter + projections flattened into one node array (the serialisation the C ABI takes)."""

    def __init__(self, filter_expr, projections):
        self.nodes = []  # plain dicts: the serialisable form of the program
        self.pool = bytearray()
        self.filter_root = -1 if filter_expr is None else self._add(filter_expr)
        self.projection_roots = [self._add(p) for p in projections]

    def _add(self, e):
        if isinstance(e, InputReferenceExpression):
            nd = dict(kind=EX_INPUT, type=e.type, op=e.field, args=[])
        elif isinstance(e, ConstantExpression):
            nd = dict(kind=EX_CONST, type=e.type, op=0, args=[], is_null=int(e.value is None))
            if e.value is not None:
                if e.type == DOUBLE:
                    nd["dval"] = float(e.value)
                elif e.type == VARCHAR:
                    b = e.value.encode("utf-8") if isinstance(e.value, str) else bytes(e.value)
                    nd["ival"], nd["slen"] = len(self.pool), len(b)
                    self.pool += b
                else:
                    nd["ival"] = int(e.value)
        elif isinstance(e, CallExpression):
            args = [self._add(a) for a in e.arguments]
            nd = dict(kind=EX_CALL, type=e.type, op=OPS[e.name], args=args, ival=e.ival)
        elif isinstance(e, SpecialForm):
            args = [self._add(a) for a in e.arguments]
            assert len(args) <= 3, "special forms take at most 3 arguments here"
            nd = dict(kind=EX_SPECIAL, type=e.type, op=FORMS[e.form], args=args)
            if e.items is not None:
                # the list: consecutive constant nodes (nothing else is added in between), named by (ival, slen) of the IN node
                nd["ival"], nd["slen"] = len(self.nodes), len(e.items)
                for item in e.items:
                    self._add(item)
        else:
            raise TypeError(e)
        self.nodes.append(nd)
        return len(self.nodes) - 1

    def to_c(self):
        arr = (_lib.ExprNode * max(1, len(self.nodes)))()
        for i, nd in enumerate(self.nodes):
            x = arr[i]
            x.kind, x.type, x.op = nd["kind"], nd["type"], nd["op"]
            x.n_args = len(nd["args"])
            for k, a in enumerate(nd["args"]):
                x.args[k] = a
            x.is_null = nd.get("is_null", 0)
            x.ival = nd.get("ival", 0)
            x.dval = nd.get("dval", 0.0)
            x.slen = nd.get("slen", 0)
        roots = (C.c_int32 * max(1, len(self.projection_roots)))(*self.projection_roots)
        pool = bytes(self.pool)
        spec = _lib.PageProcessorSpec(arr, len(self.nodes), pool, len(pool), self.filter_root, len(self.projection_roots), roots)
        return spec, [arr, roots, pool]

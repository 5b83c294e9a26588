"""Random expression programs for the kernel generator (csrc/jit.cpp) and what they must give: a seeded generator of typed trees over
the whole IR, a plain row-at-a-time evaluator, and the page processor's semantics restated over it.  Imports neither the library nor a
GPU: a tree is a tuple, `to_expr(tree, E)` turns it into the library's RowExpression given its `expressions` module.

    ("in", channel, type)                       ("const", value, type)            value None = the typed NULL
    ("call", NAME, type, (args...))             ("sf", FORM, type, (args...), items)   items: the constants of IN, else None

The evaluator follows the reference's generated code: the arguments of a call are evaluated left to right and the first NULL one skips
the rest and the call (BytecodeUtils.generateFullInvocation); AND / OR / IF / COALESCE / BETWEEN evaluate what their code generators
evaluate; a failing node throws there and then, so the FIRST EVALUATED failure of a row is the one that is raised.  Python ints decide
integer overflow exactly; DOUBLE is the Python float; the double -> integer casts round half away from zero (DoubleOperators.java:108-163).

Page semantics (PageProcessor.java:111-137, 313-338; PageFunctionCompiler's filter :502-544): the filter over the rows in order, then
every projection in index order over the selected positions in order.  The first throw wins: a filter failure before any projection,
projection k before projection k + 1, and inside one of them the first failing row.  (The reference projects in batches of at most 8,192
selected positions; every page here is smaller than that.)

LIKE / IN and the string functions are the restatements the suite already has (like_in_expected, string_fn_expected).  Subtrees under
them -- and every computed VARCHAR value -- hold no raising node: test_expr_fuzz_cpu.py replaces these subtrees by precomputed columns
to cross-check this evaluator against the C oracle, which has none of these operators, and a precomputed column cannot throw."""
import math
import random
import struct
from collections import namedtuple

import like_in_expected as LK
import string_fn_expected as SF

BIGINT, INTEGER, DATE, DOUBLE, BOOLEAN, VARCHAR = 1, 2, 3, 4, 5, 6
RANGE, DIV0, BADCAST = -2, -7, -9            # NUMERIC_VALUE_OUT_OF_RANGE, DIVISION_BY_ZERO, INVALID_CAST_ARGUMENT
ERROR_NAMES = {RANGE: "NUMERIC_VALUE_OUT_OF_RANGE", DIV0: "DIVISION_BY_ZERO", BADCAST: "INVALID_CAST_ARGUMENT"}
MAX_PROJ, MAX_COLS, MAX_DEPTH, MAX_VARCHAR_PROJ = 12, 20, 5, 2
ROW_COUNTS = (1, 64, 1025, 2049)             # one row, one wave, a tile + 1, two tiles + 1 of fp_emit
CMPS = ("EQUAL", "NOT_EQUAL", "LESS_THAN", "LESS_THAN_OR_EQUAL", "GREATER_THAN", "GREATER_THAN_OR_EQUAL")
ARITH = ("ADD", "SUBTRACT", "MULTIPLY", "DIVIDE", "MODULUS")
STRING_OPS = ("LIKE", "LENGTH", "SUBSTR", "CONCAT", "STRPOS", "STARTS_WITH")
# every (from, to) gen_call / gen_string accept
CAST_PAIRS = ([(t, t) for t in (BIGINT, INTEGER, DATE, DOUBLE, BOOLEAN, VARCHAR)] +
              [(BIGINT, DOUBLE), (INTEGER, DOUBLE), (INTEGER, BIGINT), (BIGINT, INTEGER), (BIGINT, BOOLEAN), (INTEGER, BOOLEAN), (DOUBLE, BOOLEAN),
               (BOOLEAN, BIGINT), (BOOLEAN, INTEGER), (BOOLEAN, DOUBLE), (DOUBLE, BIGINT), (DOUBLE, INTEGER),
               (BIGINT, VARCHAR), (INTEGER, VARCHAR), (BOOLEAN, VARCHAR)])
RAISING_CASTS = {(BIGINT, INTEGER), (DOUBLE, BIGINT), (DOUBLE, INTEGER)}
I64_MIN, I64_MAX, I32_MIN, I32_MAX = -2**63, 2**63 - 1, -2**31, 2**31 - 1


class ExprError(Exception):
    def __init__(self, code):
        super().__init__(ERROR_NAMES[code])
        self.code = code


Values = namedtuple("Values", "positions columns")            # the selected input positions, one value list per projection
Failure = namedtuple("Failure", "code position where")        # where: "filter" or the projection index
Program = namedtuple("Program", "name types filter projections")


# ---- the evaluator ------------------------------------------------------------------------------------------------------------
def type_of(t):
    return t[2]


def _limits(t):
    return (I64_MIN, I64_MAX) if t == BIGINT else (I32_MIN, I32_MAX)


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _int_arith(op, t, a, b):
    lo, hi = _limits(t)
    if op in ("DIVIDE", "MODULUS"):
        if b == 0:
            raise ExprError(DIV0)
        r = _tdiv(a, b) if op == "DIVIDE" else a - _tdiv(a, b) * b
    else:
        r = a + b if op == "ADD" else a - b if op == "SUBTRACT" else a * b
    if r < lo or r > hi:
        raise ExprError(RANGE)
    return r


def _double_arith(op, a, b):
    if op == "ADD":
        return a + b
    if op == "SUBTRACT":
        return a - b
    if op == "MULTIPLY":
        return a * b
    if op == "DIVIDE":
        if b == 0:
            if a == 0 or a != a:
                return math.nan
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b
    if a != a or b != b or math.isinf(a) or b == 0:          # C fmod
        return math.nan
    return math.fmod(a, b)


def round_half_away(x):
    """nearest integer, ties away from zero, of a finite double; exact"""
    if abs(x) >= 2.0**52:
        return int(x)
    t = math.trunc(x)
    return t + (1 if x > 0 else -1) if abs(x - t) >= 0.5 else t


def _cast(frm, to, v):
    if frm == to:
        return v
    if to == DOUBLE:
        return (1.0 if v else 0.0) if frm == BOOLEAN else float(v)
    if to == BOOLEAN:
        return v != 0                                        # NaN != 0: true
    if to == VARCHAR:
        return SF.cast_boolean(v) if frm == BOOLEAN else SF.cast_integer(v)
    if frm == BOOLEAN:
        return 1 if v else 0
    if frm == INTEGER:
        return v
    if frm == BIGINT:                                        # -> INTEGER
        if v < I32_MIN or v > I32_MAX:
            raise ExprError(RANGE)
        return v
    # DOUBLE -> BIGINT: castToLong :153-163, everything that is no long is INVALID_CAST_ARGUMENT
    if to == BIGINT:
        if v != v or math.isinf(v):
            raise ExprError(BADCAST)
        z = round_half_away(v)
        if z < I64_MIN or z > I64_MAX:
            raise ExprError(BADCAST)
        return z
    # DOUBLE -> INTEGER: castToInteger :108-121, NaN is INVALID_CAST_ARGUMENT, what toIntExact refuses NUMERIC_VALUE_OUT_OF_RANGE
    if v != v:
        raise ExprError(BADCAST)
    if math.isinf(v):
        raise ExprError(RANGE)
    z = round_half_away(v)
    if z < I32_MIN or z > I32_MAX:
        raise ExprError(RANGE)
    return z


def _compare(op, t, a, b):
    if t == BOOLEAN:
        a, b = int(a), int(b)
    if op == "EQUAL":
        return a == b
    if op == "NOT_EQUAL":
        return a != b
    if op == "LESS_THAN":
        return a < b
    if op == "LESS_THAN_OR_EQUAL":
        return a <= b
    if op == "GREATER_THAN":
        return a > b
    return a >= b


def _bytes(v):
    return v.encode("utf-8") if isinstance(v, str) else v


def evaluate(tree, row):
    """tree over `row` (one Python value per channel, None = NULL, VARCHAR as str or bytes) -> the value (VARCHAR: bytes), None = NULL;
    raises ExprError at the first evaluated failing node"""
    kind = tree[0]
    if kind == "in":
        v = row[tree[1]]
        return _bytes(v) if tree[2] == VARCHAR else v
    if kind == "const":
        return _bytes(tree[1]) if tree[2] == VARCHAR else tree[1]
    args = tree[3]
    if kind == "call":
        name, t = tree[1], tree[2]
        vals = []
        for a in args:
            v = evaluate(a, row)
            if v is None:
                return None
            vals.append(v)
        at = type_of(args[0])
        if name in ARITH:
            return _double_arith(name, vals[0], vals[1]) if t == DOUBLE else _int_arith(name, t, vals[0], vals[1])
        if name == "NEGATE":
            if t == DOUBLE:
                return -vals[0]
            if vals[0] == _limits(t)[0]:
                raise ExprError(RANGE)
            return -vals[0]
        if name in CMPS:
            return _compare(name, at, vals[0], vals[1])
        if name == "NOT":
            return not vals[0]
        if name == "CAST":
            return _cast(at, t, vals[0])
        if name == "LIKE":
            return LK.like(vals[0], vals[1].decode("utf-8"), vals[2].decode("utf-8") if len(vals) == 3 else None, len(vals) == 3)
        if name == "LENGTH":
            return SF.length(vals[0])
        if name == "SUBSTR":
            return SF.substring(vals[0], vals[1], vals[2] if len(vals) == 3 else None, len(vals) == 3)
        if name == "CONCAT":
            return SF.concat(vals[0], vals[1])
        if name == "STRPOS":
            return SF.strpos(vals[0], vals[1])
        if name == "STARTS_WITH":
            return SF.starts_with(vals[0], vals[1])
        raise ValueError(name)
    form = tree[1]
    if form in ("AND", "OR"):
        decides = form == "OR"
        l = evaluate(args[0], row)
        if l is not None and bool(l) == decides:
            return decides
        r = evaluate(args[1], row)
        if r is None:
            return None
        if bool(r) == decides:
            return decides
        return None if l is None else not decides
    if form == "IF":
        c = evaluate(args[0], row)
        return evaluate(args[1] if c else args[2], row)
    if form == "IS_NULL":
        return evaluate(args[0], row) is None
    if form == "COALESCE":
        for a in args:
            v = evaluate(a, row)
            if v is not None:
                return v
        return None
    if form == "BETWEEN":
        t = type_of(args[0])
        v = evaluate(args[0], row)
        lo = evaluate(args[1], row)
        l_null = v is None or lo is None
        l_val = False if l_null else _compare("GREATER_THAN_OR_EQUAL", t, v, lo)
        if not l_null and not l_val:
            return False
        hi = evaluate(args[2], row)
        if v is None or hi is None:
            return None
        if not _compare("LESS_THAN_OR_EQUAL", t, v, hi):
            return False
        return None if l_null else True
    if form == "IN":
        v = evaluate(args[0], row)
        return LK.in_list(v, [None if i[1] is None else (_bytes(i[1]) if i[2] == VARCHAR else i[1]) for i in tree[4]])
    raise ValueError(form)


def run_program(program, page):
    """page: [(type, values)] -> Values(positions, columns) or Failure(code, position, where)"""
    n = len(page[0][1]) if page else 0
    rows = [[vals[i] for _, vals in page] for i in range(n)]
    positions = list(range(n))
    if program.filter is not None:
        positions = []
        for i, row in enumerate(rows):
            try:
                if evaluate(program.filter, row):
                    positions.append(i)
            except ExprError as e:
                return Failure(e.code, i, "filter")
    if not positions:
        return Values([], [[] for _ in program.projections])     # an input page that selects no row gives no output page
    columns = []
    for k, p in enumerate(program.projections):
        col = []
        for i in positions:
            try:
                col.append(evaluate(p, rows[i]))
            except ExprError as e:
                return Failure(e.code, i, k)
        columns.append(col)
    return Values(positions, columns)


def bits(t, v):
    """a cell as something == compares exactly: doubles by bit pattern with every NaN alike, VARCHAR as bytes"""
    if v is None:
        return None
    if t == DOUBLE:
        return "nan" if v != v else struct.pack("<d", float(v))
    if t == VARCHAR:
        return _bytes(v)
    if t == BOOLEAN:
        return bool(v)
    return int(v)


# ---- trees: walking, lowering ---------------------------------------------------------------------------------------------------
def children(tree):
    return tree[3] if tree[0] in ("call", "sf") else ()


def walk(tree):
    yield tree
    for c in children(tree):
        yield from walk(c)


def height(tree):
    return 1 + max((height(c) for c in children(tree)), default=0)


def can_raise_here(tree):
    if tree[0] != "call":
        return False
    if tree[1] in ARITH or tree[1] == "NEGATE":
        return tree[2] in (BIGINT, INTEGER)
    return tree[1] == "CAST" and (type_of(tree[3][0]), tree[2]) in RAISING_CASTS


def can_raise(tree):
    return any(can_raise_here(t) for t in walk(tree))


def is_stringy(tree):
    """the subtrees the C oracle cannot evaluate: LIKE, IN, the string functions, and every computed VARCHAR value"""
    if tree[0] == "call" and tree[1] in STRING_OPS:
        return True
    if tree[0] == "sf" and tree[1] == "IN":
        return True
    return tree[0] in ("call", "sf") and tree[2] == VARCHAR


def is_built(tree):
    """a VARCHAR value made of pieces (CONCAT, CAST of an integer), which only a projection, CONCAT, LENGTH, IF, COALESCE and IS_NULL take"""
    if tree[2] != VARCHAR or tree[0] in ("in", "const"):
        return False
    if tree[0] == "call":
        if tree[1] == "CONCAT":
            return True
        if tree[1] == "CAST":
            return type_of(tree[3][0]) in (BIGINT, INTEGER) or is_built(tree[3][0])
        return False
    return any(is_built(a) for a in (tree[3][1:] if tree[1] == "IF" else tree[3]))


def operators(tree):
    """the names test_expr_fuzz_cpu.py counts: operator and form names, CAST as ("CAST", from, to), plus INPUT / CONST / NULL"""
    out = set()
    for t in walk(tree):
        if t[0] == "in":
            out.add("INPUT")
        elif t[0] == "const":
            out.add("NULL" if t[1] is None else "CONST")
        elif t[0] == "call" and t[1] == "CAST":
            out.add("CAST")
            out.add(("CAST", type_of(t[3][0]), t[2]))
        else:
            out.add(t[1])
            if t[1] in ARITH or t[1] == "NEGATE":
                out.add((t[1], t[2]))
            if t[1] in CMPS:
                out.add(("CMP", type_of(t[3][0])))
            if t[1] == "IN":
                out.add("IN_NULL" if any(i[1] is None for i in t[4]) else "IN_PLAIN")
            if t[1] == "LIKE":
                out.add("LIKE_ESCAPE" if len(t[3]) == 3 else "LIKE_PLAIN")
            if t[1] == "COALESCE":
                out.add(("COALESCE", len(t[3])))
    return out


def to_expr(tree, E):
    """the library's RowExpression (E = its `expressions` module).  A special form takes three arguments there: COALESCE(a, b, c, d) is
    lowered to COALESCE(a, b, COALESCE(c, d)), which evaluates the same arguments in the same order."""
    kind = tree[0]
    if kind == "in":
        return E.field(tree[1], tree[2])
    if kind == "const":
        return E.constant(tree[1], tree[2])
    args = [to_expr(a, E) for a in tree[3]]
    if kind == "call":
        return E.call(tree[1], tree[2], *args)
    if tree[1] == "IN":
        return E.SpecialForm("IN", BOOLEAN, args, [E.constant(i[1], i[2]) for i in tree[4]])
    if tree[1] == "COALESCE" and len(args) > 3:
        args = args[:2] + [E.SpecialForm("COALESCE", tree[2], args[2:])]
    return E.SpecialForm(tree[1], tree[2], args)


def lower(program, E):
    """-> (input types, filter expression or None, projection expressions)"""
    return list(program.types), None if program.filter is None else to_expr(program.filter, E), [to_expr(p, E) for p in program.projections]


def rewrite_for_oracle(program, page):
    """-> (program, page) with every maximal stringy subtree replaced by a reference to an extra, precomputed column"""
    types, cols, memo = list(program.types), list(page), {}
    n = len(page[0][1])
    rows = [[vals[i] for _, vals in page] for i in range(n)]

    def rw(tree):
        if is_stringy(tree):
            if tree not in memo:
                assert not can_raise(tree), tree
                memo[tree] = len(types)
                types.append(tree[2])
                cols.append((tree[2], [evaluate(tree, r) for r in rows]))
            return ("in", memo[tree], tree[2])
        if tree[0] == "call":
            return ("call", tree[1], tree[2], tuple(rw(a) for a in tree[3]))
        if tree[0] == "sf":
            return ("sf", tree[1], tree[2], tuple(rw(a) for a in tree[3]), tree[4])
        return tree

    f = None if program.filter is None else rw(program.filter)
    return Program(program.name, tuple(types), f, tuple(rw(p) for p in program.projections)), cols


# ---- input pages: fixed pools ----------------------------------------------------------------------------------------------------
_CP2, _CP3, _CP4 = "é", "名", "😀"


def _edge_strings():
    def fill(nbytes, unit):
        s = unit * (nbytes // len(unit.encode()))
        return s + "x" * (nbytes - len(s.encode()))
    out = [""]
    for nbytes in (7, 8, 9, 64, 300):
        out += [fill(nbytes, "ab"), fill(nbytes, _CP2), fill(nbytes, _CP3), fill(nbytes, _CP4), fill(nbytes, "a" + _CP3 + _CP4 + _CP2)]
    return out


QUIET_STRINGS = ["", "ab", "abc", "abcd", "abd", "b", "ab" + _CP3, "Customer#1", "Customer#12"]
EDGE_STRINGS = _edge_strings()
EDGE_BIGINTS = [0, 1, -1, 2**31, -2**31, 2**31 - 1, -(2**31 - 1), 2**62, -2**62, I64_MAX, I64_MIN]
EDGE_INTEGERS = [0, 1, -1, I32_MAX, I32_MIN]
EDGE_DOUBLES = [math.nan, math.inf, -math.inf, 0.0, -0.0, 0.5, -0.5, 2.5, -2.5, 0.49999999999999994, 2147483647.5, -2147483648.5, 2.0**31, -2.0**31,
                2.0**52, -2.0**52, 2.0**63, -2.0**63, 9223372036854774784.0, 5e-324]
# channel -> (type, pool of values or a callable of the rng, null fraction)
CHANNELS = [
    (BIGINT, lambda r: r.randint(-50, 50), 0.15),           # 0  quiet
    (BIGINT, EDGE_BIGINTS, 0.15),                           # 1  edge
    (BIGINT, lambda r: r.randint(-50, 50), 0.0),            # 2  quiet, never NULL
    (INTEGER, lambda r: r.randint(-100, 100), 0.15),        # 3  quiet
    (INTEGER, EDGE_INTEGERS, 0.15),                         # 4  edge
    (DOUBLE, lambda r: r.randint(-32, 32) * 0.25, 0.15),    # 5  quiet
    (DOUBLE, EDGE_DOUBLES, 0.15),                           # 6  edge
    (DATE, lambda r: r.randint(8990, 9010), 0.15),          # 7
    (BOOLEAN, [True, False], 0.15),                         # 8
    (BOOLEAN, [True, False], 0.15),                         # 9
    (VARCHAR, QUIET_STRINGS, 0.15),                         # 10 quiet
    (VARCHAR, EDGE_STRINGS, 0.15),                          # 11 edge
    (INTEGER, [0], 1.0),                                    # 12 always NULL
]
TYPES = tuple(c[0] for c in CHANNELS)
QUIET_CH = {BIGINT: (0, 2), INTEGER: (3,), DOUBLE: (5,), DATE: (7,), BOOLEAN: (8, 9), VARCHAR: (10,)}
ALL_CH = {BIGINT: (0, 1, 2), INTEGER: (3, 4, 12), DOUBLE: (5, 6), DATE: (7,), BOOLEAN: (8, 9), VARCHAR: (10, 11)}
_pages = {}


def page(n):
    """the first n rows of one fixed 2049-row page: [(type, values)]"""
    if "full" not in _pages:
        r = random.Random(20240)
        cols = []
        for t, pool, nulls in CHANNELS:
            vals = []
            for _ in range(max(ROW_COUNTS)):
                v = pool(r) if callable(pool) else r.choice(pool)
                vals.append(None if r.random() < nulls else v)
            cols.append((t, vals))
        _pages["full"] = cols
    return [(t, vals[:n]) for t, vals in _pages["full"]]


# ---- the generator -----------------------------------------------------------------------------------------------------------------
LIKE_PATTERNS = [("ab%", None), ("%b", None), ("a_c", None), ("%", None), ("abc", None), ("%" + _CP3 + "%", None), ("_%_", None), ("a%b%c", None), ("%a_" + _CP2 + "%", None),
                 ("ab#%%", "#"), ("#_%", "#"), ("a%", ""), ("Customer#%", None), (None, None)]
EDGE_CONSTS = {BIGINT: [0, 1, -1, 2**31, 2**62, I64_MAX, I64_MIN], INTEGER: [0, 1, -1, I32_MAX, I32_MIN], DOUBLE: [math.nan, math.inf, -0.0, 0.5, 2.5, 2.0**63],
               DATE: [9000, 8990, 9010], BOOLEAN: [True, False], VARCHAR: ["", "ab", "abc", "a" + _CP3, _CP4 * 2]}
QUIET_CONSTS = {BIGINT: [2, 3, -7, 10], INTEGER: [2, 3, -7, 10], DOUBLE: [0.25, -1.5, 2.0, 4.0]}


class Generator:
    """mode "quiet": raising operators draw their operands from the quiet channels and small constants, and a divisor is a non-zero
    constant or IF(b = 0, 1, b); mode "loud": no such restraint"""

    def __init__(self, seed, mode, only=None):
        self.r = random.Random(seed)
        self.mode = mode
        self.only = only        # a channel: every input reference reads this one (the shape the dictionary-aware path takes)
        self.pool = []          # subtrees already made: reused between the filter and the projections

    def const(self, t, quiet=False):
        r = self.r
        if not quiet and r.random() < 0.12:
            return ("const", None, t)
        pool = QUIET_CONSTS[t] if quiet and t in QUIET_CONSTS else EDGE_CONSTS[t]
        return ("const", r.choice(pool), t)

    def leaf(self, t, quiet=False):
        if self.r.random() < 0.3:
            return self.const(t, quiet)
        if self.only is not None:
            frm = TYPES[self.only]
            if frm == t:
                return ("in", self.only, t)
            if (frm, t) in CAST_PAIRS and ((frm, t) not in RAISING_CASTS or self.mode == "loud") and t != VARCHAR:
                return ("call", "CAST", t, (("in", self.only, frm),))
            return self.const(t, quiet)
        return ("in", self.r.choice((QUIET_CH if quiet else ALL_CH)[t]), t)

    def operand(self, t, d, safe):
        """the operand of a raising operator; d: the height it may have.  Quiet: a leaf of a quiet channel, a widening cast of one, or one
        more +, -, * over such leaves -- |values| <= 100, so neither that nor the operator above it can overflow, and compositions of the
        raising operators give values, not only error codes"""
        if self.mode == "loud":
            return self.leaf(t) if self.r.random() < 0.4 else self.gen(t, d, safe)
        if d >= 2 and self.r.random() < 0.35:
            return ("call", self.r.choice(ARITH[:3]), t, (self.leaf(t, True), self.leaf(t, True)))
        if d >= 2 and t == BIGINT and self.r.random() < 0.2:
            return ("call", "CAST", BIGINT, (self.leaf(INTEGER, True),))
        return self.leaf(t, True)

    def divisor(self, t, d, safe):
        if self.mode == "loud":
            return self.gen(t, d, safe)
        if d < 3 or self.r.random() < 0.5:
            return ("const", self.r.choice([1, -1, 2, 3, -7]), t)
        b = self.leaf(t, True)
        if b[0] == "const":
            b = ("in", QUIET_CH[t][0], t)
        return ("sf", "IF", t, (("call", "EQUAL", BOOLEAN, (b, ("const", 0, t))), ("const", 1, t), b), None)

    def gen(self, t, d, safe=False, view=False):
        """a tree of type t and height <= d; safe: no raising node (inside what the oracle cross-check precomputes); view: a VARCHAR value
        that is no built one"""
        r = self.r
        if d <= 1 or r.random() < 0.12:
            return self.leaf(t)
        if r.random() < 0.2:
            fit = [s for s in self.pool if s[2] == t and height(s) <= d and not (safe and can_raise(s)) and not (view and is_built(s))]
            if fit:
                return r.choice(fit)
        tree = self.make(t, d, safe, view)
        if tree[0] in ("call", "sf"):
            self.pool.append(tree)
        return tree

    def special(self, t, d, safe, view):
        r, k = self.r, self.r.random()
        if k < 0.5:
            return ("sf", "IF", t, (self.gen(BOOLEAN, d - 1, safe), self.gen(t, d - 1, safe, view), self.gen(t, d - 1, safe, view)), None)
        return ("sf", "COALESCE", t, tuple(self.gen(t, d - 1, safe, view) for _ in range(r.randint(1, 4))), None)

    def make(self, t, d, safe, view):
        r = self.r
        g = lambda tt, **kw: self.gen(tt, d - 1, safe or kw.get("safe", False), kw.get("view", False))
        if t == VARCHAR:
            k = r.random()
            if k < 0.3:
                args = (self.gen(VARCHAR, d - 1, True, True), self.gen(BIGINT, min(d - 1, 2), True))
                if r.random() < 0.5:
                    args += (self.gen(BIGINT, min(d - 1, 2), True),)
                return ("call", "SUBSTR", VARCHAR, args)
            if k < 0.4:
                return ("call", "CAST", VARCHAR, (self.gen(r.choice((VARCHAR, BOOLEAN)), d - 1, True, True),))
            if k < 0.6:
                return self.special(VARCHAR, d, True, view)
            if view:
                return self.leaf(VARCHAR)
            if k < 0.85:
                return ("call", "CONCAT", VARCHAR, (self.gen(VARCHAR, d - 1, True), self.gen(VARCHAR, d - 1, True)))
            return ("call", "CAST", VARCHAR, (self.gen(r.choice((BIGINT, INTEGER)), d - 1, True),))
        if t == DATE:
            k = r.random()
            if k < 0.3:
                return ("call", "CAST", DATE, (g(DATE),))
            return self.special(DATE, d, safe, False)
        if t == BOOLEAN:
            k = r.randrange(14)
            if k < 3:
                ct = r.choice((BIGINT, INTEGER, DOUBLE, DATE, BOOLEAN, VARCHAR))
                ops = CMPS[:2] if ct == BOOLEAN else CMPS
                return ("call", r.choice(ops), BOOLEAN, (g(ct, view=True), g(ct, view=True)))
            if k == 3:
                return ("call", "NOT", BOOLEAN, (g(BOOLEAN),))
            if k in (4, 5):
                return ("sf", r.choice(("AND", "OR")), BOOLEAN, (g(BOOLEAN), g(BOOLEAN)), None)
            if k == 6:
                return ("sf", "IS_NULL", BOOLEAN, (g(r.choice((BIGINT, INTEGER, DOUBLE, DATE, BOOLEAN, VARCHAR))),), None)
            if k == 7:
                ct = r.choice((BIGINT, INTEGER, DOUBLE, DATE, VARCHAR))
                return ("sf", "BETWEEN", BOOLEAN, (g(ct, view=True), g(ct, view=True), g(ct, view=True)), None)
            if k == 8:
                ct = r.choice((BIGINT, INTEGER, DOUBLE, DATE, BOOLEAN, VARCHAR))
                items = [("const", v, ct) for v in r.sample(EDGE_CONSTS[ct], min(len(EDGE_CONSTS[ct]), r.randint(1, 4)))]
                if r.random() < 0.5:
                    items.insert(r.randrange(len(items) + 1), ("const", None, ct))
                return ("sf", "IN", BOOLEAN, (self.gen(ct, d - 1, True, True),), tuple(items))
            if k == 9:
                pat, esc = r.choice(LIKE_PATTERNS)
                args = (self.gen(VARCHAR, d - 1, True, True), ("const", pat, VARCHAR))
                if esc is not None:
                    args += (("const", esc, VARCHAR),)
                return ("call", "LIKE", BOOLEAN, args)
            if k == 10:
                return ("call", "STARTS_WITH", BOOLEAN, (self.gen(VARCHAR, d - 1, True, True), self.gen(VARCHAR, d - 1, True, True)))
            if k == 11:
                return ("call", "CAST", BOOLEAN, (g(r.choice((BIGINT, INTEGER, DOUBLE, BOOLEAN))),))
            return self.special(BOOLEAN, d, safe, False)
        # BIGINT / INTEGER / DOUBLE
        k = r.randrange(12)
        raising = t != DOUBLE
        if k < 5 and not (raising and safe):
            op = r.choice(ARITH)
            if not raising:
                return ("call", op, t, (g(t), g(t)))
            b = self.divisor(t, d - 1, safe) if op in ("DIVIDE", "MODULUS") else self.operand(t, d - 1, safe)
            return ("call", op, t, (self.operand(t, d - 1, safe), b))
        if k == 5 and not (raising and safe):
            return ("call", "NEGATE", t, (self.operand(t, d - 1, safe) if raising else g(t),))
        if k in (6, 7, 8):
            frm = r.choice([f for f, to in CAST_PAIRS if to == t])
            if (frm, t) in RAISING_CASTS:
                if safe:
                    return self.leaf(t)
                return ("call", "CAST", t, (self.operand(frm, d - 1, safe),))
            return ("call", "CAST", t, (g(frm),))
        if k == 9 and t == BIGINT:
            if r.random() < 0.5:
                return ("call", "LENGTH", BIGINT, (self.gen(VARCHAR, d - 1, True),))
            return ("call", "STRPOS", BIGINT, (self.gen(VARCHAR, d - 1, True, True), self.gen(VARCHAR, d - 1, True, True)))
        return self.special(t, d, safe, False)


def random_program(seed, mode, only=None):
    g = Generator(seed, mode, only)
    r = g.r
    filt = g.gen(BOOLEAN, MAX_DEPTH) if r.random() < (0.75 if mode == "quiet" else 0.5) else None
    projections, varchars = [], 0
    for _ in range(r.randint(2, 7) if r.random() < 0.8 else r.randint(8, MAX_PROJ)):
        if r.random() < 0.15 and only is None:
            t = r.choice((BIGINT, INTEGER, DOUBLE, DATE, BOOLEAN, VARCHAR))
            projections.append(("in", r.choice(ALL_CH[t]), t))                    # an identity projection
            continue
        t = r.choice((BIGINT, BIGINT, INTEGER, DOUBLE, DOUBLE, BOOLEAN, BOOLEAN, DATE, VARCHAR))
        if t == VARCHAR and varchars == MAX_VARCHAR_PROJ:
            t = BIGINT
        tree = g.gen(t, r.randint(2, MAX_DEPTH))
        if tree[0] == "const":
            tree = ("sf", "COALESCE", t, (tree,), None)
        varchars += t == VARCHAR and tree[0] != "in"
        projections.append(tree)
    return Program("%s%d" % (mode, seed) + ("" if only is None else "_ch%d" % only), TYPES, filt, tuple(projections))


# ---- constructed programs: which failure of several a page raises -----------------------------------------------------------------------
def _in(ch):
    return ("in", ch, TYPES[ch])


def _c(v, t=BIGINT):
    return ("const", v, t)


def _call(name, t, *args):
    return ("call", name, t, tuple(args))


def first_failure(tree, rows):
    for i, row in enumerate(rows):
        try:
            evaluate(tree, row)
        except ExprError as e:
            return i, e.code
    return None


def order_program(k):
    """a projection of index >= 1 fails while a LATER projection fails on an EARLIER row with another code.  Over channel 1's edge values
    `x * 4` overflows at |x| >= 2^61, `7 / x` and `7 % x` divide by zero at x = 0, CAST(1.0 / x AS BIGINT) is an invalid cast at x = 0,
    CAST(x AS INTEGER) is out of range beyond 32 bits and `-(x - 1)` overflows at -2^63; of a pair that fails on different rows, the one
    that fails later on the 2049-row page comes first.  Channel 2 (never NULL) is the projection in front and the always-true filter."""
    x, q = _in(1), _in(2)
    mul = _call("MULTIPLY", BIGINT, x, _c(4))
    div = _call("DIVIDE", BIGINT, _c(7), x)
    mod = _call("MODULUS", BIGINT, _c(7), x)
    dcast = _call("CAST", BIGINT, _call("DIVIDE", DOUBLE, _c(1.0, DOUBLE), _call("CAST", DOUBLE, x)))
    icast = _call("CAST", INTEGER, x)
    neg = _call("NEGATE", BIGINT, _call("SUBTRACT", BIGINT, x, _c(1)))
    a, b = [(mul, div), (dcast, mul), (icast, mod), (neg, dcast), (icast, dcast), (neg, mod)][k]
    rows = [[vals[i] for _, vals in page(max(ROW_COUNTS))] for i in range(max(ROW_COUNTS))]
    fa, fb = first_failure(a, rows), first_failure(b, rows)
    assert fa and fb and fa[0] != fb[0] and fa[1] != fb[1], (k, fa, fb)
    if fa[0] < fb[0]:
        a, b = b, a
    return Program("order%d" % k, TYPES, _call("GREATER_THAN_OR_EQUAL", BOOLEAN, q, _c(-50)), (q,) * (1 + k // 3) + (a, b))


ORDER_PROGRAMS = 6
QUIET_SEEDS = list(range(1, 25)) + [27, 35, 38, 82]
LOUD_SEEDS = [103, 104, 106, 107, 109, 110, 125, 127, 136, 147, 159, 166, 172, 213, 247, 255] + ["order%d" % k for k in range(ORDER_PROGRAMS)]
_programs, _outcomes = {}, {}


# (mode, seed, channel): programs whose expressions read one channel only
SINGLE_CHANNEL = [("loud", 310, 1), ("loud", 319, 1), ("quiet", 335, 1), ("quiet", 344, 0), ("quiet", 318, 6), ("loud", 307, 6), ("quiet", 308, 10), ("quiet", 306, 11),
                  ("loud", 322, 4), ("quiet", 344, 4)]


def program(seed, mode=None, only=None):
    """seed: an int of QUIET_SEEDS (mode "quiet") / LOUD_SEEDS (mode "loud"), or the name of a constructed program"""
    if isinstance(seed, str):
        return order_program(int(seed[5:]))
    key = (seed, mode, only)
    if key not in _programs:
        _programs[key] = random_program(seed, mode, only)
    return _programs[key]


def all_programs():
    return [program(s, "quiet") for s in QUIET_SEEDS] + [program(s, "loud") for s in LOUD_SEEDS]


def outcome(prog, n):
    """run_program on page(n), computed once"""
    key = (prog.name, n)
    if key not in _outcomes:
        _outcomes[key] = run_program(prog, page(n))
    return _outcomes[key]


# ---- join filter functions: a BOOLEAN tree over (build channels..., probe channels...) --------------------------------------------------
JOIN_SIDE = len(TYPES) + 1          # each side of the join: the page's channels and a BIGINT row number
JOIN_TYPES = TYPES + (BIGINT,)


def map_inputs(tree, fn):
    """the tree with every input reference ("in", channel, type) replaced by fn(channel, type)"""
    if tree[0] == "in":
        return fn(tree[1], tree[2])
    if tree[0] == "call":
        return ("call", tree[1], tree[2], tuple(map_inputs(a, fn) for a in tree[3]))
    if tree[0] == "sf":
        return ("sf", tree[1], tree[2], tuple(map_inputs(a, fn) for a in tree[3]), tree[4])
    return tree


def join_filter(seed, mode):
    """a seeded BOOLEAN tree whose input references are dealt out between the build side (channels 0 .. JOIN_SIDE - 1) and the probe side
    (JOIN_SIDE ..), reference by reference"""
    g = Generator(seed, mode)
    tree = g.gen(BOOLEAN, MAX_DEPTH)
    while sum(t[0] == "in" for t in walk(tree)) < 2:
        tree = g.gen(BOOLEAN, MAX_DEPTH)
    return map_inputs(tree, lambda ch, t: ("in", ch + (JOIN_SIDE if g.r.random() < 0.5 else 0), t))


JOIN_FILTER_SEEDS = [("quiet", s) for s in (1, 2, 5, 11, 14, 22)] + [("loud", s) for s in (104, 105, 111, 132)]

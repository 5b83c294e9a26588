"""What StreamingAggregationOperator puts out (M/operator/StreamingAggregationOperator.java:216-347), in plain Python: no GPU, no oracle.

A page is a list of columns, a column a KeyCol of tests/key_cases.py (type, values, nulls; VARCHAR: a list of str / None).  The model walks
the pages the way processInput does: row 0 against the carried row (currentGroup), findNextGroupStart with rowNotDistinctFromRow, one set
of accumulators that is evaluated and replaced when a group ends.  A Python float addition is the Java double addition, a Python int
with a range check on the total is sum(bigint) as this library defines it (tests/bigint_sum_cases.py: 128-bit accumulation, the total
decides).

An output row is Row(page, row, values): the KEY CELLS are named, not copied -- they are those of row `row` of input page `page`
(key_cells() fetches them as bit tokens), so a test sees which row the operator read:
  a group that ends inside page P (the next group starts in P): the first row of its segment in P -- row 0 of P when it began earlier;
  a group whose last row is the last row of P, flushed by the next page's first row or by finish: that last row of P.
`values` holds one entry per output channel behind the keys: SINGLE / FINAL one per aggregate (None = NULL), PARTIAL the flattened
states of tgpu_hash_aggregation_factory_create (count; count, sum; count, extreme)."""
import math
import struct
from typing import NamedTuple

import key_cases as K

COUNT_ALL, COUNT_COLUMN, SUM_BIGINT, SUM_DOUBLE, AVG_BIGINT, AVG_DOUBLE, MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
SINGLE, PARTIAL, FINAL = 0, 1, 2
INT64_MIN, INT64_MAX = -(2**63), 2**63 - 1
_COUNTS = (COUNT_ALL, COUNT_COLUMN)
_DOUBLE_SUMS = (SUM_DOUBLE, AVG_BIGINT, AVG_DOUBLE)
_MINMAX = (MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE)


class NumericValueOutOfRange(Exception):
    """TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE (-2)"""


class Row(NamedTuple):
    page: int
    row: int
    values: tuple


def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _semantic_tokens(col):
    """one token per cell under IS NOT DISTINCT FROM: NULL is one value, every NaN is one value, -0.0 is +0.0"""
    toks = K.cells(col)
    if col.type == K.DOUBLE:
        return [None if v is None else ("nan" if K.is_nan_bits(v) else (0 if v == K.NEG_ZERO else v)) for v in toks]
    if col.type == K.BOOLEAN:
        return [None if v is None else (v != 0) for v in toks]
    return toks


def key_tokens(page, group_by_channels):
    """per row the tuple of semantic tokens of its key cells"""
    cols = [_semantic_tokens(page[c]) for c in group_by_channels]
    return list(zip(*cols))


def _values(col):
    """a column's cells as Python values (None = NULL): ints, floats, bools' bytes, str"""
    if col.type == K.VARCHAR:
        return list(col.values)
    vals = col.values.tolist()
    if col.nulls is None:
        return vals
    return [None if f else v for v, f in zip(vals, col.nulls.tolist())]


def _double_less(a, b):
    """Double.compare(a, b) < 0: -0.0 below +0.0, NaN above everything (DoubleType.java:194-198)"""
    if a != a:
        return False
    if b != b:
        return True
    if a == b:
        return math.copysign(1.0, a) < math.copysign(1.0, b)
    return a < b


class Accumulator:
    """one aggregate of one group"""

    def __init__(self, spec, step):
        self.function, self.channel = spec[0], spec[1]
        self.mask = spec[2] if len(spec) > 2 else -1
        self.step = step
        self.count = 0
        self.total = 0 if self.function == SUM_BIGINT else 0.0
        self.extreme = None

    def _fold(self, v):
        f = self.function
        if f == SUM_BIGINT:
            self.total += v
        elif f in _DOUBLE_SUMS:
            self.total = self.total + float(v)
        elif f == MIN_BIGINT:
            self.extreme = v if self.extreme is None else min(self.extreme, v)
        elif f == MAX_BIGINT:
            self.extreme = v if self.extreme is None else max(self.extreme, v)
        elif f == MIN_DOUBLE:
            if self.extreme is None or _double_less(v, self.extreme):
                self.extreme = v
        elif f == MAX_DOUBLE:   # tgpu.h TGPU_AGG_MAX_DOUBLE: a NaN gives way to any value; among zeros of both signs +0.0
            if self.extreme is None or self.extreme != self.extreme or (v == v and _double_less(self.extreme, v)):
                self.extreme = v

    def add(self, cols, r):
        """raw input (SINGLE / PARTIAL): cols = the page's columns as Python values"""
        if self.mask >= 0 and not cols[self.mask][r]:   # NULL or false
            return
        if self.function == COUNT_ALL:
            self.count += 1
            return
        v = cols[self.channel][r]
        if v is None:
            return
        self.count += 1
        if self.function != COUNT_COLUMN:
            self._fold(v)

    def combine(self, cols, r):
        """intermediate input (FINAL): the state channels start at the aggregate's input channel"""
        c = cols[self.channel][r]
        self.count += c
        if self.function in _COUNTS:
            return
        v = cols[self.channel + 1][r]
        if self.function in _MINMAX:
            if c:
                self._fold(v)
        else:
            self._fold(v)

    def evaluate(self):
        f = self.function
        if f == SUM_BIGINT and not INT64_MIN <= self.total <= INT64_MAX:
            raise NumericValueOutOfRange("bigint addition overflow")
        if self.step == PARTIAL:
            if f in _COUNTS:
                return (self.count,)
            if f in _MINMAX:
                return (self.count, self.extreme if self.count else 0)
            return (self.count, self.total)
        if f in _COUNTS:
            return (self.count,)
        if self.count == 0:
            return (None,)
        if f in _MINMAX:
            return (float("nan") if self.extreme != self.extreme else self.extreme,)
        if f in (AVG_BIGINT, AVG_DOUBLE):
            return (self.total / self.count,)
        return (self.total,)


def stream(pages, group_by_channels, aggs, step=SINGLE):
    """generator: the rows every call emits -- one list per input page (add_input), then one for finish.  A sum(bigint) whose total
    leaves int64 raises NumericValueOutOfRange from the call that completes its group; the rows of that call are lost with it."""
    fresh = lambda: [Accumulator(a, step) for a in aggs]
    accs = fresh()
    current = None   # (page, row, key tokens) of the open group's reference row

    def flush(page, row, out):
        nonlocal accs
        vals = tuple(v for a in accs for v in a.evaluate())
        out.append(Row(page, row, vals))
        accs = fresh()

    for p, page in enumerate(pages):
        n = page[0].n if page else 0
        out = []
        if n == 0:
            yield out
            continue
        keys = key_tokens(page, group_by_channels)
        cols = [_values(c) for c in page]
        feed = (lambda a, r: a.combine(cols, r)) if step == FINAL else (lambda a, r: a.add(cols, r))
        if current is not None and current[2] != keys[0]:
            flush(current[0], current[1], out)   # the page starts with a new group (:283-286)
        start = 0
        while True:
            nxt = start + 1
            while nxt < n and keys[nxt] == keys[start]:   # findNextGroupStart (:338-347)
                nxt += 1
            for r in range(start, nxt):
                for a in accs:
                    feed(a, r)
            if nxt < n:
                flush(p, start, out)   # ends in the middle of the page (:296-300)
                start = nxt
            else:
                current = (p, n - 1, keys[n - 1])   # :303
                break
        yield out
    out = []
    if current is not None:
        flush(current[0], current[1], out)
    yield out


def aggregate(pages, group_by_channels, aggs, step=SINGLE):
    """all output rows of the stream, in order"""
    return [row for rows in stream(pages, group_by_channels, aggs, step) for row in rows]


def key_cells(pages, group_by_channels, rows):
    """the key cells of output rows as bit tokens (key_cases.cells): one tuple per row"""
    toks = {}
    out = []
    for r in rows:
        if r.page not in toks:
            toks[r.page] = [K.cells(pages[r.page][c]) for c in group_by_channels]
        out.append(tuple(t[r.row] for t in toks[r.page]))
    return out


def value_token(v):
    """an aggregate value as something == compares bit for bit: doubles by their bits"""
    return ("d", double_bits(v)) if isinstance(v, float) else v


def run_groups(pages, group_by_channels):
    """the group number of every row of the concatenated stream (0, 1, 2, ... in stream order)"""
    ids, g, last = [], -1, object()
    for page in pages:
        if not page or page[0].n == 0:
            continue
        for k in key_tokens(page, group_by_channels):
            if k != last:
                g += 1
                last = k
            ids.append(g)
    return ids


# ---- the golden fixture's page and expectation generators (RowPagesBuilder / SequencePageBuilder) ---------------------------------------
TYPE_CODES = {"BIGINT": K.BIGINT, "INTEGER": K.INTEGER, "DATE": K.DATE, "DOUBLE": K.DOUBLE, "BOOLEAN": K.BOOLEAN, "VARCHAR": K.VARCHAR}
FUNCTION_CODES = {"count": COUNT_COLUMN, "count_all": COUNT_ALL, "sum_bigint": SUM_BIGINT, "sum_double": SUM_DOUBLE}
STEP_CODES = {"SINGLE": SINGLE, "PARTIAL": PARTIAL, "FINAL": FINAL}


def _sequence_cell(type_id, i):
    """SequencePageBuilder.createSequencePage: BOOLEAN i % 2 == 0, DOUBLE (double) i, VARCHAR String.valueOf(i), BIGINT i"""
    if type_id == K.BOOLEAN:
        return i % 2 == 0
    if type_id == K.DOUBLE:
        return float(i)
    if type_id == K.VARCHAR:
        return str(i)
    return i


def column_of(type_id, cells):
    """a KeyCol from Python cells (None = NULL, "NaN" = a NaN)"""
    import numpy as np
    if type_id == K.VARCHAR:
        return K.KeyCol(K.VARCHAR, cells)
    nulls = np.array([c is None for c in cells], dtype=np.uint8)
    vals = [0 if c is None else (float("nan") if c == "NaN" else c) for c in cells]
    return K.KeyCol(type_id, np.array(vals, dtype=K._NP[type_id]), nulls if nulls.any() else None)


def golden_pages(case):
    types = [TYPE_CODES[t] for t in case["types"]]
    pages = []
    for p in case["pages"]:
        if "sequence" in p:
            length, initial = p["sequence"]["length"], p["sequence"]["initial"]
            pages.append([column_of(t, [_sequence_cell(t, first + i) for i in range(length)]) for t, first in zip(types, initial)])
        else:
            pages.append([column_of(t, [r[c] for r in p["rows"]]) for c, t in enumerate(types)])
    return types, pages


def golden_expected(case):
    """the expected rows as tuples of cells: key cells as Python values (None, "NaN", float, str), then the aggregate values"""
    e = case["expected"]
    if "rows" in e:
        return [tuple(r) for r in e["rows"]]
    g = e["sequence"]
    key_type = TYPE_CODES[g["key_type"]]
    return [(_sequence_cell(key_type, g["key_initial"] + i), g["count"], g["sum_initial"] + i) for i in range(g["length"])]


def golden_aggs(case):
    return [(FUNCTION_CODES[f], ch) for f, ch in case["aggregates"]]

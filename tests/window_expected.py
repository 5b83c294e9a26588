"""Expected values of WindowOperator: a Python restatement of the reference's row loop (M/operator/window/WindowPartition.java:184-214: per row
updatePeerGroup :238-247, the frame :281-345, then every function) for the three frames without offsets and the functions of include/tgpu.h, over a
STABLE sort of all rows with the comparator of tests/top_n_ranking_expected.py (partition channels ASC_NULLS_LAST, then the sort channels; rows that
compare equal keep arrival order across pages).  Partition and peer equality are IS NOT DISTINCT FROM, written separately from the comparator: -0.0
and +0.0 are one partition / peers although the sort tells them apart, NaN = NaN, null = null.  Aggregates run over a frame that only grows, row by
row from the partition's start, as AggregateWindowFunction.java does: sum(bigint) raises where Math.addExact would.  min / max(double) follow the
rules the tgpu_agg_function comments document (Double.compare order; NaN only when nothing else came; of both zeros max gives +0.0).
Rows are tuples of Python values (None = null), one per source channel."""
import functools
from collections import namedtuple

from top_n_ranking_expected import ASC_NULLS_LAST, BIGINT, BOOLEAN, DATE, DOUBLE, INTEGER, VARCHAR, cell_token, compare_rows, compare_values, tokens  # noqa: F401

ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST, LAG, LEAD, FIRST_VALUE, LAST_VALUE, AGGREGATE = range(10)
FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT = 0, 1, 2
COUNT_ALL, COUNT_COLUMN, SUM_BIGINT, MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE = 1, 2, 3, 7, 8, 9, 10

Fn = namedtuple("Fn", "function args frame agg", defaults=((), FRAME_RANGE_TO_CURRENT, 0))


class NumericValueOutOfRange(Exception):
    """BigintOperators.add under LongSumAggregation: "bigint addition overflow" """


class InvalidArgument(Exception):
    """LagFunction / LeadFunction checkCondition: "Offset must be at least 0" """


def not_distinct(type_id, a, b):
    """IS NOT DISTINCT FROM on two cells"""
    if a is None or b is None:
        return a is None and b is None
    if type_id == DOUBLE:
        return (a != a and b != b) or a == b   # NaN = NaN (DoubleType.java:181-192); -0.0 == 0.0
    if type_id == BOOLEAN:
        return bool(a) == bool(b)
    return a == b


def rows_not_distinct(types, channels, left, right):
    return all(not_distinct(types[c], left[c], right[c]) for c in channels)


class Accumulator:
    """one aggregate over a frame [0, end] that only grows"""

    def __init__(self, agg, channel):
        self.agg, self.channel, self.count, self.value, self.added = agg, channel, 0, None, 0

    def add(self, row):
        if self.agg == COUNT_ALL:
            self.count += 1
            return
        v = row[self.channel]
        if v is None:
            return
        self.count += 1
        if self.agg == COUNT_COLUMN:
            return
        if self.value is None:
            self.value = v
        elif self.agg == SUM_BIGINT:
            self.value += v
        elif self.agg == MIN_BIGINT:
            self.value = min(self.value, v)
        elif self.agg == MAX_BIGINT:
            self.value = max(self.value, v)
        elif self.agg == MIN_DOUBLE:   # Double.compare: NaN is the greatest, so it stays only while nothing else came
            if compare_values(DOUBLE, v, self.value) < 0:
                self.value = v
        elif self.agg == MAX_DOUBLE:   # a NaN state gives way to any value and never replaces one; +0.0 above -0.0
            if self.value != self.value or (v == v and compare_values(DOUBLE, v, self.value) > 0):
                self.value = v
        if self.agg == SUM_BIGINT and not -2**63 <= self.value < 2**63:   # Math.addExact
            raise NumericValueOutOfRange("bigint addition overflow")

    def upto(self, rows, end):
        while self.added <= end:
            self.add(rows[self.added])
            self.added += 1
        if self.agg in (COUNT_ALL, COUNT_COLUMN):
            return self.count
        if self.count == 0:
            return None
        return float("nan") if self.value != self.value else self.value


def partition_values(types, sort_channels, functions, rows):
    """the function values of one partition's rows (already in order): one tuple per row"""
    size = len(rows)
    accs = [Accumulator(f.agg, f.args[0] if f.args else None) if f.function == AGGREGATE else None for f in functions]
    out = []
    peer_start, peer_end = 0, 0   # [peer_start, peer_end)
    rank = dense = 0
    for cur in range(size):
        if cur == peer_end:   # updatePeerGroup
            peer_start = cur
            peer_end = cur + 1
            while peer_end < size and rows_not_distinct(types, sort_channels, rows[peer_start], rows[peer_end]):
                peer_end += 1
            rank = peer_start + 1
            dense += 1
        vals = []
        for f, acc in zip(functions, accs):
            frame_end = {FRAME_PARTITION: size - 1, FRAME_RANGE_TO_CURRENT: peer_end - 1, FRAME_ROWS_TO_CURRENT: cur}[f.frame]
            if f.function == ROW_NUMBER:
                v = cur + 1
            elif f.function == RANK:
                v = rank
            elif f.function == DENSE_RANK:
                v = dense
            elif f.function == PERCENT_RANK:
                v = 0.0 if size == 1 else float(rank - 1) / float(size - 1)
            elif f.function == CUME_DIST:
                v = float(peer_end) / float(size)
            elif f.function == FIRST_VALUE:
                v = rows[0][f.args[0]]
            elif f.function == LAST_VALUE:
                v = rows[frame_end][f.args[0]]
            elif f.function in (LAG, LEAD):
                offset = rows[cur][f.args[1]] if len(f.args) > 1 else 1
                if offset is None:
                    v = None
                else:
                    if offset < 0:
                        raise InvalidArgument("Offset must be at least 0")
                    p = cur - offset if f.function == LAG else cur + offset
                    if p >= 2**63:
                        p -= 2**64   # Java long arithmetic wraps
                    inside = 0 <= p <= cur if f.function == LAG else 0 <= p < size
                    v = rows[p][f.args[0]] if inside else (rows[cur][f.args[2]] if len(f.args) > 2 else None)
            elif f.function == AGGREGATE:
                v = acc.upto(rows, frame_end)
            else:
                raise ValueError(f.function)
            vals.append(v)
        out.append(tuple(vals))
    return out


def expected_output(types, pages_rows, output_channels, functions, partition_channels, sort_channels, sort_orders):
    """the operator's one output page as rows: the output channels, then one value per function ([] = no page)"""
    rows = [tuple(r) for page in pages_rows for r in page]
    if partition_channels or sort_channels:
        keys = list(partition_channels) + list(sort_channels)
        orders = [ASC_NULLS_LAST] * len(partition_channels) + list(sort_orders)   # WindowOperator.java:254
        rows = sorted(rows, key=functools.cmp_to_key(functools.partial(compare_rows, types, keys, orders)))   # stable
    out, start = [], 0
    while start < len(rows):
        end = start + 1
        while end < len(rows) and rows_not_distinct(types, partition_channels, rows[start], rows[end]):
            end += 1
        part = rows[start:end]
        for row, vals in zip(part, partition_values(types, sort_channels, functions, part)):
            out.append(tuple(row[c] for c in output_channels) + vals)
        start = end
    return out


def golden_case(case):
    """(type ids, pages as row tuples, functions, expected rows) of a case of tests/golden/window_vectors.json; "NaN" decodes to a NaN"""
    names = {"BIGINT": BIGINT, "INTEGER": INTEGER, "DATE": DATE, "DOUBLE": DOUBLE, "BOOLEAN": BOOLEAN, "VARCHAR": VARCHAR}
    fnames = {"ROW_NUMBER": ROW_NUMBER, "RANK": RANK, "DENSE_RANK": DENSE_RANK, "PERCENT_RANK": PERCENT_RANK, "CUME_DIST": CUME_DIST, "LAG": LAG, "LEAD": LEAD,
              "FIRST_VALUE": FIRST_VALUE, "LAST_VALUE": LAST_VALUE, "AGGREGATE": AGGREGATE}
    frames = {"PARTITION": FRAME_PARTITION, "RANGE_TO_CURRENT": FRAME_RANGE_TO_CURRENT, "ROWS_TO_CURRENT": FRAME_ROWS_TO_CURRENT}
    aggs = {None: 0, "COUNT_ALL": COUNT_ALL, "COUNT_COLUMN": COUNT_COLUMN, "SUM_BIGINT": SUM_BIGINT, "MIN_BIGINT": MIN_BIGINT, "MAX_BIGINT": MAX_BIGINT,
            "MIN_DOUBLE": MIN_DOUBLE, "MAX_DOUBLE": MAX_DOUBLE}
    decode = lambda v: float("nan") if v == "NaN" else v
    types = [names[t] for t in case["types"]]
    pages = [[tuple(decode(v) for v in r) for r in page] for page in case["pages"]]
    functions = [Fn(fnames[f["function"]], tuple(f.get("args", ())), frames[f.get("frame", "RANGE_TO_CURRENT")], aggs[f.get("agg")]) for f in case["functions"]]
    expected = [tuple(decode(v) for v in r) for r in case["expected"]]
    return types, pages, functions, expected

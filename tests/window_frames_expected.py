"""Expected values of WindowOperator under frames with bounds (tgpu_window_factory_create_framed): a row-by-row Python restatement of the reference's
getFrameRange (M/operator/window/WindowPartition.java: ROWS :281-323 with emptyFrame :541-573 and preceding / following :575-589; GROUPS :609-694 with
emptyFrame(Range) :523-528; RANGE by peers :327-344) and of the functions over the frame [start, end] it yields (FirstValueFunction, LastValueFunction,
NthValueFunction.java:41-77, NTileFunction.java:45-74, AggregateWindowFunction).  Every function is recomputed over its frame FROM SCRATCH, one frame at a
time, nothing slides: sum(bigint) raises exactly when a frame's own exact sum leaves int64.  The sort, the partitions, the peers and the Accumulator are
those of tests/window_expected.py.  A frame of WIDE rows or more takes the same from-scratch aggregate as ONE numpy reduction over the frame's slice of
the partition's column (WideColumns; tests/test_window_frames_cpu.py holds it against the Accumulator), so that the GPU tests stay quick where frames
reach through a whole partition.  A function whose frame is one of the three old FRAME_* codes is computed by window_expected.partition_values itself
(a frame that grows from the partition's start, prefix overflow included).
Rows are tuples of Python values (None = null), one per source channel."""
import functools
import struct
from collections import namedtuple

import numpy as np

from window_expected import (AGGREGATE, ASC_NULLS_LAST, COUNT_ALL, COUNT_COLUMN, FIRST_VALUE, LAST_VALUE, SUM_BIGINT, Accumulator, Fn, InvalidArgument,  # noqa: F401
                             NumericValueOutOfRange, compare_rows, partition_values, rows_not_distinct)

NTH_VALUE, NTILE = 10, 11
RANGE, ROWS, GROUPS = 0, 1, 2
UNBOUNDED_PRECEDING, PRECEDING, CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING = range(5)

# start_channel / end_channel: the offset's source channel (PRECEDING / FOLLOWING bounds only)
Frame = namedtuple("Frame", "type start end start_channel end_channel", defaults=(-1, -1))


def valid_bounds(start, end):
    """the analyzer's rules"""
    if start == UNBOUNDED_FOLLOWING or end == UNBOUNDED_PRECEDING:
        return False
    if start == CURRENT_ROW and end == PRECEDING:
        return False
    if start == FOLLOWING and end not in (FOLLOWING, UNBOUNDED_FOLLOWING):
        return False
    return True


def offset_of(row, channel, side):
    """getFrameValue, :601-607"""
    v = row[channel]
    if v is None:
        raise InvalidArgument("Window frame %s offset must not be null" % side)
    if v < 0:
        raise InvalidArgument("Window frame offset must not be negative")
    return v


def rows_frame(frame, row, cur, last):
    """ROWS: (start, end) in partition positions, or None for an empty frame; cur = the row's position, last = the partition's last position"""
    a = offset_of(row, frame.start_channel, "starting") if frame.start in (PRECEDING, FOLLOWING) else None
    b = offset_of(row, frame.end_channel, "ending") if frame.end in (PRECEDING, FOLLOWING) else None
    behind = last - cur
    # emptyFrame(frameInfo, rowPosition, endPosition)
    if frame.start == UNBOUNDED_PRECEDING and frame.end == PRECEDING:
        if b > cur:
            return None
    elif frame.start == FOLLOWING and frame.end == UNBOUNDED_FOLLOWING:
        if a > behind:
            return None
    elif frame.start == frame.end == PRECEDING:
        if a < b or (a > cur and b > cur):
            return None
    elif frame.start == frame.end == FOLLOWING:
        if a > b or a > behind:
            return None

    def position(kind, value, unbounded):
        if kind in (UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING):
            return unbounded
        if kind == PRECEDING:
            return 0 if value > cur else cur - value
        if kind == FOLLOWING:
            return last if value > behind else cur + value
        return cur
    return position(frame.start, a, 0), position(frame.end, b, last)


def groups_frame(frame, row, group, groups, last):
    """GROUPS, and RANGE by peers (the same without offsets): `groups` = [(first, last position)] of the partition's peer groups, group = the row's"""
    a = offset_of(row, frame.start_channel, "starting") if frame.start in (PRECEDING, FOLLOWING) else None
    b = offset_of(row, frame.end_channel, "ending") if frame.end in (PRECEDING, FOLLOWING) else None
    top = len(groups) - 1
    if frame.start == UNBOUNDED_PRECEDING:
        start = 0
    elif frame.start == CURRENT_ROW:
        start = groups[group][0]
    elif frame.start == PRECEDING:
        start = groups[group - a][0] if group - a >= 0 else 0
    else:
        start = groups[group + a][0] if group + a <= top else last + 1   # behind the partition
    if frame.end == UNBOUNDED_FOLLOWING:
        end = last
    elif frame.end == CURRENT_ROW:
        end = groups[group][1]
    elif frame.end == PRECEDING:
        end = groups[group - b][1] if group - b >= 0 else -1
    else:
        end = groups[group + b][1] if group + b <= top else last
    if start > end or start > last or end < 0:   # emptyFrame(Range)
        return None
    return start, end


WIDE = 16   # frames of at least this many rows are reduced with numpy
I64_MIN, I64_MAX = -2**63, 2**63 - 1


class WideColumns:
    """one partition's argument columns as arrays, made on first use: the aggregates over rows[start .. end] as one reduction each"""

    def __init__(self, rows):
        self.rows, self.made = rows, {}

    def column(self, channel, kind):
        key = (channel, kind)
        if key not in self.made:
            values = [r[channel] for r in self.rows]
            present = np.array([v is not None for v in values], dtype=np.int64)
            if kind == "present":
                made = present
            elif kind == "bigint":   # (values with 0 for null, small enough for an int64 sum of any slice, as objects otherwise)
                ints = [0 if v is None else v for v in values]
                small = all(abs(v) < 2**31 for v in ints)
                made = (np.array(ints, dtype=np.int64 if small else object), small)
            elif kind in ("min_bigint", "max_bigint"):   # nulls can never win
                fill = I64_MAX if kind == "min_bigint" else I64_MIN
                made = np.array([fill if v is None else v for v in values], dtype=np.int64)
            else:   # the Double.compare order as an int64 key; min: NaN above every value, null above NaN; max: NaN below every value, null below NaN
                def order(v):
                    bits = struct.unpack("<q", struct.pack("<d", v))[0]
                    return bits if bits >= 0 else bits ^ I64_MAX
                if kind == "min_double":
                    made = np.array([I64_MAX if v is None else (I64_MAX - 1 if v != v else order(v)) for v in values], dtype=np.int64)
                else:
                    made = np.array([I64_MIN if v is None else (I64_MIN + 1 if v != v else order(v)) for v in values], dtype=np.int64)
            self.made[key] = made
        return self.made[key]

    def aggregate(self, agg, channel, start, end):
        if agg == COUNT_ALL:
            return end - start + 1
        count = int(self.column(channel, "present")[start:end + 1].sum())
        if agg == COUNT_COLUMN:
            return count
        if count == 0:
            return None
        if agg == SUM_BIGINT:
            values, small = self.column(channel, "bigint")
            total = int(values[start:end + 1].sum()) if small else sum(values[start:end + 1].tolist())
            if not I64_MIN <= total <= I64_MAX:
                raise NumericValueOutOfRange("bigint addition overflow")
            return total
        kind = {7: "min_bigint", 8: "max_bigint", 9: "min_double", 10: "max_double"}[agg]
        keys = self.column(channel, kind)[start:end + 1]
        at = start + int(keys.argmin() if kind.startswith("min") else keys.argmax())
        v = self.rows[at][channel]
        return float("nan") if v != v else v


def over_frame(f, rows, cur, frame, wide=None):
    """one function over frame = (start, end) or None"""
    if f.function == FIRST_VALUE:
        return None if frame is None else rows[frame[0]][f.args[0]]
    if f.function == LAST_VALUE:
        return None if frame is None else rows[frame[1]][f.args[0]]
    if f.function == NTH_VALUE:
        offset = rows[cur][f.args[1]]
        if frame is None or offset is None:
            return None
        if offset < 1:
            raise InvalidArgument("Offset must be at least 1")
        at = frame[0] + offset - 1
        return rows[at][f.args[0]] if at <= frame[1] else None
    assert f.function == AGGREGATE
    if frame is None:
        return 0 if f.agg in (COUNT_ALL, COUNT_COLUMN) else None
    if wide is not None and frame[1] - frame[0] + 1 >= WIDE:
        return wide.aggregate(f.agg, f.args[0] if f.args else None, frame[0], frame[1])
    if f.agg == SUM_BIGINT:   # the exact sum of this frame alone; only it has to fit
        values = [r[f.args[0]] for r in rows[frame[0]:frame[1] + 1] if r[f.args[0]] is not None]
        if not values:
            return None
        if not -2**63 <= sum(values) < 2**63:
            raise NumericValueOutOfRange("bigint addition overflow")
        return sum(values)
    acc = Accumulator(f.agg, f.args[0] if f.args else None)
    acc.added = frame[0]
    return acc.upto(rows, frame[1])


def ntile(row, channel, cur, size):
    buckets = row[channel]
    if buckets is None:
        return None
    if buckets <= 0:
        raise InvalidArgument("Buckets must be greater than 0")
    if size < buckets:
        return cur + 1
    remainder, per = size % buckets, size // buckets
    if cur < (per + 1) * remainder:
        return cur // (per + 1) + 1
    return (cur - remainder) // per + 1


def partition_values_framed(types, sort_channels, functions, rows):
    """the function values of one partition's rows (already in order): one tuple per row.  f.frame is a Frame or an old FRAME_* code."""
    size = len(rows)
    groups, group_of = [], []
    for cur in range(size):
        if cur > 0 and rows_not_distinct(types, sort_channels, rows[cur - 1], rows[cur]):
            groups[-1] = (groups[-1][0], cur)
        else:
            groups.append((cur, cur))
        group_of.append(len(groups) - 1)
    reads_frame = (AGGREGATE, FIRST_VALUE, LAST_VALUE, NTH_VALUE)
    # an old frame code, or a function that ignores whatever frame it has: window_expected's own loop, once for the partition
    old = [i for i, f in enumerate(functions) if f.function != NTILE and (f.function not in reads_frame or (not isinstance(f.frame, Frame) and f.function != NTH_VALUE))]
    as_old = lambda f: Fn(f.function, f.args, 0 if isinstance(f.frame, Frame) else f.frame, f.agg)
    old_values = partition_values(types, sort_channels, [as_old(functions[i]) for i in old], rows) if old else None
    old_at = {i: k for k, i in enumerate(old)}
    out = []
    wide = WideColumns(rows)
    for cur in range(size):
        vals, frames = [], {}   # the row's frame per distinct Frame
        for i, f in enumerate(functions):
            if i in old_at:
                vals.append(old_values[cur][old_at[i]])
            elif f.function == NTILE:
                vals.append(ntile(rows[cur], f.args[0], cur, size))
            elif not isinstance(f.frame, Frame):
                raise ValueError("nth_value needs a Frame")
            else:
                if f.frame not in frames:
                    if f.frame.type == ROWS:
                        frames[f.frame] = rows_frame(f.frame, rows[cur], cur, size - 1)
                    else:
                        assert f.frame.type == GROUPS or (f.frame.start not in (PRECEDING, FOLLOWING) and f.frame.end not in (PRECEDING, FOLLOWING))
                        frames[f.frame] = groups_frame(f.frame, rows[cur], group_of[cur], groups, size - 1)
                vals.append(over_frame(f, rows, cur, frames[f.frame], wide))
        out.append(tuple(vals))
    return out


def expected_output(types, pages_rows, output_channels, functions, partition_channels, sort_channels, sort_orders):
    """the operator's one output page as rows: the output channels, then one value per function ([] = no page)"""
    rows = [tuple(r) for page in pages_rows for r in page]
    if partition_channels or sort_channels:
        keys = list(partition_channels) + list(sort_channels)
        orders = [ASC_NULLS_LAST] * len(partition_channels) + list(sort_orders)
        rows = sorted(rows, key=functools.cmp_to_key(functools.partial(compare_rows, types, keys, orders)))   # stable
    out, start = [], 0
    while start < len(rows):
        end = start + 1
        while end < len(rows) and rows_not_distinct(types, partition_channels, rows[start], rows[end]):
            end += 1
        part = rows[start:end]
        for row, vals in zip(part, partition_values_framed(types, sort_channels, functions, part)):
            out.append(tuple(row[c] for c in output_channels) + vals)
        start = end
    return out


# ---- tests/golden/window_frame_vectors.json ------------------------------------------------------------------------------------------------------
TYPE_NAMES = {"BIGINT": 1, "INTEGER": 2, "DATE": 3, "DOUBLE": 4, "BOOLEAN": 5, "VARCHAR": 6}
FRAME_TYPES = {"RANGE": RANGE, "ROWS": ROWS, "GROUPS": GROUPS}
BOUNDS = {"UNBOUNDED_PRECEDING": UNBOUNDED_PRECEDING, "PRECEDING": PRECEDING, "CURRENT_ROW": CURRENT_ROW, "FOLLOWING": FOLLOWING, "UNBOUNDED_FOLLOWING": UNBOUNDED_FOLLOWING}
FUNCTION_NAMES = {"FIRST_VALUE": FIRST_VALUE, "LAST_VALUE": LAST_VALUE, "AGGREGATE": AGGREGATE, "NTH_VALUE": NTH_VALUE, "NTILE": NTILE}
AGG_NAMES = {None: 0, "COUNT_ALL": COUNT_ALL, "COUNT_COLUMN": COUNT_COLUMN, "SUM_BIGINT": SUM_BIGINT, "MIN_BIGINT": 7, "MAX_BIGINT": 8}


def golden_frame(f):
    return Frame(FRAME_TYPES[f["type"]], BOUNDS[f["start"]], BOUNDS[f["end"]], f.get("start_channel", -1), f.get("end_channel", -1))


def golden_case(case):
    """(type ids, pages as row tuples, functions, expected rows) of a case of "cases" """
    types = [TYPE_NAMES[t] for t in case["types"]]
    pages = [[tuple(r) for r in page] for page in case["pages"]]
    functions = [Fn(FUNCTION_NAMES[f["function"]], tuple(f.get("args", ())), golden_frame(f["frame"]), AGG_NAMES[f.get("agg")]) for f in case["functions"]]
    return types, pages, functions, [tuple(r) for r in case["expected"]]


def golden_group_case(case):
    """a case of "groups": (type ids, pages, functions, expected rows) with the functions and their values DERIVED from the listed array_agg frames:
    count(*), count(a), first_value(a), last_value(a), and for a BIGINT a also min(a) and max(a)"""
    types = [TYPE_NAMES[t] for t in case["types"]]
    pages = [[tuple(r) for r in page] for page in case["pages"]]
    frame, a = golden_frame(case["frame"]), case["value_channel"]
    functions = [Fn(AGGREGATE, (), frame, COUNT_ALL), Fn(AGGREGATE, (a,), frame, COUNT_COLUMN), Fn(FIRST_VALUE, (a,), frame), Fn(LAST_VALUE, (a,), frame)]
    numeric = case["types"][a] == "BIGINT"
    if numeric:
        functions += [Fn(AGGREGATE, (a,), frame, AGG_NAMES["MIN_BIGINT"]), Fn(AGGREGATE, (a,), frame, AGG_NAMES["MAX_BIGINT"])]
    expected = []
    for outputs, listed in zip(case["outputs"], case["frames"]):
        present = [v for v in (listed or []) if v is not None]
        derived = [len(listed or []), len(present), listed[0] if listed else None, listed[-1] if listed else None]
        if numeric:
            derived += [min(present) if present else None, max(present) if present else None]
        expected.append(tuple(outputs) + tuple(derived))
    return types, pages, functions, expected

"""Expected frames of WindowOperator under RANGE BETWEEN x PRECEDING / FOLLOWING AND y PRECEDING / FOLLOWING (tgpu_window_factory_create_ranged), twice and
independently:
  walk_frames     the reference's STATEFUL walk restated row by row (M/operator/window/WindowPartition.java: getFrameRange :325-389, getFrameStartPreceding
                  .. getFrameEndFollowing :391-481, seek :495-521, emptyFrame / nearestValidFrame :523-539, the recent ranges of :135-153 and :258-264).  It
                  raises WalkLeftPartition where the reference would index outside the partition (bounds no planner produces).
  closed_frames   the closed form include/tgpu.h states, by linear scans: no search, no state.
The functions over a frame are those of tests/window_frames_expected.py; frames of every other kind are computed there.  Rows are tuples of Python
values (None = null), one per source channel; a comparison is that of the type's order code (DOUBLE: -0.0 < +0.0, every NaN equal and above +inf)."""
import functools
import struct
from collections import namedtuple

from window_expected import ASC_NULLS_LAST, Fn, InvalidArgument, compare_rows, rows_not_distinct  # noqa: F401
from window_frames_expected import (AGGREGATE, CURRENT_ROW, FIRST_VALUE, FOLLOWING, LAST_VALUE, NTH_VALUE, PRECEDING, RANGE, UNBOUNDED_FOLLOWING,  # noqa: F401
                                    UNBOUNDED_PRECEDING, Frame, WideColumns, over_frame, partition_values_framed, valid_bounds)

BIGINT, INTEGER, DATE, DOUBLE = 1, 2, 3, 4
ASC_NULLS_FIRST, DESC_NULLS_FIRST, DESC_NULLS_LAST = 0, 2, 3
MASK = 2**64 - 1

# a RANGE frame with value bounds: start_channel / end_channel = the bound VALUE, start_key / end_key = the comparison key channel
RangeFrame = namedtuple("RangeFrame", "start end start_channel end_channel start_key end_key", defaults=(-1, -1, -1, -1))


class WalkLeftPartition(Exception):
    """the reference's seek would read a position outside the partition, or compare a null"""


def ascending(order):
    return order in (ASC_NULLS_FIRST, ASC_NULLS_LAST)


def nulls_first(order):
    return order in (ASC_NULLS_FIRST, DESC_NULLS_FIRST)


def order_code(t, v):
    """the unsigned 64-bit order code of a non-null value (device_order.h cell_order_bits)"""
    if t == DOUBLE:
        bits = 0x7ff8000000000000 if v != v else struct.unpack("<Q", struct.pack("<d", v))[0]
        return (~bits & MASK) if bits >> 63 else bits | 1 << 63
    return v + 2**63


def has_value(bound):
    return bound in (PRECEDING, FOLLOWING)


class Partition:
    """one partition's rows in sorted order as the two searches see them"""

    def __init__(self, types, sort_channel, order, frame, rows):
        self.n, self.frame, self.asc = len(rows), frame, ascending(order)
        self.key_null = [r[sort_channel] is None for r in rows]
        self.peer_s, self.peer_e = [0] * self.n, [0] * self.n
        first = 0
        for p in range(1, self.n + 1):
            if p == self.n or not rows_not_distinct(types, [sort_channel], rows[p - 1], rows[p]):
                for q in range(first, p):
                    self.peer_s[q], self.peer_e[q] = first, p - 1
                first = p
        code = lambda ch, r: None if ch < 0 or r[ch] is None else order_code(types[ch], r[ch])
        self.start_key = [code(frame.start_key, r) if has_value(frame.start) else None for r in rows]
        self.end_key = [code(frame.end_key, r) if has_value(frame.end) else None for r in rows]
        self.start_bound = [code(frame.start_channel, r) if has_value(frame.start) else None for r in rows]
        self.end_bound = [code(frame.end_channel, r) if has_value(frame.end) else None for r in rows]

    def check_nulls(self):
        """the errors of get_output, in the library's order"""
        live = [p for p in range(self.n) if not self.key_null[p]]
        if has_value(self.frame.start) and any(self.start_bound[p] is None for p in live):
            raise InvalidArgument("Window frame starting offset must not be null")
        if has_value(self.frame.end) and any(self.end_bound[p] is None for p in live):
            raise InvalidArgument("Window frame ending offset must not be null")
        if (has_value(self.frame.start) and any(self.start_key[p] is None for p in live)) or (has_value(self.frame.end) and any(self.end_key[p] is None for p in live)):
            raise InvalidArgument("Window frame comparison key must not be null where the sort key is not null")


# ---- the closed form ---------------------------------------------------------------------------------------------------------------------------
def closed_frames(part):
    """[(start, end) or None] per row"""
    n, f = part.n, part.frame
    live = [p for p in range(n) if not part.key_null[p]]
    lo, hi = (live[0], live[-1]) if live else (0, -1)
    precedes = (lambda k, b: k <= b) if part.asc else (lambda k, b: k >= b)   # K[p] <~ B
    out = []
    for cur in range(n):
        if part.key_null[cur]:
            s = 0 if f.start == UNBOUNDED_PRECEDING else part.peer_s[cur]
            e = n - 1 if f.end == UNBOUNDED_FOLLOWING else part.peer_e[cur]
        else:
            if f.start == UNBOUNDED_PRECEDING:
                s = 0
            elif f.start == CURRENT_ROW:
                s = part.peer_s[cur]
            else:
                s = next((p for p in range(lo, hi + 1) if precedes(part.start_bound[cur], part.start_key[p])), hi + 1)
            if f.end == UNBOUNDED_FOLLOWING:
                e = n - 1
            elif f.end == CURRENT_ROW:
                e = part.peer_e[cur]
            else:
                e = next((p for p in range(hi, lo - 1, -1) if precedes(part.end_key[p], part.end_bound[cur])), lo - 1)
        out.append(None if s > e or s > n - 1 or e < 0 else (s, e))
    return out


# ---- the reference's walk ----------------------------------------------------------------------------------------------------------------------
def walk_frames(part):
    """[(start, end) or None] per row, with the recent range carried from row to row"""
    n, f = part.n, part.frame
    recent = (0, n - 1) if f.end == UNBOUNDED_FOLLOWING else (0, part.peer_e[0])   # initializeRangeCache

    def is_null(flags, p):
        if not 0 <= p < n:
            raise WalkLeftPartition(p)
        return flags[p] if flags is part.key_null else flags[p] is None

    def seek(keys, bound, cur, position, step, reverse, limit, stop):
        def compare(p):
            if not 0 <= p < n or keys[p] is None:
                raise WalkLeftPartition(p)
            c = (keys[p] > bound) - (keys[p] < bound)
            return -c if reverse else c
        comparison = compare(position)
        while comparison < 0:
            position -= step
            if stop(position):
                return position
            comparison = compare(position)
        while True:
            if position == limit or is_null(keys, position + step):
                break
            if compare(position + step) >= 0:
                position += step
            else:
                break
        return position

    out = []
    for cur in range(n):
        if part.key_null[cur]:
            rng = (0 if f.start == UNBOUNDED_PRECEDING else part.peer_s[cur], n - 1 if f.end == UNBOUNDED_FOLLOWING else part.peer_e[cur])
        else:
            if f.start == UNBOUNDED_PRECEDING:
                s = 0
            elif f.start == CURRENT_ROW:
                s = part.peer_s[cur]
            elif f.start == PRECEDING:      # getFrameStartPreceding
                if is_null(part.key_null, recent[0]):
                    s = cur
                else:
                    s = seek(part.start_key, part.start_bound[cur], cur, recent[0], -1, not part.asc, 0, lambda p: False)
            else:                           # getFrameStartFollowing
                position = recent[0]
                if recent[0] == 0 and part.key_null[0]:
                    position = cur
                while is_null(part.key_null, position):
                    position -= 1
                s = seek(part.start_key, part.start_bound[cur], cur, position, -1, not part.asc, 0, lambda p: p >= n or part.start_key[p] is None)
            if f.end == UNBOUNDED_FOLLOWING:
                e = n - 1
            elif f.end == CURRENT_ROW:
                e = part.peer_e[cur]
            elif f.end == PRECEDING:        # getFrameEndPreceding
                position = recent[1]
                while is_null(part.key_null, position):
                    position += 1
                e = seek(part.end_key, part.end_bound[cur], cur, position, 1, part.asc, n - 1, lambda p: p < 0 or part.end_key[p] is None)
            else:                           # getFrameEndFollowing
                position = recent[1]
                if is_null(part.key_null, recent[1]):
                    position = cur
                e = seek(part.end_key, part.end_bound[cur], cur, position, 1, part.asc, n - 1, lambda p: False)
            rng = (s, e)
        if rng[0] > rng[1] or rng[0] >= n or rng[1] < 0:   # emptyFrame, then nearestValidFrame
            recent = (min(n - 1, rng[0]), max(0, rng[1]))
            out.append(None)
        else:
            recent = rng
            out.append(rng)
    return out


FRAMES = {"walk": walk_frames, "closed": closed_frames}


# ---- the operator's page -----------------------------------------------------------------------------------------------------------------------
def partition_values_ranged(types, sort_channels, sort_orders, functions, rows, how):
    """as window_frames_expected.partition_values_framed, with RangeFrame frames too"""
    ranged = [i for i, f in enumerate(functions) if isinstance(f.frame, RangeFrame) and f.function in (AGGREGATE, FIRST_VALUE, LAST_VALUE, NTH_VALUE)]
    as_plain = lambda f: f._replace(frame=Frame(RANGE, UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING)) if isinstance(f.frame, RangeFrame) else f   # (ignored by the function)
    plain = [i for i in range(len(functions)) if i not in ranged]
    plain_values = partition_values_framed(types, sort_channels, [as_plain(functions[i]) for i in plain], rows) if plain else None
    frames = {}
    for i in ranged:
        if functions[i].frame not in frames:
            frames[functions[i].frame] = FRAMES[how](Partition(types, sort_channels[0], sort_orders[0], functions[i].frame, rows))
    wide = WideColumns(rows)
    plain_at = {i: k for k, i in enumerate(plain)}
    out = []
    for cur in range(len(rows)):
        out.append(tuple(plain_values[cur][plain_at[i]] if i in plain_at else over_frame(f, rows, cur, frames[f.frame][cur], wide) for i, f in enumerate(functions)))
    return out


def sorted_partitions(types, pages_rows, partition_channels, sort_channels, sort_orders):
    rows = [tuple(r) for page in pages_rows for r in page]
    if partition_channels or sort_channels:
        keys = list(partition_channels) + list(sort_channels)
        orders = [ASC_NULLS_LAST] * len(partition_channels) + list(sort_orders)
        rows = sorted(rows, key=functools.cmp_to_key(functools.partial(compare_rows, types, keys, orders)))   # stable
    parts, start = [], 0
    while start < len(rows):
        end = start + 1
        while end < len(rows) and rows_not_distinct(types, partition_channels, rows[start], rows[end]):
            end += 1
        parts.append(rows[start:end])
        start = end
    return parts


def expected_output(types, pages_rows, output_channels, functions, partition_channels, sort_channels, sort_orders, how="walk"):
    """the operator's one output page as rows: the output channels, then one value per function ([] = no page).  The null errors of the bounds come
    first, whatever else the page holds."""
    parts = sorted_partitions(types, pages_rows, partition_channels, sort_channels, sort_orders)
    frames = []
    for f in functions:
        if isinstance(f.frame, RangeFrame) and f.frame not in frames and f.function in (AGGREGATE, FIRST_VALUE, LAST_VALUE, NTH_VALUE):
            frames.append(f.frame)
    checks = [Partition(types, sort_channels[0], sort_orders[0], frame, part) for frame in frames for part in parts]
    for message in ("starting offset", "ending offset", "comparison key"):
        for c in checks:
            try:
                c.check_nulls()
            except InvalidArgument as e:
                if message in str(e):
                    raise
    out = []
    for part in parts:
        for row, vals in zip(part, partition_values_ranged(types, sort_channels, sort_orders, functions, part, how)):
            out.append(tuple(row[c] for c in output_channels) + vals)
    return out

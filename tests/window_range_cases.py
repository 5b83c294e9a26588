"""Inputs for the RANGE-frame tests (tests/test_window_range_cpu.py, tests/test_gpu_window_range.py): a seeded corpus of tables whose bound channels are
what a planner computes in front of the window -- sort key -/+ a non-negative finite offset, without overflow -- and one of tables whose bounds have
nothing to do with the keys.  Channels of every table: 0 BIGINT partition key, 1 the sort key (nullable), 2 BIGINT row id, 3 BIGINT values with
nulls, 4 the start bound, 5 the end bound (both of the sort key's type; the comparison key of both bounds is channel 1 itself)."""
import numpy as np

from window_range_expected import (BIGINT, CURRENT_ROW, DATE, DOUBLE, FOLLOWING, INTEGER, PRECEDING, UNBOUNDED_FOLLOWING, UNBOUNDED_PRECEDING, RangeFrame, ascending,
                                   valid_bounds)

KEY_TYPES = (BIGINT, INTEGER, DATE, DOUBLE)
ORDERS = (0, 1, 2, 3)
COMBINATIONS = [(s, e) for s in range(5) for e in range(5) if valid_bounds(s, e)]   # 13
I64_MIN, I64_MAX, I32_MIN, I32_MAX = -2**63, 2**63 - 1, -2**31, 2**31 - 1
INF, NAN = float("inf"), float("nan")
OFFSETS = (0, 0, 1, 1, 2, 3, 7, 1000)   # 1000: beyond the whole small domain
DOUBLE_SPECIALS = (-0.0, 0.0, NAN, INF, -INF, 0.5, -1.5)
EDGES = {BIGINT: (I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MAX - 2, I64_MAX - 1, I64_MAX), INTEGER: (I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX),
         DATE: (I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX)}


def frame_of(start, end):
    return RangeFrame(start, end, 4, 5, 1, 1)


def bound_value(t, key, offset, subtract):
    """key -/+ offset as the planner's checked arithmetic gives it; the offset is cut where that would overflow (such a query fails upstream)"""
    if key is None:
        return None
    if t == DOUBLE:
        return key - offset if subtract else key + offset
    low, high = (I64_MIN, I64_MAX) if t == BIGINT else (I32_MIN, I32_MAX)
    return max(low, key - offset) if subtract else min(high, key + offset)


def make_case(rng, t, order, start, end, n, parts, null_fraction, flavour, conforming=True):
    """flavour: "small" keys -5 .. 5, "edges" (the type's extremes, DOUBLE: zeros, NaN, infinities), "one" (a single value)"""
    def key():
        if rng.random() < null_fraction:
            return None
        if flavour == "one":
            return 3.0 if t == DOUBLE else 3
        if flavour == "edges":
            pool = DOUBLE_SPECIALS if t == DOUBLE else EDGES[t]
            return pool[int(rng.integers(len(pool)))]
        v = int(rng.integers(-5, 6))
        return float(v) / 2 if t == DOUBLE else v
    constant = bool(rng.integers(2))
    const_a, const_b = (OFFSETS[int(rng.integers(len(OFFSETS)))] for _ in range(2))
    rows = []
    for i in range(n):
        k = key()
        a = const_a if constant else OFFSETS[int(rng.integers(len(OFFSETS)))]
        b = const_b if constant else OFFSETS[int(rng.integers(len(OFFSETS)))]
        if start == end and not constant and rng.random() < 0.7:   # mostly frames that are not empty by construction
            a, b = (max(a, b), min(a, b)) if start == PRECEDING else (min(a, b), max(a, b))
        if t == DOUBLE:
            a, b = float(a) / 2, float(b) / 2
        if conforming:
            asc = ascending(order)
            lo_bound = bound_value(t, k, a, (start == PRECEDING) == asc)
            hi_bound = bound_value(t, k, b, (end == PRECEDING) == asc)
            if k is None and rng.random() < 0.5:
                lo_bound, hi_bound = key(), None   # whatever: never read
        else:
            lo_bound, hi_bound = key(), key()
            if k is not None and lo_bound is None:
                lo_bound = k
            if k is not None and hi_bound is None:
                hi_bound = k
        value = None if rng.random() < 0.2 else int(rng.integers(-1000, 1000))
        rows.append((int(rng.integers(parts)), k, i, value, lo_bound, hi_bound))
    return {"types": [BIGINT, t, BIGINT, BIGINT, t, t], "order": order, "frame": frame_of(start, end), "rows": rows,
            "name": "t%d o%d %d-%d n%d p%d nulls%.1f %s" % (t, order, start, end, n, parts, null_fraction, flavour)}


def corpus(seed, per_combination=2, max_rows=40, conforming=True):
    """every key type x sort order x bound combination, `per_combination` tables each"""
    rng = np.random.default_rng(seed)
    cases = []
    for t in KEY_TYPES:
        for order in ORDERS:
            for start, end in COMBINATIONS:
                for _ in range(per_combination):
                    n = int(rng.integers(1, max_rows + 1))
                    parts = int(rng.integers(1, 4))
                    null_fraction = (0.0, 0.1, 0.5, 1.0)[int(rng.integers(4))]
                    flavour = ("small", "small", "edges", "one")[int(rng.integers(4))]
                    cases.append(make_case(rng, t, order, start, end, n, parts, null_fraction, flavour, conforming))
    return cases


# ---- tests/golden/window_range_vectors.json -------------------------------------------------------------------------------------------------------
TYPE_IDS = {"BIGINT": BIGINT, "INTEGER": INTEGER, "DATE": DATE, "DOUBLE": DOUBLE}
ORDER_IDS = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}
BOUND_IDS = {"UNBOUNDED_PRECEDING": UNBOUNDED_PRECEDING, "PRECEDING": PRECEDING, "CURRENT_ROW": CURRENT_ROW, "FOLLOWING": FOLLOWING, "UNBOUNDED_FOLLOWING": UNBOUNDED_FOLLOWING}
VARCHAR = 6
COUNT_ALL, COUNT_COLUMN, SUM_BIGINT, MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE = 1, 2, 3, 7, 8, 9, 10
FIRST_VALUE, LAST_VALUE, AGGREGATE = 7, 8, 9


def golden_table(case):
    """A golden case as an operator: (types, rows, output channels, functions, partition channels, sort order, expected rows).  The bound channels are
    computed as a planner would: in the key's type for whole-number offsets, in DOUBLE (the key cast to DOUBLE as the comparison key) for the decimal ones,
    with date_add for an interval on a DATE key.  Every array_agg(a) the reference lists becomes count(*), count(a), first_value(a), last_value(a) and,
    over a BIGINT or DOUBLE copy of a (a DATE as its day count), sum / min / max: `expected` holds what the listed arrays say, in the listed order."""
    import date_fn_expected as D
    from window_expected import Fn

    def days(v):
        y, m, d = (int(x) for x in v.split("-"))
        return D.to_days(y, m, d)
    columns, key_name, key_type = case["columns"], case["key"], TYPE_IDS[case["key_type"]]
    raw = case["rows"]
    is_date = lambda v: isinstance(v, str) and len(v) == 10 and v[4] == "-" and v[7] == "-"
    convert = lambda v: days(v) if is_date(v) else v
    column = lambda name: [convert(r[columns.index(name)]) for r in raw]
    key = column(key_name)
    if key_type == DOUBLE:
        key = [None if v is None else float(v) for v in key]
    windows = [o for o in case["outputs"] if "key" in o and "skip" not in o]
    order = ORDER_IDS[windows[0]["order"]]
    partition = windows[0]["partition"]
    assert all(ORDER_IDS[w["order"]] == order and w["partition"] == partition for w in windows)
    types, table = [key_type], [key]   # channel 0: the sort key
    partition_channels = []
    if partition is not None:
        types.append(VARCHAR)
        table.append(column(partition))
        partition_channels = [1]

    def add(t, values):
        types.append(t)
        table.append(values)
        return len(types) - 1
    as_double = None
    functions, derive = [], []
    for w in windows:
        def offsets(b):
            if "column" in b:
                return [r[columns.index(b["column"])] * b["by"] if b["op"] == "*" else r[columns.index(b["column"])] / b["by"] for r in raw]
            return [b["value"]] * len(raw)
        spec = {}
        for side in ("start", "end"):
            b = w[side]
            kind = BOUND_IDS[b["type"]]
            spec[side] = (kind, -1, -1)
            if kind not in (PRECEDING, FOLLOWING):
                continue
            subtract = (kind == PRECEDING) == ascending(order)
            offs = offsets(b)
            if "unit" in b:
                values = [None if k is None else D.date_add(b["unit"], -o if subtract else o, k) for k, o in zip(key, offs)]
                spec[side] = (kind, add(DATE, values), 0)
            elif key_type == DOUBLE or any(isinstance(o, float) for o in offs):
                if as_double is None:
                    as_double = 0 if key_type == DOUBLE else add(DOUBLE, [None if k is None else float(k) for k in key])
                values = [None if k is None else (float(k) - float(o) if subtract else float(k) + float(o)) for k, o in zip(key, offs)]
                spec[side] = (kind, add(DOUBLE, values), as_double)
            else:
                spec[side] = (kind, add(key_type, [bound_value(key_type, k, o, subtract) for k, o in zip(key, offs)]), 0)
        frame = RangeFrame(spec["start"][0], spec["end"][0], spec["start"][1], spec["end"][1], spec["start"][2], spec["end"][2])
        values = column(w["argument"])
        floats = any(isinstance(v, float) for v in values)
        if floats:
            values = [None if v is None else float(v) for v in values]
        argument = 0 if w["argument"] == key_name else add(DOUBLE if floats else (DATE if any(is_date(r[columns.index(w["argument"])]) for r in raw) else BIGINT), values)
        number = add(DOUBLE if floats else BIGINT, values)
        functions += [Fn(AGGREGATE, (), frame, COUNT_ALL), Fn(AGGREGATE, (argument,), frame, COUNT_COLUMN), Fn(FIRST_VALUE, (argument,), frame), Fn(LAST_VALUE, (argument,), frame)]
        if floats:
            functions += [Fn(AGGREGATE, (number,), frame, MIN_DOUBLE), Fn(AGGREGATE, (number,), frame, MAX_DOUBLE)]
        else:
            functions += [Fn(AGGREGATE, (number,), frame, SUM_BIGINT), Fn(AGGREGATE, (number,), frame, MIN_BIGINT), Fn(AGGREGATE, (number,), frame, MAX_BIGINT)]
        derive.append(floats)
    outputs = [o for o in case["outputs"] if "key" not in o]
    output_channels = [0 if o["column"] == key_name else partition_channels[0] for o in outputs]
    expected = []
    for listed in case["expected"]:
        row, at = [], 0
        for o in case["outputs"]:
            if "skip" in o:
                at += 1
                continue
            v = listed[at]
            at += 1
            if "key" not in o:
                v = convert(v)
                row.append(float(v) if key_type == DOUBLE and o["column"] == key_name and v is not None else v)
                continue
            floats = derive[len([x for x in case["outputs"][:case["outputs"].index(o)] if "key" in x and "skip" not in x])]
            frame_values = [convert(x) for x in (v or [])]
            if floats:
                frame_values = [None if x is None else float(x) for x in frame_values]
            present = [x for x in frame_values if x is not None]
            row += [len(frame_values), len(present), frame_values[0] if frame_values else None, frame_values[-1] if frame_values else None]
            if not floats:
                row.append(sum(present) if present else None)
            row += [min(present) if present else None, max(present) if present else None]
        expected.append(tuple(row))
    rows = [tuple(col[i] for col in table) for i in range(len(raw))]
    return types, rows, output_channels, functions, partition_channels, order, expected

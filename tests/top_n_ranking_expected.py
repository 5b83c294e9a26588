"""Expected values of TopNRankingOperator: the oracle's GroupByHash over the pages in order for the group ids (BigintGroupByHash for a single BIGINT
key, MultiChannelGroupByHash otherwise, none without partition channels -- exactly as tests/row_number_expected.py takes them), then a Python
restatement of SimplePageWithPositionComparator (M/operator/SimplePageWithPositionComparator.java:58-79: nulls placed by the SortOrder, Long /
Integer / Boolean compare, Double.compare, Slice.compareTo = unsigned bytes then length, negated for DESC) under a STABLE sort per group, so
that rows that compare equal rank in arrival order, and the two keep rules:
  ROW_NUMBER  the first n rows of a group in that order, numbered 1 ..
  RANK        every row whose rank (1 + the rows of its group that sort strictly before it) is <= n; peers (comparator == 0) share a rank.
Rows are tuples of Python values (None = null), one per source channel."""
import functools
import struct

from row_number_expected import RowNumberOracle

BIGINT, INTEGER, DATE, DOUBLE, BOOLEAN, VARCHAR = 1, 2, 3, 4, 5, 6
ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST = 0, 1, 2, 3
ROW_NUMBER, RANK = 0, 1


def _double_bits(v):
    """Double.doubleToLongBits: every NaN is the canonical one; as a signed long"""
    if v != v:
        return 0x7FF8000000000000
    return struct.unpack("<q", struct.pack("<d", v))[0]


def compare_values(type_id, a, b):
    """the type's COMPARISON operator on two non-null values: <0, 0, >0"""
    if type_id == DOUBLE:   # Double.compare: -0.0 < 0.0, NaN above everything and equal to itself
        if a < b:
            return -1
        if a > b:
            return 1
        x, y = _double_bits(a), _double_bits(b)
        return (x > y) - (x < y)
    if type_id == VARCHAR:
        x = a.encode("utf-8") if isinstance(a, str) else bytes(a)
        y = b.encode("utf-8") if isinstance(b, str) else bytes(b)
        return (x > y) - (x < y)   # bytes compare as unsigned, then by length
    if type_id == BOOLEAN:
        a, b = bool(a), bool(b)
    return (a > b) - (a < b)


def compare_rows(types, sort_channels, sort_orders, left, right):
    for ch, order in zip(sort_channels, sort_orders):
        a, b = left[ch], right[ch]
        nulls_first = order in (ASC_NULLS_FIRST, DESC_NULLS_FIRST)
        if a is None or b is None:   # TypeOperators.orderNulls
            if a is None and b is None:
                continue
            return (-1 if nulls_first else 1) if a is None else (1 if nulls_first else -1)
        c = compare_values(types[ch], a, b)
        if c:
            return c if order in (ASC_NULLS_FIRST, ASC_NULLS_LAST) else -c
    return 0


class TopNRankingOracle:
    def __init__(self, oracle, types, partition_channels, sort_channels, sort_orders, ranking_type, max_rank, expected_positions=10):
        assert ranking_type in (ROW_NUMBER, RANK) and max_rank > 0
        self.types, self.sort_channels, self.sort_orders = list(types), list(sort_channels), list(sort_orders)
        self.ranking_type, self.max_rank = ranking_type, max_rank
        self.groups = RowNumberOracle(oracle, [types[c] for c in partition_channels], None, expected_positions)
        self.rows = {}   # group id -> its rows in arrival order

    def add_page(self, key_cols, rows):
        """key_cols: the oracle columns of the partition channels; rows: the page's rows as tuples over all source channels"""
        ids = self.groups.group_ids(key_cols, len(rows))
        for g, row in zip(ids, rows):
            self.rows.setdefault(int(g), []).append(tuple(row))

    def result(self):
        """[(row, ranking)] in output order: groups by id, rows by the comparator, equal rows in arrival order"""
        cmp = functools.partial(compare_rows, self.types, self.sort_channels, self.sort_orders)
        out = []
        for g in sorted(self.rows):
            ordered = sorted(self.rows[g], key=functools.cmp_to_key(cmp))   # stable
            rank = 0
            for i, row in enumerate(ordered):
                if self.ranking_type == ROW_NUMBER:
                    rank = i + 1
                elif i == 0 or cmp(ordered[i - 1], row) != 0:
                    rank = i + 1
                if rank > self.max_rank:
                    break   # rankings never decrease along a group
                out.append((row, rank))
        return out


def cell_token(v):
    """a value that compares bit for bit: doubles by their bytes (NaN == NaN, -0.0 != 0.0)"""
    return ("double", struct.pack("<d", v)) if isinstance(v, float) else v


def tokens(rows):
    return [tuple(cell_token(v) for v in r) for r in rows]


def expected_output(oracle, types, pages_rows, key_pages, output_channels, partition_channels, sort_channels, sort_orders, ranking_type, max_rank, partial=False,
                    expected_positions=10):
    """the operator's one output page as rows: the output channels, then the ranking unless partial ([] = no page)"""
    o = TopNRankingOracle(oracle, types, partition_channels, sort_channels, sort_orders, ranking_type, max_rank, expected_positions)
    for keys, rows in zip(key_pages, pages_rows):
        o.add_page(keys, rows)
    return [tuple(row[c] for c in output_channels) + (() if partial else (rank,)) for row, rank in o.result()]


NP_TYPES = {BIGINT: "int64", INTEGER: "int32", DATE: "int32", DOUBLE: "float64", BOOLEAN: "uint8"}


def oracle_col(oracle, type_id, values):
    """one oracle column from Python values (None = null)"""
    import numpy as np

    if type_id == VARCHAR:
        return oracle.Col(VARCHAR, list(values))
    nulls = np.array([v is None for v in values], dtype=np.uint8)
    data = np.array([0 if v is None else v for v in values], dtype=NP_TYPES[type_id])
    return oracle.Col(type_id, data, nulls if nulls.any() else None)


def golden_case_inputs(case):
    """(type ids, pages as row tuples with NaN decoded, expected rows with NaN decoded) of a case of tests/golden/top_n_ranking_vectors.json"""
    names = {"BIGINT": BIGINT, "INTEGER": INTEGER, "DATE": DATE, "DOUBLE": DOUBLE, "BOOLEAN": BOOLEAN, "VARCHAR": VARCHAR}
    decode = lambda v: float("nan") if v == "NaN" else v
    types = [names[t] for t in case["types"]]
    pages = [[tuple(decode(v) for v in r) for r in page] for page in case["pages"]]
    expected = [tuple(decode(v) for v in r) for r in case["expected"]]
    return types, pages, expected

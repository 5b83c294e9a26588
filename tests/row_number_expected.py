"""Expected values of RowNumberOperator and LimitOperator: the oracle's GroupByHash over the pages in order (BigintGroupByHash for a single
BIGINT key, MultiChannelGroupByHash otherwise, as GroupByHash.createGroupByHash picks; no hash at all without partition channels), then the
reference's two loops in Python (M/operator/RowNumberOperator.java:301-311 createRowNumberBlock, :313-342 getSelectedRows), and
LimitOperator.addInput's arithmetic (M/operator/LimitOperator.java:98-111)."""
import numpy as np

BIGINT = 1


class RowNumberOracle:
    """one operator's hash + partitionRowCount; key_cols are lists of oracle columns (oracle.Col), one per partition channel"""

    def __init__(self, oracle, partition_types, max_rows=None, expected_positions=10):
        self.partition_types = list(partition_types)
        self.max_rows = max_rows
        self.single_bigint = self.partition_types == [BIGINT]
        self.hash = None
        if self.partition_types:
            self.hash = oracle.BigintGroupByHash(expected_positions) if self.single_bigint else oracle.MultiChannelGroupByHash(self.partition_types, expected_positions)
        self.count = {}   # LongBigArray partitionRowCount

    def group_ids(self, key_cols, n):
        if self.hash is None or n == 0:
            return np.zeros(n, dtype=np.int64)
        return np.asarray(self.hash.get_group_ids(key_cols[0]) if self.single_bigint else self.hash.get_group_ids(key_cols))

    def finished_early(self):
        """isFinished without finish() (:191-196): the single partition of an operator with a limit is full"""
        return self.hash is None and self.max_rows is not None and self.count.get(0, 0) == self.max_rows

    def page(self, key_cols, n):
        """(kept positions, their row numbers) of one input page, or None where the reference returns no page"""
        ids = self.group_ids(key_cols, n)
        positions, numbers = [], []
        for i in range(n):
            g = int(ids[i])
            c = self.count.get(g, 0)
            if self.max_rows is not None and c == self.max_rows:   # :323-325
                continue
            positions.append(i)
            numbers.append(c + 1)
            self.count[g] = c + 1
        if self.max_rows is not None and not positions:   # :335-337
            return None
        return positions, numbers


def expected_row_numbers(oracle, partition_types, key_pages, sizes, max_rows=None):
    """per input page the operator takes: (positions, row numbers) or None.  An operator without partition channels stops taking pages
    once its limit is reached (needsInput is false, :204-207): later pages have no entry."""
    o = RowNumberOracle(oracle, partition_types, max_rows)
    out = []
    for cols, n in zip(key_pages, sizes):
        if o.finished_early():
            break
        out.append(o.page(cols, n))
    return out


def expected_limit(sizes, limit):
    """LimitOperator over pages of the given sizes: rows that come out of every page the operator takes (needsInput: remaining > 0)"""
    out, remaining = [], limit
    for n in sizes:
        if remaining == 0:
            break
        take = n if n <= remaining else remaining
        remaining -= take
        out.append(take)
    return out

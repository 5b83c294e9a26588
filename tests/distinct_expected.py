"""Expected values of MarkDistinctOperator and DistinctLimitOperator: the oracle's GroupByHash over the pages in order (BigintGroupByHash for a
single BIGINT key, MultiChannelGroupByHash otherwise, as GroupByHash.createGroupByHash picks), then the reference's two loops in Python
(M/operator/MarkDistinctHash.java:58-66, M/operator/DistinctLimitOperator.java:191-201)."""
import numpy as np

BIGINT = 1


class DistinctOracle:
    """one operator's hash + nextDistinctId; key_pages are lists of oracle columns (oracle.Col), one list per page"""

    def __init__(self, oracle, key_types, expected_size=10_000):
        self.key_types = list(key_types)
        self.single_bigint = self.key_types == [BIGINT]
        self.hash = oracle.BigintGroupByHash(expected_size) if self.single_bigint else oracle.MultiChannelGroupByHash(self.key_types, expected_size)
        self.next_distinct_id = 0

    def group_ids(self, key_cols):
        if key_cols[0].n == 0:
            return np.zeros(0, dtype=np.int64)
        return self.hash.get_group_ids(key_cols[0]) if self.single_bigint else self.hash.get_group_ids(key_cols)

    def mark(self, key_cols):
        """MarkDistinctHash.markDistinctRows (:58-66): one bool per row"""
        ids = self.group_ids(key_cols)
        out = np.zeros(len(ids), dtype=bool)
        for i, g in enumerate(ids):
            if g == self.next_distinct_id:
                out[i] = True
                self.next_distinct_id += 1
        return out

    def distinct_positions(self, key_cols, remaining):
        """DistinctLimitOperator.getOutput (:191-201): (kept positions, remaining limit after the page)"""
        ids = self.group_ids(key_cols)
        kept = []
        for i, g in enumerate(ids):
            if g == self.next_distinct_id:
                kept.append(i)
                remaining -= 1
                self.next_distinct_id += 1
                if remaining == 0:
                    break
        return kept, remaining


def expected_marks(oracle, key_types, key_pages):
    o = DistinctOracle(oracle, key_types)
    return [o.mark(cols) for cols in key_pages]


def expected_distinct_limit(oracle, key_types, key_pages, limit):
    """per input page the operator takes: the kept positions (an empty list = no output page).  Pages after the limit is reached are
    not taken (needsInput is false) and have no entry."""
    o = DistinctOracle(oracle, key_types, max(1, min(limit, 10_000)))
    out, remaining = [], limit
    for cols in key_pages:
        if remaining == 0:
            break
        kept, remaining = o.distinct_positions(cols, remaining)
        out.append(kept)
    return out

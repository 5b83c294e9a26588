"""What the merge of sorted page streams must give, restated in plain Python (imports neither the library nor a GPU).

MergeSortedPages.mergeSortedPages (M/util/MergeSortedPages.java:41-142) over WorkProcessorUtils.mergeSorted (M/operator/WorkProcessorUtils.java:110-152):
the rows of k sorted streams in the order of SimplePageWithPositionComparator (SimplePageWithPositionComparator.java:58-79 + TypeOperators.java:578-596:
nulls placed by the SortOrder, values by the type's COMPARISON operator, negated for DESC).  The reference's binary heap leaves the order of rows
that compare equal across streams unspecified; the library's rule is deterministic -- lower stream first (in addSplit order), inside a stream in
arrival order -- and that is a STABLE sort of the rows listed stream by stream.

A row is a tuple over all channels (None = null); a page a list of rows; a stream a list of pages.  Types are the library's type codes."""
import functools
import struct

BIGINT, INTEGER, DATE, DOUBLE, BOOLEAN, VARCHAR = 1, 2, 3, 4, 5, 6
ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST = 0, 1, 2, 3
TYPE_CODES = {"BIGINT": BIGINT, "INTEGER": INTEGER, "DATE": DATE, "DOUBLE": DOUBLE, "BOOLEAN": BOOLEAN, "VARCHAR": VARCHAR}
ORDER_CODES = {"ASC_NULLS_FIRST": 0, "ASC_NULLS_LAST": 1, "DESC_NULLS_FIRST": 2, "DESC_NULLS_LAST": 3}


def _double_key(v):
    """Double.compare as an integer key: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN, all NaNs equal"""
    if v != v:
        return 1 << 64
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~bits & 0xFFFFFFFFFFFFFFFF) if bits >> 63 else (bits | (1 << 63))


def compare_cells(type_id, a, b):
    """the type's COMPARISON operator on two non-null cells: <0, 0, >0"""
    if type_id == DOUBLE:
        a, b = _double_key(a), _double_key(b)
    elif type_id == VARCHAR:   # Slice.compareTo: unsigned bytes, then length
        a = a.encode("utf-8") if isinstance(a, str) else bytes(a)
        b = b.encode("utf-8") if isinstance(b, str) else bytes(b)
    elif type_id == BOOLEAN:
        a, b = bool(a), bool(b)
    return -1 if a < b else (1 if a > b else 0)


def compare_rows(types, sort_channels, sort_orders, ra, rb):
    for ch, order in zip(sort_channels, sort_orders):
        a, b = ra[ch], rb[ch]
        nulls_first = order in (ASC_NULLS_FIRST, DESC_NULLS_FIRST)
        if a is None or b is None:
            if a is None and b is None:
                continue
            if a is None:
                return -1 if nulls_first else 1
            return 1 if nulls_first else -1
        c = compare_cells(types[ch], a, b)
        if c:
            return c if order in (ASC_NULLS_FIRST, ASC_NULLS_LAST) else -c
    return 0


def check_sorted(types, sort_channels, sort_orders, rows):
    for i in range(1, len(rows)):
        if compare_rows(types, sort_channels, sort_orders, rows[i - 1], rows[i]) > 0:
            raise ValueError("stream is not sorted at row %d: %r before %r" % (i, rows[i - 1], rows[i]))


def flatten(stream):
    return [tuple(row) for page in stream for row in page]


def merge_rows(types, sort_channels, sort_orders, streams):
    """the merged rows over all channels: a stable sort of the rows listed stream by stream.  Refuses a stream that is not sorted (the library
    does not check it and promises nothing about the order then)."""
    rows = []
    for stream in streams:
        flat = flatten(stream)
        check_sorted(types, sort_channels, sort_orders, flat)
        rows += flat
    return sorted(rows, key=functools.cmp_to_key(lambda a, b: compare_rows(types, sort_channels, sort_orders, a, b)))


def merge(types, sort_channels, sort_orders, output_channels, streams):
    return [tuple(row[c] for c in output_channels) for row in merge_rows(types, sort_channels, sort_orders, streams)]


def settled_counts(types, sort_channels, sort_orders, buffered, finished):
    """The settled-set rule.  buffered[s] = stream s's buffered rows, finished[s] = no row will follow them.  B = the smallest (last buffered
    row, stream index) over the unfinished streams, t_B its stream; a buffered row (r, s) is settled when (r, s) <= (B, t_B) lexicographically;
    with every stream finished every buffered row is.  -> the settled count per stream (a prefix: the streams are sorted), or None when an
    unfinished stream has no buffered row (there is no round then)."""
    cmp = lambda a, b: compare_rows(types, sort_channels, sort_orders, a, b)
    tb = None
    for s, (rows, done) in enumerate(zip(buffered, finished)):
        if done:
            continue
        if not rows:
            return None
        if tb is None or cmp(rows[-1], buffered[tb][-1]) < 0:
            tb = s
    if tb is None:
        return [len(rows) for rows in buffered]
    bound = buffered[tb][-1]
    counts = []
    for s, rows in enumerate(buffered):
        n = 0
        for r in rows:
            c = cmp(r, bound)
            if c < 0 or (c == 0 and s <= tb):
                n += 1
        counts.append(n)
    return counts


class StreamingModel:
    """The operator fed page by page: arrive(s, page) buffers a page of stream s, end(s) marks the stream finished, round() gives the rows
    (all channels) one round emits, or None when there is no round."""

    def __init__(self, types, sort_channels, sort_orders, k):
        self.types, self.sort_channels, self.sort_orders = types, sort_channels, sort_orders
        self.buffered = [[] for _ in range(k)]
        self.finished = [False] * k

    def arrive(self, s, page):
        self.buffered[s] += [tuple(r) for r in page]

    def end(self, s):
        self.finished[s] = True

    def round(self):
        counts = settled_counts(self.types, self.sort_channels, self.sort_orders, self.buffered, self.finished)
        if counts is None:
            return None
        taken = [[rows[:n]] for rows, n in zip(self.buffered, counts)]
        self.buffered = [rows[n:] for rows, n in zip(self.buffered, counts)]
        return merge_rows(self.types, self.sort_channels, self.sort_orders, taken)

    def done(self):
        return all(self.finished) and not any(self.buffered)


def cut_pages(rng, rows, page_rows, empty_pages=True):
    """`rows` cut into pages of 1..page_rows rows (random cuts), with an empty page here and there"""
    pages, at = [], 0
    while at < len(rows):
        if empty_pages and rng.random() < 0.15:
            pages.append([])
        n = int(rng.integers(1, page_rows + 1))
        pages.append(rows[at:at + n])
        at += n
    if empty_pages and rng.random() < 0.3:
        pages.append([])
    return pages


def sorted_streams(rng, types, sort_channels, sort_orders, make_row, lengths, page_rows, empty_pages=True):
    """k = len(lengths) sorted streams: stream s holds lengths[s] rows make_row(rng, s, i) (i = its sequence number before sorting, so that a
    payload channel can carry (stream, sequence)), sorted stably, cut into pages.  A length of 0 gives an empty stream (sometimes one empty page)."""
    key = functools.cmp_to_key(lambda a, b: compare_rows(types, sort_channels, sort_orders, a, b))
    streams = []
    for s, n in enumerate(lengths):
        rows = sorted((tuple(make_row(rng, s, i)) for i in range(n)), key=key)
        streams.append(cut_pages(rng, rows, page_rows, empty_pages) if n else ([[]] if rng.random() < 0.5 else []))
    return streams


def merge_ascending_bigint(keys, payloads):
    """the stable merge specialised to one non-null BIGINT key ascending, on arrays (one key array and one payload array per stream, each
    sorted): a stable sort of the concatenation by key.  The tile-edge tests run thousands of rows through it."""
    import numpy as np

    k = np.concatenate([np.asarray(x, dtype=np.int64) for x in keys] or [np.zeros(0, dtype=np.int64)])
    p = np.concatenate([np.asarray(x, dtype=np.int64) for x in payloads] or [np.zeros(0, dtype=np.int64)])
    for x in keys:
        if len(x) > 1 and (np.diff(np.asarray(x, dtype=np.int64)) < 0).any():
            raise ValueError("stream is not sorted")
    order = np.argsort(k, kind="stable")
    return k[order], p[order]

"""MergeOperator on the GPU through the C ABI: the reference's test literals with their choreography, a differential against the plain Python
model (tests/merge_expected.py) over types, sort orders, feeding patterns and stream counts, ties, the edges of the merge-path tile, the
streaming contract round by round, the route by profile scopes, and errors / lifecycle.  Every case is a few thousand rows at most."""
import json
import os
import struct

import numpy as np
import pytest

import merge_expected as M
from key_cases import special_doubles

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_vectors.json")
NOT_SUPPORTED, INVALID_ARGUMENT, INTERNAL = -8, -1, -5
T, I = 2304, 9   # the merge-path kernel's tile (pairs per workgroup) and items per lane: csrc/merge.h kMergeTile, kMergeItems
WOULD_BLOCK = 1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def norm(row):
    """a row with doubles as their bits: NaN payloads and the sign of zero must survive the merge"""
    return tuple(struct.pack("<d", v) if isinstance(v, float) else v for v in row)


def make_page(pkg, types, rows):
    return pkg.Page(*[pkg.Block(t, [r[c] for r in rows]) for c, t in enumerate(types)], position_count=len(rows))


def make_armed_source(pkg):
    class ArmedSource(pkg.PageSource):
        """a page source that hands out only what it was armed with: get_next_page returns 0 until arm() queues a page; end() finishes the
        stream once the queue is drained; is_blocked says 1 while the queue is empty and the stream has not ended; fail_next: the next
        get_next_page returns that (negative) code"""

        def __init__(self):
            super().__init__([])
            self.queue, self.ended, self.fail_next, self.closes = [], False, 0, 0

        def arm(self, page):
            self.queue.append(page)

        def end(self):
            self.ended = True

        def _next(self, user, out):
            if self.fail_next:
                return self.fail_next
            if not self.queue:
                return 0
            self.current = self.queue.pop(0)
            cp, self._keep = self.current.to_c()
            out[0].position_count, out[0].channel_count, out[0].blocks = cp.position_count, cp.channel_count, cp.blocks
            return 1

        def _finished(self, user):
            return 1 if self.ended and not self.queue else 0

        def _blocked(self, user):
            return 1 if not self.queue and not self.ended else 0

        def _close(self, user):
            self.closes += 1
            self.closed = True

    return ArmedSource


def new_operator(pkg, ctx, types, out, sort_channels, orders):
    fac = pkg.MergeOperatorFactory(ctx, 3, types, out, sort_channels, orders)
    return fac, fac.createOperator()


def drain(op, limit=10_000):
    """pullAvailablePages: getOutput until finished; -> the pages' rows, page by page"""
    pages = []
    for _ in range(limit):
        if op.isFinished():
            break
        assert not op.needsInput()
        o = op.getOutput()
        if o is not None:
            pages.append(o.to_host().rows())
            o.release()
    assert op.isFinished() and not op.needsInput() and not op.isBlocked()
    return pages


def run_all_at_once(pkg, ctx, types, sort_channels, orders, out, streams):
    fac, op = new_operator(pkg, ctx, types, out, sort_channels, orders)
    sources = [pkg.PageSource([make_page(pkg, types, p) for p in s]) for s in streams]
    for s in sources:
        op.addSplit(s)
    op.noMoreSplits()
    rows = [r for page in drain(op) for r in page]
    assert all(s.closed for s in sources) and op.memoryBytes() == 0
    op.close()
    fac.close()
    return rows


def run_page_per_poll(pkg, ctx, types, sort_channels, orders, out, streams, last_stream=None, watch=None):
    """One page per stream per getOutput (last_stream: that stream delivers only after every other stream has ended), every round checked
    against the model's settled set: no row early, none held back.  -> all output rows.  watch(op) is called after every poll."""
    Armed = make_armed_source(pkg)
    fac, op = new_operator(pkg, ctx, types, out, sort_channels, orders)
    sources = [Armed() for _ in streams]
    for s in sources:
        op.addSplit(s)
    op.noMoreSplits()
    model = M.StreamingModel(types, sort_channels, orders, len(streams))
    at = [0] * len(streams)
    rows = []
    for _ in range(100_000):
        if op.isFinished():
            break
        others_done = all(model.finished[s] for s in range(len(streams)) if s != last_stream)
        for s, stream in enumerate(streams):
            if model.finished[s] or (s == last_stream and not others_done):
                continue
            if at[s] < len(stream):
                sources[s].arm(make_page(pkg, types, stream[at[s]]))
                model.arrive(s, stream[at[s]])
                at[s] += 1
            if at[s] >= len(stream):
                sources[s].end()
                model.end(s)
        want = model.round()
        o = op.getOutput()
        if want is None or not want:
            assert o is None
            if want is None:
                assert op.last_get_output_status == WOULD_BLOCK and op.isBlocked() and not op.isFinished()
        else:
            assert o is not None, "a round held its settled rows back"
            got = o.to_host().rows()
            o.release()
            assert [norm(r) for r in got] == [norm(tuple(r[c] for c in out)) for r in want]
            rows += got
        if watch:
            watch(op)
    assert op.isFinished() and model.done() and all(s.closes == 1 for s in sources)
    op.close()
    fac.close()
    return rows


# ---- the reference's literals --------------------------------------------------------------------------------------------------------
def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def decode(case):
    types = [M.TYPE_CODES[t] for t in case["types"]]
    orders = [M.ORDER_CODES[o] for o in case["sort_orders"]]
    streams = [[[tuple(r) for r in page] for page in stream] for stream in case["streams"]]
    return types, case["sort_channels"], orders, case["output_channels"], streams, [tuple(r) for r in case["expected"]]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_golden_cases_through_the_c_abi(pkg, ctx, case):
    types, sort_channels, orders, out, streams, expected = decode(case)
    assert run_all_at_once(pkg, ctx, types, sort_channels, orders, out, streams) == expected
    assert run_page_per_poll(pkg, ctx, types, sort_channels, orders, out, streams) == expected


@pytest.mark.parametrize("case", [c for c in golden_cases() if "steps" in c], ids=lambda c: c["name"])
def test_golden_choreography(pkg, ctx, case):
    """TestMergeOperator: blocked before noMoreSplits, blocked on each source in turn, unblocked when its page is there, needsInput false,
    addInput refused, finished and unblocked at the end"""
    types, sort_channels, orders, out, streams, expected = decode(case)
    Armed = make_armed_source(pkg)
    fac, op = new_operator(pkg, ctx, types, out, sort_channels, orders)
    assert not op.isFinished() and op.isBlocked() and not op.needsInput()
    sources = [Armed() for _ in streams]
    for s in sources:
        op.addSplit(s)
        assert not op.isFinished() and op.isBlocked()
    assert op.getOutput() is None and op.last_get_output_status == WOULD_BLOCK
    op.noMoreSplits()
    with pytest.raises(pkg.TgpuError) as e:
        op.addInput(make_page(pkg, types, streams[0][0]))
    assert e.value.code == NOT_SUPPORTED
    rows = []
    for step in case["steps"]:
        if step[0] == "blocked":
            o = op.getOutput()
            if o is not None:   # rows that are settled already may leave early; the reference's page cuts are not part of the contract
                rows += o.to_host().rows()
                o = op.getOutput()
            assert o is None and op.last_get_output_status == WOULD_BLOCK and not op.isFinished() and op.isBlocked()
        elif step[0] == "add":
            _, s, page, last = step
            sources[s].arm(make_page(pkg, types, streams[s][page]))
            if last:
                sources[s].end()
        elif step[0] == "unblocked":
            assert not op.isBlocked()
        else:
            assert not op.isBlocked()
            rows += [r for p in drain(op) for r in p]
    assert rows == expected and op.isFinished() and not op.isBlocked() and all(s.closes == 1 for s in sources)
    op.close()
    fac.close()


# ---- differential against the model ----------------------------------------------------------------------------------------------------
VARCHAR_TIES = ["", "a", "abcdefgh", "abcdefghA", "abcdefghB", "abcdefghAB", "abcdefg", "abcdefghé", "zzzzzzzzzzzzzzzz", "abcdefghA"]


def cell_maker(type_id, cardinality, nulls, specials):
    def cell(rng):
        if nulls and rng.random() < nulls:
            return None
        if type_id == M.BIGINT:
            return int(rng.integers(0, cardinality)) * (2**40 + 1) - 2**45 if cardinality > 4 else int(rng.integers(0, cardinality))
        if type_id in (M.INTEGER, M.DATE):
            return int(rng.integers(-cardinality // 2, cardinality // 2 + 1))
        if type_id == M.DOUBLE:
            return specials[int(rng.integers(0, len(specials)))] if specials is not None else float(rng.integers(0, cardinality)) / 4 - 3
        if type_id == M.BOOLEAN:
            return bool(rng.integers(0, 2))
        return VARCHAR_TIES[int(rng.integers(0, len(VARCHAR_TIES)))] if cardinality <= 16 else "k%05d" % rng.integers(0, cardinality)
    return cell


def differential(pkg, ctx, seed, types, sort_channels, orders, out, lengths, cardinality=50, nulls=0.1, page_rows=300, feeds=("all", "poll", "last")):
    rng = np.random.default_rng(seed)
    specials = [v.item() for v in special_doubles(rng, 64, (-5, 5))]
    makers = [cell_maker(t, cardinality if c == sort_channels[0] else 1000, nulls, specials if c in sort_channels else None) for c, t in enumerate(types)]

    def make_row(rng, s, i):
        row = [m(rng) for m in makers]
        row[-1] = s * 1_000_000 + i   # the last channel (BIGINT, never a sort key) carries (stream, sequence)
        return row
    streams = M.sorted_streams(rng, types, sort_channels, orders, make_row, lengths, page_rows)
    want = [norm(r) for r in M.merge(types, sort_channels, orders, out, streams)]
    if "all" in feeds:
        assert [norm(r) for r in run_all_at_once(pkg, ctx, types, sort_channels, orders, out, streams)] == want
    if "poll" in feeds:
        assert [norm(r) for r in run_page_per_poll(pkg, ctx, types, sort_channels, orders, out, streams)] == want
    if "last" in feeds and len(streams) > 1:
        assert [norm(r) for r in run_page_per_poll(pkg, ctx, types, sort_channels, orders, out, streams, last_stream=len(streams) // 2)] == want


ALL_TYPES = [M.BIGINT, M.INTEGER, M.DATE, M.DOUBLE, M.BOOLEAN, M.VARCHAR]


@pytest.mark.parametrize("key_type", ALL_TYPES)
@pytest.mark.parametrize("order", [M.ASC_NULLS_FIRST, M.ASC_NULLS_LAST, M.DESC_NULLS_FIRST, M.DESC_NULLS_LAST])
def test_every_type_as_the_sort_key_under_every_order(pkg, ctx, key_type, order):
    """one sort key (DOUBLE keys from special_doubles: NaN payloads, both zeros, infinities; VARCHAR keys that share their first 8 bytes, a
    prefix of another, the empty string next to null), k = 3, a VARCHAR and a DOUBLE payload"""
    types = [key_type, M.VARCHAR, M.DOUBLE, M.BIGINT]
    differential(pkg, ctx, 100 + key_type * 4 + order, types, [0], [order], [0, 1, 2, 3], [700, 400, 0], cardinality=12 if key_type == M.VARCHAR else 60, feeds=("all", "poll"))


@pytest.mark.parametrize("nkeys", [2, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 33])
def test_several_keys_low_cardinality_first_key_and_channel_lists(pkg, ctx, nkeys, k):
    """a first key of 3 distinct values (most comparisons fall through to the full comparator), mixed orders, output channel lists that drop
    and reorder channels, every stream count, all three feeding patterns"""
    types = [M.INTEGER, M.VARCHAR, M.DOUBLE, M.BOOLEAN, M.BIGINT]
    sort_channels, orders = [0, 1, 2][:nkeys], [M.DESC_NULLS_LAST, M.ASC_NULLS_FIRST, M.DESC_NULLS_FIRST][:nkeys]
    rng = np.random.default_rng(k)
    lengths = [int(x) for x in rng.integers(0, 2400 // k + 2, k)]
    differential(pkg, ctx, 7 * k + nkeys, types, sort_channels, orders, [4, 1, 0] if nkeys == 2 else [2, 4], lengths, cardinality=3, page_rows=150 if k < 8 else 40)


def test_bigint_low_cardinality_single_key(pkg, ctx):
    differential(pkg, ctx, 5, [M.BIGINT, M.BIGINT], [0], [M.ASC_NULLS_LAST], [1, 0], [900, 900, 900, 17], cardinality=4, nulls=0.05)


@pytest.mark.parametrize("k", [2, 5])
def test_ties_come_out_stream_major_then_in_arrival_order(pkg, ctx, k):
    types, n = [M.BIGINT, M.VARCHAR, M.BIGINT], 1200
    streams = [[[(7, "same", s * 1_000_000 + p * 100 + i) for i in range(100)] for p in range(n // 100)] for s in range(k)]
    want = [(s * 1_000_000 + p * 100 + i,) for s in range(k) for p in range(n // 100) for i in range(100)]
    for sort_channels, orders in (([0], [M.ASC_NULLS_FIRST]), ([1, 0], [M.DESC_NULLS_LAST, M.ASC_NULLS_FIRST])):
        assert run_all_at_once(pkg, ctx, types, sort_channels, orders, [2], streams) == want
        assert run_page_per_poll(pkg, ctx, types, sort_channels, orders, [2], streams) == want


# ---- tile edges: BIGINT key + payload as arrays -----------------------------------------------------------------------------------------
def run_arrays(pkg, ctx, streams):
    """streams[s] = (keys, payload) int64 arrays, each stream one page; -> (keys, payload) of the output"""
    fac, op = new_operator(pkg, ctx, [M.BIGINT, M.BIGINT], [0, 1], [0], [M.ASC_NULLS_FIRST])
    for keys, payload in streams:
        op.addSplit(pkg.PageSource([pkg.Page(pkg.Block(pkg.BIGINT, keys), pkg.Block(pkg.BIGINT, payload))] if len(keys) else []))
    op.noMoreSplits()
    got_k, got_p = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for _ in range(1000):
        if op.isFinished():
            break
        o = op.getOutput()
        if o is not None:
            h = o.to_host()
            got_k.append(h.getBlock(0).values.copy())
            got_p.append(h.getBlock(1).values.copy())
            o.release()
    assert op.isFinished()
    op.close()
    fac.close()
    return np.concatenate(got_k), np.concatenate(got_p)


def check_arrays(pkg, ctx, key_arrays):
    streams = [(np.asarray(k, dtype=np.int64), s * 10_000_000 + np.arange(len(k), dtype=np.int64)) for s, k in enumerate(key_arrays)]
    want_k, want_p = M.merge_ascending_bigint([k for k, _ in streams], [p for _, p in streams])
    got_k, got_p = run_arrays(pkg, ctx, streams)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_p, want_p), [len(k) for k in key_arrays]


EDGE_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]
PAIRS = [(a, T) for a in EDGE_LENGTHS] + [(a, a) for a in EDGE_LENGTHS] + [(2 * T + 1, 1), (1, 2 * T + 1), (T - 1, T + 1), (257, 65), (T, 0), (0, T)] + \
        [(a, n - a) for n in (I - 1, I, I + 1) for a in (0, 1, n // 2, n)]
TRIPLES = [(a, T, 257) for a in EDGE_LENGTHS] + [(T + 1, a, T - 1) for a in EDGE_LENGTHS] + [(1, 1, 1), (0, 0, 5), (2 * T + 1, 2 * T + 1, 2 * T + 1), (3, 3, 3), (3, 3, 2), (4, 3, 3)]


def pattern_keys(pattern, lengths):
    k = len(lengths)
    if pattern == "interleaved":      # stream s holds s, s + k, s + 2k, ...: every output alternates between the streams
        return [s + k * np.arange(n, dtype=np.int64) for s, n in enumerate(lengths)]
    if pattern == "equal":            # every key the same: the full comparator and the tie rule decide every step
        return [np.zeros(n, dtype=np.int64) for n in lengths]
    base = 0                          # disjoint ranges: stream a entirely before stream b ("forward"), or the reverse
    out = [None] * k
    for s in (range(k) if pattern == "forward" else reversed(range(k))):
        out[s] = base + np.arange(lengths[s], dtype=np.int64)
        base += lengths[s]
    return out


@pytest.mark.parametrize("pattern", ["interleaved", "forward", "reverse", "equal"])
def test_tile_edges_two_streams(pkg, ctx, pattern):
    """T = 2,304 pairs per workgroup tile, I = 9 items per lane.  Per-stream lengths around the wave, the workgroup and the tile (T - 1, T,
    T + 1, 2T + 1) and total round sizes I - 1, I, I + 1, in four data patterns"""
    for lengths in PAIRS:
        check_arrays(pkg, ctx, pattern_keys(pattern, lengths))


@pytest.mark.parametrize("pattern", ["interleaved", "forward", "reverse", "equal"])
def test_tile_edges_three_streams(pkg, ctx, pattern):
    """three runs: the third is carried through the first pass (T and I as above)"""
    for lengths in TRIPLES:
        check_arrays(pkg, ctx, pattern_keys(pattern, lengths))


@pytest.mark.parametrize("long_at", [0, 16, 32])
def test_one_very_long_run_against_many_one_row_runs(pkg, ctx, long_at):
    keys = [np.array([37 * s], dtype=np.int64) for s in range(33)]
    keys[long_at] = np.arange(2 * T + 1, dtype=np.int64)
    check_arrays(pkg, ctx, keys)


def test_unsorted_input_terminates_and_keeps_the_row_count(pkg, ctx):
    """which row comes out where is unspecified then; the operator still ends, emits as many rows as it took, each of them a row of the
    input, and reads nothing but its buffers"""
    rng = np.random.default_rng(3)
    streams = [(rng.integers(0, 100, n).astype(np.int64), s * 10_000_000 + np.arange(n, dtype=np.int64)) for s, n in enumerate([T + 5, 700, 2 * T + 1])]
    got_k, got_p = run_arrays(pkg, ctx, streams)
    rows = {int(p): int(k) for ks, ps in streams for k, p in zip(ks, ps)}
    assert len(got_p) == len(rows) and all(rows.get(int(p)) == int(k) for k, p in zip(got_k, got_p))


# ---- streaming ------------------------------------------------------------------------------------------------------------------------------
def test_streaming_memory_stays_near_the_pages_in_flight(pkg, ctx):
    """k = 4 streams of 64 pages of 1,024 rows, interleaved keys, one page per poll: at any time about k of the 256 pages hold an unemitted
    row, so the buffered bytes stay far below a quarter of the input (only an operator that collects everything first crosses it); 0 at the end"""
    k, pages, n = 4, 64, 1024
    Armed = make_armed_source(pkg)
    fac, op = new_operator(pkg, ctx, [M.BIGINT, M.BIGINT], [0], [0], [M.ASC_NULLS_FIRST])
    sources = [Armed() for _ in range(k)]
    for s in sources:
        op.addSplit(s)
    op.noMoreSplits()
    total_bytes = k * pages * n * 16
    seen, got = [], []
    for p in range(pages + 2):
        if op.isFinished():
            break
        for s, src in enumerate(sources):
            if p < pages:
                keys = s + k * (p * n + np.arange(n, dtype=np.int64))
                src.arm(pkg.Page(pkg.Block(pkg.BIGINT, keys), pkg.Block(pkg.BIGINT, np.full(n, s, dtype=np.int64))))
            if p == pages - 1:
                src.end()
        o = op.getOutput()
        if o is not None:
            got.append(o.to_host().getBlock(0).values.copy())
            o.release()
        seen.append(op.memoryBytes())
    assert op.isFinished() and np.array_equal(np.concatenate(got), np.arange(k * pages * n))
    assert 0 < max(seen) < total_bytes // 4 and seen[-1] == 0 and op.memoryBytes() == 0
    op.close()
    fac.close()


# ---- route -------------------------------------------------------------------------------------------------------------------------------------
def profiled(pkg, streams_of_keys):
    c = pkg.Context(0)
    c.profile_enable(True)
    try:
        check = [(np.asarray(k, dtype=np.int64), s * 10_000_000 + np.arange(len(k), dtype=np.int64)) for s, k in enumerate(streams_of_keys)]
        got_k, _ = run_arrays(pkg, c, check)
        assert np.array_equal(got_k, np.sort(np.concatenate([k for k, _ in check]), kind="stable"))
        return c.profile()
    finally:
        c.close()


def test_route_by_profile_scopes(pkg):
    count = lambda prof, name: prof.get(name, {}).get("count", 0)
    prof = profiled(pkg, [3 * np.arange(1000) + s for s in range(3)])
    assert count(prof, "merge_bound") >= 1 and count(prof, "merge_path") >= 1 and count(prof, "merge_gather") >= 1
    prof = profiled(pkg, [np.arange(5000)])   # k = 1: passed through by region
    assert count(prof, "merge_path") == 0 and count(prof, "merge_gather") == 0
    prof = profiled(pkg, [np.arange(1000), 1000 + np.arange(1000), 2000 + np.arange(1000)])   # disjoint streams, all finished: one merged round
    assert count(prof, "merge_path") >= 1


def test_disjoint_streams_one_at_a_time_take_the_pass_through(pkg):
    """stream 0 entirely before stream 1 and fed so that every round has settled rows of one stream only: each round passes a region of
    that stream's buffer through and no merge-path kernel runs"""
    c = pkg.Context(0)
    c.profile_enable(True)
    try:
        types = [M.BIGINT, M.BIGINT]
        Armed = make_armed_source(pkg)
        fac, op = new_operator(pkg, c, types, [1, 0], [0], [M.ASC_NULLS_FIRST])
        a, b = Armed(), Armed()
        op.addSplit(a)
        op.addSplit(b)
        op.noMoreSplits()
        page = lambda s, p: make_page(pkg, types, [(1000 * s + p * 100 + i, s) for i in range(100)])
        got = []
        #        round 1: both streams hold a page, B is stream 0's last row; rounds 2, 3: stream 0 alone delivers; round 4: stream 0 ends without
        #        a page, stream 1's buffered page settles; rounds 5, 6: stream 1 alone
        for arm in ([(a, 0, 0), (b, 1, 0)], [(a, 0, 1)], [(a, 0, 2)], [(a, None, None)], [(b, 1, 1)], [(b, 1, 2), (b, None, None)]):
            for src, s, p in arm:
                if s is None:
                    src.end()
                else:
                    src.arm(page(s, p))
            o = op.getOutput()
            assert o is not None and o.position_count == 100
            got += o.to_host().rows()
            o.release()
        assert op.getOutput() is None and op.isFinished()
        assert got == [(0, p * 100 + i) for p in range(3) for i in range(100)] + [(1, 1000 + p * 100 + i) for p in range(3) for i in range(100)]
        prof = c.profile()
        assert prof.get("merge_path", {}).get("count", 0) == 0 and prof.get("merge_gather", {}).get("count", 0) == 0 and prof.get("merge_bound", {}).get("count", 0) >= 6
        op.close()
        fac.close()
    finally:
        c.close()


# ---- errors and lifecycle --------------------------------------------------------------------------------------------------------------------
def test_wrong_channel_count_or_types_are_refused(pkg, ctx):
    types = [M.BIGINT, M.VARCHAR]
    for bad in (pkg.Page(pkg.Block(pkg.BIGINT, [1, 2])), pkg.Page(pkg.Block(pkg.BIGINT, [1, 2]), pkg.Block(pkg.DOUBLE, [1.0, 2.0])),
                pkg.Page(pkg.Block(pkg.INTEGER, [1, 2]), pkg.Block(pkg.VARCHAR, ["a", "b"]))):
        fac, op = new_operator(pkg, ctx, types, [0], [0], [M.ASC_NULLS_FIRST])
        src = pkg.PageSource([bad])
        op.addSplit(src)
        op.noMoreSplits()
        with pytest.raises(pkg.TgpuError) as e:
            op.getOutput()
        assert e.value.code == INVALID_ARGUMENT
        op.close()
        assert src.closed
        fac.close()
    for args in (([M.BIGINT], [1], [0], [0]), ([M.BIGINT], [0], [2], [0]), ([M.BIGINT], [0], [0], [7]), ([M.BIGINT], [0], [], [])):
        with pytest.raises(pkg.TgpuError) as e:
            pkg.MergeOperatorFactory(ctx, 0, *args)
        assert e.value.code == INVALID_ARGUMENT


def test_a_failing_source_fails_the_call_and_every_source_is_closed_once(pkg, ctx):
    Armed = make_armed_source(pkg)
    types = [M.BIGINT]
    fac, op = new_operator(pkg, ctx, types, [0], [0], [M.ASC_NULLS_FIRST])
    sources = [Armed() for _ in range(3)]
    for s in sources:
        op.addSplit(s)
        s.arm(make_page(pkg, types, [(1,), (2,)]))
    op.noMoreSplits()
    sources[1].fail_next = -1
    with pytest.raises(pkg.TgpuError) as e:
        op.getOutput()
    assert e.value.code == -1
    # the operator is usable after the failure: what was pulled before the failing call stays buffered, the failing source is asked again
    sources[1].fail_next = 0
    for s in sources:
        s.end()
    assert [r for p in drain(op) for r in p] == [(1,), (1,), (1,), (2,), (2,), (2,)]
    assert [s.closes for s in sources] == [1, 1, 1]
    # a source that keeps failing: close() still closes every source once
    op = fac.createOperator()
    sources = [Armed() for _ in range(3)]
    for s in sources:
        op.addSplit(s)
        s.arm(make_page(pkg, types, [(1,), (2,)]))
    op.noMoreSplits()
    sources[2].fail_next = -5
    with pytest.raises(pkg.TgpuError) as e:
        op.getOutput()
    assert e.value.code == -5
    op.close()
    assert [s.closes for s in sources] == [1, 1, 1]
    fac.close()


def test_splits_after_no_more_splits_close_and_finish_mid_stream_and_zero_splits(pkg, ctx):
    Armed = make_armed_source(pkg)
    types = [M.BIGINT]
    page = lambda *v: make_page(pkg, types, [(x,) for x in v])
    # add_page_source after no_more_splits
    fac, op = new_operator(pkg, ctx, types, [0], [0], [M.ASC_NULLS_FIRST])
    a = Armed()
    op.addSplit(a)
    op.noMoreSplits()
    with pytest.raises(pkg.TgpuError) as e:
        op.addSplit(Armed())
    assert e.value.code == INTERNAL and "noMoreSplits has been called already" in str(e.value)
    # close() mid-stream
    a.arm(page(1, 2, 3))
    o = op.getOutput()
    assert o is not None and o.position_count == 3 and not op.isFinished()
    o.release()
    op.close()
    assert a.closes == 1
    # finish() mid-stream: finished at once, nothing further
    op = fac.createOperator()
    a, b = Armed(), Armed()
    op.addSplit(a)
    op.addSplit(b)
    op.noMoreSplits()
    a.arm(page(1, 5))
    b.arm(page(2, 3))
    o = op.getOutput()
    assert o is not None and o.to_host().rows() == [(1,), (2,), (3,)]
    assert op.memoryBytes() > 0 and not op.isFinished()
    op.finish()
    assert op.isFinished() and op.getOutput() is None and not op.isBlocked() and op.memoryBytes() == 0 and (a.closes, b.closes) == (1, 1)
    op.close()
    assert (a.closes, b.closes) == (1, 1)
    # zero splits
    op = fac.createOperator()
    assert op.isBlocked() and not op.isFinished()
    op.noMoreSplits()
    assert op.isFinished() and op.getOutput() is None and not op.isBlocked()
    op.close()
    fac.close()


def test_dictionary_rle_and_device_pages_and_page_cuts(pkg, ctx):
    """DICTIONARY and RLE blocks go through the ingest; a device-resident page (another operator's output) is owner-shared; the context's
    max output page cuts the merged page into regions"""
    types = [M.BIGINT, M.VARCHAR]
    d = pkg.DictionaryBlock(pkg.Block(pkg.VARCHAR, ["x", "yy", None]), [0, 1, 2, 1])
    s0 = pkg.Page(pkg.Block(pkg.BIGINT, [1, 3, 5, 7]), d)
    s1 = pkg.Page(pkg.Block(pkg.BIGINT, [2, 4, 6]), pkg.RunLengthEncodedBlock(pkg.Block(pkg.VARCHAR, ["r"]), 3))
    fac, op = new_operator(pkg, ctx, types, [0, 1], [0], [M.ASC_NULLS_FIRST])
    # the third stream: the output page of a first merge, fed back as device blocks
    fac2, first = new_operator(pkg, ctx, types, [0, 1], [0], [M.ASC_NULLS_FIRST])
    first.addSplit(pkg.PageSource([pkg.Page(pkg.Block(pkg.BIGINT, [0, 8]), pkg.Block(pkg.VARCHAR, ["lo", "hi"]))]))
    first.noMoreSplits()
    dev = first.getOutput()
    for p in (s0, s1, dev.as_device_page()):
        op.addSplit(pkg.PageSource([p]))
    op.noMoreSplits()
    ctx.set_max_output_page(max_rows=4)
    try:
        pages = drain(op)
    finally:
        ctx.set_max_output_page(0, 0)
    assert [len(p) for p in pages] == [4, 4, 1]
    assert [r for p in pages for r in p] == [(0, "lo"), (1, "x"), (2, "r"), (3, "yy"), (4, "r"), (5, None), (6, "r"), (7, "yy"), (8, "hi")]
    dev.release()
    for o in (op, first):
        o.close()
    fac.close()
    fac2.close()

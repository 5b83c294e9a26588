"""MarkDistinctOperator on the GPU: the reference's TestMarkDistinctOperator case (tests/golden/distinct_vectors.json), random pages of every key type
against the oracle's GroupByHash plus MarkDistinctHash's loop (tests/distinct_expected.py), edge pages, encodings, device-resident chaining and
count(DISTINCT x) GROUP BY g through the aggregation's mask channel.  Marks are compared exactly."""
import json
import os

import numpy as np
import pytest

from distinct_gpu import DOMAINS, KEY_SPECS, PAGE_SIZES, check_marks, drive_mark, flat_rows, key_block, key_pages, with_hash

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "distinct_vectors.json")))


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def mark(pkg, ctx, types, channels, pages, hash_channel=-1, factory=None):
    f = factory or pkg.MarkDistinctOperatorFactory(ctx, 1, types, channels, hash_channel)
    op = f.createOperator()
    outs = drive_mark(op, pages)
    op.close()
    return outs


# ---- 1. the reference's case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_enabled", [False, True])
def test_reference_case(pkg, ctx, oracle, hash_enabled):
    case = next(c for c in GOLD["cases"] if c["operator"] == "mark_distinct")
    types = [getattr(pkg, t) for t in case["types"]]
    pages = [pkg.Page(pkg.Block(types[0], np.array(p, dtype=np.int64))) for p in case["pages"]]
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, case["channels"]) for p in pages], len(types), types + [pkg.BIGINT]
    outs = mark(pkg, ctx, types, case["channels"], pages, hc)
    rows = [[v for i, v in enumerate(r) if i != hc] for p in outs for r in p.rows()]   # OperatorAssertion.dropChannel
    assert rows == case["expected"]


# ---- 2. random pages against the helper -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_enabled", [False, True])
@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("spec", KEY_SPECS, ids=[s[0] for s in KEY_SPECS])
def test_random_pages_match_helper(pkg, ctx, oracle, spec, domain, hash_enabled):
    name, type_names, null_frac = spec
    rng = np.random.default_rng(1000 + 10 * [s[0] for s in KEY_SPECS].index(name) + list(DOMAINS).index(domain))
    sizes = [int(s) for s in rng.choice(PAGE_SIZES, 3)]
    types, pages = key_pages(pkg, rng, type_names, DOMAINS[domain], null_frac, sizes)
    channels = list(range(len(types)))
    payload = [pkg.Block(pkg.BIGINT, np.arange(p.getPositionCount(), dtype=np.int64)) for p in pages]
    pages = [p.appendColumn(b) for p, b in zip(pages, payload)]
    types = types + [pkg.BIGINT]
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, channels) for p in pages], len(types), types + [pkg.BIGINT]
    outs = mark(pkg, ctx, types, channels, pages, hc)
    check_marks(pkg, oracle, types, channels, pages, outs)


def test_large_domain_pages_share_keys(pkg, ctx, oracle):
    """page 1 repeats half of page 0's (mostly new) keys: G0 > 0 and the old keys stay unmarked among new ones"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1_000_000, 4097).astype(np.int64)
    b = np.where(rng.random(1025) < 0.5, rng.choice(a, 1025), rng.integers(0, 1_000_000, 1025)).astype(np.int64)
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, a)), pkg.Page(pkg.Block(pkg.BIGINT, b))]
    outs = mark(pkg, ctx, [pkg.BIGINT], [0], pages)
    check_marks(pkg, oracle, [pkg.BIGINT], [0], pages, outs)
    got = outs[1].getBlock(1).values.astype(bool)
    assert 0 < got.sum() < 1025 and not got[np.isin(b, a)].any()


# ---- 3. edge pages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "VARCHAR"])
def test_edge_pages(pkg, ctx, oracle, type_name):
    t = getattr(pkg, type_name)
    n = 1500

    def block(values):
        return pkg.Block(t, [None if v is None else ("k%d" % v if t == pkg.VARCHAR else v) for v in values])
    pages = [
        pkg.Page(block([7] * n)),                 # all rows the same new key: only row 0 is marked
        pkg.Page(block([7] * n)),                 # all rows already seen: no mark
        pkg.Page(block(range(100, 100 + n))),     # all rows distinct
        pkg.Page(block([None] * n)),              # all keys null: the null key is a group, row 0 is marked
        pkg.Page(block([])),                      # a zero-row page
        pkg.Page(block([None, 7, 100, 5000])),    # afterwards: only the last key is new
    ]
    outs = mark(pkg, ctx, [t], [0], pages)
    check_marks(pkg, oracle, [t], [0], pages, outs)
    m = [o.getBlock(1).values.astype(bool) for o in outs]
    assert m[0].tolist() == [True] + [False] * (n - 1)
    assert not m[1].any()
    assert m[2].all()
    assert m[3].tolist() == [True] + [False] * (n - 1)
    assert outs[4].getPositionCount() == 0 and outs[4].getChannelCount() == 2
    assert m[5].tolist() == [False, False, False, True]


def test_first_occurrence_and_duplicate_straddle_a_workgroup_boundary(pkg, ctx, oracle):
    """all rows distinct, except that the rows after a wave's (64), a workgroup's (256) and a workgroup's range's (1024) last row
    repeat that row: the earlier row is marked, the later one is not"""
    n = 4097
    keys = np.arange(10_000, 10_000 + n, dtype=np.int64)
    for first in (63, 255, 1023, 2047, 4095):
        keys[first + 1] = keys[first]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.arange(5, dtype=np.int64))), pkg.Page(pkg.Block(pkg.BIGINT, keys))]
    outs = mark(pkg, ctx, [pkg.BIGINT], [0], pages)
    check_marks(pkg, oracle, [pkg.BIGINT], [0], pages, outs)
    m = outs[1].getBlock(1).values.astype(bool)
    for first in (63, 255, 1023, 2047, 4095):
        assert m[first] and not m[first + 1]
    assert m.sum() == n - 5


# ---- 4. a page that crosses the group-by hash's first sub-batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["5000", "distinct"])
def test_page_larger_than_the_first_sub_batch(pkg, ctx, oracle, keys):
    n = (1 << 18) + 1
    rng = np.random.default_rng(31)
    v = rng.integers(0, 5000, n).astype(np.int64) if keys == "5000" else rng.permutation(n).astype(np.int64) * 7
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, v))]
    outs = mark(pkg, ctx, [pkg.BIGINT], [0], pages)
    check_marks(pkg, oracle, [pkg.BIGINT], [0], pages, outs)
    assert outs[0].getBlock(1).values.sum() == (len(np.unique(v)))


# ---- 5. DICTIONARY and RLE key blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "DOUBLE", "VARCHAR"])
def test_dictionary_and_rle_keys(pkg, ctx, oracle, type_name):
    rng = np.random.default_rng(17)
    t = getattr(pkg, type_name)
    dictionary = pkg.DictionaryBlock(key_block(pkg, rng, t, 40, 30, 0.1), rng.integers(0, 40, 2000).astype(np.int32))
    rle_seen = pkg.RunLengthEncodedBlock(pkg.Block(t, [dictionary.flatten().get(3)]), 500)
    rle_new = pkg.RunLengthEncodedBlock(pkg.Block(t, ["fresh" if t == pkg.VARCHAR else 12345]), 300)
    flat = key_block(pkg, rng, t, 1000, 60, 0.1)
    pages = [pkg.Page(b, pkg.Block(pkg.BIGINT, np.arange(b.getPositionCount(), dtype=np.int64))) for b in (dictionary, rle_seen, rle_new, flat)]
    outs = mark(pkg, ctx, [t, pkg.BIGINT], [0], pages)
    check_marks(pkg, oracle, [t, pkg.BIGINT], [0], pages, outs)
    flat_pages = [pkg.Page(p.getBlock(0).flatten(), p.getBlock(1)) for p in pages]
    flat_outs = mark(pkg, ctx, [t, pkg.BIGINT], [0], flat_pages)
    for a, b in zip(outs, flat_outs):
        assert flat_rows(a) == flat_rows(b)


# ---- 6. device-resident chaining ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("borrowed", [False, True])
def test_filter_then_mark_distinct_on_the_device(pkg, ctx, oracle, borrowed):
    f, B = pkg.field, pkg.BIGINT
    rng = np.random.default_rng(11)
    inputs = [pkg.Page(pkg.Block(B, rng.integers(0, 300, n).astype(np.int64), (rng.random(n) < 0.05).astype(np.uint8)), pkg.Block(B, np.arange(n, dtype=np.int64)))
              for n in (3000, 2000)]
    head = pkg.FilterAndProjectOperatorFactory(ctx, 10, [B, B], f(1, B) > 100, [f(0, B), f(1, B)]).createOperator()
    filtered = pkg.to_pages(head, inputs, to_host=False)   # device-resident OutputPages
    op = pkg.MarkDistinctOperatorFactory(ctx, 11, [B, B], [0]).createOperator()
    outs = []
    for o1 in filtered:
        if borrowed:   # caller-owned device blocks: the operator copies what it passes through, the output outlives the input
            op.addInput(o1.as_device_page())
        else:
            op.addInput(o1)
        o1.release()
        o2 = op.getOutput()
        outs.append(o2.to_host())
        o2.release()
    want_pages = [pkg.Page(pkg.Block(B, p.getBlock(0).values[101:], p.getBlock(0).nulls[101:]), pkg.Block(B, p.getBlock(1).values[101:])) for p in inputs]
    check_marks(pkg, oracle, [B, B], [0], want_pages, outs)
    head.close()
    op.close()


# ---- 7. count(DISTINCT x) GROUP BY g ----------------------------------------------------------------------------------------------------
def test_count_distinct_group_by(pkg, ctx):
    rng = np.random.default_rng(3)
    B = pkg.BIGINT
    pages = [pkg.Page(pkg.Block(B, rng.integers(0, 20, 5000).astype(np.int64)),
                      pkg.Block(B, rng.integers(0, 300, 5000).astype(np.int64), (rng.random(5000) < 0.05).astype(np.uint8))) for _ in range(3)]
    marker = pkg.MarkDistinctOperatorFactory(ctx, 1, [B, B], [0, 1]).createOperator()
    agg = pkg.HashAggregationOperatorFactory(ctx, 2, [B], [0], [(pkg.COUNT_COLUMN, 1, 2)]).createOperator()   # mask_channel = the marker
    for p in pages:
        marker.addInput(p)
        marked = marker.getOutput()
        assert agg.needsInput()
        agg.addInput(marked)   # stays on the device
        marked.release()
        assert agg.getOutput() is None
    agg.finish()
    rows = []
    while not agg.isFinished():
        o = agg.getOutput()
        if o is not None:
            rows.extend(o.to_host().rows())
            o.release()
    want = {}
    for p in pages:
        g, x = p.getBlock(0), p.getBlock(1)
        for i in range(5000):
            want.setdefault(int(g.values[i]), set())
            if not x.nulls[i]:
                want[int(g.values[i])].add(int(x.values[i]))
    assert sorted(rows) == sorted((g, len(s)) for g, s in want.items())
    marker.close()
    agg.close()


# ---- 9. protocol ------------------------------------------------------------------------------------------------------------------------
def test_protocol_memory_and_duplicate(pkg, ctx, oracle):
    f = pkg.MarkDistinctOperatorFactory(ctx, 1, [pkg.BIGINT], [0])
    f2 = f.duplicate()
    a, b = f.createOperator(), f2.createOperator()
    assert a.needsInput() and not a.isFinished() and a.getOutput() is None
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array([4, 4, 9, 4, 1], dtype=np.int64)))
    got = []
    for op in (a, b, a):   # independent hashes: b marks what a marked the first time; a's second pass marks nothing
        op.addInput(page)
        assert not op.needsInput() and not op.isFinished()
        o = op.getOutput()
        got.append(o.to_host().getBlock(1).to_list())
        o.release()
        assert op.needsInput() and op.memoryBytes() > 0
    assert got == [[True, False, True, False, True]] * 2 + [[False] * 5]
    a.addInput(page)
    a.finish()
    assert not a.isFinished() and not a.needsInput()   # a page is still pending
    a.getOutput().release()
    assert a.isFinished()
    for op in (a, b):
        op.close()


@pytest.mark.parametrize("types, channels, hash_channel", [
    ([1], [], -1), ([1], [1], -1), ([1], [-1], -1), ([1, 1], [0], 2), ([1, 2], [0], 1), ([], [0], -1), ([1, 9], [0], -1), ([1], [0] * 9, -1)])
def test_factory_argument_errors(pkg, ctx, types, channels, hash_channel):
    with pytest.raises(pkg.TgpuError) as e:
        pkg.MarkDistinctOperatorFactory(ctx, 1, types, channels, hash_channel)
    assert e.value.code == -1   # TGPU_ERR_INVALID_ARGUMENT

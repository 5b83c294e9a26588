"""DistinctLimitOperator on the GPU: the reference's TestDistinctLimitOperator data cases (tests/golden/distinct_vectors.json), random pages of every
key type against the oracle's GroupByHash plus DistinctLimitOperator.getOutput's loop (tests/distinct_expected.py), edge pages, limits that
end inside and at the end of a page, the output channel order and the protocol.  Rows and positions are compared exactly."""
import json
import os

import numpy as np
import pytest

from distinct_gpu import DOMAINS, KEY_SPECS, PAGE_SIZES, check_distinct_limit, drive_distinct_limit, key_block, key_pages, with_hash

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "distinct_vectors.json")))


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def run(pkg, ctx, oracle, types, channels, limit, pages, hash_channel=-1):
    """drives one operator over the pages and checks every output page against the helper; returns (operator, rows produced)"""
    op = pkg.DistinctLimitOperatorFactory(ctx, 1, types, channels, limit, hash_channel).createOperator()
    outs = drive_distinct_limit(op, pages)
    total = check_distinct_limit(pkg, oracle, types, channels, hash_channel, limit, pages, outs)
    return op, total, outs


def finish(op):
    op.finish()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()


# ---- 1. the reference's cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_enabled", [False, True])
@pytest.mark.parametrize("case", [c for c in GOLD["cases"] if c["operator"] == "distinct_limit"], ids=lambda c: c["name"])
def test_reference_cases(pkg, ctx, oracle, case, hash_enabled):
    types = [getattr(pkg, t) for t in case["types"]]
    pages = [pkg.Page(pkg.Block(types[0], np.array(p, dtype=np.int64))) for p in case["pages"]]
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, case["channels"]) for p in pages], len(types), types + [pkg.BIGINT]
    op = pkg.DistinctLimitOperatorFactory(ctx, 1, types, case["channels"], case["limit"], hc).createOperator()
    outs = pkg.to_pages(op, pages)   # OperatorAssertion.toPages
    op.close()
    drop = len(case["channels"]) if hash_enabled else -1   # the hash channel comes last in the output (OperatorAssertion.dropChannel)
    assert [[v for i, v in enumerate(r) if i != drop] for p in outs for r in p.rows()] == case["expected"]


# ---- 2. random pages against the helper -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_enabled", [False, True])
@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("spec", KEY_SPECS, ids=[s[0] for s in KEY_SPECS])
def test_random_pages_match_helper(pkg, ctx, oracle, spec, domain, hash_enabled):
    name, type_names, null_frac = spec
    rng = np.random.default_rng(2000 + 10 * [s[0] for s in KEY_SPECS].index(name) + list(DOMAINS).index(domain))
    sizes = [int(s) for s in rng.choice(PAGE_SIZES, 3)]
    types, pages = key_pages(pkg, rng, type_names, DOMAINS[domain], null_frac, sizes)
    channels = list(range(len(types)))
    pages = [p.appendColumn(pkg.Block(pkg.BIGINT, np.arange(p.getPositionCount(), dtype=np.int64))) for p in pages]   # a channel that is not output
    types = types + [pkg.BIGINT]
    hc = -1
    if hash_enabled:
        pages, hc, types = [with_hash(pkg, oracle, p, channels) for p in pages], len(types), types + [pkg.BIGINT]
    op, total, _ = run(pkg, ctx, oracle, types, channels, 1 << 40, pages, hc)   # every key comes out once
    assert op.needsInput() and not op.isFinished()
    finish(op)
    if total > 2:   # the same stream cut inside it
        op, cut, _ = run(pkg, ctx, oracle, types, channels, total // 2, pages, hc)
        assert cut == total // 2 and op.isFinished() and not op.needsInput()
        op.close()


# ---- 3. edge pages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "VARCHAR"])
def test_edge_pages(pkg, ctx, oracle, type_name):
    t = getattr(pkg, type_name)
    n = 1500

    def block(values):
        return pkg.Block(t, [None if v is None else ("k%d" % v if t == pkg.VARCHAR else v) for v in values])
    pages = [
        pkg.Page(block([7] * n)),                 # all rows the same new key: one output row
        pkg.Page(block([7] * n)),                 # all rows already seen: no output page
        pkg.Page(block(range(100, 100 + n))),     # all rows distinct
        pkg.Page(block([None] * n)),              # all keys null: one null row
        pkg.Page(block([])),                      # a zero-row page: no output page
        pkg.Page(block([None, 7, 100, 5000])),    # afterwards: only the last key is new
    ]
    op, total, outs = run(pkg, ctx, oracle, [t], [0], 1 << 40, pages)
    assert [None if o is None else o.getPositionCount() for o in outs] == [1, None, n, 1, None, 1]
    assert outs[3].getBlock(0).to_list() == [None]
    assert total == n + 3
    finish(op)


def test_first_occurrence_and_duplicate_straddle_a_workgroup_boundary(pkg, ctx, oracle):
    n = 4097
    keys = np.arange(10_000, 10_000 + n, dtype=np.int64)
    for first in (63, 255, 1023, 2047, 4095):
        keys[first + 1] = keys[first]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.arange(5, dtype=np.int64))), pkg.Page(pkg.Block(pkg.BIGINT, keys))]
    op, total, outs = run(pkg, ctx, oracle, [pkg.BIGINT], [0], 1 << 40, pages)
    assert outs[1].getBlock(0).values.tolist() == [int(k) for i, k in enumerate(keys) if i == 0 or keys[i - 1] != k]
    finish(op)


# ---- 4. a page that crosses the group-by hash's first sub-batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["5000", "distinct"])
def test_page_larger_than_the_first_sub_batch(pkg, ctx, oracle, keys):
    n = (1 << 18) + 1
    rng = np.random.default_rng(37)
    v = rng.integers(0, 5000, n).astype(np.int64) if keys == "5000" else rng.permutation(n).astype(np.int64) * 7
    op, total, outs = run(pkg, ctx, oracle, [pkg.BIGINT], [0], 1 << 40, [pkg.Page(pkg.Block(pkg.BIGINT, v))])
    assert total == len(np.unique(v))
    first = np.sort(np.unique(v, return_index=True)[1])
    assert np.array_equal(outs[0].getBlock(0).values, v[first])   # first occurrences, in row order
    finish(op)


# ---- 5. DICTIONARY and RLE key blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["BIGINT", "DOUBLE", "VARCHAR"])
def test_dictionary_and_rle_keys(pkg, ctx, oracle, type_name):
    rng = np.random.default_rng(19)
    t = getattr(pkg, type_name)
    dictionary = pkg.DictionaryBlock(key_block(pkg, rng, t, 40, 30, 0.1), rng.integers(0, 40, 2000).astype(np.int32))
    rle_seen = pkg.RunLengthEncodedBlock(pkg.Block(t, [dictionary.flatten().get(3)]), 500)
    rle_new = pkg.RunLengthEncodedBlock(pkg.Block(t, ["fresh" if t == pkg.VARCHAR else 12345]), 300)
    pages = [pkg.Page(b) for b in (dictionary, rle_seen, rle_new, key_block(pkg, rng, t, 1000, 60, 0.1))]
    op, total, outs = run(pkg, ctx, oracle, [t], [0], 1 << 40, pages)
    assert outs[1] is None and outs[2].getPositionCount() == 1
    finish(op)


# ---- 6. device-resident input ----------------------------------------------------------------------------------------------------------
def test_filter_then_distinct_limit_on_the_device(pkg, ctx, oracle):
    f, B = pkg.field, pkg.BIGINT
    rng = np.random.default_rng(13)
    inputs = [pkg.Page(pkg.Block(B, rng.integers(0, 300, n).astype(np.int64), (rng.random(n) < 0.05).astype(np.uint8)), pkg.Block(B, np.arange(n, dtype=np.int64)))
              for n in (3000, 2000)]
    head = pkg.FilterAndProjectOperatorFactory(ctx, 10, [B, B], f(1, B) > 100, [f(0, B), f(1, B)]).createOperator()
    filtered = pkg.to_pages(head, inputs, to_host=False)   # device-resident OutputPages
    op = pkg.DistinctLimitOperatorFactory(ctx, 11, [B, B], [0], 250).createOperator()
    outs = drive_distinct_limit(op, filtered)
    for o in filtered:
        o.release()
    want_pages = [pkg.Page(pkg.Block(B, p.getBlock(0).values[101:], p.getBlock(0).nulls[101:]), pkg.Block(B, p.getBlock(1).values[101:])) for p in inputs]
    assert check_distinct_limit(pkg, oracle, [B, B], [0], -1, 250, want_pages, outs) == 250
    assert op.isFinished()
    head.close()
    op.close()


# ---- 8. limits ------------------------------------------------------------------------------------------------------------------------
def limit_pages(pkg):
    """12 distinct keys over three pages: 5 new in page 0, 4 new in page 1 (rows 1, 2, 4, 5), 3 new in page 2"""
    pages = [[10, 11, 10, 12, 13, 14, 11], [10, 20, 21, 21, 22, 23, 12], [20, 30, 31, 31, 32]]
    return [pkg.Page(pkg.Block(pkg.BIGINT, np.array(p, dtype=np.int64))) for p in pages]


@pytest.mark.parametrize("limit", [0, 1, 7, 9, 12, 100])
def test_limits(pkg, ctx, oracle, limit):
    pages = limit_pages(pkg)
    distinct = len({v for p in pages for v in p.getBlock(0).values.tolist()})
    op = pkg.DistinctLimitOperatorFactory(ctx, 1, [pkg.BIGINT], [0], limit).createOperator()
    if limit == 0:   # finished at once, never needs input
        assert op.isFinished() and not op.needsInput() and op.getOutput() is None
        op.close()
        return
    assert op.needsInput() and not op.isFinished()
    outs = drive_distinct_limit(op, pages)
    total = check_distinct_limit(pkg, oracle, [pkg.BIGINT], [0], -1, limit, pages, outs)
    assert total == min(limit, distinct)
    rows = [v for o in outs if o is not None for v in o.getBlock(0).values.tolist()]
    assert rows == [10, 11, 12, 13, 14, 20, 21, 22, 23, 30, 31, 32][:limit]
    if limit == 1:
        assert len(outs) == 1   # reached inside page 0: the later pages are not taken
    if limit == 7:   # reached in the middle of page 1: rows after the cut are absent, and the operator is done without finish()
        assert len(outs) == 2 and outs[1].getBlock(0).values.tolist() == [20, 21]
    if limit == 9:   # reached exactly with page 1's last new key
        assert len(outs) == 2 and outs[1].getBlock(0).values.tolist() == [20, 21, 22, 23]
    if limit <= distinct:
        assert not op.needsInput() and op.isFinished()
        op.close()
    else:
        assert op.needsInput() and not op.isFinished()
        finish(op)


def test_limit_reached_at_a_page_end(pkg, ctx, oracle):
    """the page's last row is its last new key and exhausts the limit"""
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.array(p, dtype=np.int64))) for p in ([1, 2, 1, 3], [9, 9, 9])]
    op, total, outs = run(pkg, ctx, oracle, [pkg.BIGINT], [0], 3, pages)
    assert len(outs) == 1 and outs[0].getBlock(0).values.tolist() == [1, 2, 3] and op.isFinished() and not op.needsInput()
    op.close()


@pytest.mark.parametrize("hash_enabled", [False, True])
def test_output_channel_order(pkg, ctx, oracle, hash_enabled):
    """distinct channels [2, 0]: the output is channel 2, channel 0, then the hash channel"""
    rng = np.random.default_rng(41)
    n = 1025
    page = pkg.Page(key_block(pkg, rng, pkg.VARCHAR, n, 6, 0.1), pkg.Block(pkg.DOUBLE, rng.random(n)), key_block(pkg, rng, pkg.INTEGER, n, 5, 0.1))
    types, hc = [pkg.VARCHAR, pkg.DOUBLE, pkg.INTEGER], -1
    if hash_enabled:
        page, hc, types = with_hash(pkg, oracle, page, [2, 0]), 3, types + [pkg.BIGINT]
    op, total, outs = run(pkg, ctx, oracle, types, [2, 0], 20, [page, page], hc)
    assert [outs[0].getBlock(i).type for i in range(outs[0].getChannelCount())] == [pkg.INTEGER, pkg.VARCHAR] + ([pkg.BIGINT] if hash_enabled else [])
    op.close()


# ---- 9. protocol ------------------------------------------------------------------------------------------------------------------------
def test_protocol_memory_and_duplicate(pkg, ctx):
    f = pkg.DistinctLimitOperatorFactory(ctx, 1, [pkg.BIGINT], [0], 10)
    f2 = f.duplicate()
    a, b = f.createOperator(), f2.createOperator()
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.array([4, 4, 9, 4, 1], dtype=np.int64)))
    got = []
    for op in (a, b):   # independent hashes and limits
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None
        op.addInput(page)
        assert not op.needsInput() and not op.isFinished()   # a page is pending
        o = op.getOutput()
        got.append(o.to_host().getBlock(0).to_list())
        o.release()
        assert op.needsInput() and not op.isFinished() and op.memoryBytes() > 0
    assert got == [[4, 9, 1]] * 2
    a.addInput(page)   # nothing new: no output page, the operator takes the next page at once
    assert a.getOutput() is None and a.needsInput()
    a.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.array([5], dtype=np.int64))))
    a.finish()
    assert not a.isFinished() and not a.needsInput()   # finishing with a page pending
    o = a.getOutput()
    assert o.to_host().getBlock(0).to_list() == [5]
    o.release()
    assert a.isFinished()
    for op in (a, b):
        op.close()


@pytest.mark.parametrize("types, channels, limit, hash_channel", [
    ([1], [], 5, -1), ([1], [1], 5, -1), ([1], [-1], 5, -1), ([1, 1], [0], 5, 2), ([1, 2], [0], 5, 1), ([], [0], 5, -1), ([1], [0], -1, -1)])
def test_factory_argument_errors(pkg, ctx, types, channels, limit, hash_channel):
    with pytest.raises(pkg.TgpuError) as e:
        pkg.DistinctLimitOperatorFactory(ctx, 1, types, channels, limit, hash_channel)
    assert e.value.code == -1   # TGPU_ERR_INVALID_ARGUMENT

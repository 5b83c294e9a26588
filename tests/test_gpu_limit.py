"""LimitOperator on the GPU: the reference's TestLimitOperator cases (tests/golden/row_number_vectors.json), limit 0, a limit beyond the stream, a
crossing page with VARCHAR, nulls and a dictionary block, finish() before the limit and the needsInput / isFinished sequence of
M/operator/LimitOperator.java:86-96.  Pages, values and nulls are compared exactly."""
import json
import os

import numpy as np
import pytest

from row_number_expected import expected_limit

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "row_number_vectors.json")))
LIMIT_CASES = [c for c in GOLD["cases"] if c["operator"] == "limit"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def drive(op, pages):
    outs = []
    for p in pages:
        if not op.needsInput():
            break
        op.addInput(p)
        assert not op.needsInput()   # nextPage is set
        o = op.getOutput()
        assert o is not None and op.getOutput() is None
        outs.append(o.to_host())
        o.release()
    return outs


def cells(page):
    return [page.getBlock(c).flatten().to_list() for c in range(page.getChannelCount())]


@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: c["name"])
def test_reference_cases(pkg, ctx, case):
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, np.array(p, dtype=np.int64))) for p in case["pages"]]
    op = pkg.LimitOperatorFactory(ctx, 1, [pkg.BIGINT], case["limit"]).createOperator()
    outs = pkg.to_pages(op, pages)   # OperatorAssertion.toPages
    assert [o.getBlock(0).values.tolist() for o in outs if o.getPositionCount()] == case["expected_pages"]
    op.close()


def test_limit_0_is_finished_at_once(pkg, ctx):
    op = pkg.LimitOperatorFactory(ctx, 1, [pkg.BIGINT], 0).createOperator()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    with pytest.raises(pkg.TgpuError):
        op.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.arange(3, dtype=np.int64))))
    op.close()


def test_limit_beyond_the_stream_passes_every_page(pkg, ctx):
    rng = np.random.default_rng(1)
    sizes = [1, 0, 4097, 65]
    pages = [pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(0, 99, n).astype(np.int64), (rng.random(n) < 0.2).astype(np.uint8)),
                      pkg.Block(pkg.VARCHAR, [None if i % 5 == 0 else "s%d" % i for i in range(n)])) for n in sizes]
    op = pkg.LimitOperatorFactory(ctx, 1, [pkg.BIGINT, pkg.VARCHAR], 1 << 40).createOperator()
    outs = drive(op, pages)
    assert [o.getPositionCount() for o in outs] == expected_limit(sizes, 1 << 40) == sizes
    assert [cells(o) for o in outs] == [cells(p) for p in pages]
    assert op.needsInput() and not op.isFinished()
    op.finish()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()


@pytest.mark.parametrize("device_resident", [False, True])
def test_crossing_page_with_varchar_nulls_and_a_dictionary(pkg, ctx, device_resident):
    n = 1000
    def page(seed):
        r = np.random.default_rng(seed)
        return pkg.Page(pkg.Block(pkg.VARCHAR, [None if i % 9 == 0 else "row%d" % (i * seed) * (1 + i % 3) for i in range(n)]),
                        pkg.Block(pkg.DOUBLE, r.random(n), (r.random(n) < 0.3).astype(np.uint8)),
                        pkg.DictionaryBlock(pkg.Block(pkg.VARCHAR, ["a", None, "ccc", "dd"]), r.integers(0, 4, n).astype(np.int32)))
    pages = [page(1), page(2), page(3)]
    types = [pkg.VARCHAR, pkg.DOUBLE, pkg.VARCHAR]
    feed, head = pages, None
    if device_resident:
        f = pkg.field
        head = pkg.FilterAndProjectOperatorFactory(ctx, 9, types, None, [f(i, t) for i, t in enumerate(types)]).createOperator()
        feed = pkg.to_pages(head, pages, to_host=False)
    op = pkg.LimitOperatorFactory(ctx, 1, types, 1337).createOperator()
    outs = drive(op, feed)
    takes = expected_limit([n] * 3, 1337)
    assert takes == [1000, 337] and [o.getPositionCount() for o in outs] == takes   # the third page is not taken
    assert [cells(o) for o in outs] == [[c[:k] for c in cells(p)] for p, k in zip(pages, takes)]
    assert op.isFinished() and not op.needsInput()
    op.close()
    if head is not None:
        for o in feed:
            o.release()
        head.close()


def test_finish_before_the_limit(pkg, ctx):
    op = pkg.LimitOperatorFactory(ctx, 1, [pkg.BIGINT], 10).createOperator()
    op.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.arange(4, dtype=np.int64))))
    op.finish()   # remainingLimit = 0 with a page pending
    assert not op.isFinished() and not op.needsInput()
    o = op.getOutput()
    assert o.to_host().getBlock(0).values.tolist() == [0, 1, 2, 3]
    o.release()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()


def test_needs_input_and_is_finished_sequence(pkg, ctx):
    """LimitOperator.java:86-96 step by step over the crossing page"""
    f = pkg.LimitOperatorFactory(ctx, 1, [pkg.BIGINT], 5)
    a, b = f.createOperator(), f.duplicate().createOperator()
    page = pkg.Page(pkg.Block(pkg.BIGINT, np.arange(3, dtype=np.int64)))
    for op in (a, b):   # independent remainders
        assert op.needsInput() and not op.isFinished()
        op.addInput(page)
        assert not op.needsInput() and not op.isFinished()
        op.getOutput().release()
        assert op.needsInput() and not op.isFinished()      # 2 rows remain
        op.addInput(page)
        assert not op.needsInput() and not op.isFinished()  # remaining == 0, the cut page pending
        o = op.getOutput()
        assert o.to_host().getBlock(0).values.tolist() == [0, 1]
        o.release()
        assert not op.needsInput() and op.isFinished()
        with pytest.raises(pkg.TgpuError):
            op.addInput(page)
        op.close()


@pytest.mark.parametrize("types, limit", [([1], -1), ([], 5), ([99], 5)])
def test_factory_argument_errors(pkg, ctx, types, limit):
    with pytest.raises(pkg.TgpuError) as e:
        pkg.LimitOperatorFactory(ctx, 1, types, limit)
    assert e.value.code == -1   # TGPU_ERR_INVALID_ARGUMENT

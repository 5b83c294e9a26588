"""SetBuilderOperator + HashSemiJoinOperator on the GPU: the reference's TestHashSemiJoinOperator cases (tests/golden/semi_join_vectors.json), random
pages against the oracle's GroupByHash.contains plus HashSemiJoinOperator's three-valued rule (M/operator/HashSemiJoinOperator.java:191-215), the
blocking protocol, device-resident chaining and page sizes of millions of rows."""
import json
import os
import threading

import numpy as np
import pytest

from gpu_common import ocol, rand_block

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "semi_join_vectors.json")))
INT64_MIN, INT64_MAX = -(2**63), 2**63 - 1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def with_hash(pkg, oracle, page, channel=0):
    """RowPagesBuilder(hashEnabled = true): the raw hash of the key channel appended as a BIGINT channel"""
    h = oracle.hash_rows([ocol(oracle, page.getBlock(channel))])
    return page.appendColumn(pkg.Block(pkg.BIGINT, h.astype(np.int64)))


def build_set(pkg, ctx, types, pages, hash_channel=-1):
    bf = pkg.SetBuilderOperatorFactory(ctx, 1, types, 0, hash_channel, expected_positions=10)
    op = bf.createOperator()
    for p in pages:
        assert op.needsInput() and not op.isBlocked()
        op.addInput(p)
        assert op.getOutput() is None
    op.finish()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()
    return bf


def probe(pkg, ctx, supplier, probe_types, pages, hash_channel=-1, factory=None):
    jf = factory or pkg.HashSemiJoinOperatorFactory(ctx, 2, supplier, probe_types, 0, hash_channel)
    op = jf.createOperator()
    out = pkg.to_pages(op, pages)
    op.close()
    return out


def rows_without(pages, channel):
    """OperatorAssertion.dropChannel: the hash channel is compared away"""
    return [tuple(v for i, v in enumerate(r) if i != channel) for p in pages for r in p.rows()]


# ---- 1. the reference's cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_enabled", [False, True])
@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_reference_cases(pkg, ctx, oracle, case, hash_enabled):
    bt = getattr(pkg, case["build_type"])
    build = pkg.Page(pkg.Block(bt, case["build"]))
    btypes = [bt]
    if hash_enabled:
        build, btypes = with_hash(pkg, oracle, build), [bt, pkg.BIGINT]
    bf = build_set(pkg, ctx, btypes, [build], hash_channel=1 if hash_enabled else -1)
    pt = [getattr(pkg, t) for t in case["probe_types"]]
    page = pkg.Page(*[pkg.Block(t, list(c)) for t, c in zip(pt, zip(*case["probe"]))])
    hc = -1
    if hash_enabled:
        page, hc, pt = with_hash(pkg, oracle, page), len(pt), pt + [pkg.BIGINT]
    out = probe(pkg, ctx, bf.set_supplier, pt, [page], hc)
    assert len(out) == 1 and out[0].getChannelCount() == len(pt) + 1
    assert rows_without(out, hc) == [tuple(r) for r in case["expected"]]


def test_memory_limit_case(pkg, ctx):
    """testMemoryLimit (:433): the reference's 100-byte pool throws on the 10 000-row page -- the builder reports more than that"""
    bf = pkg.SetBuilderOperatorFactory(ctx, 1, [pkg.BIGINT], 0)
    op = bf.createOperator()
    op.addInput(pkg.Page(pkg.Block(pkg.BIGINT, np.arange(20, 10_020, dtype=np.int64))))
    assert op.memoryBytes() > 100
    op.finish()
    st = bf.set_supplier.stats()
    assert st["size"] == 10_000 and not st["contains_null"] and st["layout"] == pkg.SET_BITMAP
    assert op.memoryBytes() == st["bytes"] > 0
    op.close()


# ---- 3. random pages against the oracle ---------------------------------------------------------------------------------------------
def expected_verdicts(oracle, pkg, type_id, build_blocks, probe_block):
    """GroupByHash.contains over the build keys (ChannelSet.java:70-78) + HashSemiJoinOperator.java:191-215"""
    cols = [ocol(oracle, b) for b in build_blocks]
    if type_id == pkg.BIGINT:
        g = oracle.BigintGroupByHash(16)
        for c in cols:
            if c.n:
                g.get_group_ids(c)
    else:
        g = oracle.MultiChannelGroupByHash([type_id], 16)
        for c in cols:
            if c.n:
                g.get_group_ids([c])
    empty = sum(c.n for c in cols) == 0
    contains_null = any(c.nulls is not None and c.nulls[: c.n].any() for c in cols)
    pc = ocol(oracle, probe_block)
    hashes = oracle.hash_rows([pc]) if pc.n else []
    out = []
    for pos in range(pc.n):
        if pc.nulls is not None and pc.nulls[pos]:
            out.append(False if empty else None)
            continue
        hit = g.contains(pc, pos) if type_id == pkg.BIGINT else g.contains([pc], pos, hashes[pos])
        out.append(None if (not hit and contains_null) else hit)
    return out, g.group_count


def special_block(pkg, rng, type_id, n, null_frac, kind):
    """keys of the case: values drawn from a domain that makes build and probe overlap, plus the edge values of the type"""
    if kind == "bigint_dense":
        b = rand_block(pkg, rng, pkg.BIGINT, n, null_frac, domain=(1000, 6000))
    elif kind == "bigint_sparse":
        b = rand_block(pkg, rng, pkg.BIGINT, n, null_frac, domain=(-(2**62), 2**62))
        v = b.values.copy()
        pool = np.array([0, -1, INT64_MIN, INT64_MAX, 1 << 40, -(1 << 50)], dtype=np.int64)
        pick = rng.random(n) < 0.5
        v[pick] = rng.choice(np.concatenate([pool, v[: max(1, n // 8)]]), int(pick.sum()))
        b = pkg.Block(pkg.BIGINT, v, b.nulls)
    elif kind == "integer":
        b = rand_block(pkg, rng, pkg.INTEGER, n, null_frac)
        v = b.values.copy()
        pick = rng.random(n) < 0.5
        v[pick] = rng.choice(np.array([0, -1, -(2**31), 2**31 - 1, 7, 123456], dtype=np.int32), int(pick.sum()))
        b = pkg.Block(pkg.INTEGER, v, b.nulls)
    elif kind == "date":
        b = rand_block(pkg, rng, pkg.DATE, n, null_frac, domain=(8000, 10000))
    elif kind == "double":
        v = rng.integers(-40, 40, n).astype(np.float64) / 4.0
        pick = rng.random(n) < 0.2
        v[pick] = rng.choice(np.array([np.nan, 0.0, -0.0, np.inf, -np.inf]), int(pick.sum()))
        b = pkg.Block(pkg.DOUBLE, v, rand_block(pkg, rng, pkg.DOUBLE, n, null_frac).nulls)
    else:
        b = rand_block(pkg, rng, pkg.VARCHAR, n, null_frac, domain=(0, 150))
        vals = b.to_list()
        for i in np.nonzero(rng.random(n) < 0.1)[0]:
            if vals[i] is not None:
                vals[i] = ""
        b = pkg.Block(pkg.VARCHAR, vals)
    return b


def comparable(values):
    return [("NaN",) if isinstance(v, float) and v != v else v for v in values]


KINDS = {"bigint_dense": "BIGINT", "bigint_sparse": "BIGINT", "integer": "INTEGER", "date": "DATE", "double": "DOUBLE", "varchar": "VARCHAR"}
LAYOUT = {"bigint_dense": 0, "bigint_sparse": 1, "integer": 1, "date": 0, "double": 2, "varchar": 2}


@pytest.mark.parametrize("probe_nulls", [0.0, 0.03, 0.5])
@pytest.mark.parametrize("build_nulls", [0.0, 0.03, 0.5])
@pytest.mark.parametrize("kind", list(KINDS))
def test_random_pages_match_oracle(pkg, ctx, oracle, kind, build_nulls, probe_nulls):
    rng = np.random.default_rng(list(KINDS).index(kind) * 100 + int(build_nulls * 100) * 10 + int(probe_nulls * 10))
    t = getattr(pkg, KINDS[kind])
    build_blocks = [special_block(pkg, rng, t, n, build_nulls, kind) for n in (1500, 0, 1, 700)]
    bf = build_set(pkg, ctx, [t, pkg.BIGINT], [pkg.Page(b, pkg.Block(pkg.BIGINT, np.arange(b.position_count, dtype=np.int64))) for b in build_blocks])
    st = bf.set_supplier.stats()
    flat = special_block(pkg, rng, t, 3000, probe_nulls, kind)
    dict_values = special_block(pkg, rng, t, 40, probe_nulls, kind)
    dictionary = pkg.DictionaryBlock(dict_values, rng.integers(0, 40, 2000).astype(np.int32))
    rle = pkg.RunLengthEncodedBlock(special_block(pkg, rng, t, 1, probe_nulls, kind), 500)
    probes = [flat, dictionary, rle, special_block(pkg, rng, t, 0, 0.0, kind)]
    pages = [pkg.Page(b, pkg.Block(pkg.BIGINT, np.arange(b.getPositionCount(), dtype=np.int64))) for b in probes]
    out = probe(pkg, ctx, bf.set_supplier, [t, pkg.BIGINT], pages)
    assert [p.getPositionCount() for p in out] == [p.getPositionCount() for p in pages if p.getPositionCount() > 0]   # one page per page
    for page, got in zip([p for p in pages if p.getPositionCount() > 0], out):
        want, groups = expected_verdicts(oracle, pkg, t, build_blocks, page.getBlock(0))
        assert got.getBlock(2).to_list() == want
        assert comparable(got.getBlock(0).to_list()) == comparable(page.getBlock(0).flatten().to_list())   # the probe channels pass through unchanged
        assert got.getBlock(1).to_list() == page.getBlock(1).to_list()
        if isinstance(page.getBlock(0), pkg.Block):   # a flat key: a null vector only when the rule can produce a null
            can_null = (page.getBlock(0).nulls is not None and page.getBlock(0).nulls.any()) or st["contains_null"]
            assert (got.getBlock(2).nulls is not None) == bool(can_null)
    assert st["size"] == groups
    assert st["contains_null"] == (build_nulls > 0)
    assert st["layout"] == LAYOUT[kind]


# ---- 4. edge sets ---------------------------------------------------------------------------------------------------------------
def test_zero_build_rows(pkg, ctx):
    bf = build_set(pkg, ctx, [pkg.BIGINT], [])
    assert bf.set_supplier.stats()["size"] == 0
    out = probe(pkg, ctx, bf.set_supplier, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, [1, None, 3]))])
    assert out[0].getBlock(1).to_list() == [False, False, False] and out[0].getBlock(1).nulls is None   # an empty set never yields null


def test_only_null_build_rows(pkg, ctx):
    bf = build_set(pkg, ctx, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, [None, None]))])
    st = bf.set_supplier.stats()
    assert st["size"] == 1 and st["contains_null"]
    out = probe(pkg, ctx, bf.set_supplier, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, [None, 5]))])
    assert out[0].getBlock(1).to_list() == [None, None]


@pytest.mark.parametrize("type_name", ["BIGINT", "INTEGER", "DATE", "DOUBLE", "VARCHAR"])
def test_single_key(pkg, ctx, type_name):
    t = getattr(pkg, type_name)
    k, other = ("7", "8") if t == pkg.VARCHAR else ((7.0, 8.0) if t == pkg.DOUBLE else (7, 8))
    bf = build_set(pkg, ctx, [t], [pkg.Page(pkg.Block(t, [k]))])
    assert bf.set_supplier.stats()["size"] == 1
    out = probe(pkg, ctx, bf.set_supplier, [t], [pkg.Page(pkg.Block(t, [k, other, None]))])
    assert out[0].getBlock(1).to_list() == [True, False, None]


def test_sparse_set_sentinel_key(pkg, ctx):
    """the hash layout's free-slot value is INT64_MIN: absent, it must not be found; present, it must"""
    for keys, want in (([1, 2**62], [False, True, False]), ([INT64_MIN, 2**62], [True, True, False])):
        bf = build_set(pkg, ctx, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, np.array(keys, dtype=np.int64)))])
        assert bf.set_supplier.stats()["layout"] == pkg.SET_HASH
        out = probe(pkg, ctx, bf.set_supplier, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, np.array([INT64_MIN, 2**62, 0], dtype=np.int64)))])
        assert out[0].getBlock(1).to_list() == want


def test_probe_type_must_match_the_set(pkg, ctx):
    bf = pkg.SetBuilderOperatorFactory(ctx, 1, [pkg.BIGINT], 0)
    with pytest.raises(pkg.TgpuError) as e:
        pkg.HashSemiJoinOperatorFactory(ctx, 2, bf.set_supplier, [pkg.INTEGER], 0)
    assert e.value.code == -1


# ---- 5. protocol ----------------------------------------------------------------------------------------------------------------
def test_probe_blocks_until_the_set_is_built(pkg, ctx):
    bf = pkg.SetBuilderOperatorFactory(ctx, 1, [pkg.BIGINT], 0)
    jf = pkg.HashSemiJoinOperatorFactory(ctx, 2, bf.set_supplier, [pkg.BIGINT], 0)
    pr = jf.createOperator()
    assert pr.isBlocked() and not pr.needsInput() and pr.getOutput() is None
    with pytest.raises(pkg.TgpuError):
        bf.set_supplier.stats()
    b = bf.createOperator()
    b.addInput(pkg.Page(pkg.Block(pkg.BIGINT, [1, 2, 3])))
    assert pr.isBlocked()
    b.finish()
    assert not pr.isBlocked() and pr.needsInput()
    pr.addInput(pkg.Page(pkg.Block(pkg.BIGINT, [3, 4])))
    assert not pr.needsInput()
    o = pr.getOutput()
    assert o.to_host().rows() == [(3, True), (4, False)]
    o.release()
    pr.finish()
    assert pr.isFinished()
    pr.close()
    b.close()


def test_probe_finished_without_input_while_blocked(pkg, ctx):
    bf = pkg.SetBuilderOperatorFactory(ctx, 1, [pkg.BIGINT], 0)
    jf = pkg.HashSemiJoinOperatorFactory(ctx, 2, bf.set_supplier, [pkg.BIGINT], 0)
    pr = jf.createOperator()
    assert pr.isBlocked()
    pr.finish()
    assert pr.isFinished() and not pr.isBlocked() and pr.getOutput() is None
    pr.close()


def test_two_probe_operators_on_two_threads_share_one_set(pkg, ctx, oracle):
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 50_000, 20_000).astype(np.int64)
    bf = build_set(pkg, ctx, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, keys))])
    jf = pkg.HashSemiJoinOperatorFactory(ctx, 2, bf.set_supplier, [pkg.BIGINT], 0)
    jf2 = jf.duplicate()
    inputs = [[pkg.Page(pkg.Block(pkg.BIGINT, rng.integers(-100, 50_100, 30_000).astype(np.int64))) for _ in range(4)] for _ in range(2)]
    results, errors = [None, None], []

    def run(i, f):
        try:
            results[i] = probe(pkg, ctx, None, None, inputs[i], factory=f)
        except Exception as e:   # reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=run, args=(0, jf)), threading.Thread(target=run, args=(1, jf2))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        got = np.concatenate([p.getBlock(1).values.astype(bool) for p in results[i]])
        want = np.isin(np.concatenate([p.getBlock(0).values for p in inputs[i]]), keys)
        assert np.array_equal(got, want)


# ---- 6. device-resident chaining: WHERE x IN (...) / NOT IN ---------------------------------------------------------------------------
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("borrowed", [False, True])
def test_filter_semi_join_filter_on_the_device(pkg, ctx, oracle, negate, borrowed):
    f = pkg.field
    B = pkg.BIGINT
    rng = np.random.default_rng(11)
    build_keys = pkg.Block(B, rng.integers(0, 400, 300).astype(np.int64), (rng.random(300) < 0.02).astype(np.uint8))
    bf = build_set(pkg, ctx, [B], [pkg.Page(build_keys)])
    x = pkg.Block(B, rng.integers(0, 800, 5000).astype(np.int64), (rng.random(5000) < 0.05).astype(np.uint8))
    y = pkg.Block(B, np.arange(5000, dtype=np.int64))
    head = pkg.FilterAndProjectOperatorFactory(ctx, 10, [B, B], f(1, B) > 100, [f(0, B), f(1, B)]).createOperator()
    semi = pkg.HashSemiJoinOperatorFactory(ctx, 11, bf.set_supplier, [B, B], 0).createOperator()
    pred = pkg.not_(f(2, pkg.BOOLEAN)) if negate else f(2, pkg.BOOLEAN)
    tail = pkg.FilterAndProjectOperatorFactory(ctx, 12, [B, B, pkg.BOOLEAN], pred, [f(0, B), f(1, B)]).createOperator()
    head.addInput(pkg.Page(x, y))
    o1 = head.getOutput()
    if borrowed:   # the semi join sees caller-owned device blocks and must copy what it passes through
        dev = o1.as_device_page()
        semi.addInput(dev)
        o1.release()
    else:
        semi.addInput(o1)
        o1.release()
    o2 = semi.getOutput()
    tail.addInput(o2)
    o2.release()
    o3 = tail.getOutput()
    got = o3.to_host().rows() if o3 is not None else []
    if o3 is not None:
        o3.release()
    keep = [i for i in range(5000) if i > 100]
    sub = pkg.Block(B, x.values[keep], x.nulls[keep])
    verdict, _ = expected_verdicts(oracle, pkg, B, [build_keys], sub)
    want = [(sub.get(i), keep[i]) for i, v in enumerate(verdict) if (v is False if negate else v is True)]
    assert got == want
    for op in (head, semi, tail):
        op.close()


# ---- 7. size: 2^22-row probe pages against a 2^20-key set ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bitmap", "hash"])
def test_large_pages(pkg, ctx, layout):
    rng = np.random.default_rng(23)
    n_set, n_probe = 1 << 20, 1 << 22
    if layout == "bitmap":
        keys = rng.choice(np.arange(1 << 22, dtype=np.int64), n_set, replace=False)
        probe_keys = rng.integers(-1000, (1 << 22) + 1000, n_probe).astype(np.int64)
    else:
        keys = rng.integers(-(2**62), 2**62, n_set).astype(np.int64)
        probe_keys = np.where(rng.random(n_probe) < 0.5, rng.choice(keys, n_probe), rng.integers(-(2**62), 2**62, n_probe)).astype(np.int64)
    bf = build_set(pkg, ctx, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, keys[: n_set // 2])), pkg.Page(pkg.Block(pkg.BIGINT, keys[n_set // 2:]))])
    st = bf.set_supplier.stats()
    assert st["layout"] == (pkg.SET_BITMAP if layout == "bitmap" else pkg.SET_HASH) and st["size"] == len(np.unique(keys))
    nulls = (rng.random(n_probe) < 0.03).astype(np.uint8)
    out = probe(pkg, ctx, bf.set_supplier, [pkg.BIGINT], [pkg.Page(pkg.Block(pkg.BIGINT, probe_keys, nulls))] * 2)
    want = np.isin(probe_keys, keys) & (nulls == 0)
    for p in out:
        b = p.getBlock(1)
        assert np.array_equal(b.values.astype(bool), want)
        assert np.array_equal(b.nulls.astype(bool), nulls.astype(bool))   # a null key against a non-empty set without nulls: null

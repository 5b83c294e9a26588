"""TopN, OrderBy and the VARCHAR min / max of DynamicFilterSourceOperator on pages large enough to leave the plain path of csrc/topn.hip.

sorted_positions() chooses by three thresholds:
  * rows > 4 * 65536 and min(n, rows) < 32768: the SAMPLED CUTOFF (profile scope topn_sample_cut, S below);
  * more than max(8 * want, 1 << 18) candidates: the COARSE-CODE RADIX sort and its cut at the ties of the n-th code (topn_code_radix, R);
  * TopNGpu::add_page FOLDS its store once it holds more than max(4 * n, 65536) rows: one more sorted_positions call, so a stream of
    non-empty pages shows topn_select `pages + folds + 1` times (the + 1 is the final result(), absent when the last page folded).
Every case asserts (a) the output's sequence column == oracle.top_n exactly (same rows, same order, input order among equal rows), (b) every
other output column == the input column gathered at those positions (fixed width bit for bit where not null, null vectors equal, VARCHAR
through to_list()), (c) the set of {S, R} scopes the profile saw.  There is no tolerance anywhere."""
import numpy as np
import pytest

from gpu_common import ocol, rand_block

pytestmark = pytest.mark.gpu
S, R, SELECT = "topn_sample_cut", "topn_code_radix", "topn_select"
ROWS = 300_007   # above the sampling threshold (262 144), odd, no multiple of a block


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def topn_scopes(ctx, fn):
    """(fn(), which of S / R the profile saw while fn ran, how often topn_select ran)"""
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        result = fn()
        ctx.synchronize()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    count = lambda k: prof.get(k, {"count": 0})["count"]
    return result, {k for k in (S, R) if count(k) > 0}, count(SELECT)


def seq_block(pkg, n):
    return pkg.Block(pkg.BIGINT, np.arange(n, dtype=np.int64))


def null_vector(rng, n, frac):
    return (rng.random(n) < frac).astype(np.uint8)


def quarters_block(pkg, rng, n, null_frac):
    """DOUBLE in {-5 .. 5} / 4: eleven values, heavy ties"""
    return pkg.Block(pkg.DOUBLE, rng.integers(-5, 6, n).astype(np.float64) / 4.0, null_vector(rng, n, null_frac))


def customer_block(pkg, ids, nulls):
    """VARCHAR "Customer#%09d" (18 bytes, the first 8 shared: every order code is equal); null rows are empty"""
    n = len(ids)
    cells = np.char.mod("Customer#%09d", ids).astype("S18").view(np.uint8).reshape(n, 18)
    keep = nulls == 0
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.where(keep, 18, 0))
    return pkg.Block(pkg.VARCHAR, np.ascontiguousarray(cells[keep]).ravel(), nulls, offsets)


def cut(pkg, b, a, z):
    """rows [a, z) of a flat block"""
    nulls = None if b.nulls is None else b.nulls[a:z]
    if b.type == pkg.VARCHAR:
        lo, hi = int(b.offsets[a]), int(b.offsets[z])
        return pkg.Block(pkg.VARCHAR, b.values[lo:hi] if hi > lo else np.zeros(1, dtype=np.uint8), nulls, b.offsets[a:z + 1] - lo)
    return pkg.Block(b.type, b.values[a:z], nulls)


def pages_of(pkg, blocks, sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] == blocks[0].position_count
    if len(sizes) == 1:
        return [pkg.Page(*blocks)]
    return [pkg.Page(*[cut(pkg, b, int(a), int(z)) for b in blocks]) for a, z in zip(edges[:-1], edges[1:])]


def assert_gathered(pkg, got, want, positions, want_list=None):
    """block `got` == the rows `positions` of block `want`"""
    assert got.type == want.type and got.position_count == len(positions)
    if want.type == pkg.VARCHAR:
        expect = [want.get(int(i)) for i in positions] if want_list is None else [want_list[i] for i in positions]
        assert got.to_list() == expect
        return
    wn = np.zeros(len(positions), dtype=bool) if want.nulls is None else want.nulls[positions].astype(bool)
    gn = np.zeros(len(positions), dtype=bool) if got.nulls is None else got.nulls.astype(bool)
    assert np.array_equal(gn, wn)
    width = want.values.dtype.itemsize
    g = np.ascontiguousarray(got.values).view(np.uint8).reshape(-1, width)[~gn]
    w = np.ascontiguousarray(want.values[positions]).view(np.uint8).reshape(-1, width)[~wn]
    assert np.array_equal(g, w)


def check_top_n(pkg, ctx, oracle, blocks, sizes, n, sort_channels, sort_orders, lists=None, order_by=False):
    """runs the operator over `blocks` (the last one the sequence 0 .. rows-1) cut into pages of `sizes` rows, asserts (a) and (b) and returns
    (the S / R scopes, the count of topn_select) for (c).  lists: channel -> to_list() of a large VARCHAR block, made once"""
    types = [b.type for b in blocks]
    seq = len(blocks) - 1
    assert np.array_equal(blocks[seq].values, np.arange(blocks[seq].position_count))
    pages = pages_of(pkg, blocks, sizes)
    if order_by:
        fac = pkg.OrderByOperatorFactory(ctx, 0, types, list(range(len(types))), 10, sort_channels, sort_orders)
    else:
        fac = pkg.TopNOperatorFactory(ctx, 0, types, n, sort_channels, sort_orders)
    op = fac.createOperator()
    out, scopes, selects = topn_scopes(ctx, lambda: pkg.to_pages(op, pages))
    op.close()
    fac.close()
    want = oracle.top_n([ocol(oracle, b) for b in blocks], n, sort_channels, sort_orders)
    got = np.concatenate([p.getBlock(seq).values for p in out]) if out else np.zeros(0, dtype=np.int64)
    assert np.array_equal(got, want), (sort_channels, sort_orders)                                       # (a)
    at = 0
    for p in out:
        positions = want[at:at + p.position_count].astype(np.int64)
        at += p.position_count
        for ch in range(seq):
            assert_gathered(pkg, p.getBlock(ch), blocks[ch], positions, (lists or {}).get(ch))           # (b)
    return scopes, selects


# ---- the size threshold -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,scopes", [(262_144, set()), (262_145, {S})])
def test_sampling_starts_above_262144_rows(pkg, ctx, oracle, rows, scopes):
    rng = np.random.default_rng(71)
    blocks = [pkg.Block(pkg.BIGINT, rng.permutation(rows).astype(np.int64)), seq_block(pkg, rows)]
    assert check_top_n(pkg, ctx, oracle, blocks, [rows], 10, [0], [pkg.ASC_NULLS_LAST])[0] == scopes


# ---- fine codes: a continuous DOUBLE key ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fine(pkg):
    rng = np.random.default_rng(72)
    bits = rng.standard_normal(ROWS).view(np.uint64).copy()
    special = rng.random(ROWS) < 0.01   # two NaNs (Double.compare: equal), both infinities, both zeros (-0.0 < 0.0)
    bits[special] = rng.choice(np.array([0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000000, 0xfff0000000000000, 0, 0x8000000000000000], dtype=np.uint64),
                               int(special.sum()))
    return [pkg.Block(pkg.DOUBLE, bits.view(np.float64), null_vector(rng, ROWS, 0.05)), rand_block(pkg, rng, pkg.BIGINT, ROWS, 0.05, (-50, 50)), seq_block(pkg, ROWS)]


@pytest.mark.parametrize("order", ["ASC_NULLS_FIRST", "ASC_NULLS_LAST", "DESC_NULLS_FIRST", "DESC_NULLS_LAST"])
def test_fine_codes_every_sort_order(pkg, ctx, oracle, fine, order):
    """the winners are the nulls (nulls first), the -inf rows (ascending) or the rows of both NaNs (descending): hundreds of rows that tie on
    the first key, so the second key and the input order decide; (b) sees the NaN payloads come through"""
    assert check_top_n(pkg, ctx, oracle, fine, [ROWS], 10, [0, 1], [getattr(pkg, order), pkg.DESC_NULLS_FIRST])[0] == {S}


# ---- codes drop the key's low bit -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def low_bits(pkg):
    """a permutation k of 0 .. rows-1 as BIGINT and as the DOUBLE 1.0 + k * 2**-52: 2k and 2k + 1 share an order code, no two rows are equal"""
    k = np.random.default_rng(73).permutation(ROWS).astype(np.int64)
    return [pkg.Block(pkg.BIGINT, k), pkg.Block(pkg.DOUBLE, (k + 0x3ff0000000000000).view(np.float64)), seq_block(pkg, ROWS)]


@pytest.mark.parametrize("order", ["ASC_NULLS_LAST", "DESC_NULLS_LAST"])
@pytest.mark.parametrize("n", [10, 11])
@pytest.mark.parametrize("channel", [0, 1])
def test_keys_that_share_a_code_through_the_low_bit(pkg, ctx, oracle, low_bits, channel, n, order):
    """one of n = 10 and n = 11 ends between two pairs of one code, the other inside a pair: ascending the pairs are (0, 1), (2, 3), ..., so it is
    n = 11 that splits one; descending the largest value 300 006 has a code of its own, so it is n = 10"""
    assert check_top_n(pkg, ctx, oracle, low_bits, [ROWS], n, [channel], [getattr(pkg, order)])[0] == {S}


# ---- the n threshold of the sample and the 8 * n threshold of the radix branch ----------------------------------------------------------
@pytest.fixture(scope="module")
def five_classes(pkg):
    rng = np.random.default_rng(74)
    return [pkg.Block(pkg.BIGINT, rng.integers(0, 5, ROWS).astype(np.int64)), quarters_block(pkg, rng, ROWS, 0.05), seq_block(pkg, ROWS)]


@pytest.mark.parametrize("n,scopes", [(32_767, {S}), (32_768, {R}), (37_500, {R}), (37_501, set())])
def test_n_thresholds(pkg, ctx, oracle, five_classes, n, scopes):
    """five classes of about 60 000 rows.  n = 32 767 is sampled and keeps four classes (240 000 candidates: not above max(8 n, 1 << 18));
    n = 32 768 is not sampled and 300 007 rows exceed 1 << 18 = 8 n: radix; 8 * 37 500 = 300 000 < 300 007 <= 8 * 37 501"""
    assert check_top_n(pkg, ctx, oracle, five_classes, [ROWS], n, [0, 1], [pkg.ASC_NULLS_LAST, pkg.DESC_NULLS_FIRST])[0] == scopes


# ---- the radix branch behind the sample -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values,rare,n", [((9000, 9001, 9002), True, 10), ((9000, 9001, 9002), True, 12), ((9000, 9001, 9002), True, 13), ((9000, 9001, 9002), False, 10),
                                           ((9000, 9002, 9004), True, 10), ((9000, 9002, 9004), True, 12), ((9000, 9002, 9004), True, 13)])
def test_radix_behind_the_sample(pkg, ctx, oracle, values, rare, n):
    """600 011 rows of two DATE values at random; with `rare` a smaller third one in exactly 12 rows, at 1 + 9000 j: the sample (stride
    600 011 // 65 536 = 9, rows 9 i) sees none of them and cuts at the class above, about 300 000 candidates.  9000 and 9001 share a code (the
    radix step keeps every candidate), 9000 / 9002 / 9004 do not (it narrows to the 12 rows for n <= 12, n = 13 spills into the next class)"""
    rows = 600_011
    rng = np.random.default_rng(75)
    low, mid, high = values
    date = rng.choice(np.array([mid, high], dtype=np.int32), rows)
    if rare:
        date[1 + 9000 * np.arange(12)] = low
    blocks = [pkg.Block(pkg.DATE, date), rand_block(pkg, rng, pkg.DOUBLE, rows, 0.05), seq_block(pkg, rows)]
    assert check_top_n(pkg, ctx, oracle, blocks, [rows], n, [0, 1], [pkg.ASC_NULLS_LAST, pkg.ASC_NULLS_FIRST])[0] == {S, R}


# ---- VARCHAR whose first 8 bytes are shared: every code is equal ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def customers(pkg):
    """[VARCHAR "Customer#%09d" of 100 000 ids (ties) with 2 % nulls, BIGINT -50 .. 50, DOUBLE, sequence] and the VARCHAR's to_list()"""
    rng = np.random.default_rng(76)
    blocks = [customer_block(pkg, rng.integers(0, 10**5, ROWS), null_vector(rng, ROWS, 0.02)), rand_block(pkg, rng, pkg.BIGINT, ROWS, 0.05, (-50, 50)),
              rand_block(pkg, rng, pkg.DOUBLE, ROWS, 0.05), seq_block(pkg, ROWS)]
    return blocks, {0: blocks[0].to_list()}


@pytest.mark.parametrize("order,n,scopes", [("ASC_NULLS_LAST", 10, {S, R}), ("ASC_NULLS_LAST", 5000, {S, R}), ("DESC_NULLS_LAST", 10, {S, R}), ("DESC_NULLS_LAST", 5000, {S, R}),
                                            ("ASC_NULLS_FIRST", 10, {S})])
def test_shared_prefix_varchar(pkg, ctx, oracle, customers, order, n, scopes):
    """nulls last: the cutoff is the one code of every value, 294 000 candidates, the radix step keeps them all and the comparator decides.
    Nulls first: the ten winners are nulls, the second key decides"""
    blocks, lists = customers
    assert check_top_n(pkg, ctx, oracle, blocks, [ROWS], n, [0, 1], [getattr(pkg, order), pkg.DESC_NULLS_FIRST], lists)[0] == scopes


def test_order_by_large_shared_prefix_varchar(pkg, ctx, oracle, customers):
    """OrderBy sorts every row: neither the sample (n >= 32 768) nor the radix step (rows <= 8 n)"""
    blocks, lists = customers
    scopes, _ = check_top_n(pkg, ctx, oracle, blocks, [200_000, 100_007], ROWS, [0, 2], [pkg.DESC_NULLS_FIRST, pkg.ASC_NULLS_LAST], lists, order_by=True)
    assert scopes == set()


# ---- VARCHAR at the edges of the 8-byte code --------------------------------------------------------------------------------------------
def edge_family(base):
    """around an 8-byte string: itself, one byte more (0x00, 0x01, 'z'), 40 bytes more, one byte less, and its neighbour in the last bit of
    the eighth byte -- all but the 7-byte one share an order code"""
    assert len(base) == 8
    return [base, base + b"\x00", base + b"\x01", base + b"z", base + bytes(range(40, 80)), base[:7], base[:7] + bytes([base[7] ^ 1])]


@pytest.fixture(scope="module")
def code_edges(pkg):
    """rare strings (1 to 6 rows each) below and above 2000 filler strings, so that they are the winners in both directions: the empty string,
    strings shorter than 8 bytes, the edge family of "abcdefgh" below; strings of bytes >= 0x80 (they compare unsigned) and the edge family of
    an 8-byte string that begins with U+00FF above.  2 % nulls"""
    rng = np.random.default_rng(77)
    rare = [b"", b"a", b"ab", b"abc"] + edge_family(b"abcdefgh") + ["é".encode(), "éclair".encode(), "zé".encode(), "ÿ".encode(), "ÿÿ".encode()] \
        + edge_family("ÿbcdefg".encode())
    pool = rare + [("k%04d-filler-%s" % (i, "x" * (i % 5))).encode() for i in range(2000)]
    idx = rng.integers(len(rare), len(pool), ROWS)
    counts = rng.integers(1, 7, len(rare))
    where = rng.choice(ROWS, int(counts.sum()), replace=False)
    idx[where] = np.repeat(np.arange(len(rare)), counts)
    nulls = null_vector(rng, ROWS, 0.02)
    items = [None if nulls[i] else pool[k] for i, k in enumerate(idx)]
    blocks = [pkg.Block(pkg.VARCHAR, items), rand_block(pkg, rng, pkg.BIGINT, ROWS, 0.05, (-50, 50)), seq_block(pkg, ROWS)]
    return blocks, {0: [None if v is None else v.decode("utf-8", "replace") for v in items]}


@pytest.mark.parametrize("order", ["ASC_NULLS_FIRST", "ASC_NULLS_LAST", "DESC_NULLS_FIRST", "DESC_NULLS_LAST"])
@pytest.mark.parametrize("n", [10, 100])
def test_varchar_code_edges(pkg, ctx, oracle, code_edges, n, order):
    blocks, lists = code_edges
    assert check_top_n(pkg, ctx, oracle, blocks, [ROWS], n, [0, 1], [getattr(pkg, order), pkg.ASC_NULLS_LAST], lists)[0] == {S}


# ---- streaming: large and small pages into one operator ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(pkg):
    """the column mix of test_gpu_parity.py::test_top_n_matches_oracle (nulls, NaN / +-0.0 / infinities, few distinct values, varchar longer
    than the order code), by its generator, for pages of 300 007, 1000 and 280 000 rows"""
    n_rows = ROWS + 1000 + 280_000
    rng = np.random.default_rng(78)
    dbl = rng.integers(-5, 6, n_rows).astype(np.float64) / 4.0
    special = rng.integers(0, n_rows, max(n_rows // 50, 1))
    dbl[special] = rng.choice([np.nan, np.inf, -np.inf, -0.0, 0.0], len(special))
    strs = [None if k % 17 == 0 else "key-prefix-%03d%s" % (k % 40, "x" * (k % 3)) for k in rng.integers(0, 1000, n_rows)]
    blocks = [pkg.Block(pkg.DOUBLE, dbl, (rng.random(n_rows) < 0.05).astype(np.uint8)), pkg.Block(pkg.VARCHAR, strs),
              rand_block(pkg, rng, pkg.BIGINT, n_rows, 0.05, (-50, 50)), rand_block(pkg, rng, pkg.DATE, n_rows, 0.0, (9000, 9020)), seq_block(pkg, n_rows)]
    return blocks, {1: strs}


@pytest.mark.parametrize("n", [10, 5000])
def test_streaming_large_and_small_pages(pkg, ctx, oracle, mixed, n):
    blocks, lists = mixed
    for sort_channels, sort_orders in ([[0], [pkg.DESC_NULLS_LAST]], [[0], [pkg.ASC_NULLS_FIRST]], [[1, 2], [pkg.ASC_NULLS_LAST, pkg.DESC_NULLS_FIRST]],
                                      [[3, 0, 1], [pkg.DESC_NULLS_FIRST, pkg.ASC_NULLS_LAST, pkg.DESC_NULLS_LAST]]):
        scopes, selects = check_top_n(pkg, ctx, oracle, blocks, [ROWS, 1000, 280_000], n, sort_channels, sort_orders, lists)
        assert S in scopes and selects == 3 + 0 + 1, (sort_channels, sort_orders)


# ---- the fold of the candidate store ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pages,rows,n,selects", [(7, 20_000, 17_000, 9), (70, 1000, 1000, 72), (66, 1000, 1000, 67)])
def test_fold_of_the_candidate_store(pkg, ctx, oracle, pages, rows, n, selects):
    """heavy ties through every fold.  n = 17 000: the store passes max(4 n, 65 536) = 68 000 rows with page 5 (85 000), one fold: 7 + 1 + 1.
    n = 1000: it passes 65 536 with page 66: 70 + 1 + 1; where page 66 is the last one the folded store is the answer as it stands: 66 + 1"""
    rng = np.random.default_rng(79)
    total = pages * rows
    blocks = [rand_block(pkg, rng, pkg.BIGINT, total, 0.1, (-20, 20)), quarters_block(pkg, rng, total, 0.1), seq_block(pkg, total)]
    scopes, got = check_top_n(pkg, ctx, oracle, blocks, [rows] * pages, n, [0, 1], [pkg.ASC_NULLS_FIRST, pkg.DESC_NULLS_LAST])
    assert scopes == set() and got == selects


# ---- DynamicFilterSourceOperator: VARCHAR min / max = sorted_positions(..., 1, ...) in both directions ----------------------------------
def test_dynamic_filter_varchar_min_max_of_a_large_page(pkg, ctx, oracle):
    """more than 50 distinct values: the operator turns to min / max over the 294 000 distinct values of page 1 (want = 1 and one code for every
    value: sample, then radix, in both directions); page 2 brings a new minimum and a new maximum to the running pair"""
    rng = np.random.default_rng(80)
    ids2 = rng.integers(1000, 10**9 - 1000, 5000)
    nulls2 = null_vector(rng, 5000, 0.02)
    ids2[17], ids2[4000] = 5, 10**9 - 5
    nulls2[17] = nulls2[4000] = 0
    pages = [customer_block(pkg, rng.integers(1000, 10**9 - 1000, ROWS), null_vector(rng, ROWS, 0.02)), customer_block(pkg, ids2, nulls2)]
    fac = pkg.DynamicFilterSourceOperatorFactory(ctx, 0, [pkg.VARCHAR], [0], 50, 1 << 30, 1 << 30)
    op = fac.createOperator()
    ref = oracle.DynamicFilterSource([pkg.VARCHAR], [0], 50, 1 << 30, 1 << 30)

    def feed(block):
        assert op.needsInput()
        op.addInput(pkg.Page(block))
        out = op.getOutput()
        assert out is not None
        host = out.to_host().getBlock(0)
        out.release()
        return host
    for i, block in enumerate(pages):
        host, scopes, _ = topn_scopes(ctx, lambda: feed(block))
        assert scopes == ({S, R} if i == 0 else set())
        end = int(block.offsets[-1])   # the page passes through unchanged
        assert host.nulls is not None and np.array_equal(host.nulls, block.nulls)
        assert np.array_equal(host.offsets, block.offsets) and np.array_equal(host.values[:end], block.values[:end])
        ref.add([ocol(oracle, block)])
    op.finish()
    assert op.isFinished()
    values = [v for b in pages for v in b.to_list() if v is not None]
    lo, hi = min(values, key=lambda v: v.encode()), max(values, key=lambda v: v.encode())
    assert (lo, hi) == ("Customer#000000005", "Customer#999999995")
    assert op.domain(0) == ("range", lo, hi) == ref.domain(0)
    op.close()
    fac.close()

"""Shared helpers of the MarkDistinctOperator / DistinctLimitOperator GPU tests: random key pages, the drivers and the comparison with
tests/distinct_expected.py."""
import numpy as np

from distinct_expected import DistinctOracle
from gpu_common import ocol, rand_block

PAGE_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4097]
# (name, key types, null fraction): every key type alone, then the multi-channel keys with 10 % nulls
KEY_SPECS = [
    ("bigint", ["BIGINT"], 0.03),
    ("integer", ["INTEGER"], 0.03),
    ("date", ["DATE"], 0.03),
    ("double", ["DOUBLE"], 0.03),
    ("boolean", ["BOOLEAN"], 0.03),
    ("varchar", ["VARCHAR"], 0.03),
    ("bigint_varchar", ["BIGINT", "VARCHAR"], 0.10),
    ("integer_double_boolean", ["INTEGER", "DOUBLE", "BOOLEAN"], 0.10),
]
DOMAINS = {"small": 50, "large": 1_000_000}


def key_block(pkg, rng, type_id, n, domain, null_frac):
    """n keys drawn from `domain` values (BOOLEAN has two); DOUBLE keys carry NaN, 0.0 and -0.0"""
    if type_id == pkg.BOOLEAN:
        return rand_block(pkg, rng, type_id, n, null_frac)
    b = rand_block(pkg, rng, type_id, n, null_frac, domain=(0, domain))
    if type_id == pkg.DOUBLE:
        v = b.values.copy()
        pick = rng.random(n) < 0.15
        v[pick] = rng.choice(np.array([np.nan, 0.0, -0.0]), int(pick.sum()))
        b = pkg.Block(pkg.DOUBLE, v, b.nulls)
    return b


def multi_domain(domain, channels):
    """per-channel domain so that the product of the channels' domains is about `domain`"""
    return max(2, int(round(domain ** (1.0 / channels))))


def take(pkg, block, idx):
    if block.type == pkg.VARCHAR:
        vals = block.to_list()
        return pkg.Block(pkg.VARCHAR, [vals[i] for i in idx])
    return pkg.Block(block.type, block.values[idx], None if block.nulls is None else block.nulls[idx])


def key_pages(pkg, rng, type_names, domain, null_frac, sizes):
    """pages of the given sizes; about half of the rows of every later page repeat a row of page 0, so that whatever the domain the later
    pages meet keys the hash already holds (G0 > 0) between new ones"""
    types = [getattr(pkg, t) for t in type_names]
    d = multi_domain(domain, len(types))
    total = int(sum(sizes))
    pool = [key_block(pkg, rng, t, total, d, null_frac) for t in types]
    pages, start = [], 0
    for k, n in enumerate(sizes):
        idx = np.arange(start, start + n)
        if k > 0:
            back = rng.random(n) < 0.5
            idx[back] = rng.integers(0, sizes[0], int(back.sum()))
        pages.append(pkg.Page(*[take(pkg, b, idx) for b in pool]))
        start += n
    return types, pages


def with_hash(pkg, oracle, page, channels):
    """RowPagesBuilder(hashEnabled = true): the raw hash of the key channels appended as a BIGINT channel"""
    n = page.getPositionCount()
    h = oracle.hash_rows([ocol(oracle, page.getBlock(c)) for c in channels]) if n else np.zeros(0, dtype=np.int64)
    return page.appendColumn(pkg.Block(pkg.BIGINT, np.asarray(h, dtype=np.int64)))


def key_cols(oracle, page, channels):
    return [ocol(oracle, page.getBlock(c)) for c in channels]


def comparable(rows):
    return [tuple(("NaN",) if isinstance(v, float) and v != v else (("-0.0",) if isinstance(v, float) and v == 0 and np.signbit(v) else v) for v in r) for r in rows]


def flat_rows(page):
    return comparable(pkg_page_rows(page))


def pkg_page_rows(page):
    cols = [page.getBlock(c).flatten().to_list() for c in range(page.getChannelCount())]
    return [tuple(c[i] for c in cols) for i in range(page.getPositionCount())]


def drive_mark(op, pages):
    """one output page per input page, zero-row pages included; checks needsInput / isFinished on the way"""
    outs = []
    for p in pages:
        assert op.needsInput() and not op.isFinished()
        op.addInput(p)
        assert not op.needsInput() and not op.isFinished()
        o = op.getOutput()
        assert o is not None and op.getOutput() is None
        outs.append(o.to_host())
        o.release()
    assert op.needsInput()
    op.finish()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    return outs


def check_marks(pkg, oracle, types, channels, pages, outs):
    """outs[i] = pages[i] + the BOOLEAN marker of the helper, without a null vector"""
    o = DistinctOracle(oracle, [types[c] for c in channels])
    assert len(outs) == len(pages)
    for page, got in zip(pages, outs):
        want = o.mark(key_cols(oracle, page, channels))
        assert got.getPositionCount() == page.getPositionCount() and got.getChannelCount() == page.getChannelCount() + 1
        marker = got.getBlock(page.getChannelCount())
        assert marker.type == pkg.BOOLEAN and marker.nulls is None
        assert np.array_equal(marker.values.astype(bool), want), np.nonzero(marker.values.astype(bool) != want)[0][:10]
        head = pkg.Page(*got.blocks[:-1], position_count=got.getPositionCount())
        assert flat_rows(head) == flat_rows(page)   # the input channels pass through unchanged


def drive_distinct_limit(op, pages):
    """per page the operator takes: its output page on the host, or None; stops offering pages when needsInput turns false"""
    outs = []
    for p in pages:
        if not op.needsInput():
            break
        op.addInput(p)
        o = op.getOutput()
        assert op.getOutput() is None
        if o is None:
            outs.append(None)
        else:
            assert o.position_count > 0
            outs.append(o.to_host())
            o.release()
    return outs


def check_distinct_limit(pkg, oracle, types, channels, hash_channel, limit, pages, outs):
    """outs against DistinctLimitOperator.getOutput's loop over the helper's ids; returns the rows produced"""
    o = DistinctOracle(oracle, [types[c] for c in channels], max(1, min(limit, 10_000)))
    remaining, total, taken = limit, 0, 0
    out_channels = list(channels) + ([hash_channel] if hash_channel >= 0 else [])
    for page in pages:
        if remaining == 0:
            break
        kept, remaining = o.distinct_positions(key_cols(oracle, page, channels), remaining)
        got = outs[taken]
        taken += 1
        if not kept:
            assert got is None   # no output page for a page that contributes no row
            continue
        assert got is not None and got.getChannelCount() == len(out_channels)
        rows = pkg_page_rows(page)
        assert flat_rows(got) == comparable([tuple(rows[i][c] for c in out_channels) for i in kept])
        assert [got.getBlock(i).type for i in range(len(out_channels))] == [types[c] for c in out_channels]
        total += len(kept)
    assert taken == len(outs)
    assert total == (limit if remaining == 0 else o.hash.group_count)   # min(limit, distinct keys)
    return total

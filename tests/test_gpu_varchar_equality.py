"""VARCHAR `=` and `<>` in generated kernels (jit.cpp cmp_expr): the lengths first, then the bytes in 8- / 4-byte pieces that never leave
[a, a + len); constants are compared as immediates.  Expected values come from numpy / Python on the host."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17]
ALPHABET = b"abcdefghijklmnopqrstuvwxyz"


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def base(n):
    return bytes(ALPHABET[i % 26] for i in range(n))


def strings():
    """every length: the base string, one that differs only in its LAST byte, one that differs only in its first; equal prefixes of
    different length come from the bases themselves (base(7) is a prefix of base(8), ...)"""
    out = []
    for n in LENGTHS:
        out.append(base(n))
        if n > 0:
            out.append(base(n)[:-1] + b"#")
            out.append(b"#" + base(n)[1:])
    return out


@pytest.fixture(scope="module")
def cases():
    """(left values, right values) of equal length, None = null: every string against every string (equal, prefix, last byte, first byte)"""
    ss = strings()
    left, right = [], []
    for a in ss:
        for b in ss:
            left.append(a)
            right.append(b)
    rng = np.random.default_rng(5)
    for i in rng.integers(0, len(left), 40):
        left[int(i)] = None
    for i in rng.integers(0, len(right), 40):
        right[int(i)] = None
    return left, right


def expected(left, right, negate):
    return [None if a is None or b is None else ((a == b) != negate) for a, b in zip(left, right)]


def filter_positions(pkg, ctx, page, types, filt):
    """positions the filter keeps (a BIGINT row-number channel is projected)"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, filt, [pkg.field(len(types) - 1, pkg.BIGINT)])
    out = pkg.to_pages(fac.createOperator(), [page])
    return [int(v) for p in out for v in p.getBlock(0).values]


def project_bool(pkg, ctx, page, types, expr):
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, None, [expr])
    out = pkg.to_pages(fac.createOperator(), [page])
    return [v for p in out for v in p.getBlock(0).to_list()]


@pytest.mark.parametrize("negate", [False, True])
def test_column_against_column(pkg, ctx, cases, negate):
    left, right = cases
    n = len(left)
    V, B = pkg.VARCHAR, pkg.BIGINT
    page = pkg.Page(pkg.Block(V, left), pkg.Block(V, right), pkg.Block(B, np.arange(n, dtype=np.int64)))
    f = pkg.field
    e = f(0, V).ne(f(1, V)) if negate else f(0, V).eq(f(1, V))
    want = expected(left, right, negate)
    assert project_bool(pkg, ctx, page, [V, V, B], e) == want
    assert filter_positions(pkg, ctx, page, [V, V, B], e) == [i for i, w in enumerate(want) if w]
    assert sum(1 for w in want if w) > 10 and sum(1 for w in want if w is False) > 10


def project_all(pkg, ctx, page, types, exprs):
    """several boolean projections in ONE generated kernel (one compilation): a list of value lists"""
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, types, None, exprs)
    out = pkg.to_pages(fac.createOperator(), [page])
    return [[v for p in out for v in p.getBlock(ch).to_list()] for ch in range(len(exprs))]


@pytest.mark.parametrize("negate", [False, True])
def test_column_against_constants(pkg, ctx, cases, negate):
    left, _ = cases
    n = len(left)
    V, B = pkg.VARCHAR, pkg.BIGINT
    page = pkg.Page(pkg.Block(V, left), pkg.Block(B, np.arange(n, dtype=np.int64)))
    f = pkg.field
    # every length: the base string, and the one that differs from it in the last byte only; both operand orders
    consts = [base(k) for k in LENGTHS] + [base(k)[:-1] + b"#" for k in LENGTHS if k > 0]
    for group, flipped in ((consts[:10], False), (consts[10:], False), (consts[3:9], True)):
        exprs = []
        for k in group:
            c = pkg.constant(k.decode(), V)
            a, b = (c, f(0, V)) if flipped else (f(0, V), c)
            exprs.append(a.ne(b) if negate else a.eq(b))
        got = project_all(pkg, ctx, page, [V, B], exprs)
        for k, g in zip(group, got):
            assert g == expected(left, [k] * n, negate), k
    k = pkg.constant(base(9).decode(), V)
    assert filter_positions(pkg, ctx, page, [V, B], f(0, V).ne(k) if negate else f(0, V).eq(k)) == [i for i, w in enumerate(expected(left, [base(9)] * n, negate)) if w]


@pytest.mark.parametrize("length", [1, 3, 4, 7, 8, 9, 15, 16, 17])
def test_last_string_ends_with_the_allocation_and_regions_of_a_pool(pkg, ctx, length):
    """device blocks: the byte tensor is sized to the byte and its last string ends with it (a wide piece that reached past the string
    would leave the allocation); the second block is a region of the same pool -- its offsets do not start at 0.  The programs do not
    depend on `length` (one compilation for all cases): column against column, and against a constant of every length"""
    import torch

    V, B = pkg.VARCHAR, pkg.BIGINT
    vals = [base(5), base(length)[:-1] + b"#", base(12), base(length)]       # the pool ends with base(length)
    pool = b"".join(vals)
    offs = np.zeros(len(vals) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(v) for v in vals])
    d_pool = torch.tensor(list(pool), dtype=torch.uint8, device="cuda:0")
    assert d_pool.numel() == len(pool) and d_pool.untyped_storage().nbytes() == len(pool)
    d_offs = torch.tensor(offs, dtype=torch.int32, device="cuda:0")
    d_rows = torch.arange(len(vals), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    f = pkg.field
    exprs = [f(0, V).eq(f(1, V)), f(0, V).ne(f(1, V))] + [f(0, V).eq(pkg.constant(base(k).decode(), V)) for k in LENGTHS]
    for first in (0, 2):     # the whole pool; the region [2, 4): offsets[0] > 0
        n = len(vals) - first
        page = pkg.Page(pkg.DeviceBlock(V, n, d_pool, None, d_offs.data_ptr() + 4 * first), pkg.DeviceBlock(V, n, d_pool, None, d_offs.data_ptr() + 4 * first),
                        pkg.DeviceBlock(B, n, d_rows.data_ptr() + 8 * first))
        sub = vals[first:]
        got = project_all(pkg, ctx, page, [V, V, B], exprs)
        assert got[0] == [True] * n and got[1] == [False] * n
        for k, g in zip(LENGTHS, got[2:]):
            assert g == [v == base(k) for v in sub], k
        assert filter_positions(pkg, ctx, page, [V, V, B], f(0, V).eq(f(1, V))) == [first + i for i in range(n)]
    ctx.synchronize()

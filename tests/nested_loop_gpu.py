"""Shared by the GPU tests of the nested loop join: pages from rows, the build / probe drivers, and the model's expected output taken through
INDEX pages -- the model (nested_loop_expected.py) joins pages whose only channel is the row number, and the expected columns are the inputs
gathered by those numbers, so a product of tens of thousands of rows is compared column by column.  Importing this needs no GPU."""
import expr_fuzz as F
import nested_loop_expected as NL

B, I, DT, D, BO, V = F.BIGINT, F.INTEGER, F.DATE, F.DOUBLE, F.BOOLEAN, F.VARCHAR
SIX = (B, I, DT, D, BO, V)
STRINGS = ["", "a", "é漢", "0123456789abcdef", "0123456789abcdefg", "x" * 37, "\U0001F600z", "ab"]
LARGE = (1, 2, 63, 64, 65, 255, 256, 257, 1025)   # a wave, a 256-lane tile and four of them, each less one, exact, and plus one
SMALL = (1, 2, 3, 64, 65)                         # ... and the strip of small rows one wave evaluates (32) is crossed by 64 and 65


def value(t, i, salt=0):
    k = i * 7 + salt
    if t == B:
        return (k * 1_000_003) % 2001 - 1000 + (2**40 if k % 5 == 0 else 0)
    if t in (I, DT):
        return (k * 31) % 401 - 200
    if t == D:
        return [float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 1.5, -2.25, 1e300][k % 8] if k % 3 == 0 else (k % 97) / 4.0 - 10.0
    if t == BO:
        return k % 3 == 0
    return STRINGS[k % len(STRINGS)] + (str(k) if k % 4 == 1 else "")


def column(t, n, nulls="some", salt=0):
    """nulls: "none", "some" (every fifth row, shifted by the salt) or "all" """
    return [None if nulls == "all" or (nulls == "some" and (i + salt) % 5 == 2) else value(t, i, salt) for i in range(n)]


def columns(types, n, nulls="some", salt=0):
    return [column(t, n, nulls, salt + 3 * c) for c, t in enumerate(types)]


def page_of(pkg, types, cols, n=None):
    if not types:
        return pkg.Page(position_count=n)
    return pkg.Page(*[pkg.Block(t, list(c)) for t, c in zip(types, cols)])


def build(pkg, ctx, types, pages, operator_id=1):
    """-> (build factory, build operator) with the pages added and finish() called"""
    bf = pkg.NestedLoopBuildOperatorFactory(ctx, operator_id, types)
    bop = bf.createOperator()
    for pg in pages:
        assert bop.needsInput()
        bop.addInput(pg)
        assert bop.getOutput() is None
    bop.finish()
    return bf, bop


def end(bf, bop, *probe_factories):
    """the probe operators are closed: the probe factories see noMoreOperators, which lets the build operator finish (without a probe
    factory nothing ever does, as for the hash builder: the operator is closed as it stands)"""
    for jf in probe_factories:
        jf.noMoreOperators()
    if probe_factories:
        assert bop.isFinished() and not bop.isBlocked()
    else:
        assert bop.isBlocked() and not bop.isFinished()
    bop.close()
    for jf in probe_factories:
        jf.close()
    bf.bridge.close()
    bf.close()


def bits_columns(types, pages):
    """the output pages' columns, cell by cell as expr_fuzz.bits"""
    out = [[] for _ in types]
    for pg in pages:
        for c, t in enumerate(types):
            out[c] += [F.bits(t, v) for v in pg.getBlock(c).to_list()]
    return out


def index_pairs(probe_sizes, build_sizes, probe_channels, build_channels, build_has_channels=True):
    """the model over index pages: (probe page, probe row, build page, build row) per output row, None for a side without output channels"""
    probe_pages = [[((k, i),) for i in range(n)] for k, n in enumerate(probe_sizes)]
    build_pages = [[((k, i),) for i in range(n)] for k, n in enumerate(build_sizes)] if build_has_channels else list(build_sizes)
    rows = NL.reference_rows(probe_pages, build_pages, [0] if probe_channels else [], [0] if build_channels else [])
    at = 1 if probe_channels else 0
    return [(r[0] if probe_channels else None, r[at] if build_channels else None) for r in rows]


def expected_columns(probe_types, probe_cols, build_types, build_cols, probe_channels, build_channels, pairs):
    """probe_cols / build_cols: per page, the page's columns"""
    out = []
    for ch in probe_channels:
        out.append([F.bits(probe_types[ch], probe_cols[k][ch][i]) for (k, i), _ in pairs])
    for ch in build_channels:
        out.append([F.bits(build_types[ch], build_cols[k][ch][i]) for _, (k, i) in pairs])
    return out

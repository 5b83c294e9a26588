"""Which error a page raises when more than one of its cells fails: the reference throws at the first failing node it
evaluates -- inside a row the first evaluated one, over a page the filter before the projections, then the lowest projection index, then
its first failing row (PageProcessor.java:313-338).  A generated kernel evaluates all of that at once and keeps one error word per page.

Hand-built cases on 16-row pages; the expectation is expr_fuzz.run_program's and is also written out next to every case.  Every
expression reads ONE column x, whose low bits say what fails on a row: bit 0 `7 / (x % 2 - 1)` divides by zero (DIVISION_BY_ZERO), bit 1
`(x / 2 % 2) * 2^62 * 4` overflows (NUMERIC_VALUE_OUT_OF_RANGE), bit 2 CAST(IF(x / 4 % 2 = 1, NaN, 1.5) AS BIGINT) is an
INVALID_CAST_ARGUMENT.  So every case runs down three paths: the flat page, x as a DictionaryBlock (the dictionary-aware path: the
expressions over the entries, among them one that fails everything and that no row refers to, and the fallback when an entry raises) and
the fused aggregation, where the projections are the aggregates' inputs."""
import pytest

import expr_fuzz as F
import expr_harness as H
from expr_fuzz import BIGINT, BOOLEAN, DOUBLE, INTEGER, Failure

pytestmark = pytest.mark.gpu
N = 16
K, X = ("in", 0, BIGINT), ("in", 1, BIGINT)       # channel 0: the aggregation's group key (row % 4), read by no expression
TYPES = (BIGINT, BIGINT)
DIV0, RANGE, BADCAST = F.DIV0, F.RANGE, F.BADCAST
PATHS = ["flat", "dictionary", "aggregation"]


def c(v, t=BIGINT):
    return ("const", v, t)


def call(name, t, *args):
    return ("call", name, t, tuple(args))


def sf(form, t, *args):
    return ("sf", form, t, tuple(args), None)


def bit(k):
    """bit k of x as 0 / 1"""
    return call("MODULUS", BIGINT, call("DIVIDE", BIGINT, X, c(2**k)), c(2))


DIV = call("DIVIDE", BIGINT, c(7), call("SUBTRACT", BIGINT, bit(0), c(1)))                                       # -7, fails where bit 0 is set
MUL = call("MULTIPLY", BIGINT, call("MULTIPLY", BIGINT, bit(1), c(2**62)), c(4))                                 # 0, fails where bit 1 is set
CAST = call("CAST", BIGINT, sf("IF", DOUBLE, call("EQUAL", BOOLEAN, bit(2), c(1)), c(float("nan"), DOUBLE), c(1.5, DOUBLE)))   # 2, fails where bit 2 is set
CODE = {id(DIV): DIV0, id(MUL): RANGE, id(CAST): BADCAST}


def page(zero=(), big=(), nan=()):
    return [(BIGINT, [i % 4 for i in range(N)]), (BIGINT, [(i in zero) + 2 * (i in big) + 4 * (i in nan) for i in range(N)])]


def gt(x):
    return call("GREATER_THAN", BOOLEAN, x, c(-100))


@pytest.fixture(scope="module")
def ctx(pkg):
    cx = pkg.Context(0)
    yield cx
    cx.close()


def run(pkg, ctx, path, filt, projs, pg):
    """-> (what the library gives, what run_program gives), both as Failure(code, position, None) or the value columns.  The aggregation
    raises its code without a position, and gives no columns to compare: (Failure(code, None, None) or None, the same of run_program)"""
    prog = F.Program("case", TYPES, filt, tuple(projs))
    want = F.run_program(prog, pg)
    blocks = [pkg.Block(t, vals) for t, vals in pg]
    if path == "dictionary":
        entries = sorted(set(pg[1][1]) | {7}) + [None]           # 7 fails everything; on most pages no row refers to it, and none to the NULL
        assert len(entries) * 2 <= N                             # or the operator would not try the dictionary
        blocks[1] = pkg.DictionaryBlock(pkg.Block(BIGINT, entries), [entries.index(v) for v in pg[1][1]])
    if path == "aggregation":
        aggs = [(pkg.SUM_BIGINT if F.type_of(p) == BIGINT else pkg.COUNT_COLUMN, k) for k, p in enumerate(projs, 1)] + [(pkg.COUNT_ALL, -1)]
        prog = F.Program("case", TYPES, filt, (K,) + tuple(projs))
        fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 0, *F.lower(prog, pkg.expressions), [BIGINT], [0], aggs)
    else:
        fac = pkg.FilterAndProjectOperatorFactory(ctx, 0, *F.lower(prog, pkg.expressions))
    op = fac.createOperator()
    outs, err = H.drive_pages(pkg, op, [pkg.Page(*blocks)])
    op.close()
    fac.close()
    if path == "aggregation":
        return (None if err is None else Failure(err[0].code, None, None)), (Failure(want.code, None, None) if isinstance(want, Failure) else None)
    if err is not None:
        got = Failure(err[0].code, err[2], None)
    else:
        got = [[v for o in outs for v in o.getBlock(k).to_list()] for k in range(len(projs))]
    return got, Failure(want.code, want.position, None) if isinstance(want, Failure) else want.columns


def expect(path, code, position):
    """the literal expectation of a case"""
    return Failure(code, None if path == "aggregation" else position, None)


# ---- (a) one row, one expression: the first EVALUATED failure, not the smaller code ----------------------------------------------
def forms(first, second):
    """every form in which `first` fails, becomes NULL, and `second` is evaluated after it all the same"""
    return {
        "and": sf("AND", BOOLEAN, gt(first), gt(second)),
        "or": sf("OR", BOOLEAN, gt(first), gt(second)),
        "if_condition": sf("IF", BIGINT, gt(first), c(1), second),
        "coalesce": sf("COALESCE", BIGINT, first, second),
        "between_low": sf("BETWEEN", BOOLEAN, X, first, second),
        "between_high": sf("BETWEEN", BOOLEAN, first, c(-100), second),
        "is_null_and": sf("AND", BOOLEAN, sf("IS_NULL", BOOLEAN, first), gt(second)),
        "binary_call": call("ADD", BIGINT, first, second),      # the left argument is NULL: the right one is not evaluated at all
    }


# every pair both ways round: where the kept error is the minimum over the codes, one of the two orders agrees by accident
PAIRS = {"div0_then_overflow": (DIV, MUL), "overflow_then_div0": (MUL, DIV), "cast_then_overflow": (CAST, MUL), "overflow_then_cast": (MUL, CAST),
         "div0_then_cast": (DIV, CAST), "cast_then_div0": (CAST, DIV)}
FORM_NAMES = sorted(forms(DIV, MUL))
PLACES = [("projection", p) for p in sorted(PAIRS)] + [("filter", "div0_then_overflow"), ("filter", "overflow_then_div0")]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("where,pair", PLACES, ids=["%s-%s" % p for p in PLACES])
@pytest.mark.parametrize("form", FORM_NAMES)
def test_first_evaluated_failure_of_a_row(pkg, ctx, form, where, pair, path):
    first, second = PAIRS[pair]
    tree = forms(first, second)[form]
    pg = page(zero={5}, big={5}, nan={5})                     # both operands fail on row 5 and nowhere else
    if where == "filter":
        got, want = run(pkg, ctx, path, tree if tree[2] == BOOLEAN else sf("IS_NULL", BOOLEAN, tree), [X], pg)
    else:
        got, want = run(pkg, ctx, path, None, [X, tree], pg)
    assert want == expect(path, CODE[id(first)], 5)              # stated literally: the code of the operand evaluated first, row 5
    assert got == want, (path, where, form, pair, got)


# ---- (b), (c) several projections: the lowest projection index, then its first failing row -----------------------------------------
PROJECTION_CASES = {
    # name: (projections, page, the expected code and row)
    "p0_overflows_row9_p1_div0_row2": ([MUL, DIV], page(big={9}, zero={2}), (RANGE, 9)),
    "p0_div0_row9_p1_overflows_row2": ([DIV, MUL], page(zero={9}, big={2}), (DIV0, 9)),
    "p0_cast_row9_p1_overflows_row2": ([CAST, MUL], page(nan={9}, big={2}), (BADCAST, 9)),
    "three_projections": ([X, DIV, MUL, CAST], page(zero={9}, big={2}, nan={0}), (DIV0, 9)),
    "clean_p0_then_two_rows_in_p1": ([X, MUL, DIV], page(big={9, 12}, zero={2}), (RANGE, 9)),
    "same_row_div0_first": ([DIV, MUL], page(zero={4}, big={4}), (DIV0, 4)),
    "same_row_overflow_first": ([MUL, DIV], page(zero={4}, big={4}), (RANGE, 4)),
    "same_row_cast_first": ([CAST, MUL, DIV], page(zero={4}, big={4}, nan={4}), (BADCAST, 4)),
}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(PROJECTION_CASES))
def test_lowest_projection_then_first_row(pkg, ctx, name, path):
    projs, pg, literal = PROJECTION_CASES[name]
    got, want = run(pkg, ctx, path, None, projs, pg)
    assert want == expect(path, *literal)
    assert got == want, (path, name, got)


# ---- the filter --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_filter_first_failing_row(pkg, ctx, path):
    filt = sf("AND", BOOLEAN, gt(DIV), gt(MUL))
    got, want = run(pkg, ctx, path, filt, [X], page(big={3}, zero={5}))
    assert want == expect(path, RANGE, 3) and got == want, got            # row 3 overflows before row 5 divides by zero
    got, want = run(pkg, ctx, path, filt, [X], page(big={5}, zero={3}))
    assert want == expect(path, DIV0, 3) and got == want, got


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("failing", ["overflow", "div0", "cast"])
def test_filter_error_wins_over_projection_errors(pkg, ctx, failing, path):
    in_filter, in_proj, pg = {"overflow": (MUL, DIV, page(big={9}, zero={2})), "div0": (DIV, MUL, page(zero={9}, big={2})),
                              "cast": (CAST, MUL, page(nan={9}, big={2}))}[failing]
    got, want = run(pkg, ctx, path, gt(in_filter), [X, in_proj], pg)
    assert want == expect(path, CODE[id(in_filter)], 9)                      # the filter's row 9, though the projection fails on row 2
    assert got == want, got


@pytest.mark.parametrize("path", ["flat", "dictionary"])
def test_projection_error_on_a_rejected_row_is_not_raised(pkg, ctx, path):
    """row 5 fails in every projection and is the one row the filter rejects"""
    to_int = call("CAST", INTEGER, call("MULTIPLY", BIGINT, bit(1), c(2**40)))          # 2^40 is no INTEGER
    d_int = call("CAST", INTEGER, CAST[3][0])                                           # NaN is no INTEGER either
    neg = call("NEGATE", BIGINT, call("MULTIPLY", BIGINT, bit(1), c(F.I64_MIN)))        # -(-2^63)
    mod = call("MODULUS", BIGINT, c(7), call("SUBTRACT", BIGINT, bit(0), c(1)))
    filt = call("NOT_EQUAL", BOOLEAN, X, c(7))
    pg = page(zero={5}, big={5}, nan={5})
    got, want = run(pkg, ctx, path, filt, [X, DIV, MUL, CAST, to_int, d_int, neg, mod], pg)
    assert want == [[0] * 15, [-7] * 15, [0] * 15, [2] * 15, [0] * 15, [2] * 15, [0] * 15, [0] * 15]
    assert got == want
    # ... and with the filter gone every one of them is raised, the first projection's first
    got, want = run(pkg, ctx, path, None, [X, to_int, d_int, neg], pg)
    assert want == Failure(RANGE, 5, None) and got == want, got
    got, want = run(pkg, ctx, path, None, [X, d_int, to_int], pg)
    assert want == Failure(BADCAST, 5, None) and got == want, got


def test_dictionary_entry_that_no_row_refers_to_raises_nothing(pkg, ctx):
    """the dictionary holds 7, which fails every expression; the page's rows are all 0"""
    got, want = run(pkg, ctx, "dictionary", gt(DIV), [X, MUL, CAST, sf("COALESCE", BIGINT, DIV, MUL)], page())
    assert want == [[0] * N, [0] * N, [2] * N, [-7] * N] and got == want, got

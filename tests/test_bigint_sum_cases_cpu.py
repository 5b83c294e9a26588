"""The yardstick of the sum(bigint) tests (tests/bigint_sum_cases.py): the Python-int reference against a second formulation and against
the C oracle's row-order Math.addExact, the families against models of plausible kernel bugs, and the fixed positions of the special rows
against the page cuts and waves the GPU file (tests/test_gpu_bigint_sums.py) uses."""
from fractions import Fraction

import numpy as np
import pytest

from agg_paths import FUSED_GENERAL, ORDERED_PATHS, PARTIAL_FINAL_MANY, PATHS, page_sizes
from bigint_sum_cases import (FAMILIES, FILTER_BELOW, HIGH_WORD_TOTALS, INT64_MAX, INT64_MIN, RAISES, TRANSIENT_FREE, VARIANTS, WRONG_MODELS, heavy_group,
                              make_stream, narrow, past_limit_groups, reference)

CASES = [(name, variant) for name in FAMILIES for variant in VARIANTS[name]]
N = 31_000
CUTS = (12_000, 15_000)


def stream(name, variant, ngroups, n=N, cuts=CUTS, with_filter=True, seed=0):
    rng = np.random.default_rng(800 + 10 * FAMILIES.index(name) + ngroups + seed)
    return make_stream(name, rng, ngroups, n, with_filter=with_filter, variant=variant, cuts=cuts)


def selections(s):
    """(values, rows that count) of sum(big), sum(big, mask), sum(big_nullable)"""
    keep = s.filt < FILTER_BELOW
    return (s.big, keep), (s.big, keep & (s.mask != 0)), (s.big_nullable, keep & (s.big_nulls == 0))


def test_narrow_at_the_edges():
    assert narrow(INT64_MAX) == INT64_MAX and narrow(INT64_MIN) == INT64_MIN and narrow(0) == 0
    assert narrow(INT64_MAX + 1) == RAISES and narrow(INT64_MIN - 1) == RAISES and all(narrow(t) == RAISES for t in HIGH_WORD_TOTALS)


@pytest.mark.parametrize("name,variant", CASES)
@pytest.mark.parametrize("ngroups", [1, 3, 7])
def test_reference_equals_a_second_formulation(name, variant, ngroups):
    """the same totals from the rows in reverse order, as fractions of 2^32-scaled halves: sum = 2^32 x sum(v >> 32) + sum(v & 0xffffffff)"""
    s = stream(name, variant, ngroups)
    ref = reference(s, ngroups)
    for (vals, keep), want, cnt in zip(selections(s), (ref.sums, ref.sums_masked, ref.sums_nullable), (ref.count_all, ref.count_masked, ref.count_nullable)):
        for g in range(ngroups):
            v = vals[keep & (s.gids == g)][::-1].tolist()
            hi = sum(x >> 32 for x in v)
            lo = Fraction(sum(x & 0xFFFFFFFF for x in v), 2**32)
            assert (hi + lo) * 2**32 == want[g] and len(v) == cnt[g], (name, g)
    keep = s.filt < FILTER_BELOW
    assert ref.mins == [int(s.big[keep & (s.gids == g)].min()) for g in range(ngroups)]


@pytest.mark.parametrize("name,variant", CASES)
@pytest.mark.parametrize("ngroups", [1, 3, 7])
def test_families_are_what_they_say(name, variant, ngroups):
    s = stream(name, variant, ngroups)
    ref = reference(s, ngroups)
    spec = s.big[s.special]
    assert s.special.any() and not (s.big_nulls[s.special].any() or (s.mask[s.special] == 0).any() or (s.filt[s.special] >= FILTER_BELOW).any())
    noise = s.big[~s.special & (s.mask != 0) & (s.filt < FILTER_BELOW)]
    assert np.abs(noise).max() <= 1000
    if name in ("extremes_cancel", "carry_every_row", "high_halves"):
        assert all(abs(t) < 2**44 for t in ref.sums + ref.sums_masked + ref.sums_nullable)
    if name == "extremes_cancel":
        assert {INT64_MAX, INT64_MIN, -INT64_MAX, 2**62, -(2**62)} <= set(spec.tolist())
    if name == "same_sign_near_limit":
        assert all(2**62 <= abs(t) < 2**63 for t in ref.sums + ref.sums_masked + ref.sums_nullable)
        assert ngroups == 1 or {t > 0 for t in ref.sums} == {True, False}
    if name == "total_at_limit":
        assert set(ref.sums) <= {INT64_MAX, INT64_MIN} and (ngroups == 1 or len(set(ref.sums)) == 2) and not ref.raises()
    if name == "total_past_limit":
        over, under = past_limit_groups(ngroups, variant)
        edge = 0 if variant == "excluded" else 1
        assert over is None or ref.sums[over] == INT64_MAX + edge
        assert under is None or ref.sums[under] == INT64_MIN - edge
        assert all(abs(ref.sums[g]) < 2**40 for g in range(ngroups) if g not in (over, under))
        assert ref.raises() == (variant != "excluded")
        if variant == "excluded":       # all three sums sit at the limit, and one more row of any excluded kind would cross it
            for g, lim in ((over, INT64_MAX), (under, INT64_MIN)):
                if g is None:
                    continue
                assert ref.sums_masked[g] == ref.sums_nullable[g] == lim
                rows = s.gids == g
                push = (lambda a: a > 0) if lim > 0 else (lambda a: a < 0)
                assert push(s.big_nullable[rows & (s.big_nulls != 0)]).all() and (s.big_nulls[rows] != 0).any()
                assert push(s.big[rows & (s.filt >= FILTER_BELOW)]).all() and (s.filt[rows] >= FILTER_BELOW).any()
                assert push(s.big[rows & (s.mask == 0) & (s.filt < FILTER_BELOW)]).any()
    if name == "high_word_only":
        assert set(ref.sums) <= set(HIGH_WORD_TOTALS) and all(narrow(t) == RAISES for t in ref.sums + ref.sums_masked + ref.sums_nullable)
        assert all(-(2**63) <= (t + 2**63) % 2**64 - 2**63 < 2**63 for t in ref.sums)
    if name == "high_halves":
        assert ((spec & 0xFFFFFFFF) == 0xFFFFFFFF).all() and (np.abs(spec >> 32) >= 2**28).all() and (spec > 0).any() and (spec < 0).any()
        assert all((s.special & (s.gids == g)).sum() >= 2000 for g in range(ngroups))
    if name == "carry_every_row":
        for g in range(ngroups):
            v = s.big[s.special & (s.gids == g)].tolist()
            assert all((a % 2**64) + (b % 2**64) == 2**64 and a < 0 < b for a, b in zip(v[0::2], v[1::2]))


def prefix_leaves_int64(vals):
    t = 0
    for v in vals:
        t += v
        if not INT64_MIN <= t <= INT64_MAX:
            return True
    return False


@pytest.mark.parametrize("name,variant", CASES)
@pytest.mark.parametrize("ngroups", [1, 3, 7])
def test_oracle_row_order_sum_against_the_reference(oracle, name, variant, ngroups):
    """The reference's accumulator is a long and Math.addExact in row order (oracle.agg_long_sum).  On a transient-free family it
    returns the reference's counts and sums, or raises -2 exactly where a total leaves int64.  On the others (extremes_cancel,
    high_halves) a prefix leaves int64 on the way to a small total: the oracle raises -2, the product returns the total -- "the reference
    also raises on a transient prefix overflow that a reordered sum cannot see" (DESIGN.md).  Both sides are pinned here."""
    s = stream(name, variant, ngroups)
    ref = reference(s, ngroups)
    for (vals, keep), want, cnt in zip(selections(s), (ref.sums, ref.sums_masked, ref.sums_nullable), (ref.count_all, ref.count_masked, ref.count_nullable)):
        transient = any(prefix_leaves_int64(vals[keep & (s.gids == g)].tolist()) for g in range(ngroups))
        expect_raise = any(narrow(t) == RAISES for t in want)
        assert TRANSIENT_FREE[name] == (transient == expect_raise), name
        if TRANSIENT_FREE[name] and not expect_raise:
            c, got = oracle.agg_long_sum(s.gids[keep], vals[keep], ngroups)
            assert list(c) == cnt and [int(x) for x in got] == want
        else:
            assert transient
            with pytest.raises(oracle.OracleError) as e:
                oracle.agg_long_sum(s.gids[keep], vals[keep], ngroups)
            assert e.value.code == -2
            if not TRANSIENT_FREE[name]:
                assert not expect_raise and all(narrow(t) == t for t in want)


# a family that cannot tell a model from the truth, by construction:
#   no total leaves int64 and the high word of every total is the low word's sign: nothing for an evaluate that skips the check to miss;
#   same-sign totals inside int64, prefixes monotone: saturation never clips, and at the limit it clips to the right value;
#   totals far outside int64 (high_word_only): float64 is wrong by rounding only, an unsigned reading only by more, and still outside
CANNOT_SEPARATE = {
    ("extremes_cancel", "wrap_no_raise"), ("extremes_cancel", "ignore_high_word"), ("extremes_cancel", "high_word_any_sign"),
    ("high_halves", "wrap_no_raise"), ("high_halves", "ignore_high_word"), ("high_halves", "high_word_any_sign"),
    ("carry_every_row", "wrap_no_raise"), ("carry_every_row", "ignore_high_word"), ("carry_every_row", "high_word_any_sign"),
    ("carry_every_row", "saturate"),
    ("same_sign_near_limit", "wrap_no_raise"), ("same_sign_near_limit", "ignore_high_word"), ("same_sign_near_limit", "high_word_any_sign"),
    ("same_sign_near_limit", "saturate"),
    ("total_at_limit", "wrap_no_raise"), ("total_at_limit", "ignore_high_word"), ("total_at_limit", "high_word_any_sign"), ("total_at_limit", "saturate"),
    ("high_word_only", "float64"), ("high_word_only", "addend_unsigned"), ("high_word_only", "high_half_unsigned"),
}


def separated(name, model):
    """a group of some variant / group count whose expected result differs from the model's: another value, or raise against no raise"""
    for variant in VARIANTS[name]:
        for ngroups in (3, 7):
            s = stream(name, variant, ngroups)
            ref = reference(s, ngroups)
            for (vals, keep), want in zip(selections(s), (ref.sums, ref.sums_masked, ref.sums_nullable)):
                for g in range(ngroups):
                    if WRONG_MODELS[model](vals[keep & (s.gids == g)].tolist()) != narrow(want[g]):
                        return True
    return False


@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_tells_the_wrong_models_apart(name):
    for model in WRONG_MODELS:
        assert separated(name, model) != ((name, model) in CANNOT_SEPARATE), (name, model)


@pytest.mark.parametrize("model", WRONG_MODELS)
def test_every_wrong_model_is_caught_by_two_families(model):
    assert sum((name, model) not in CANNOT_SEPARATE for name in FAMILIES) >= 2


def test_wrong_models_on_hand_computed_cases():
    m = WRONG_MODELS
    assert m["wrap_no_raise"]([INT64_MAX, 1]) == INT64_MIN and m["ignore_high_word"]([INT64_MAX, INT64_MAX, 2]) == 0
    assert m["high_word_any_sign"]([INT64_MAX, 1]) == INT64_MIN and m["high_word_any_sign"]([INT64_MAX, INT64_MAX, 2]) == RAISES
    assert m["drop_carry_in_fold"]([-1, 1]) == RAISES and m["drop_carry_in_fold"]([5, 6, 7, 8, 9]) == 35
    assert m["addend_unsigned"]([-1, 1]) == RAISES and m["addend_unsigned"]([3, 4]) == 7
    assert m["high_half_unsigned"]([-1, 1]) == RAISES and m["high_half_unsigned"]([2**40, 5]) == 2**40 + 5
    assert m["float64"]([2**53, 1]) == 2**53 and m["float64"]([INT64_MAX]) == RAISES
    assert m["saturate"]([INT64_MAX, 5, -5]) == INT64_MAX - 5
    for f in m.values():
        assert f([1, 2, 3]) == 6


@pytest.mark.parametrize("name,variant", CASES)
@pytest.mark.parametrize("path", PATHS + (FUSED_GENERAL, PARTIAL_FINAL_MANY) + ORDERED_PATHS)
def test_special_rows_cover_waves_and_page_cuts(name, variant, path):
    """the special rows of every family fall into at least 3 of the 4 waves of a 256-thread block, and into the last block before and the
    first block after every page cut of every path of the GPU file"""
    sizes = page_sizes(path)
    cuts = np.cumsum(sizes)[:-1].tolist()
    ngroups = 20_000 if "many" in path or "handoff" in path else 3
    s = make_stream(name, np.random.default_rng(41), ngroups, sum(sizes), with_filter=path.startswith("fused"), variant=variant, cuts=cuts,
                    heavy=heavy_group(name, ngroups, variant) if path.endswith("handoff") else None)
    rows = np.nonzero(s.special)[0]
    starts = np.concatenate([[0], cuts]).astype(np.int64)
    in_page = rows - starts[np.searchsorted(starts, rows, side="right") - 1]      # (a kernel maps a page's rows to lanes from the page's start)
    assert len(set(((in_page % 256) // 64).tolist())) >= 3
    for c in cuts:
        assert ((rows >= c - 256) & (rows < c)).any() and ((rows >= c) & (rows < c + 256)).any(), (path, c)
    if path.endswith("handoff"):
        heavy = heavy_group(name, ngroups, variant)
        at = 0
        for m in sizes:      # the heavy group: more than kOrdHandoffRows selected rows in each page, special rows in the walked part and in the tail
            z = np.nonzero((s.gids[at:at + m] == heavy) & (s.filt[at:at + m] < FILTER_BELOW))[0]
            assert len(z) > 4096 + 256 and s.special[at:at + m][z[:4096]].any() and s.special[at:at + m][z[4096:]].any()
            at += m


@pytest.mark.parametrize("name", ["extremes_cancel", "high_halves"])
def test_spilled_runs_carry_a_high_word(name):
    """the revokes of the spilled path fall at the page cuts: the first run's state of some group is a total outside int64 -- a high
    word that is neither 0 nor ~0 -- while the final total is small"""
    for ngroups in (1, 3, 6):
        s = stream(name, None, ngroups, with_filter=False)
        run = reference(s, ngroups, rows=np.arange(0, CUTS[0]))
        assert any((t >> 64) not in (0, -1) for t in run.sums)
        assert not reference(s, ngroups).raises()


def test_partial_final_splits_of_both_kinds():
    """PARTIAL narrows its own total: with the GPU file's split (the first page | the rest) total_past_limit has every partial in range
    and their sum outside -- FINAL raises; extremes_cancel has a partial outside although the total is small -- that partial raises"""
    rows = (np.arange(0, CUTS[0]), np.arange(CUTS[0], N))
    for ngroups in (1, 3, 6):
        for variant in ("first", "middle", "last"):
            s = stream("total_past_limit", variant, ngroups, with_filter=False)
            assert not any(reference(s, ngroups, rows=r).raises() for r in rows) and reference(s, ngroups).raises()
        s = stream("extremes_cancel", None, ngroups, with_filter=False)
        assert reference(s, ngroups, rows=rows[0]).raises() and not reference(s, ngroups).raises()

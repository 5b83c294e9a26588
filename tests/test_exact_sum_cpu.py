"""The exact DOUBLE-sum yardstick: tests/exact_sum.py on hand-computed cases and against math.fsum, and the oracle's Shewchuk sum
(oracle.agg_double_sum_exact) against it on every adversarial family -- intermediate overflow included."""
import math

import numpy as np
import pytest

from exact_sum import DBL_MAX, FAMILIES, TINY, bits_equal, exact_double_sum, family, make_stream


def one(values):
    return exact_double_sum(np.array(values, dtype=np.float64), None, 1)[1][0]


@pytest.mark.parametrize("values,want", [
    ([1.0, 2.0**-53], 1.0),                                   # a tie: to even
    ([1.0, 2.0**-53, TINY], 1.0 + 2.0**-52),                  # just above the tie
    ([1.0 + 2.0**-52, 2.0**-53], 1.0 + 2.0**-51),             # a tie from an odd mantissa: up
    ([DBL_MAX, 2.0**970], math.inf),                          # a tie above DBL_MAX: even = overflow
    ([DBL_MAX, 2.0**970 - 2.0**918], DBL_MAX),
    ([DBL_MAX, 2.0**970, -TINY], DBL_MAX),
    ([-DBL_MAX, -(2.0**970)], -math.inf),
    ([1e308, 1e308, -1e308], 1e308),
    ([0.1, -0.1], 0.0),
    ([-0.0], 0.0),
    ([-0.0, -0.0, -0.0], 0.0),
    ([-(2.0**-1022), 2.0**-1023, TINY], -(2.0**-1023) + TINY),
    ([-3 * TINY], -3 * TINY),
    ([2.0**-1023, 2.0**-1023], 2.0**-1022),
    ([2.0**1000, TINY, -(2.0**1000)], TINY),
    ([2.0**53, 1.0, 2.0**-60, -(2.0**53), -1.0], 2.0**-60),
    ([math.inf, 1.0], math.inf),
    ([-math.inf, DBL_MAX, DBL_MAX], -math.inf),
    ([math.inf, -math.inf], math.nan),
    ([math.nan, 1.0], math.nan),
    ([math.inf, math.nan], math.nan),
])
def test_reference_on_hand_computed_cases(values, want):
    assert bits_equal(one(values), want), (values, one(values), want)


def test_reference_groups_nulls_and_mask():
    v = np.array([1.0, 2.0**-53, 5.0, -0.0, 7.0, 2.0**-53])
    gids = np.array([0, 0, 1, 2, 1, 0])
    nulls = np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8)
    mask = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)
    counts, sums = exact_double_sum(v, gids, 3, nulls=nulls, mask=mask)
    assert list(counts) == [2, 1, 1]
    assert bits_equal(sums, [1.0, 5.0, 0.0])
    counts, sums = exact_double_sum(v, gids, 3)
    assert list(counts) == [3, 2, 1] and bits_equal(sums, [1.0 + 2.0**-52, 12.0, 0.0])


def test_bits_equal_tells_the_zeros_apart():
    assert bits_equal([0.0, math.nan], [0.0, -math.nan])
    assert not bits_equal([0.0], [-0.0])
    assert not bits_equal([1.0], [1.0 + 2.0**-52])


@pytest.mark.parametrize("seed", range(4))
def test_reference_equals_fsum_on_random_data(seed):
    rng = np.random.default_rng(900 + seed)
    checked = 0
    for _ in range(200):
        n = int(rng.integers(1, 60))
        v = rng.standard_normal(n) * 2.0 ** rng.integers(-1074, 1000, n).astype(np.float64)
        v[rng.random(n) < 0.2] *= -1
        if rng.random() < 0.3:
            v = np.concatenate([v, -v[: n // 2]])
        try:
            want = math.fsum(v.tolist())
        except OverflowError:
            continue
        want = want + 0.0   # (fsum keeps a -0.0; the sum of a group starts from +0.0)
        assert bits_equal(one(v), want), v
        checked += 1
    assert checked > 150


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("ngroups", [1, 3, 7])
def test_oracle_exact_sum_equals_the_reference_on_every_family(oracle, name, ngroups):
    rng = np.random.default_rng(700 + ngroups * 10 + FAMILIES.index(name))
    gids, vals, nulls, mask, _, _ = make_stream(name, rng, ngroups, 30_000)
    for nl, mk in ((None, None), (nulls, mask)):
        want_c, want = exact_double_sum(vals, gids, ngroups, nulls=nl, mask=mk)
        got_c, got = oracle.agg_double_sum_exact(gids, vals, ngroups, nulls=nl, mask=mk)
        assert list(got_c) == list(want_c)
        assert bits_equal(got, want), (name, got, want)


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_exact_sum_on_each_cluster_alone(oracle, name):
    """every cluster of a family as a group of its own: the smallest inputs, in the given order and reversed"""
    rng = np.random.default_rng(77)
    for g in range(8):
        for cl in family(name, rng, g)[0]:
            for vals in (cl, cl[::-1]):
                v = np.array(vals, dtype=np.float64)
                _, got = oracle.agg_double_sum_exact(np.zeros(len(v), dtype=np.int64), v, 1)
                assert bits_equal(got, [one(v)]), (name, vals, got)


def test_oracle_exact_sum_intermediate_overflow(oracle):
    for vals, want in (([1e308, 1e308, -1e308], 1e308), ([DBL_MAX, 2.0**970], math.inf), ([DBL_MAX, 2.0**970, -TINY], DBL_MAX),
                       ([-DBL_MAX, -DBL_MAX, DBL_MAX, 2.0**-1074], -DBL_MAX), ([DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, 3.0], 3.0)):
        _, got = oracle.agg_double_sum_exact(np.zeros(len(vals), dtype=np.int64), np.array(vals), 1)
        assert bits_equal(got, [want]), (vals, got)

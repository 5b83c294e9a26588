"""An exact reference for DOUBLE sums, independent of the oracle's C code: every finite double is an integer multiple of 2^-1074, so
a group's sum is a Python int scaled by 2^1074, rounded back to a double once (round half to even).  Also the adversarial value families
the CPU and GPU tests of the EXACT sum share."""
import math
from fractions import Fraction

import numpy as np

SCALE = 2**1074
DBL_MAX = float.fromhex("0x1.fffffffffffffp+1023")
TINY = 2.0**-1074


def _scaled(x):
    n, d = x.as_integer_ratio()
    return n * (SCALE // d)


def round_scaled(total):
    """the double nearest to total * 2^-1074 (ties to even); zero is +0.0 (Java's sum starts from +0.0); overflow gives +-inf"""
    if total == 0:
        return 0.0
    try:
        return float(Fraction(total, SCALE))
    except OverflowError:
        return math.inf if total > 0 else -math.inf


def exact_double_sum(values, gids, ngroups, nulls=None, mask=None):
    """(counts, sums) per group: the correctly rounded exact sum of the selected, non-null values.  NaN when a NaN or both infinities
    occur, else the infinity that occurred."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    g = np.zeros(len(v), dtype=np.int64) if gids is None else np.asarray(gids, dtype=np.int64)
    keep = np.ones(len(v), dtype=bool)
    if nulls is not None:
        keep &= np.asarray(nulls) == 0
    if mask is not None:
        keep &= np.asarray(mask) != 0
    counts = np.bincount(g[keep], minlength=ngroups).astype(np.int64)
    totals = [0] * ngroups
    nan, pinf, ninf = [False] * ngroups, [False] * ngroups, [False] * ngroups
    for gi, x in zip(g[keep].tolist(), v[keep].tolist()):
        if x != x:
            nan[gi] = True
        elif x == math.inf:
            pinf[gi] = True
        elif x == -math.inf:
            ninf[gi] = True
        elif x != 0.0:
            totals[gi] += _scaled(x)
    sums = np.empty(ngroups, dtype=np.float64)
    for i in range(ngroups):
        if nan[i] or (pinf[i] and ninf[i]):
            sums[i] = math.nan
        elif pinf[i] or ninf[i]:
            sums[i] = math.inf if pinf[i] else -math.inf
        else:
            sums[i] = round_scaled(totals[i])
    return counts, sums


def bits_equal(a, b):
    """element-wise identity of float64 bit patterns, every NaN taken as the same one (+0.0 and -0.0 differ)"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64)).copy()
    b = np.atleast_1d(np.asarray(b, dtype=np.float64)).copy()
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- adversarial families ------------------------------------------------------------------------------------------------------------
# family(name, rng, g) -> (clusters, pad): the values group g receives, as clusters that the caller places together (next to each other,
# one lane, or spread over the stream), and the value of the group's padding rows.  A cluster's values only make their point together.
FAMILIES = ("five_rows", "cancel_wide", "overflow", "ties", "subnormal", "zeros", "nonfinite", "benign")

_OVERFLOW = (
    [1e308, 1e308, -1e308],                             # 1e308: the running sum overflows on the way
    [DBL_MAX, 2.0**970],                                # a tie above DBL_MAX: rounds to even = +inf
    [DBL_MAX, 2.0**970 - 2.0**918],                     # below the tie: DBL_MAX
    [DBL_MAX, 2.0**970, -TINY],                         # one unit of 2^-1074 below the tie: DBL_MAX
    [-DBL_MAX, -(2.0**970)],                            # -inf
    [-1e308, -1e308, 1e308, -DBL_MAX, DBL_MAX],         # -1e308
    [-DBL_MAX, -(2.0**970), TINY],                      # -DBL_MAX
)
_TIES = ([1.0, 2.0**-53], [1.0, 2.0**-53, TINY], [1.0 + 2.0**-52, 2.0**-53])
_SUBNORMAL = (
    [2.0**-1022, -(2.0**-1023), -TINY],                 # positive subnormal
    [-(2.0**-1022), 2.0**-1023, TINY, TINY],            # negative subnormal
    [2.0**-1023, 2.0**-1023],                           # crosses 2^-1022 upwards
    [2.0**-1022, -TINY],                                # the largest subnormal
    [2.0**1000, TINY, -(2.0**1000)],                    # a borrow chain over every limb: 2^-1074
    [-(2.0**1000), 2.0**-1000, 2.0**1000],              # 2^-1000
    [-3 * TINY],
)


def _cancel_wide(rng, pairs=1500):
    r = 1.0 + rng.random(pairs)
    k = rng.integers(0, 901, pairs)
    s = np.where(rng.random(pairs) < 0.5, -1.0, 1.0)
    v = s * np.ldexp(r, k)
    vals = np.concatenate([v, -v, [3 * 2.0**-500, 2.0**-520, -(2.0**-530)]])
    rng.shuffle(vals)
    return vals.tolist()


def family(name, rng, g):
    if name == "five_rows":
        return [[2.0**53, 1.0, 2.0**-60, -(2.0**53), -1.0]] * 3, 0.0
    if name == "cancel_wide":
        return [_cancel_wide(rng)], 0.0
    if name == "overflow":
        return [_OVERFLOW[g % len(_OVERFLOW)]], 0.0
    if name == "ties":
        return [_TIES[g % len(_TIES)]] * 2, 0.0
    if name == "subnormal":
        return [_SUBNORMAL[g % len(_SUBNORMAL)]], 0.0
    if name == "zeros":
        if g % 2:
            return [[-0.0] * 8], -0.0                    # nothing but -0.0: +0.0
        x = (rng.standard_normal(6) * 10.0 ** rng.integers(-300, 300, 6)).tolist()
        return [x + [-y for y in x]], 0.0
    if name == "nonfinite":
        extra = ([math.inf], [math.nan], [math.inf, -math.inf], [-math.inf])[g % 4]
        base = _cancel_wide(rng, 300) if g % 2 == 0 else _OVERFLOW[g % len(_OVERFLOW)]
        return [base + extra], 0.0
    if name == "benign":
        if g % 2 == 0:
            qty = rng.integers(1, 51, 400).astype(np.float64)
            return [(qty * rng.integers(90000, 210000, 400) / 100.0).tolist()], 0.0
        return [rng.standard_normal(400).tolist()], 0.0
    raise ValueError(name)


PLACEMENTS = ("adjacent", "lane", "spread")


def place(rng, lo, n, free, cluster, how):
    """row numbers in [lo, n) for a cluster's values, taken from the set `free`: next to each other (neighbouring lanes of one workgroup),
    256 rows apart (one lane of a fused 2048-row tile, the same lane number of neighbouring workgroups elsewhere), or anywhere (long
    clusters always)"""
    m = len(cluster)
    how = how if m <= 64 else "spread"
    for _ in range(1000):
        if how == "spread":
            cand = rng.choice(np.fromiter(free, dtype=np.int64), m, replace=False) if len(free) >= m else None
        else:
            step = 1 if how == "adjacent" else 256
            start = int(rng.integers(lo, max(lo + 1, n - step * m)))
            cand = start + step * np.arange(m)
        if cand is not None and all(int(c) in free for c in cand):
            return [int(c) for c in cand]
    raise RuntimeError("no room for a cluster")


def make_stream(name, rng, ngroups, n, first_row=None, with_filter=False):
    """one stream of n rows: columns (gids, val, val2 nulls, mask, bigint, filter) where the adversarial rows of family `name` are never null,
    never masked and always selected.  first_row[g]: group g gets no row before it (a group that arrives late)."""
    first_row = first_row or [0] * ngroups
    pad_g = rng.integers(0, ngroups, n)
    gids = np.where(np.asarray(first_row)[pad_g] > np.arange(n), 0, pad_g).astype(np.int64)
    avail = list(range(ngroups))
    pads = {}
    vals = np.zeros(n)
    adv = np.zeros(n, dtype=bool)
    for g in avail:
        clusters, pad = family(name, rng, g)
        pads[g] = pad
        free = set(range(first_row[g], n)) - set(np.nonzero(adv)[0].tolist())
        for c, cl in enumerate(clusters):
            how = PLACEMENTS[(g + c + FAMILIES.index(name)) % 3]
            rows = place(rng, first_row[g], n, free, cl, how)
            for r, x in zip(rows, cl):
                vals[r] = x
                gids[r] = g
                adv[r] = True
                free.discard(r)
    for g, pad in pads.items():
        vals[(gids == g) & ~adv] = pad
    nulls = ((rng.random(n) < 0.05) & ~adv).astype(np.uint8)
    mask = (rng.integers(0, 2, n).astype(bool) | adv).astype(np.uint8)
    big = np.where(adv, rng.integers(-(2**62), 2**62, n), rng.integers(-1000, 1000, n)).astype(np.int64)
    filt = np.where(adv, 0.0, rng.random(n)) if with_filter else np.zeros(n)
    return gids, vals, nulls, mask, big, filt

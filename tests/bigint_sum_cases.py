"""sum(bigint) at the int64 edges: adversarial addend families and an exact reference in plain Python ints, shared by the CPU and GPU tests.
No GPU, no oracle.  The rule under test ("DOUBLE policy"): a group's sum is accumulated in 128 bits and only its TOTAL decides
-- the exact total if it lies in [-2^63, 2^63), else NUMERIC_VALUE_OUT_OF_RANGE (-2); what the running sum does on the way is not seen.

A stream has the columns (group id, big, big_nullable, mask, filter).  The family's special rows are never null, never masked and always
selected, and sit at fixed positions (special_positions).  Every other row is small noise in [-1000, 1000].  What an aggregate must not
read carries extreme bytes: big_nullable under a null and every column of a row the filter drops hold INT64_MIN / INT64_MAX / random
words, the mask's byte under a null mask says "true".  sum(big) and sum(big, mask) read the same column, so a masked-out row cannot hold
arbitrary bytes: such rows hold pairs -x, +x (x just below 2^63) that cancel within sum(big) -- a masked sum that reads one of them is
off by 2^63."""
from typing import NamedTuple

import numpy as np

INT64_MAX = 2**63 - 1
INT64_MIN = -(2**63)
RAISES = "raises -2"
FILTER_BELOW = 0.9                 # a row is selected when its filter column is < this

FAMILIES = ("extremes_cancel", "same_sign_near_limit", "total_at_limit", "total_past_limit", "high_word_only", "high_halves", "carry_every_row")
# transient free: no prefix of a group, in row order, leaves int64 unless the group's total does -- there the reference's row-order
# Math.addExact (oracle.agg_long_sum) and the total-only rule agree
TRANSIENT_FREE = {"extremes_cancel": False, "same_sign_near_limit": True, "total_at_limit": True, "total_past_limit": True,
                  "high_word_only": True, "high_halves": False, "carry_every_row": True}
# total_past_limit: which group overflows (the one after it underflows), or "excluded": nothing overflows unless a null, masked or
# filtered row is read
VARIANTS = {name: (None,) for name in FAMILIES}
VARIANTS["total_past_limit"] = ("first", "middle", "last", "excluded")
# masked-out rows with cancelling pairs: not where a pair could itself become the transient of a transient-free family
_PAIRS = {name: name != "carry_every_row" for name in FAMILIES}
HIGH_WORD_TOTALS = (2**64, -(2**64), 2**64 - 1, 2**65 + 7, 3 * 2**64 - 5)


class Stream(NamedTuple):
    gids: np.ndarray            # int64
    big: np.ndarray             # int64, never null: sum, avg, masked sum, min
    big_nulls: np.ndarray       # uint8: the nulls of big_nullable
    mask: np.ndarray            # uint8: the mask's truth (true and not null)
    filt: np.ndarray            # float64: selected when < FILTER_BELOW
    special: np.ndarray         # bool: the family's rows
    big_nullable: np.ndarray    # int64: big where not null, extreme bytes under a null
    mask_values: np.ndarray     # uint8: the mask block's bytes ("true" under a null mask)
    mask_nulls: np.ndarray      # uint8


def special_groups(name, ngroups, variant=None, heavy=None):
    """the groups that receive special rows: all of a few, else a handful (first, second, middle, the last two) and the heavy one"""
    if ngroups <= 8:
        return list(range(ngroups))
    gs = {0, 1, ngroups // 2, ngroups - 2, ngroups - 1}
    if heavy is not None:
        gs.add(heavy)
    return sorted(gs)


def heavy_group(name, ngroups, variant=None):
    """the group that gets a tenth of the rows where a test wants one: the one that overflows, if any"""
    return past_limit_groups(ngroups, variant)[0] if name == "total_past_limit" else ngroups // 3


def past_limit_groups(ngroups, variant):
    """(the group whose total is one above the limit or None, the one whose total is one below or None)"""
    if ngroups == 1:
        return (None, 0) if variant == "last" else (0, None)
    over = {"first": 0, "middle": ngroups // 2, "last": ngroups - 1, "excluded": 0}[variant]
    return over, (over + 1) % ngroups


def _split(rng, total, parts):
    """`parts` positive ints of similar size that sum to `total`"""
    base = total // parts
    out = [base - int(rng.integers(0, base // 4)) for _ in range(parts - 1)]
    return out + [total - sum(out)]


def family(name, rng, g, ngroups, variant=None, salt=0):
    """-> (the special addends of group g in row order, with None for the one that is computed last so that the group's sum(big) hits
    `target` exactly; target or None; sign: +1 / -1 when every addend and every noise row of the group has that sign, else 0;
    quiet: the group's null and masked-out rows hold 0 in `big`, so that all three sums hit the target)"""
    if name == "extremes_cancel":
        up = [INT64_MAX, 2**62, INT64_MAX, INT64_MAX, 2**62] * 10
        down = [INT64_MIN, -(2**62), INT64_MIN, -INT64_MAX, -(2**62)] * 10          # up + down == -20
        return (up + down if (g + salt) % 2 == 0 else down + up), None, 0, False
    if name == "same_sign_near_limit":
        sign = 1 if (g + salt) % 2 == 0 else -1
        vals = [int(rng.integers(2**56, 2**56 + 2**55 + 2**54)) | (0xFFFFFFFF if i % 3 == 0 else 0) for i in range(64)]   # 2^62 <= sum < 1.75 * 2^62 + 2^38
        return [sign * v for v in vals], None, sign, False
    if name in ("total_at_limit", "total_past_limit"):
        if name == "total_at_limit":
            sign = 1 if (g + salt) % 2 == 0 else -1
            target = INT64_MAX if sign > 0 else INT64_MIN
            quiet = False
        else:
            over, under = past_limit_groups(ngroups, variant)
            if g not in (over, under):
                return [], None, 0, False
            sign = 1 if g == over else -1
            edge = 0 if variant == "excluded" else 1
            target = INT64_MAX + edge if sign > 0 else INT64_MIN - edge
            quiet = variant == "excluded"
        vals = [sign * int(rng.integers(2**56, 2**56 + 2**55)) for _ in range(63)]
        vals.insert(int(rng.integers(0, 64)), None)
        return vals, target, sign, quiet
    if name == "high_word_only":
        target = HIGH_WORD_TOTALS[(g + salt) % len(HIGH_WORD_TOTALS)]
        sign = 1 if target > 0 else -1
        near = [INT64_MAX - int(rng.integers(0, 2**20)) for _ in range(abs(target) // 2**63 - 1)]    # addends near 2^63 ...
        rest = _split(rng, abs(target) - sum(near) - 2**60, 63 - len(near))                           # ... and 2^57 .. 2^58 each
        vals = near + rest
        order = rng.permutation(len(vals))
        vals = [sign * vals[i] for i in order]
        vals.insert(int(rng.integers(0, 64)), None)         # about sign * 2^60: fixed once the noise is known
        return vals, target, sign, False
    if name == "high_halves":
        hi = rng.integers(2**28, 2**31, 1000).tolist()
        up = [(h << 32) | 0xFFFFFFFF for h in hi]                       # (uint32)v == 0xFFFFFFFF, v >> 32 == h
        down = [((-h - 1) << 32) | 0xFFFFFFFF for h in hi]              # (uint32)v == 0xFFFFFFFF, v >> 32 == -h - 1; up + down == 2^32 - 2
        return (up + down if (g + salt) % 2 == 0 else down + up), None, 0, False
    if name == "carry_every_row":
        vals = []
        for _ in range(48):
            k = int(rng.integers(2**41, 2**42))
            vals += [INT64_MIN + k, 2**63 - k]      # 2^63 + k as a signed negative, then 2^63 - k: the low words sum to exactly 2^64
        return vals, None, 0, False
    raise ValueError(name)


def special_positions(lo, n, m, g, cuts, taken):
    """m fixed row numbers in [lo, n) for the special rows of the g-th group that has any, ascending: next to every page cut on both
    sides (cut - 1 - g and cut + g), the rest at an even stride with a quarter-block stagger so that they fall into every wave of a 256-thread block.  A row
    that is taken already gives way to the next free one."""
    span = n - lo
    assert m <= span
    want = []
    for c in cuts:
        for p in (c - 1 - g, c + g):
            if lo <= p < n and len(want) < m:
                want.append(p)
    rest = m - len(want)
    step = max(1, span // (rest + 1))
    want += [lo + (j * step + (j % 4) * 64 + 17 * g + 5) % span for j in range(rest)]
    out = []
    for p in want:
        while taken[p]:
            p = lo + (p + 1 - lo) % span
        taken[p] = True
        out.append(p)
    return sorted(out)


def _garbage(rng, m, sign=0):
    """extreme words for rows nothing may read: INT64_MIN, INT64_MAX, random; sign != 0: only values that push that way"""
    pick = rng.integers(0, 3, m)
    rnd = rng.integers(INT64_MIN, INT64_MAX, m, endpoint=True)
    out = np.where(pick == 0, INT64_MIN, np.where(pick == 1, INT64_MAX, rnd)).astype(np.int64)
    if sign > 0:
        out = np.where(out <= 0, INT64_MAX, out)
    if sign < 0:
        out = np.where(out >= 0, INT64_MIN, out)
    return out


def make_stream(name, rng, ngroups, n, first_row=None, with_filter=False, variant=None, cuts=(), heavy=None):
    """one stream of n rows (see the module's docstring).  first_row[g]: group g gets no row before it (a group that arrives late);
    cuts: the row numbers at which the caller cuts the stream into pages; heavy: a group that also gets a tenth of all rows"""
    first_row = np.asarray(first_row if first_row is not None else [0] * ngroups)
    salt = int(rng.integers(0, 10))
    pad_g = rng.integers(0, ngroups, n)
    if heavy is not None:
        pad_g = np.where(rng.random(n) < 0.1, heavy, pad_g)
    gids = np.where(first_row[pad_g] > np.arange(n), 0, pad_g).astype(np.int64)
    big = rng.integers(-1000, 1001, n).astype(np.int64)
    special = np.zeros(n, dtype=bool)
    taken = np.zeros(n, dtype=bool)
    fix, signs, quiet_groups = {}, {}, set()
    for rank, g in enumerate(special_groups(name, ngroups, variant, heavy)):
        vals, target, sign, quiet = family(name, rng, g, ngroups, variant, salt)
        if sign:
            signs[g] = sign
        if quiet:
            quiet_groups.add(g)
        rows = special_positions(int(first_row[g]), n, len(vals), rank, cuts, taken)
        for r, v in zip(rows, vals):
            gids[r] = g
            special[r] = True
            if v is None:
                fix[g] = (r, target)
            else:
                big[r] = v
    for g, sign in signs.items():               # a same-sign group: its noise has the sign too, every prefix is monotone
        rows = (gids == g) & ~special
        big[rows] = sign * np.abs(big[rows])
    filt = np.where(special, 0.0, rng.random(n)) if with_filter else np.zeros(n)
    keep = filt < FILTER_BELOW
    big_nulls = ((rng.random(n) < 0.05) & ~special).astype(np.uint8)
    mask_nulls = ((rng.random(n) < 0.03) & ~special).astype(np.uint8)
    mask_values = (rng.integers(0, 2, n).astype(bool) | special | (mask_nulls != 0)).astype(np.uint8)   # ("true" under a null mask)
    mask = (mask_values != 0) & (mask_nulls == 0)
    for g in quiet_groups:
        big[(gids == g) & ~special & (~mask | (big_nulls != 0))] = 0
    if _PAIRS[name]:
        free = keep & ~mask & (big_nulls == 0) & ~special
        for g in special_groups(name, ngroups, variant, heavy):
            rows = np.nonzero(free & (gids == g))[0]
            for i in range(0, len(rows) - 1, max(2, len(rows) // 6)):        # neighbours among the group's rows, in one page
                a, b = rows[i], rows[i + 1]
                if any(a < c <= b for c in cuts):
                    continue
                x = 2**63 - 2**41 - int(rng.integers(0, 2**40))
                big[a], big[b] = (x, -x) if signs.get(g, 0) < 0 else (-x, x)     # (towards zero first: no prefix leaves int64)
    for g, (r, target) in fix.items():
        rest = sum(big[(gids == g) & keep].tolist()) - int(big[r])
        v = target - rest
        assert INT64_MIN <= v <= INT64_MAX and (v > 0) == (target > 0), (name, g, v)
        big[r] = v
    big_nullable = big.copy()
    for g in range(ngroups) if ngroups <= 8 else [None]:
        rows = (big_nulls != 0) if g is None else (big_nulls != 0) & (gids == g)
        big_nullable[rows] = _garbage(rng, int(rows.sum()), signs.get(g, 0))
    drop = np.nonzero(~keep)[0]
    big[drop] = _garbage(rng, len(drop))
    big_nullable[drop] = _garbage(rng, len(drop))
    for g in quiet_groups:                      # "excluded": a dropped row of the group at the limit would push it over
        rows = drop[gids[drop] == g]
        big[rows] = _garbage(rng, len(rows), signs[g])
        big_nullable[rows] = _garbage(rng, len(rows), signs[g])
    return Stream(gids, big, big_nulls, mask.astype(np.uint8), filt, special, big_nullable, mask_values, mask_nulls)


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def totals(gids, values, ngroups, keep):
    """(counts, exact totals) per group over the rows `keep` selects: Python ints, no bound"""
    cnt, tot = [0] * ngroups, [0] * ngroups
    sel = np.nonzero(keep)[0]
    for g, v in zip(np.asarray(gids)[sel].tolist(), np.asarray(values)[sel].tolist()):
        cnt[g] += 1
        tot[g] += v
    return cnt, tot


def narrow(total):
    """what sum(bigint) returns for an exact total"""
    return total if INT64_MIN <= total <= INT64_MAX else RAISES


class Reference(NamedTuple):
    sums: list             # per group: exact total of big over the selected rows
    sums_masked: list      # ... whose mask is true and not null
    sums_nullable: list    # ... of big_nullable where it is not null
    mins: list             # per group: min(big) or None
    count_all: list
    count_masked: list
    count_nullable: list

    def raises(self):
        return any(narrow(t) == RAISES for col in (self.sums, self.sums_masked, self.sums_nullable) for t in col)


def reference(s, ngroups, rows=None):
    """the exact totals of a stream (rows: a slice or index array restricting it, e.g. one PARTIAL operator's pages)"""
    keep = s.filt < FILTER_BELOW
    if rows is not None:
        only = np.zeros(len(keep), dtype=bool)
        only[rows] = True
        keep &= only
    c_all, t_all = totals(s.gids, s.big, ngroups, keep)
    c_m, t_m = totals(s.gids, s.big, ngroups, keep & (s.mask != 0))
    c_n, t_n = totals(s.gids, s.big_nullable, ngroups, keep & (s.big_nulls == 0))
    mins = [None] * ngroups
    sel = np.nonzero(keep)[0]
    for g, v in zip(s.gids[sel].tolist(), s.big[sel].tolist()):
        mins[g] = v if mins[g] is None or v < mins[g] else mins[g]
    return Reference(t_all, t_m, t_n, mins, c_all, c_m, c_n)


# ---- plausible kernel bugs, as functions of a group's addends in row order -> int or RAISES ----------------------------------------------
def _words(total):
    """an exact total as the kernels' (low, high) words, evaluated the way agg_evaluate_kernel does"""
    lo, hi = total % 2**64, (total >> 64) % 2**64
    val = lo - 2**64 if lo >= 2**63 else lo
    return RAISES if hi != (2**64 - 1 if val < 0 else 0) else val


def _wrap(total):
    return (total + 2**63) % 2**64 - 2**63


def model_wrap_no_raise(vals):
    return _wrap(sum(vals))


def model_ignore_high_word(vals):
    """evaluate returns the low word and never looks at the high one (the outcome of wrap_no_raise, by another bug)"""
    return _wrap(sum(vals) % 2**64)


def model_high_word_any_sign(vals):
    """evaluate accepts a high word of 0 or ~0 without comparing it with the low word's sign"""
    t = sum(vals)
    return _wrap(t) if (t >> 64) in (0, -1) else RAISES


def model_drop_carry_in_fold(vals):
    """four lane-private 128-bit sums, folded word by word without the carry out of the low words"""
    lanes = [sum(vals[i::4]) for i in range(4)]
    lo = sum(t % 2**64 for t in lanes)
    hi = sum((t >> 64) % 2**64 for t in lanes) % 2**64
    return _words(((hi << 64) | (lo % 2**64)) - (2**128 if hi >= 2**63 else 0))


def model_addend_unsigned(vals):
    return _words(sum(v % 2**64 for v in vals))


def model_high_half_unsigned(vals):
    return _words(2**32 * sum((v >> 32) % 2**32 for v in vals) + sum(v & 0xFFFFFFFF for v in vals))


def model_float64(vals):
    t = 0.0
    for v in vals:
        t += float(v)
    return int(t) if -(2.0**63) <= t < 2.0**63 else RAISES


def model_saturate(vals):
    t = 0
    for v in vals:
        t = max(INT64_MIN, min(INT64_MAX, t + v))
    return t


WRONG_MODELS = {"wrap_no_raise": model_wrap_no_raise, "ignore_high_word": model_ignore_high_word, "high_word_any_sign": model_high_word_any_sign,
                "drop_carry_in_fold": model_drop_carry_in_fold, "addend_unsigned": model_addend_unsigned,
                "high_half_unsigned": model_high_half_unsigned, "float64": model_float64, "saturate": model_saturate}

"""Inputs of the LIKE / IN tests: the boundary page, the randomised values and patterns, the IN lists.  Pure Python, no GPU."""
import functools
import random

LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33]
CYCLE = "ab01c0ba"
ALPHABET = ["a", "b", "%", "_", "\\", "\n", "é", "名", "\U0001F600"]   # a b % _ \ newline, 2-, 3- and 4-byte code points


def cyc(n, start=0):
    return (CYCLE * 8)[start:start + n]


def boundary_values():
    """65 rows: the last row sits alone in the second wave.  Row 0 begins the pool and the last row ends it (neither is null or empty)."""
    vals = []
    for n in LENGTHS:
        vals.append(cyc(n))                                  # begins with ab..., every length
        vals.append(("xy" * 20)[:max(0, n - 2)] + "ab"[:n])  # ends with ab
    vals += ["aba", "aab", "abab", "ab01c0", "abc", "xbc", "abx", "ba", "abba", "abxba", "abbac",
             "é", "名", "\U0001F600", "ébc", "aéc", "abé", "名bc", "a名c", "ab名", "\U0001F600bc", "a\U0001F600c", "ab\U0001F600",
             "\U0001F600名é", "a\nc", "ab\n", "%", "_", "a%c", "ab\\", "a", "ab"] + [cyc(k) + cyc(33, 3)[-k:] for k in (8, 9, 17)]
    assert len(vals) == 61
    vals += [None, None, None]
    vals = [v for v in vals if v != ""] + [""]               # one empty string, not at either end
    rows = [cyc(16)] + vals[:-1]
    rows.insert(7, vals[-1])
    rows.insert(20, None)
    rows = rows[:64] + [cyc(33, 3)]                          # the lone row of wave 2, 33 bytes, ends the pool
    assert len(rows) == 65 and rows[0] and rows[-1]
    assert {len(v.encode()) for v in rows if v is not None} >= set(LENGTHS)
    return rows


def boundary_patterns():
    """(pattern, escape or None)"""
    pats = ["", "%", "%%", "_", "___", "_%", "%_", "%_%",
            "ab", "ab%", "%ab", "%ab%", "ab%ba",
            "%ab%c%",
            "a_c", "_bc", "ab_", "%_b", "a%_"]
    for k in (8, 9, 17):                                     # literals of 8, 9 and 17 bytes at each anchor
        lit, end = cyc(k), cyc(33, 3)[-k:]
        pats += [lit + "%", "%" + end, "%" + cyc(k, 1) + "%", lit[:k] + "%" + end, lit]
    pats.append("".join(c + "%" for c in cyc(33)) + "%%%%")  # 70 tokens; matches the 33-byte row that begins the cycle
    assert len(pats[-1]) == 70
    pats += ["_bc", "a_c", "ab_", "%_c", "a_%", "_", "__", "___", "%_名_%", "_名é", "\U0001F600__", "%é", "名%", "%\U0001F600%", "a\nc", "a_c%", "%\n"]
    out = [(p, None) for p in pats]
    out += [("a\\%c", "\\"), ("\\_", "\\"), ("%\\%", "\\"), ("a#%%", "#"), ("ab\\", None), ("\\%", ""), ("ab%", "")]
    return out


def random_values(seed=11, count=512):
    rng = random.Random(seed)
    vals = ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 20))) for _ in range(count)]
    for i in rng.sample(range(count), 24):
        vals[i] = None
    return vals


def random_patterns(seed=12, count=240):
    """(pattern, escape or None): 0..8 tokens over the alphabet, wildcards favoured; every second pattern carries the escape backslash"""
    rng = random.Random(seed)
    toks = ALPHABET + ["%", "%", "_", "a", "b", "a", "b"]
    return [("".join(rng.choice(toks) for _ in range(rng.randint(0, 8))), "\\" if i % 2 else None) for i in range(count)]


def chunks(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


IN_SMALL_LIST = 8   # jit.cpp kInSmallList: up to this many distinct non-null items are compared one by one, longer lists go through a hash table
                    # (tests/test_like_in_cpu.py pins the threshold on the generated source, so a drift between the two shows)
ROW_COUNTS = [1, 63, 64, 65, 1000]


def _lists(rng, draw, sizes=(1, 2, IN_SMALL_LIST - 1, IN_SMALL_LIST, IN_SMALL_LIST + 1, 33, 5001)):
    """distinct items per size (so that the size is the strategy's), then: with a null item, with duplicates, only a null item"""
    out = []
    for n in sizes:
        items = []
        seen = set()
        while len(items) < n:
            x = draw(rng)
            if repr(x) not in seen:
                seen.add(repr(x))
                items.append(x)
        out.append(items)
    out.append(out[1] + [None])
    out.append(out[4] + [None] + out[4][:3])
    out.append(out[2] + out[2])
    out.append([None])
    return out


@functools.lru_cache(maxsize=None)
def in_cases():
    """[(type name, 1,000 values with nulls, item lists)]; the first rows hold the type's edge values, so that every row count sees some"""
    nan, inf = float("nan"), float("inf")
    cases = []

    def column(rng, edges, draw, lists):
        vals = list(edges) + [draw(rng) for _ in range(1000 - len(edges))]
        for i in rng.sample(range(1, 1000), 60):
            vals[i] = None
        hit = [x for l in lists for x in l[:3] if x is not None]
        for i in rng.sample(range(1, 1000), 200):            # a fifth of the rows are items of some list
            if vals[i] is not None:
                vals[i] = rng.choice(hit)
        return vals

    rng = random.Random(21)
    big = [2**31, -2**31 - 1, 2**63 - 1, -2**63, 0, -1, 2**32 + 5, 5]
    draw = lambda r: r.choice(big) if r.random() < 0.05 else r.randint(-3000, 3000) * (2**33 if r.random() < 0.3 else 1)
    lists = _lists(rng, draw) + [big, [2**63 - 1, -2**63], [0x8000000000000001 - 2**64, 7, 8, 9, 10, 11, 12, 13, 14, 15]]
    cases.append(("bigint", column(rng, big, draw, lists), lists))

    rng = random.Random(22)
    dbl = [nan, 0.0, -0.0, inf, -inf, 1.5, -1.5, 1e300]
    draw = lambda r: r.choice(dbl) if r.random() < 0.1 else r.randint(-20000, 20000) / 4.0
    lists = _lists(rng, draw) + [[nan], [nan, 1.5], [-0.0], [0.0, inf], [-inf, nan, None],
                                 [nan, -0.0, inf, -inf] + [float(i) + 0.25 for i in range(12)], [0.0] + [float(i) + 0.25 for i in range(12)]]
    cases.append(("double", column(rng, dbl, draw, lists), lists))

    rng = random.Random(23)
    strs = ["", "a", "ab", "abc", "abd", "xbc", "abcdefgh", "abcdefgx", "xbcdefgh", "abcdefghi", "abcdefghijklmnopq", "abcdefghijklmnopx", "é", "名"]
    draw = lambda r: r.choice(strs) if r.random() < 0.2 else "".join(r.choice("abcx") for _ in range(r.randint(0, 10)))
    lists = _lists(rng, draw) + [[""], ["", None], ["abc", "abd", "xbc"], strs, ["abcdefgh", "abcdefghi", "abcdefghijklmnopq"] + ["s%d" % i for i in range(10)]]
    cases.append(("varchar", column(rng, strs, draw, lists), lists))

    rng = random.Random(24)
    draw = lambda r: r.randint(-40000, 40000)
    ints = [2**31 - 1, -2**31, 0, -1]
    lists = _lists(rng, draw, sizes=(1, 2, 7, 8, 9, 33)) + [ints]
    cases.append(("integer", column(rng, ints, draw, lists), lists))
    lists = _lists(rng, draw, sizes=(1, 2, 7, 8, 9, 33)) + [[0, 10471, -1]]
    cases.append(("date", column(rng, [10471, 0, -1], draw, lists), lists))

    rng = random.Random(25)
    draw = lambda r: r.random() < 0.5
    lists = [[True], [False], [True, False], [True, None], [None], [False, False, None]]
    cases.append(("boolean", column(rng, [True, False], draw, lists), lists))
    return cases

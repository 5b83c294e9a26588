"""Inputs of the string-function tests: the boundary values, a seeded random set, the substr argument pairs and the row counts."""
import random

ROW_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 2049]   # the wave, tile and multi-tile edges of fp_emit / fp_vwrite
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 5000]
LONGEST = 5000
INT64_EDGES = [0, -1, 1, 2**63 - 1, -(2**63 - 1), -2**63] + [s * 10**k + s * d for k in range(19) for s in (1, -1) for d in (0, -1) if abs(s * 10**k + s * d) < 2**63]


def ascii_value(n, salt=0):
    return bytes(97 + (i * 7 + salt) % 26 for i in range(n))


def boundary_values():
    """every length at which a copy or a count changes its path; 2-, 3- and 4-byte code points first, last and at every alignment mod 8;
    NULLs; a few malformed sequences (a lone continuation byte, a truncated lead)"""
    out = [ascii_value(n, n) for n in LENGTHS]
    for cp in ("é", "名", "\U0001F600"):
        c = cp.encode()
        for a in range(8):
            out.append(b"x" * a + c + b"yz")        # first (a == 0) and at alignment a
            out.append(b"ab" + b"x" * a + c)        # last
        out.append(c * 3)
    out += [None, b"\x80abc", b"ab\xe5\x90", b"\xc3", b"a\x80\x80b", b"\x80\x80", None, b"abab", b"aab", b"13-555", b"31-999"]
    return out


def cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


def random_values(n=1500, seed=11):
    rng = random.Random(seed)
    alphabet = ["a", "b", "c", "ab", " ", "-", "1", "3", "é", "名", "\U0001F600"]
    out = []
    for i in range(n):
        if rng.random() < 0.06:
            out.append(None)
            continue
        k = rng.choice([0, 1, 2, 3, 5, 8, 13, 21, 40, 90, 300]) if rng.random() < 0.9 else rng.randrange(1000, 1400)
        out.append("".join(rng.choice(alphabet) for _ in range(k)).encode())
    return out


def random_ints(n=1500, seed=12):
    rng = random.Random(seed)
    return [None if rng.random() < 0.05 else rng.choice([rng.randrange(-50, 50), rng.randrange(-2**63, 2**63), rng.randrange(-2**31, 2**31)]) for _ in range(n)]


STARTS = [0, 1, -1, 2, -2, 7, -7, 8, -8, 9, -9, 16, -16, 17, -17, 1024, -1024, 1025, -1025, 1026, -1026, 5000, -5000, 5001, -5001,
          2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**63 - 1, -2**63]
SUBSTR_LENGTHS = [0, -1, 1, 2, 7, 8, 9, 1024, 5000, 5001, 2**31 - 1, 2**31, 2**63 - 1, -2**63]


def substr_pairs():
    """(start, length) covering every branch of substring :321-367: 0, +-1, +-len, +-(len + 1) for the lengths of the boundary set, the
    int32 and int64 edges.  With a negative start the length stays <= 2^31 - 1 - code points, where the reference itself is defined."""
    return [(s, l) for s in STARTS for l in SUBSTR_LENGTHS if s >= 0 or l <= 2**31 - 1 - LONGEST - 1]


def chunks(items, n):
    return [items[i:i + n] for i in range(0, len(items), n)]

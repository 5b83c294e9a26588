"""The row-at-a-time model of min / max over INTEGER, DATE and VARCHAR (tests/minmax_expected.py) against literals transcribed from the
reference's own aggregation tests (tests/golden/minmax_vectors.json), the layouts of PARTIAL -> FINAL, and the 7-byte round code of the
VARCHAR extremes against Python's `bytes` order.  No GPU."""
import json
import os
import random

import pytest

import minmax_expected as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minmax_vectors.json")
with open(GOLDEN) as fh:
    CASES = json.load(fh)["cases"]


def decoded(case):
    fn = getattr(M, case["function"])
    conv = (lambda v: None if v is None else bytes.fromhex(v)) if M.is_varchar(fn) else (lambda v: v)
    return fn, [conv(v) for v in case["values"]], conv(case["expected"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_literals(case):
    fn, values, expected = decoded(case)
    taken = sum(v is not None for v in values)
    assert M.single([(values, None, None)], fn) == [(taken, expected)]
    # the same positions cut into pages of 1, 3 and as two PARTIALs into a FINAL
    for width in (1, 3):
        pages = [(values[i:i + width], None, None) for i in range(0, len(values), width)]
        assert M.single(pages, fn) == [(taken, expected)]
        assert M.partial_final([pages[:2], pages[2:]], fn) == [(taken, expected)]


def test_functions_cover_the_golden_file():
    assert {c["function"] for c in CASES} == {"MIN_INTEGER", "MAX_INTEGER", "MAX_DATE", "MIN_VARCHAR", "MAX_VARCHAR"}
    assert (M.MIN_INTEGER, M.MAX_INTEGER, M.MIN_DATE, M.MAX_DATE, M.MIN_VARCHAR, M.MAX_VARCHAR) == (11, 12, 13, 14, 15, 16)


def test_groups_masks_and_layouts():
    values = [5, None, -2 ** 31, 7, 2 ** 31 - 1, -1, 0, None]
    gids = [0, 0, 1, 1, 2, 2, 3, 3]
    mask = [True, True, False, None, True, False, True, True]
    assert M.single([(values, gids, None)], M.MIN_INTEGER, 5) == [(1, 5), (2, -2 ** 31), (2, -1), (1, 0), (0, None)]
    assert M.single([(values, gids, mask)], M.MAX_DATE, 5) == [(1, 5), (0, None), (1, 2 ** 31 - 1), (1, 0), (0, None)]
    # the flattened NullableLongState: value 0 where the count is 0; VARCHAR: a NULL cell
    assert M.partial([(values, gids, mask)], M.MAX_DATE, 5) == [(1, 5), (0, 0), (1, 2 ** 31 - 1), (1, 0), (0, 0)]
    texts = [b"", None, b"a", b"a\x00", b"\x7f", b"\x80", None, None]
    assert M.single([(texts, gids, None)], M.MIN_VARCHAR, 5) == [(1, b""), (2, b"a"), (2, b"\x7f"), (0, None), (0, None)]
    assert M.single([(texts, gids, None)], M.MAX_VARCHAR, 5) == [(1, b""), (2, b"a\x00"), (2, b"\x80"), (0, None), (0, None)]
    assert M.partial([(texts, gids, None)], M.MAX_VARCHAR, 5)[3:] == [(0, None), (0, None)]
    # FINAL ignores the value cell of a row whose count is 0, whatever it holds, and adds the counts
    assert M.final([([0, 0, 0], [0, 2, 3], [-99, 4, 1])], M.MIN_INTEGER) == [(5, 1)]
    assert M.final([([0, 0], [0, 0], [b"zz", b""])], M.MAX_VARCHAR) == [(0, None)]


def random_pair(rng, shared):
    """two byte strings that share `shared` leading bytes: embedded zero bytes, bytes from 0x80 up, one the other's prefix, equal ones"""
    alphabet = [0x00, 0x01, 0x7f, 0x80, 0xff, 0x61]
    prefix = bytes(rng.choice(alphabet) for _ in range(shared))
    tails = []
    for _ in range(2):
        tails.append(bytes(rng.choice(alphabet) if rng.random() < 0.7 else rng.randrange(256) for _ in range(rng.choice([0, 0, 1, 1, 2, 6, 7, 8, 13, 14, 15, 40]))))
    if rng.random() < 0.1:
        tails[1] = tails[0]
    return prefix + tails[0], prefix + tails[1]


def test_round_code_orders_like_bytes():
    rng = random.Random(20240611)
    seen = set()
    for i in range(5000):
        a, b = random_pair(rng, i % 31)
        want = (a > b) - (a < b)
        assert M.compare_by_rounds(a, b) == want, (a, b)
        seen.add(want)
    assert seen == {-1, 0, 1}


def test_round_code_layout():
    assert M.round_code(b"", 0) == 0
    assert M.round_code(b"a", 0) == 0x61 << 56 | 1
    assert M.round_code(b"a\x00", 0) == 0x61 << 56 | 2
    assert M.round_code(b"abcdefg", 0) == int.from_bytes(b"abcdefg", "big") << 8 | 7
    assert M.round_code(b"abcdefgh", 0) == int.from_bytes(b"abcdefg", "big") << 8 | 8
    assert M.round_code(b"abcdefgh", 1) == 0x68 << 56 | 1
    assert M.round_code(b"abcdefg", 1) == 0          # exactly 7k bytes: an empty rest, below every extension

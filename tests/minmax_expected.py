"""Row-at-a-time model of the reference's min / max aggregation loop (AbstractMinMaxAggregationFunction.java: input :233-249,
combine :251-272 over NullableLongState for the long.class types INTEGER and DATE, BlockPositionState :245,269,325 for the Slice types)
for the functions MIN_/MAX_ INTEGER, DATE and VARCHAR of include/tgpu.h.  No GPU, no numpy: plain Python values -- ints for INTEGER / DATE,
`bytes` for VARCHAR, whose comparison IS Slice.compareTo's order (unsigned bytes left to right, a proper prefix first).  None is NULL.

A page is (values, gids, mask): `gids` None = the global aggregation (group 0), `mask` None = no mask channel, else a list of
True / False / None (a NULL mask cell excludes the row, AccumulatorCompiler.java:487-566)."""

MIN_INTEGER, MAX_INTEGER, MIN_DATE, MAX_DATE, MIN_VARCHAR, MAX_VARCHAR = 11, 12, 13, 14, 15, 16
FUNCTIONS = (MIN_INTEGER, MAX_INTEGER, MIN_DATE, MAX_DATE, MIN_VARCHAR, MAX_VARCHAR)


def is_min(function):
    assert function in FUNCTIONS, function
    return function % 2 == 1


def is_varchar(function):
    return function in (MIN_VARCHAR, MAX_VARCHAR)


def _better(function, value, state):
    """the comparison of input() / combine(): a value replaces the state only when it is strictly better"""
    return value < state if is_min(function) else value > state


def _check_value(function, v):
    if is_varchar(function):
        assert isinstance(v, bytes), v
    else:
        assert isinstance(v, int) and -2 ** 31 <= v < 2 ** 31, v


def accumulate(pages, function, ngroups=1):
    """-> [[count, value or None]] per group: count = the rows taken (unmasked, non-null)"""
    state = [[0, None] for _ in range(ngroups)]
    for values, gids, mask in pages:
        for i, v in enumerate(values):
            if mask is not None and not mask[i]:        # False or None
                continue
            if v is None:
                continue
            _check_value(function, v)
            s = state[0 if gids is None else gids[i]]
            if s[0] == 0 or _better(function, v, s[1]):
                s[1] = v
            s[0] += 1
    return state


def single(pages, function, ngroups=1):
    """SINGLE: [(count, value or None)] per group; the output cell is the value, NULL where the count is 0"""
    return [(c, v if c else None) for c, v in accumulate(pages, function, ngroups)]


def partial(pages, function, ngroups=1):
    """PARTIAL's two channels per group: INTEGER / DATE (count BIGINT, extreme BIGINT, 0 where the count is 0 -- the flattened
    NullableLongState); VARCHAR (count BIGINT, value VARCHAR, NULL where the count is 0)"""
    return [(c, v if c else (None if is_varchar(function) else 0)) for c, v in accumulate(pages, function, ngroups)]


def final(intermediate_pages, function, ngroups=1):
    """FINAL over pages of (gids or None, counts, values): the value cell of a row whose count is 0 is ignored whatever it holds; the
    counts add up.  -> [(count, value or None)] per group"""
    state = [[0, None] for _ in range(ngroups)]
    for gids, counts, values in intermediate_pages:
        for i, c in enumerate(counts):
            if c == 0:
                continue
            _check_value(function, values[i])
            s = state[0 if gids is None else gids[i]]
            if s[0] == 0 or _better(function, values[i], s[1]):
                s[1] = values[i]
            s[0] += c
    return [(c, v if c else None) for c, v in state]


def partial_final(page_sets, function, ngroups=1):
    """one PARTIAL per page set, their intermediate rows (every group, empty ones included) into one FINAL"""
    inter = []
    for pages in page_sets:
        rows = partial(pages, function, ngroups)
        inter.append((list(range(ngroups)), [c for c, _ in rows], [v for _, v in rows]))
    return final(inter, function, ngroups)


# ---- the 7-byte round code of the VARCHAR extremes, restated -----------------------------------------------------------------------------
def round_code(value, k):
    """round k looks at bytes [7k, 7k + 7) of the value: the high 56 bits are those bytes, big-endian and zero-padded, the low byte is
    min(length - 7k, 8) -- the remaining length, 8 = more follows.  Only defined while 7k <= length."""
    rest = len(value) - 7 * k
    assert rest >= 0
    window = value[7 * k:7 * k + 7]
    return int.from_bytes(window + b"\x00" * (7 - len(window)), "big") << 8 | min(rest, 8)


def compare_by_rounds(a, b):
    """-1 / 0 / 1 the way the rounds decide: the first round whose codes differ, or equal when both end in the same round"""
    k = 0
    while True:
        ca, cb = round_code(a, k), round_code(b, k)
        if ca != cb:
            return -1 if ca < cb else 1
        if ca & 0xff <= 7:          # both end here with the same bytes
            return 0
        k += 1

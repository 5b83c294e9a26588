"""Inputs and bit-exact comparisons of the key-semantics tests (test_key_semantics_cpu.py, test_gpu_key_types.py): key columns whose DOUBLE
channels carry NaNs of several payloads, both zeros, infinities and denormals as BIT PATTERNS at fixed positions, the key schemas whose
register signatures take every layout the fused aggregation generates, and two deliberately WRONG groupings / matchings in numpy (by raw
bits; with IEEE / SQL `=`) that every input family must tell apart from the reference semantics -- otherwise a GPU test over it could not fail.

Reference semantics (oracle/trino_oracle.c cells_not_distinct / cells_equal_nonnull):
  grouping  IS NOT DISTINCT FROM: all NaNs one group, -0.0 and +0.0 one group, NULL its own group; a group's key = the cells of its first row
  joins     EQUAL: -0.0 matches +0.0, NaN matches nothing (not even its own bits), NULL matches nothing

A column here is a KeyCol (type, values, nulls) that needs neither the product nor the oracle; to_block / to_ocol convert it.  Doubles are
never compared with == or through rows(): cells() turns every cell into a token -- None for NULL, the raw bits as an int, the bytes of a
VARCHAR -- and everything is compared through those."""
import numpy as np

BIGINT, INTEGER, DATE, DOUBLE, BOOLEAN, VARCHAR = 1, 2, 3, 4, 5, 6
_NP = {BIGINT: np.int64, INTEGER: np.int32, DATE: np.int32, DOUBLE: np.float64, BOOLEAN: np.uint8}
_BITS = {BIGINT: np.uint64, DOUBLE: np.uint64, INTEGER: np.int32, DATE: np.int32, BOOLEAN: np.uint8}

NAN_CANONICAL = 0x7FF8000000000000
NAN_BITS = [NAN_CANONICAL, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FF8000000000123]   # quiet, negative quiet, signalling, payload
NAN_NEVER_INSERTED = 0x7FF8000000000777                                                   # for contains(): a payload no generator writes
NEG_ZERO, POS_ZERO = 0x8000000000000000, 0x0000000000000000
POS_INF, NEG_INF = 0x7FF0000000000000, 0xFFF0000000000000
DENORMAL, NEG_DENORMAL = 0x0000000000000001, 0x8000000000000001                           # 5e-324, -5e-324
MAX_SPECIAL_SLOTS = 64


def bits_to_doubles(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def special_cycle(first_zero="neg", first_nan_canonical=False, extremes=True):
    """the specials in the order the slots take them: slot 0 is the stream's first zero, slot 1 its first NaN"""
    z0, z1 = (NEG_ZERO, POS_ZERO) if first_zero == "neg" else (POS_ZERO, NEG_ZERO)
    nans = NAN_BITS if first_nan_canonical else [NAN_BITS[1], NAN_BITS[0], NAN_BITS[2], NAN_BITS[3]]
    cyc = [z0, nans[0], z1, nans[1], z0, nans[2], z1, nans[3]]
    if extremes:
        cyc = cyc[:4] + [POS_INF, NEG_INF] + cyc[4:6] + [DENORMAL, NEG_DENORMAL] + cyc[6:]
    return cyc


def special_slots(n, slots=MAX_SPECIAL_SLOTS):
    """positions 0, step, 2 * step, ...: at most `slots` of them, position 0 always"""
    step = max(1, n // slots)
    return np.arange(0, n, step)[:slots]


def special_doubles(rng, n, domain, first_zero="neg", first_nan_canonical=False, extremes=True, slots=MAX_SPECIAL_SLOTS):
    """integer-valued doubles from `domain` with the specials of special_cycle() written in as bit patterns at special_slots(): which
    special sits where depends on n alone, never on the draw.  first_zero: the sign of the first zero of the stream ("neg" / "pos"; both
    signs then alternate); first_nan_canonical=False: the first NaN is 0xfff8...01, so a group key that comes out as the canonical NaN
    is visibly not the first row's.  extremes: +-inf and +-5e-324 too (four more groups)."""
    bits = rng.integers(domain[0], domain[1], n).astype(np.float64).view(np.uint64).copy()
    cyc = special_cycle(first_zero, first_nan_canonical, extremes)
    for j, p in enumerate(special_slots(n, slots)):
        bits[p] = cyc[j % len(cyc)]
    return bits.view(np.float64)


class KeyCol:
    def __init__(self, type_id, values, nulls=None):
        self.type = type_id
        if type_id == VARCHAR:
            self.values = list(values)
            self.nulls = None
            self.n = len(self.values)
        else:
            self.values = np.ascontiguousarray(values, dtype=_NP[type_id])
            self.nulls = None if nulls is None else np.ascontiguousarray(nulls, dtype=np.uint8)
            self.n = len(self.values)


def to_block(pkg, col):
    return pkg.Block(col.type, col.values, col.nulls)


def to_ocol(oracle, col):
    return oracle.Col(col.type, col.values, col.nulls)


def concat(cols):
    if cols[0].type == VARCHAR:
        return KeyCol(VARCHAR, [v for c in cols for v in c.values])
    nulls = None
    if any(c.nulls is not None for c in cols):
        nulls = np.concatenate([c.nulls if c.nulls is not None else np.zeros(c.n, dtype=np.uint8) for c in cols])
    return KeyCol(cols[0].type, np.concatenate([c.values for c in cols]), nulls)


def concat_pages(pages):
    return [concat([pg[c] for pg in pages]) for c in range(len(pages[0]))]


def take(col, idx):
    idx = np.asarray(idx, dtype=np.int64)
    if col.type == VARCHAR:
        return KeyCol(VARCHAR, [col.values[i] for i in idx])
    return KeyCol(col.type, col.values[idx], None if col.nulls is None else col.nulls[idx])


# VARCHAR key values: the empty string, one- and two-byte values that differ in the second byte only, one value past the 16 bytes an LDS
# record holds, and two-byte values that share their first byte (equal register signatures: "open" rows)
VARCHAR_VOCABULARY = ["", "a", "ab", "ac", "a value longer than 16 bytes", "b", "k0", "k1"] + ["v%d" % i for i in range(400)]


def key_col(rng, type_id, n, domain, null_frac=0.05, **special):
    """one key channel: `domain` = (lo, hi) of the integer draw (DOUBLE: before the specials go in; VARCHAR: indices into the vocabulary;
    BOOLEAN: ignored).  Null cells of fixed-width channels keep whatever was drawn underneath, as blocks of the engine do."""
    nulls = (rng.random(n) < null_frac).astype(np.uint8) if null_frac > 0 else None
    if type_id == DOUBLE:
        return KeyCol(DOUBLE, special_doubles(rng, n, domain, **special), nulls)
    if type_id == BOOLEAN:
        return KeyCol(BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), nulls)
    if type_id == VARCHAR:
        ks = rng.integers(domain[0], domain[1], n)
        return KeyCol(VARCHAR, [None if (nulls is not None and nulls[i]) else VARCHAR_VOCABULARY[k] for i, k in enumerate(ks)])
    return KeyCol(type_id, rng.integers(domain[0], domain[1], n), nulls)


# name -> types; the signature of the fused aggregation's register records = null mask (one bit per key) + the fields
KEY_SCHEMAS = {
    "DOUBLE": [DOUBLE],                                            # 1 + 64: two words
    "BOOLEAN": [BOOLEAN],                                          # 2: narrow
    "INTEGER": [INTEGER],                                          # 33: one wide word, the first size above the narrow limit
    "DATE_BOOLEAN": [DATE, BOOLEAN],                               # 35
    "INTEGER_DATE": [INTEGER, DATE],                               # 66: the second field moves to word two
    "DOUBLE_BIGINT": [DOUBLE, BIGINT],                             # 130: three words
    "BOOLEAN_VARCHAR_VARCHAR": [BOOLEAN, VARCHAR, VARCHAR],        # 24: narrow, with "open" rows
    "VARCHAR_DOUBLE_BOOLEAN_DATE": [VARCHAR, DOUBLE, BOOLEAN, DATE],   # four fields
}
# per schema the draw domains of the group-by-hash / join / unfused-aggregation families (a few hundred groups at most)
SCHEMA_DOMAINS = {
    "DOUBLE": [(-20, 20)], "BOOLEAN": [None], "INTEGER": [(-40, 40)], "DATE_BOOLEAN": [(9000, 9030), None], "INTEGER_DATE": [(-6, 6), (9000, 9008)],
    "DOUBLE_BIGINT": [(-3, 4), (-2, 2)], "BOOLEAN_VARCHAR_VARCHAR": [None, (0, 6), (0, 8)], "VARCHAR_DOUBLE_BOOLEAN_DATE": [(0, 5), (-2, 2), None, (9000, 9003)],
}


def key_page(rng, types, n, domains, null_frac=0.05, **special):
    return [key_col(rng, t, n, d, null_frac, **special) for t, d in zip(types, domains)]


# ---- bit-exact views ----------------------------------------------------------------------------------------------------------------
def _flat(block):
    """(type, values, nulls, offsets) of a KeyCol, a product Block or an oracle Col"""
    if isinstance(block, KeyCol) and block.type == VARCHAR:
        return VARCHAR, block.values, None, None
    b = block.flatten() if hasattr(block, "flatten") else block
    return b.type, b.values, b.nulls, getattr(b, "offsets", None)


def cells(block):
    """one token per cell: None (NULL), the raw bits as a Python int, or the bytes of a VARCHAR"""
    t, values, nulls, offsets = _flat(block)
    if t == VARCHAR:
        if offsets is None:
            return [None if v is None else (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for v in values]
        n = len(offsets) - 1
        return [None if (nulls is not None and nulls[i]) else bytes(values[offsets[i]:offsets[i + 1]]) for i in range(n)]
    raw = np.ascontiguousarray(values, dtype=_NP[t]).view(_BITS[t]).tolist()
    if nulls is None:
        return raw
    return [None if f else v for v, f in zip(raw, np.asarray(nulls).tolist())]


def block_bits(block):
    """(null flags, the non-null cells): the cells as a uint64 / int32 / uint8 array, or the list of byte strings of a VARCHAR"""
    t = _flat(block)[0]
    toks = cells(block)
    nulls = np.array([v is None for v in toks], dtype=bool)
    live = [v for v in toks if v is not None]
    return nulls, (live if t == VARCHAR else np.array(live, dtype=_BITS[t]))


def row_tokens(blocks):
    cs = [cells(b) for b in blocks]
    return list(zip(*cs)) if cs else []


def from_block(block):
    """a product Block (or oracle Col) as a KeyCol"""
    t, values, nulls, offsets = _flat(block)
    if t == VARCHAR:
        return KeyCol(VARCHAR, [None if v is None else v.decode("utf-8") for v in cells(block)])
    return KeyCol(t, values, nulls)


def col_from_tokens(type_id, tokens):
    """the inverse of cells()"""
    if type_id == VARCHAR:
        return KeyCol(VARCHAR, [None if v is None else v.decode("utf-8") for v in tokens])
    nulls = np.array([v is None for v in tokens], dtype=np.uint8)
    raw = np.array([0 if v is None else v for v in tokens], dtype=_BITS[type_id])
    return KeyCol(type_id, raw.view(_NP[type_id]), nulls if nulls.any() else None)


def take_or_null(col, idx):
    """take() where a negative index gives a NULL cell (the outer side of a join)"""
    idx = np.asarray(idx, dtype=np.int64)
    miss = idx < 0
    safe = np.where(miss, 0, idx)
    if col.type == VARCHAR:
        return KeyCol(VARCHAR, [None if m else col.values[i] for i, m in zip(safe.tolist(), miss.tolist())])
    if col.n == 0:
        return KeyCol(col.type, np.zeros(len(idx), dtype=_NP[col.type]), np.ones(len(idx), dtype=np.uint8))
    nulls = miss.astype(np.uint8) if col.nulls is None else (miss | (col.nulls[safe] != 0)).astype(np.uint8)
    return KeyCol(col.type, col.values[safe], nulls)


def same_bits(got, want):
    """two columns hold the same cells: equal null flags and, where not null, equal bits (what lies under a NULL is ignored)"""
    got = got if isinstance(got, KeyCol) else from_block(got)
    want = want if isinstance(want, KeyCol) else from_block(want)
    if got.type != want.type or got.n != want.n:
        return False
    if got.type == VARCHAR:
        return got.values == want.values
    gn = np.zeros(got.n, dtype=bool) if got.nulls is None else got.nulls != 0
    wn = np.zeros(want.n, dtype=bool) if want.nulls is None else want.nulls != 0
    live = ~wn
    return bool(np.array_equal(gn, wn) and np.array_equal(got.values.view(_BITS[got.type])[live], want.values.view(_BITS[want.type])[live]))


def first_row_keys(cols, gids):
    """the key cells every group puts out: those of the first row that got the id (DoubleType.appendTo copies the long)"""
    gids = np.asarray(gids)
    uniq, first = np.unique(gids, return_index=True)
    assert list(uniq) == list(range(len(uniq)))
    rows = row_tokens(cols)
    return [rows[int(r)] for r in first]


# ---- groupings: the two wrong ones (tripwires) and, for the family checks, the right one restated -------------------------------------------
def is_nan_bits(b):
    return (b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000


def _group(keys):
    ids, seen = np.zeros(len(keys), dtype=np.int64), {}
    for i, k in enumerate(keys):
        ids[i] = seen.setdefault(k, len(seen))
    return ids


def _raw_rows(cols):
    """per row the tuple of (null flag, raw bits) -- the bits UNDER a null cell included"""
    out = []
    for c in cols:
        if c.type == VARCHAR:
            out.append([(v is None, b"" if v is None else v.encode()) for v in c.values])
        else:
            raw = c.values.view(_BITS[c.type]).tolist()
            nl = [0] * c.n if c.nulls is None else c.nulls.tolist()
            out.append(list(zip(nl, raw)))
    return list(zip(*out))


def _semantic_rows(cols, nan_token, null_token):
    """per row the tuple of tokens under a chosen semantics: nan_token(row) / null_token(row) give what a NaN / NULL cell compares as"""
    out = []
    for c in cols:
        toks = cells(c)
        if c.type == DOUBLE:
            toks = [v if v is None else (nan_token(i) if is_nan_bits(v) else (0 if v == NEG_ZERO else v)) for i, v in enumerate(toks)]
        out.append([null_token(i) if v is None else v for i, v in enumerate(toks)])
    return list(zip(*out))


def group_ids_bitwise(cols):
    """WRONG on purpose: rows are one group when their bytes are -- NaN payloads, zero signs and the bytes under a NULL all tell rows apart"""
    return _group(_raw_rows(cols))


def group_ids_ieee(cols):
    """WRONG on purpose: rows are one group when `=` holds -- -0.0 = +0.0, but a NaN equals nothing and neither does a NULL"""
    return _group(_semantic_rows(cols, lambda i: ("nan", i), lambda i: ("null", i)))


def group_ids_not_distinct(cols):
    """the reference semantics restated (the tests compare with the oracle, this one only cross-checks the generators)"""
    return _group(_semantic_rows(cols, lambda i: "nan", lambda i: "null"))


def _pairs(build_rows, probe_rows):
    """(probe, build) pairs of rows with equal tokens, probe ascending, newest build row first (the order of a PagesHash chain)"""
    where = {}
    for j, k in enumerate(build_rows):
        if k is not None:
            where.setdefault(k, []).append(j)
    return [(i, j) for i, k in enumerate(probe_rows) if k is not None for j in reversed(where.get(k, []))]


def join_pairs_bitwise(build, probe):
    """WRONG on purpose: keys match when their cells' bytes do, null flag and the bytes under it included (-0.0 misses +0.0, a NaN finds
    its own payload, a NULL finds a NULL over the same bytes)"""
    return _pairs(_raw_rows(build), _raw_rows(probe))


def join_pairs_not_distinct(build, probe):
    """WRONG on purpose: the grouping semantics in a join (NaN matches NaN, NULL matches NULL)"""
    return _pairs(_semantic_rows(build, lambda i: "nan", lambda i: "null"), _semantic_rows(probe, lambda i: "nan", lambda i: "null"))


def join_pairs_equal(build, probe):
    """the reference semantics restated (cross-check of the generators only)"""
    def rows(cols):
        sem = _semantic_rows(cols, lambda i: None, lambda i: None)
        return [None if any(v is None for v in r) else r for r in sem]
    return _pairs(rows(build), rows(probe))


# ---- input families of test_gpu_key_types.py (the CPU file checks each of them against the tripwires) ---------------------------------------
def _seed(name, salt):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 7919 + salt) % 2**31


GBH_PAGE_ROWS = (1, 257, 20_000, 3)


def group_by_hash_pages(schema):
    """(a): pages of 1, 257, 20 000 and 3 rows; the first zero is -0.0 and the first NaN 0xfff8...01 (page 0 is that zero alone, the NaN
    opens its group in page 1)"""
    rng = np.random.default_rng(_seed(schema, 1))
    types = KEY_SCHEMAS[schema]
    return [key_page(rng, types, n, SCHEMA_DOMAINS[schema], first_zero="neg", first_nan_canonical=False) for n in GBH_PAGE_ROWS]


AGG_SCHEMAS = ["DOUBLE", "BOOLEAN", "DOUBLE_BIGINT", "VARCHAR_DOUBLE_BOOLEAN_DATE"]


def aggregation_pages(schema):
    """(b): four pages of keys + (BIGINT value, integer-valued DOUBLE value, both with nulls); this family starts with +0.0"""
    rng = np.random.default_rng(_seed(schema, 2))
    types = KEY_SCHEMAS[schema]
    pages = []
    for n in (3000, 1, 5000, 700):
        keys = key_page(rng, types, n, SCHEMA_DOMAINS[schema], first_zero="pos", first_nan_canonical=False)
        vals = [KeyCol(BIGINT, rng.integers(-10**6, 10**6, n), (rng.random(n) < 0.1).astype(np.uint8)),
                KeyCol(DOUBLE, rng.integers(-1000, 1000, n).astype(np.float64), (rng.random(n) < 0.1).astype(np.uint8))]
        pages.append(keys + vals)
    return pages


# (c) the fused aggregation: group-count tiers around FG_REG_GROUPS (4), FG_LDS_GROUPS = the one-pass limit (16) and the one-byte ids (256)
FUSED_TIERS = (4, 5, 16, 17, 300)
FUSED_PAGES, FUSED_PAGE_ROWS, FUSED_LATE_PAGE = 12, 9000, 6


def fused_tiers(schema):
    """the group counts a schema runs at: BOOLEAN alone reaches false / true / NULL only"""
    return [3] if schema == "BOOLEAN" else list(FUSED_TIERS)


def fused_tier_is_staggered(tier):
    """a tier just above the one-pass limit (17 groups = 14 early + 3 late) must not settle BELOW the limit first, or one-pass launches over
    its 14 early groups would be legitimate: page 0 holds 9 of the early groups and each page up to the late one opens one more, so no two
    consecutive pages are without a new group until all 17 exist"""
    return tier > 16 and tier - 3 <= 16


# a cell of a group descriptor: k >= 0 = the channel's k-th ordinary value (DOUBLE: 0 = the ZERO group value), or one of
_NAN, _NULL = -1, -2


def _fused_radix(types, count):
    """values per channel of the early groups' product: BOOLEAN has two, the others as many as make the product reach `count`"""
    wide = sum(1 for t in types if t != BOOLEAN)
    r = 2
    while (r ** wide) * (2 ** (len(types) - wide)) < count:
        r += 1
    return [2 if t == BOOLEAN else r for t in types]


def fused_groups(schema, tier):
    """-> (descriptors of the early groups in first-seen order, late "a", late "null", late "b"); a descriptor = one cell code per channel.
    The groups are a PRODUCT over the channels, not a function of one index, so that groups differ in exactly one channel while every
    other channel's value and null flag are equal -- a comparator that ignores one field's value merges them:
      early   g0 = (0, ..., 0) (a DOUBLE channel: the zero); then g0 with ONE channel at its value 1, the last channel first (with g0 these
              are the groups of the register signatures: ids 0..3); from 16 groups on g0 with one channel NULL, for every channel but the late
              NULL group's; then the product's remaining tuples, last channel fastest
      "a"     g0 with its DOUBLE channel NaN (NaN against zero, nothing else differs); no DOUBLE channel: g0 with a new value in one channel
              (the last one that no early group varies alone, if there is one)
      "b"     g0 with a new value in ONE other channel (the last one that no early group and not "a" already varies alone, if there is one)
      "null"  g0 with one channel NULL; which one rotates with the tier over ALL channels, VARCHAR included (from 16 groups on, where the
              early NULL groups cover the other channels)
    With g groups, one of them the NULL group, at most g - 2 pairs can differ in one channel's value alone, each in another channel (such
    pairs form a tree over the g - 1 others: a cycle would use a channel twice): 4 groups cover two channels, 5 groups three."""
    types = KEY_SCHEMAS[schema]
    nk = len(types)
    if schema == "BOOLEAN":
        return [(0,), (1,)], None, (_NULL,), None
    n_early = tier - 3
    null_channel = tier % nk
    if tier < 16 and types[null_channel] == VARCHAR:      # below 16 groups this is the stream's only NULL: it must lie over bytes, or grouping
        null_channel = next(c for c in range(nk) if types[c] != VARCHAR)                                   # by raw bits would pass
    g0 = (0,) * nk
    bump = lambda c, v: g0[:c] + (v,) + g0[c + 1:]
    early = [g0]
    for c in reversed(range(nk)):
        if len(early) < n_early:
            early.append(bump(c, 1))
    if tier >= 16:
        early += [bump(c, _NULL) for c in range(nk) if c != null_channel][: max(0, n_early - len(early))]
    radix = _fused_radix(types, n_early)
    idx = 0
    while len(early) < n_early:
        t, rest = [], idx
        for c in reversed(range(nk)):
            t.append(rest % radix[c])
            rest //= radix[c]
        t = tuple(reversed(t))
        if t not in early:
            early.append(t)
        idx += 1
    alone = {c for c in range(nk) if bump(c, 1) in early}                  # channels that an early group varies alone
    fresh = lambda c: None if types[c] == BOOLEAN and c in alone else (1 if types[c] == BOOLEAN else max(radix[c], 2))
    usable = [c for c in reversed(range(nk)) if fresh(c) is not None]
    a_channel = types.index(DOUBLE) if DOUBLE in types else ([c for c in usable if c not in alone] + usable)[0]
    a = bump(a_channel, _NAN if DOUBLE in types else fresh(a_channel))
    order = [c for c in reversed(range(nk)) if c not in alone and c != a_channel] + [c for c in reversed(range(nk)) if c != a_channel] + [a_channel]
    b_channel = next(c for c in order if fresh(c) is not None and not (c == a_channel and types[c] == BOOLEAN))
    b = bump(b_channel, fresh(b_channel) + (1 if b_channel == a_channel and DOUBLE not in types else 0))
    return early, a, bump(null_channel, _NULL), b


def fused_aggregation_pages(schema, tier):
    """(c): twelve pages of 9000 rows: [keys..., filter column (BIGINT; the filter keeps > 1: about 80 %), BIGINT value, DOUBLE value].
    The group count is fixed by construction: the `tier - 3` early groups of fused_groups() from page 0 on (rows 2.. of every page hold
    them once each, in order, in rows the filter keeps; the other rows draw from them), and on the late page (FUSED_LATE_PAGE, from its
    middle on) the three late ones.  A zero cell's sign alternates by row, a NaN cell's payload rotates by row, a NULL cell lies over
    other bytes in every row.  (BOOLEAN alone: false / true, only the NULL group is new.  Tier 17: see fused_tier_is_staggered.)
    In page 0, rows 0 and 1 are rows the filter REJECTS: they belong to g0 and to "a", and DOUBLE channels hold +0.0 and the canonical NaN
    there.  Every zero group is then opened by -0.0 and the NaN group by the late page's 0xfff8...01: a rejected row must not lend its bits."""
    rng = np.random.default_rng(_seed(schema, 3) + tier)
    types = KEY_SCHEMAS[schema]
    n = FUSED_PAGE_ROWS
    early, a, null, b = fused_groups(schema, tier)
    table = np.array(early + [g for g in (a, null, b) if g is not None], dtype=np.int64)
    code = {"a": len(early), "null": len(early) + (1 if a is not None else 0), "b": len(early) + 2}
    base = len(early)
    pages = []
    staggered = fused_tier_is_staggered(tier)
    for p in range(FUSED_PAGES):
        avail = base - max(0, FUSED_LATE_PAGE - 1 - p) if staggered else base
        sel = rng.integers(0, avail, n)
        keep = rng.integers(0, 10, n).astype(np.int64)
        sel[2:2 + avail], keep[2:2 + avail] = np.arange(avail), 9
        if p == FUSED_LATE_PAGE:
            late = {n // 2: "a", n // 2 + 7: "null", n // 2 + 11: "b", n // 2 + 300: "null", n // 2 + 301: "a", n // 2 + 302: "b", n // 2 + 303: "a"}
            for r, what in late.items():
                if a is not None or what == "null":
                    sel[r], keep[r] = code[what], 5
        if p == 0:
            keep[:2] = [0, 1]
            sel[0], sel[1] = 0, (code["a"] if a is not None else 1)
        cols = [_fused_channel(t, ci, table[sel, ci], p == 0, 2 + avail) for ci, t in enumerate(types)]
        vals = [KeyCol(BIGINT, keep), KeyCol(BIGINT, rng.integers(-10**6, 10**6, n), (rng.random(n) < 0.1).astype(np.uint8)),
                KeyCol(DOUBLE, rng.integers(-1000, 1000, n).astype(np.float64), (rng.random(n) < 0.1).astype(np.uint8))]
        pages.append(cols + vals)
    return pages


def _fused_channel(t, ci, codes, first_page, forced_end):
    """the cells of one channel from the rows' cell codes"""
    n = len(codes)
    rows = np.arange(n)
    nulls = (codes == _NULL).astype(np.uint8)
    k = np.where(codes < 0, 0, codes)
    sign = 1 if ci % 2 == 0 else -1
    if t == VARCHAR:
        return KeyCol(VARCHAR, [None if c == _NULL else VARCHAR_VOCABULARY[c + ci] for c in codes.tolist()])
    if t == DOUBLE:
        bits = (k * float(sign)).astype(np.float64).view(np.uint64).copy()
        zero = codes == 0
        opens = (rows < forced_end) | ((rows >= n // 2) & (rows < n // 2 + 16))                # rows that may open a group: -0.0
        bits[zero] = np.where(opens[zero] | (rows[zero] % 2 == 0), np.uint64(NEG_ZERO), np.uint64(POS_ZERO))
        nan = codes == _NAN
        bits[nan] = np.array(NAN_BITS, dtype=np.uint64)[(rows[nan] - n // 2 + 1) % 4]       # the late page's first NaN row: 0xfff8...01
        if first_page:
            bits[0] = POS_ZERO                                                             # rows the filter rejects
            if nan[1]:
                bits[1] = NAN_CANONICAL
        bits[nulls != 0] = 0x1234 + rows[nulls != 0].astype(np.uint64)                     # what lies under a NULL must not matter
        return KeyCol(DOUBLE, bits.view(np.float64), nulls if nulls.any() else None)
    if t == BOOLEAN:
        v = k.astype(np.uint8)
        v[nulls != 0] = rows[nulls != 0] % 2
    else:
        off = {BIGINT: -2, INTEGER: -3, DATE: 9000}[t]
        v = (k * sign + off).astype(_NP[t])
        v[nulls != 0] = (rows[nulls != 0] % 251).astype(_NP[t])
    return KeyCol(t, v, nulls if nulls.any() else None)


def drop_channel_values(cols, ci):
    """the columns with channel ci's VALUES replaced by one constant, its null flags kept: what a comparator sees that ignores the field"""
    c = cols[ci]
    if c.type == VARCHAR:
        flat = KeyCol(VARCHAR, [None if v is None else "x" for v in c.values])
    else:
        flat = KeyCol(c.type, np.zeros(c.n, dtype=_NP[c.type]), c.nulls)
    return cols[:ci] + [flat] + cols[ci + 1:]


JOIN_SCHEMAS = {"DOUBLE": [DOUBLE], "DOUBLE_VARCHAR": [DOUBLE, VARCHAR], "BOOLEAN": [BOOLEAN], "DATE": [DATE]}
JOIN_DOMAINS = {"DOUBLE": [(-30, 30)], "DOUBLE_VARCHAR": [(-3, 4), (0, 6)], "BOOLEAN": [None], "DATE": [(9000, 9200)]}
JOIN_BUILD_ROWS, JOIN_PROBE_ROWS, MAX_NAN_BUILD_ROWS = (700, 1, 1500), 5000, 48


def join_inputs(schema):
    """(d): -> (build pages, probe page), each page = key channels + a BIGINT row number.  The build side starts with -0.0, the probe side
    with +0.0.  NaN build rows all hash alike and never share a slot, so each lengthens one probe sequence: at most MAX_NAN_BUILD_ROWS."""
    rng = np.random.default_rng(_seed(schema, 4))
    types, domains = JOIN_SCHEMAS[schema], JOIN_DOMAINS[schema]
    build, at = [], 0
    for n in JOIN_BUILD_ROWS:
        keys = key_page(rng, types, n, domains, 0.03, first_zero="neg", first_nan_canonical=False, slots=40)
        build.append(keys + [KeyCol(BIGINT, np.arange(at, at + n))])
        at += n
    probe = key_page(rng, types, JOIN_PROBE_ROWS, domains, 0.03, first_zero="pos", first_nan_canonical=True) + [KeyCol(BIGINT, np.arange(JOIN_PROBE_ROWS))]
    nan_rows = 0
    for c in concat_pages(build)[:len(types)]:
        if c.type == DOUBLE:
            nan_rows += int(np.isnan(c.values).sum())
    assert nan_rows <= MAX_NAN_BUILD_ROWS, nan_rows
    return build, probe


def partition_input(n=20_000):
    """(e): [BIGINT, DOUBLE with specials, VARCHAR payload]; the partition channels are 0 and 1 or 1 alone"""
    rng = np.random.default_rng(_seed("partition", 5))
    return [key_col(rng, BIGINT, n, (0, 3), 0.03), key_col(rng, DOUBLE, n, (-5, 5), 0.05, first_zero="neg", first_nan_canonical=False),
            key_col(rng, VARCHAR, n, (0, 8), 0.05)]

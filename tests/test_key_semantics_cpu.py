"""The yardstick of test_gpu_key_types.py, checked without a GPU: the oracle's two notions of key equality pinned on a hand-written vector,
and every input family of the GPU file shown to SEPARATE the reference semantics from the two wrong ones of key_cases.py (by raw bits;
with `=`).  An input that does not is a defect of the test: a kernel with that bug would pass it."""
import numpy as np
import pytest

import key_cases as kc


def _ocols(oracle, cols):
    return [kc.to_ocol(oracle, c) for c in cols]


def _has_null(col):
    return any(v is None for v in col.values) if col.type == kc.VARCHAR else bool(col.nulls is not None and col.nulls.any())


def _oracle_ids(oracle, types, cols):
    g = oracle.MultiChannelGroupByHash(types, 16)
    return g.get_group_ids(_ocols(oracle, cols)), g


def test_oracle_pinned_on_the_hand_written_vector(oracle):
    """-0.0, +0.0, NaN (negative, payload 1), 1.0, the canonical NaN, a signalling NaN, +0.0, -0.0"""
    bits = [0x8000000000000000, 0x0000000000000000, 0xFFF8000000000001, 0x3FF0000000000000, 0x7FF8000000000000, 0x7FF0000000000001,
            0x0000000000000000, 0x8000000000000000]
    col = oracle.Col(oracle.DOUBLE, kc.bits_to_doubles(bits))
    g = oracle.MultiChannelGroupByHash([oracle.DOUBLE], 10)
    assert g.get_group_ids([col]).tolist() == [0, 0, 1, 2, 1, 1, 0, 0]
    assert g.group_rows()[0].tolist() == [0, 2, 3]
    assert kc.first_row_keys([col], [0, 0, 1, 2, 1, 1, 0, 0]) == [(0x8000000000000000,), (0xFFF8000000000001,), (0x3FF0000000000000,)]
    ph = oracle.PagesHash([col])
    probe = oracle.Col(oracle.DOUBLE, kc.bits_to_doubles([0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0x3FF0000000000000]))
    op, ob = ph.probe([probe])
    assert list(zip(op.tolist(), ob.tolist())) == [(0, 7), (0, 6), (0, 1), (0, 0), (1, 7), (1, 6), (1, 1), (1, 0), (3, 3)]
    assert ph.link_count == 3
    op, ob = ph.probe([probe], probe_outer=True)
    assert list(zip(op.tolist(), ob.tolist())) == [(0, 7), (0, 6), (0, 1), (0, 0), (1, 7), (1, 6), (1, 1), (1, 0), (2, -1), (3, 3)]
    # the raw hash: -0.0 as +0.0, every NaN as the canonical one
    h = oracle.hash_rows([col])
    assert h[0] == h[1] == h[6] and h[2] == h[4] == h[5] and len({int(h[0]), int(h[2]), int(h[3])}) == 3


def test_special_doubles_holds_what_it_promises():
    for first_zero in ("neg", "pos"):
        for canonical in (False, True):
            v = kc.special_doubles(np.random.default_rng(3), 20_000, (1, 50), first_zero=first_zero, first_nan_canonical=canonical)
            again = kc.special_doubles(np.random.default_rng(4), 20_000, (1, 50), first_zero=first_zero, first_nan_canonical=canonical)
            bits = v.view(np.uint64)
            slots = kc.special_slots(20_000)
            assert np.array_equal(bits[slots], again.view(np.uint64)[slots])            # the specials do not depend on the draw
            have = set(bits.tolist())
            for b in kc.NAN_BITS + [kc.NEG_ZERO, kc.POS_ZERO, kc.POS_INF, kc.NEG_INF, kc.DENORMAL, kc.NEG_DENORMAL]:
                assert b in have, hex(b)
            zeros = bits[(bits == kc.NEG_ZERO) | (bits == kc.POS_ZERO)]
            assert zeros[0] == (kc.NEG_ZERO if first_zero == "neg" else kc.POS_ZERO) and zeros[1] != zeros[0]
            nans = bits[np.isnan(v)]
            assert (nans[0] == kc.NAN_CANONICAL) == canonical and len(set(nans.tolist())) == 4
            assert kc.NAN_NEVER_INSERTED not in have
    assert kc.special_doubles(np.random.default_rng(0), 1, (0, 9)).view(np.uint64)[0] == kc.NEG_ZERO
    assert len(kc.special_doubles(np.random.default_rng(0), 0, (0, 9))) == 0


def test_varchar_vocabulary_holds_the_edge_values():
    v = kc.VARCHAR_VOCABULARY
    assert "" in v and "a" in v and "ab" in v and "ac" in v and any(len(x.encode()) > 16 for x in v) and len(set(v)) == len(v)


def _assert_first_row_bits_matter(cols, ids, ci, first_zero, first_nan):
    """channel ci has a zero group opened by `first_zero` that also holds the other sign, and a NaN group opened by `first_nan` that also
    holds other payloads: a path that puts out canonical bits, or those of a later row, is caught by the output-key check"""
    toks = kc.cells(cols[ci])
    members = {}
    for g, v in zip(np.asarray(ids).tolist(), toks):
        members.setdefault(g, []).append(v)
    firsts = {g: m[0] for g, m in members.items()}
    other_zero = kc.POS_ZERO if first_zero == kc.NEG_ZERO else kc.NEG_ZERO
    assert any(f == first_zero and other_zero in members[g] for g, f in firsts.items())
    assert any(f is not None and kc.is_nan_bits(f) and f != kc.NAN_CANONICAL and len(set(members[g])) > 1 for g, f in firsts.items())
    if len(cols) == 1:
        assert first_nan in firsts.values() and other_zero not in firsts.values() and sum(1 for f in firsts.values() if f is not None and kc.is_nan_bits(f)) == 1


def _assert_grouping_separates(oracle, types, cols, what):
    ids, g = _oracle_ids(oracle, types, cols)
    assert np.array_equal(ids, kc.group_ids_not_distinct(cols)), what          # the generators' own restatement agrees with the oracle
    assert not np.array_equal(ids, kc.group_ids_bitwise(cols)), what + ": grouping by raw bits would pass"
    assert not np.array_equal(ids, kc.group_ids_ieee(cols)), what + ": grouping with `=` would pass"
    return ids, g


@pytest.mark.parametrize("schema", list(kc.KEY_SCHEMAS))
def test_group_by_hash_family_separates_the_semantics(oracle, schema):
    types = kc.KEY_SCHEMAS[schema]
    cols = kc.concat_pages(kc.group_by_hash_pages(schema))
    ids, g = _assert_grouping_separates(oracle, types, cols, schema)
    assert len(kc.first_row_keys(cols, ids)) == g.group_count
    for ci, t in enumerate(types):
        if t == kc.DOUBLE:     # the output-key check means something: the zero group opens with -0.0, the NaN group with a non-canonical NaN
            _assert_first_row_bits_matter(cols, ids, ci, kc.NEG_ZERO, kc.NAN_BITS[1])


@pytest.mark.parametrize("schema", kc.AGG_SCHEMAS)
def test_aggregation_family_separates_the_semantics(oracle, schema):
    nk = len(kc.KEY_SCHEMAS[schema])
    cols = kc.concat_pages(kc.aggregation_pages(schema))[:nk]
    ids, g = _assert_grouping_separates(oracle, kc.KEY_SCHEMAS[schema], cols, schema)
    for ci, t in enumerate(kc.KEY_SCHEMAS[schema]):
        if t == kc.DOUBLE:
            _assert_first_row_bits_matter(cols, ids, ci, kc.POS_ZERO, kc.NAN_BITS[1])     # this family opens the zero group with +0.0


@pytest.mark.parametrize("schema", list(kc.KEY_SCHEMAS))
def test_fused_aggregation_family_separates_the_semantics_and_hits_its_tier(oracle, schema):
    types = kc.KEY_SCHEMAS[schema]
    nk = len(types)
    for tier in kc.fused_tiers(schema):
        pages = kc.fused_aggregation_pages(schema, tier)
        assert len(pages) == 12 and all(pg[0].n == 9000 for pg in pages)
        cols = kc.concat_pages(pages)
        keep = np.nonzero(cols[nk].values > 1)[0]
        assert 0.75 < len(keep) / cols[0].n < 0.85                          # the filter rejects about 20 %
        kept = [kc.take(c, keep) for c in cols[:nk]]
        ids, g = _assert_grouping_separates(oracle, types, kept, "%s / %d" % (schema, tier))
        assert g.group_count == tier
        # the late page opens three groups (BOOLEAN alone: one); before it the group set is complete from the first page on
        before = sum(pg[0].n for pg in pages[:kc.FUSED_LATE_PAGE])
        early = int(ids[: int((keep < before).sum())].max()) + 1
        assert tier - early == (1 if schema == "BOOLEAN" else 3)
        per_page = [int(ids[: int((keep < 9000 * (p + 1)).sum())].max()) + 1 for p in range(12)]       # groups after every page
        if kc.fused_tier_is_staggered(tier):
            # just above the one-pass limit: every page up to the late one opens a group, the stream never settles below the limit
            assert all(b > a for a, b in zip(per_page[:kc.FUSED_LATE_PAGE], per_page[1:kc.FUSED_LATE_PAGE + 1]))
        else:
            assert per_page[0] == early                                    # two clean pages follow at once
        assert per_page[kc.FUSED_LATE_PAGE] == per_page[-1] == tier and (tier > 16) == (tier in (17, 300))
        # a comparator that ignores ONE field's value (a signature word dropped or mis-shifted, a per-field comparison skipped) merges groups:
        # for every channel some groups differ in that channel's value alone -- as far as the group count allows (fused_groups)
        if nk > 1:
            merged = [c for c in range(nk) if not np.array_equal(ids, _oracle_ids(oracle, types, kc.drop_channel_values(kept, c))[0])]
            if tier - 2 >= nk:
                assert merged == list(range(nk)), (schema, tier, merged)
            else:
                assert len(merged) == tier - 2 and nk - 1 in merged, (schema, tier, merged)
            if kc.DOUBLE in types:
                assert types.index(kc.DOUBLE) in merged
            early_groups = kc.fused_groups(schema, tier)[0]
            star = [(0,) * nk] + [(0,) * c + (1,) + (0,) * (nk - 1 - c) for c in reversed(range(nk))]
            m = min(4, len(early_groups), len(star))
            assert early_groups[:m] == star[:m]       # ids 0..3, the register signatures: g0 and its last-field neighbours
            if tier >= 16:                                                    # a NULL in every channel, VARCHAR included: every mask bit
                assert all(_has_null(c) for c in kept)
        keys = kc.first_row_keys(kept, ids)
        for ci, t in enumerate(types):
            if t != kc.DOUBLE:
                continue
            # rows 0 and 1 of the stream, which the filter rejects, hold the first zero (+0.0) and the first NaN (canonical): the groups
            # are opened by later rows with other bits
            assert cols[ci].values.view(np.uint64)[0] == kc.POS_ZERO and cols[ci].values.view(np.uint64)[1] == kc.NAN_CANONICAL
            assert 0 not in keep and 1 not in keep
            col = [k[ci] for k in keys]
            assert kc.NEG_ZERO in col and kc.POS_ZERO not in col
            assert kc.NAN_BITS[1] in col and kc.NAN_CANONICAL not in col
            _assert_first_row_bits_matter(kept, ids, ci, kc.NEG_ZERO, kc.NAN_BITS[1])


@pytest.mark.parametrize("schema", list(kc.JOIN_SCHEMAS))
def test_join_family_separates_the_semantics(oracle, schema):
    nk = len(kc.JOIN_SCHEMAS[schema])
    build, probe = kc.join_inputs(schema)
    assert [pg[0].n for pg in build] == [700, 1, 1500] and probe[0].n == 5000
    bk, pk = kc.concat_pages(build)[:nk], probe[:nk]
    ph = oracle.PagesHash(_ocols(oracle, bk))
    op, ob = ph.probe(_ocols(oracle, pk))
    pairs = list(zip(op.tolist(), ob.tolist()))
    assert pairs == kc.join_pairs_equal(bk, pk)
    assert pairs != kc.join_pairs_bitwise(bk, pk), "matching by raw bits would pass"
    assert pairs != kc.join_pairs_not_distinct(bk, pk), "matching with IS NOT DISTINCT FROM would pass"
    if kc.DOUBLE in kc.JOIN_SCHEMAS[schema]:
        ci = kc.JOIN_SCHEMAS[schema].index(kc.DOUBLE)
        b_bits, p_bits = kc.cells(bk[ci]), kc.cells(pk[ci])
        assert any(p_bits[i] == kc.POS_ZERO and b_bits[j] == kc.NEG_ZERO for i, j in pairs)     # each side must put out its own bits
        assert any(p_bits[i] == kc.NEG_ZERO and b_bits[j] == kc.POS_ZERO for i, j in pairs)
        nan_rows = sum(1 for v in b_bits if v is not None and kc.is_nan_bits(v))
        assert 4 <= nan_rows <= kc.MAX_NAN_BUILD_ROWS


def test_partition_family_spreads_and_holds_the_specials(oracle):
    cols = kc.partition_input()
    bits = set(kc.cells(cols[1]))
    for b in kc.NAN_BITS + [kc.NEG_ZERO, kc.POS_ZERO, kc.POS_INF, kc.NEG_INF, kc.DENORMAL, kc.NEG_DENORMAL, None]:
        assert b in bits
    raw = oracle.hash_rows([kc.to_ocol(oracle, cols[1])])
    assert not np.array_equal(raw, oracle.hash_rows([oracle.Col(oracle.BIGINT, cols[1].values.view(np.int64), cols[1].nulls)]))   # not a hash of the raw bits
    # (small integers as doubles hash to words whose low bits are zero: alone, the channel spreads over a count like 7 only)
    assert len(set(oracle.partition_remote(raw, 7).tolist())) == 7
    both = oracle.hash_rows([kc.to_ocol(oracle, cols[0]), kc.to_ocol(oracle, cols[1])])
    for parts in (2, 7, 8):       # "every NaN lands in one partition" must not hold trivially
        assert len(set(oracle.partition_remote(both, parts).tolist())) > 1
    assert len(set(oracle.partition_local(both, 8).tolist())) > 1


def test_rand_block_special_argument_leaves_the_default_alone(pkg):
    from gpu_common import rand_block
    a = rand_block(pkg, np.random.default_rng(7), pkg.DOUBLE, 500, 0.1, (0, 30))
    b = rand_block(pkg, np.random.default_rng(7), pkg.DOUBLE, 500, 0.1, (0, 30), special=False)
    c = rand_block(pkg, np.random.default_rng(7), pkg.DOUBLE, 500, 0.1, (0, 30), special=True)
    want = np.random.default_rng(7)
    nulls = (want.random(500) < 0.1).astype(np.uint8)
    assert np.array_equal(a.values, want.integers(0, 30, 500).astype(np.float64)) and np.array_equal(a.nulls, nulls)
    assert np.array_equal(a.values.view(np.uint64), b.values.view(np.uint64))
    assert np.isnan(c.values).sum() >= 4 and np.array_equal(c.nulls, nulls)


def test_tripwires_and_bit_helpers_on_the_hand_written_vector():
    """the comparisons the GPU file relies on can fail: zero signs, NaN payloads and NULLs are told apart, bytes under a NULL are not"""
    bits = [kc.NEG_ZERO, kc.POS_ZERO, 0xFFF8000000000001, 0x3FF0000000000000, kc.NAN_CANONICAL, 0x7FF0000000000001, kc.POS_ZERO, kc.NEG_ZERO]
    col = kc.KeyCol(kc.DOUBLE, kc.bits_to_doubles(bits))
    assert kc.group_ids_not_distinct([col]).tolist() == [0, 0, 1, 2, 1, 1, 0, 0]
    assert kc.group_ids_bitwise([col]).tolist() == [0, 1, 2, 3, 4, 5, 1, 0]
    assert kc.group_ids_ieee([col]).tolist() == [0, 0, 1, 2, 3, 4, 0, 0]
    probe = kc.KeyCol(kc.DOUBLE, kc.bits_to_doubles([kc.POS_ZERO, kc.NEG_ZERO, kc.NAN_CANONICAL, 0x3FF0000000000000]))
    assert kc.join_pairs_equal([col], [probe]) == [(0, 7), (0, 6), (0, 1), (0, 0), (1, 7), (1, 6), (1, 1), (1, 0), (3, 3)]
    assert kc.join_pairs_bitwise([col], [probe]) == [(0, 6), (0, 1), (1, 7), (1, 0), (2, 4), (3, 3)]
    assert (2, 5) in kc.join_pairs_not_distinct([col], [probe]) and (2, 4) in kc.join_pairs_not_distinct([col], [probe])
    assert kc.cells(col) == bits and kc.first_row_keys([col], [0, 0, 1, 2, 1, 1, 0, 0])[1] == (0xFFF8000000000001,)
    # same_bits
    other = kc.KeyCol(kc.DOUBLE, kc.bits_to_doubles([kc.POS_ZERO] + bits[1:]))
    assert kc.same_bits(col, col) and not kc.same_bits(col, other)                                   # -0.0 is not +0.0 here
    assert not kc.same_bits(col, kc.KeyCol(kc.DOUBLE, kc.bits_to_doubles(bits[:2] + [kc.NAN_CANONICAL] + bits[3:])))   # nor one NaN another
    nulls = np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint8)
    assert kc.same_bits(kc.KeyCol(kc.DOUBLE, col.values, nulls), kc.KeyCol(kc.DOUBLE, other.values, nulls))          # bytes under a NULL
    assert not kc.same_bits(kc.KeyCol(kc.DOUBLE, col.values, nulls), col)
    assert not kc.same_bits(kc.KeyCol(kc.VARCHAR, ["a", None]), kc.KeyCol(kc.VARCHAR, ["a", ""]))
    assert not kc.same_bits(kc.KeyCol(kc.INTEGER, [1, 2]), kc.KeyCol(kc.DATE, [1, 2])) and not kc.same_bits(kc.KeyCol(kc.INTEGER, [1]), kc.KeyCol(kc.INTEGER, [1, 2]))
    # block_bits, col_from_tokens, take_or_null
    nl, live = kc.block_bits(kc.KeyCol(kc.DOUBLE, col.values, nulls))
    assert nl.tolist() == [True] + [False] * 7 and live.dtype == np.uint64 and live.tolist() == bits[1:]
    assert kc.block_bits(kc.KeyCol(kc.VARCHAR, ["ab", None, ""])) [1] == [b"ab", b""]
    assert kc.block_bits(kc.KeyCol(kc.INTEGER, [-1, 5]))[1].dtype == np.int32 and kc.block_bits(kc.KeyCol(kc.BOOLEAN, [1, 0]))[1].dtype == np.uint8
    for t, toks in ((kc.DOUBLE, [kc.NEG_ZERO, None, 0x7FF8000000000123]), (kc.INTEGER, [-3, None, 7]), (kc.BOOLEAN, [1, 0, None]), (kc.VARCHAR, [b"", None, b"ac"])):
        assert kc.cells(kc.col_from_tokens(t, toks)) == toks
    got = kc.take_or_null(kc.KeyCol(kc.DOUBLE, col.values, nulls), [1, -1, 0, 7])
    assert kc.cells(got) == [kc.POS_ZERO, None, None, kc.NEG_ZERO]
    assert kc.cells(kc.take_or_null(kc.KeyCol(kc.VARCHAR, ["x", None]), [-1, 0, 1])) == [None, b"x", None]

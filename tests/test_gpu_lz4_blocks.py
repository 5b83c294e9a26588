"""-m gpu: lz4_decode_kernel (csrc/serde.hip) on LZ4 blocks written sequence by sequence -- a list of (literals, offset, match length) encoded as
given, with no searching -- so that every overlap period against the kernel's 64-lane chunks, every length-extension chain and the wrap of its
128 KB LDS window are reached on purpose, not by what a greedy compressor happens to emit.  The blocks are the payloads of compressed
SerializedPages of one BIGINT column (like test_deserialize_lz4_compressed_pages): the page's rows are compared.  Then the malformed blocks, each
refused with code -1 by a guard of the kernel that is named beside it."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WINDOW = 128 * 1024


def length_bytes(extra):
    """the bytes behind a token nibble of 15: `extra` = length - 15 as 255s and a last byte below 255"""
    return bytes([255] * (extra // 255) + [extra % 255])


def lz4_block(sequences, last_literals=b""):
    """[(literals, offset, match length >= 4)] + the literals of the last record -> a block, exactly as given"""
    out = bytearray()
    for lit, offset, ml in sequences:
        out.append((min(len(lit), 15) << 4) | min(ml - 4, 15))
        if len(lit) >= 15:
            out += length_bytes(len(lit) - 15)
        out += lit
        out += offset.to_bytes(2, "little")
        if ml - 4 >= 15:
            out += length_bytes(ml - 4 - 15)
    out.append(min(len(last_literals), 15) << 4)
    if len(last_literals) >= 15:
        out += length_bytes(len(last_literals) - 15)
    return bytes(out + last_literals)


def inflate(sequences, last_literals=b""):
    """what the sequences say, byte by byte"""
    out = bytearray()
    for lit, offset, ml in sequences:
        out += lit
        assert 0 < offset <= len(out)
        for _ in range(ml):
            out.append(out[-offset])
    return bytes(out + last_literals)


def lits(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def header_of(oracle, n):
    """the bytes in front of the values in the payload of a page of one BIGINT block without nulls (their number does not depend on n)"""
    return oracle.serialize_page([oracle.Col(oracle.BIGINT, np.zeros(n, dtype=np.int64))])[13:][:-8 * n]


def page_of(oracle, sequences, last_literals, rng):
    """(compressed SerializedPage, its rows) whose payload is the block of `sequences`: the first literals get the header of a BIGINT block in
    front, the last ones are padded to whole values"""
    def with_head(head, pad):
        if not sequences:
            return [], head + last_literals + pad
        lit0, off0, ml0 = sequences[0]
        return [(head + lit0, off0, ml0)] + list(sequences[1:]), last_literals + pad
    h = len(header_of(oracle, 1))
    data_len = len(inflate(*with_head(bytes(h), b""))) - h
    pad = lits(rng, -data_len % 8)
    n = (data_len + len(pad)) // 8
    head = header_of(oracle, n)
    assert len(head) == h and n > 0
    seqs, last = with_head(head, pad)
    payload, block = inflate(seqs, last), lz4_block(seqs, last)
    assert oracle.lz4_block_decompress(block, len(payload)) == payload      # the writer, against the oracle's decompressor
    rows = np.frombuffer(payload[h:], dtype="<i8")
    page = n.to_bytes(4, "little") + bytes([1]) + len(payload).to_bytes(4, "little") + len(block).to_bytes(4, "little") + block
    return page, rows


def blocks(rng, h):
    """name -> (sequences, last literals); h = the bytes page_of puts in front of the first literals"""
    out = {}
    # every offset 1..70 with match lengths 4, 63, 64, 65, 200: overlapping copies at every period against the 64-lane chunk
    for ml in (4, 63, 64, 65, 200):
        out["offsets_1_to_70_match_%d" % ml] = ([(lits(rng, 80), 1, ml)] + [(lits(rng, 3), off, ml) for off in range(2, 71)], lits(rng, 5))
    # offsets at the format's limit
    out["offsets_65535_and_65472"] = ([(lits(rng, 66_000), 65_535, 100), (lits(rng, 7), 65_536 - 64, 64), (b"", 65_535, 65), (lits(rng, 1), 65_536 - 64, 200)], lits(rng, 9))
    # literal and match lengths around the extension bytes: 14 (none), 15 (one byte 0), 15 + 254, 15 + 255 (255, 0), 15 + 255 + 255 + 3
    edge = (14, 15, 15 + 254, 15 + 255, 15 + 255 + 255 + 3)
    out["length_extension_chains"] = ([(lits(rng, max(l, 4)) if i else lits(rng, 600), 1 + (i * 37 + j * 11) % 590, m + 4) for i, l in enumerate(edge) for j, m in enumerate(edge)] +
                                       [(lits(rng, l), 3, 4) for l in edge], lits(rng, 15 + 255))
    out["only_literals"] = ([], lits(rng, 5000))
    out["last_record_without_literals"] = ([(lits(rng, 40), 7, 30), (lits(rng, 2), 40, 9)], b"")
    # more than two windows of output; matches that are written across the wrap, and matches that read across it
    # at k * WINDOW - 100: a match of 300 bytes written across the wrap, then one that reads 250 bytes back across it, one of exactly a chunk, a run
    seqs, at = [], h
    for k in (1, 2):
        fill = k * WINDOW - 100 - at
        seqs += [(lits(rng, fill), 5000, 300), (lits(rng, 3), 250, 200), (b"", 64, 130), (lits(rng, 1), 1, 70)]
        at += fill + 300 + 3 + 200 + 130 + 1 + 70
    out["output_crosses_the_window_twice"] = (seqs, lits(rng, 3000))
    return out


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def test_sequence_level_blocks_inflate_to_their_rows(pkg, ctx, oracle):
    rng = random.Random(31)
    for name, (sequences, last) in blocks(rng, len(header_of(oracle, 1))).items():
        page, rows = page_of(oracle, sequences, last, rng)
        if name == "output_crosses_the_window_twice":
            assert len(rows) * 8 > 2 * WINDOW
        got = ctx.deserialize_page(page, [pkg.BIGINT]).to_host().getBlock(0)
        assert got.nulls is None and np.array_equal(got.values, rows), name


def malformed(rng):
    """name -> (block, declared size, the guard of lz4_decode_kernel that refuses it)"""
    ok_head = [(lits(rng, 20), 5, 10)]
    whole = lz4_block(ok_head, lits(rng, 6))
    size = 20 + 10 + 6
    return {
        "ends_inside_a_literal_length_chain": (bytes([0xf0, 255, 255]), 600, "serde.hip:306 `if (ip >= src_len) bad`, in the literal-length loop"),
        "ends_inside_a_match_length_chain": (bytes([0x4f]) + lits(rng, 4) + bytes([2, 0, 255, 255]), 600, "serde.hip:328 `if (ip >= src_len) bad`, in the match-length loop"),
        "ends_between_the_literals_and_the_offset": (bytes([0x40]) + lits(rng, 4) + bytes([2]), 64, "serde.hip:321 `ip + 2 > src_len`"),
        "literal_run_past_the_end_of_the_source": (bytes([0xa0]) + lits(rng, 5), 64, "serde.hip:311 `ip + lit > src_len`"),
        "literal_run_past_the_declared_size": (lz4_block([], lits(rng, 40)), 39, "serde.hip:311 `op + lit > dst_len`"),
        "offset_0": (lz4_block([(lits(rng, 20), 0, 10)], lits(rng, 6)), size, "serde.hip:334 `offset == 0`"),
        "offset_one_beyond_the_output_so_far": (lz4_block([(lits(rng, 20), 21, 10)], lits(rng, 6)), size, "serde.hip:334 `offset > op`"),
        "match_past_the_declared_size": (lz4_block([(lits(rng, 20), 5, 10)]), 29, "serde.hip:334 `op + ml > dst_len`"),
        "ends_short_of_the_declared_size": (whole, size + 1, "serde.hip:348 `op != dst_len`"),
    }


def test_malformed_blocks_are_refused_by_a_guard_of_the_kernel(pkg, ctx, oracle):
    rng = random.Random(37)
    good = lz4_block([(lits(rng, 20), 5, 10)], lits(rng, 6))
    assert oracle.lz4_block_decompress(good, 36)      # the shape the cases below break is a block
    for name, (block, declared, guard) in malformed(rng).items():
        page = (1).to_bytes(4, "little") + bytes([1]) + declared.to_bytes(4, "little") + len(block).to_bytes(4, "little") + block
        with pytest.raises(pkg.TgpuError) as e:
            ctx.deserialize_page(page, [pkg.BIGINT])
        assert e.value.code == -1 and "LZ4" in str(e.value), (name, guard, str(e.value))

"""One seeded corpus of ORC / Parquet streams for both sides of the scan decoders:

  * tests/test_stream_walk_cpu.py feeds the base streams, their mutants, MALFORMED and ODD_BUT_LEGAL to the host walks of csrc/stream_walk.h
    (tests/stream_walk/walk_main.cpp under the host sanitizers);
  * tests/test_gpu_decode_fuzz.py decodes the WELL-FORMED ones (base streams, coverage streams, ODD_BUT_LEGAL) on the device, and passes the
    MALFORMED ones to the C ABI, which must refuse them on the host.  The mutants never go to a GPU.

A Stream knows where its header bytes, its varint fields and its width bytes are, so the mutants hit them one by one.  Everything is drawn from
random.Random(seed): the corpus does not change from run to run.
"""
import random
import struct

from oracle import orc as O
from oracle import parquet as P

M64 = (1 << 64) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
ORC_WIDTHS = list(range(1, 25)) + [26, 28, 30, 32, 40, 48, 56, 64]
VARINT_VALUES = (0, 1, 1 << 31, 1 << 32, 1 << 57, 1 << 61, 1 << 63, (1 << 64) - 1)
HEADER_BYTES = (0x00, 0x7f, 0x80, 0xff)
WIDTH_BYTES = (0, 1, 63, 64, 65, 255)
WALKERS = ("rle_v2", "rle_v1", "byte_rle", "hybrid", "delta", "byte_arrays")
MAX_CUTS = 64


def s64(u):
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def uleb(v):
    return P.uleb(v)


def uleb_end(data, at):
    while data[at] & 0x80:
        at += 1
    return at + 1


class Stream:
    """bytes + the walker's scalar arguments + where the mutable fields are: header = offsets of header bytes, varints = (start, end) of
    ULEB128 fields, le32 = offsets of 4-byte little-endian lengths, widths = offsets of width bytes"""

    def __init__(self, walker, data, name="", signed=False, bit_width=0, want=0, count=0, header=(), varints=(), le32=(), widths=(), total=None, meta=None):
        self.walker, self.data, self.name = walker, bytes(data), name
        self.signed, self.bit_width, self.want, self.count = bool(signed), bit_width, want, count
        self.header, self.varints, self.le32, self.widths = list(header), list(varints), list(le32), list(widths)
        self.total = total          # the number of values the encoder wrote (what the walker must report)
        self.meta = meta or {}

    def with_data(self, data, name, **over):
        s = Stream(self.walker, data, name, self.signed, self.bit_width, self.want, self.count, total=None)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def case_line(self):
        return "%s %d %d %d %d %s" % (self.walker, int(self.signed), self.bit_width, self.want, self.count, self.data.hex() or "-")


class Piece:
    def __init__(self, data, header=(), varints=(), n=0):
        self.data, self.header, self.varints, self.n = bytes(data), list(header), list(varints), n


def compose(walker, pieces, name, **kw):
    data, header, varints, at, n = bytearray(), [], [], 0, 0
    for p in pieces:
        header += [at + h for h in p.header]
        varints += [(at + a, at + b) for a, b in p.varints]
        data += p.data
        at += len(p.data)
        n += p.n
    return Stream(walker, data, name, header=header, varints=varints, total=n, **kw)


# ---- ORC RLEv2 pieces ----------------------------------------------------------------------------------------------------------------------------
def v2_short_repeat(value, count, signed):
    return Piece(O.rle_v2_short_repeat(value, count, signed), header=[0], n=count)


def v2_delta(first, deltas, signed, width=None):
    b = O.rle_v2_delta(first, deltas, signed, width=width)
    a = uleb_end(b, 2)
    return Piece(b, header=[0, 1], varints=[(2, a), (a, uleb_end(b, a))], n=len(deltas) + 1)


def v2_patched(rng, n, base, fb, pw, positions, base_width=None, gap_width=None, patch_values=None):
    """a PATCHED_BASE run of n values with patches at `positions` (ascending; consecutive ones at most 255 apart) -> (piece, the values)"""
    low = [rng.getrandbits(fb) for _ in range(n)]
    patches, vals, prev = [], [base + x for x in low], 0
    for k, pos in enumerate(positions):
        pv = patch_values[k] if patch_values else rng.randrange(1, 1 << pw)
        patches.append((pos - prev, pv))
        prev = pos
        if pos < n:
            vals[pos] = base + (low[pos] | (pv << (fb & 63)))       # LongInputStreamV2.java:219 (a Java shift: by fb mod 64)
    vals = [s64(v) for v in vals]
    b = O.rle_v2_patched_base([base + x for x in low], base, fb, pw, patches, base_width=base_width, gap_width=gap_width)
    bw = (b[2] >> 5) + 1
    return Piece(b, header=list(range(4 + bw)), n=n), vals


def random_v2_piece(rng, signed):
    kind = rng.randrange(5)
    n = rng.choice((1, 2, 3, 9, 65, 512) if rng.random() < 0.5 else (1, 2, 5, 17))
    if kind == 0:
        v = rng.getrandbits(rng.randrange(1, 64 if signed else 65))
        return v2_short_repeat(-v if signed and rng.random() < 0.5 else v, rng.randrange(3, 11), signed)
    if kind == 1:
        w = rng.choice(ORC_WIDTHS)
        # (the packed magnitudes as they are: a signed stream zigzag-decodes them)
        return Piece(O.rle_v2_direct([rng.getrandbits(w) for _ in range(n)], False, width=w), header=[0, 1], n=n)
    if kind == 2:
        n = max(n, 2)
        fb, pw = rng.choice(ORC_WIDTHS[:20]), rng.choice(ORC_WIDTHS[:24])
        pos = sorted(rng.sample(range(min(n, 250)), min(rng.randrange(1, 5), min(n, 250))))
        base = rng.getrandbits(rng.randrange(1, 40)) * rng.choice((1, -1))
        return v2_patched(rng, n, base, fb, pw, pos)[0]
    if kind == 3:
        first = s64(rng.getrandbits(64)) if signed else rng.getrandbits(rng.randrange(1, 65))
        return v2_delta(first, [rng.randrange(-1000, 1000)] * max(n - 1, 1), signed)
    w = rng.choice(ORC_WIDTHS[1:])
    n = max(n, 2)
    sign = rng.choice((1, -1))
    deltas = [sign * rng.randrange(0, 1 << 20)] + [rng.getrandbits(w) for _ in range(n - 2)]
    return v2_delta(rng.getrandbits(50), deltas, signed, width=w)


# ---- ORC RLEv1 / byte-RLE pieces ---------------------------------------------------------------------------------------------------------------
def vlong(v, signed):
    return uleb(O.zigzag(v) if signed else v & M64)


def v1_run(base, delta, count, signed):
    v = vlong(base, signed)
    return Piece(bytes([count - 3, delta & 0xff]) + v, header=[0, 1], varints=[(2, 2 + len(v))], n=count)


def v1_literals(values, signed):
    out, varints = bytearray([0x100 - len(values)]), []
    for v in values:
        b = vlong(v, signed)
        varints.append((len(out), len(out) + len(b)))
        out += b
    return Piece(out, header=[0], varints=varints[:2] + varints[-1:], n=len(values))


def random_v1_piece(rng, signed):
    if rng.random() < 0.5:
        return v1_run(s64(rng.getrandbits(rng.randrange(1, 65))) if signed else rng.getrandbits(rng.randrange(1, 65)), rng.randrange(-128, 128), rng.choice((3, 4, 50, 130)), signed)
    n = rng.choice((1, 2, 7, 128))
    return v1_literals([s64(rng.getrandbits(rng.randrange(1, 65))) if signed else rng.getrandbits(rng.randrange(1, 65)) for _ in range(n)], signed)


def byte_run(value, count):
    return Piece(bytes([count - 3, value]), header=[0], n=count)


def byte_literals(data):
    return Piece(bytes([0x100 - len(data)]) + bytes(data), header=[0], n=len(data))


def random_byte_piece(rng):
    if rng.random() < 0.5:
        return byte_run(rng.randrange(256), rng.choice((3, 4, 64, 130)))
    return byte_literals(bytes(rng.randrange(256) for _ in range(rng.choice((1, 2, 63, 128)))))


# ---- Parquet hybrid pieces ----------------------------------------------------------------------------------------------------------------------
def h_rle(value, count, bw):
    b = P.hybrid_rle_run(value, count, bw)
    h = uleb_end(b, 0)
    return Piece(b, header=list(range(h)), varints=[(0, h)], n=count)


def h_packed(values, bw):
    b = P.hybrid_packed_run(values, bw)
    h = uleb_end(b, 0)
    return Piece(b, header=list(range(h)), varints=[(0, h)], n=len(values))


def hybrid_stream(pieces, bw, name, want=None):
    s = compose("hybrid", pieces, name, bit_width=bw)
    s.want = s.total if want is None else want
    s.total = s.want
    return s


def random_hybrid_stream(rng, name):
    bw = rng.choice((1, 1, 2, 3, 7, 8, 9, 16, 17, 31, 32))
    pieces = []
    for _ in range(rng.randrange(1, 7)):
        if rng.random() < 0.5:
            pieces.append(h_rle(rng.getrandbits(bw), rng.choice((1, 7, 8, 9, 300)), bw))
        else:
            pieces.append(h_packed([rng.getrandbits(bw) for _ in range(8 * rng.choice((1, 1, 2, 5)))], bw))
    if rng.random() < 0.5:      # a last packed group that is only partly wanted
        pieces.append(h_packed([rng.getrandbits(bw) for _ in range(rng.randrange(1, 8))], bw))
    return hybrid_stream(pieces, bw, name)


# ---- Parquet DELTA_BINARY_PACKED ----------------------------------------------------------------------------------------------------------------
def delta_stream(values, block_size, miniblocks, name, physical=P.INT64, tail_width=0, trailing=b""):
    """a section over `values` with its fields located: the four header varints, every block's min delta, every width byte"""
    b = P.delta_encode(values, physical, block_size, miniblocks, tail_width=tail_width)
    header, varints, widths, at = [], [], [], 0
    for _ in range(4):
        e = uleb_end(b, at)
        varints.append((at, e))
        header += range(at, e)
        at = e
    mini, left = block_size // miniblocks, len(values) - 1
    while left > 0:
        e = uleb_end(b, at)
        varints.append((at, e))
        header += range(at, e)
        at = e
        ws = b[at:at + miniblocks]
        widths += range(at, at + miniblocks)
        header += range(at, at + miniblocks)
        at += miniblocks
        for w in ws:
            if left <= 0:
                break
            at += mini * w // 8
            left -= mini
    assert at == len(b), (at, len(b))
    s = Stream("delta", b + trailing, name, want=len(values), header=header, varints=varints, widths=widths, total=len(values))
    s.meta = {"values": [s64(v) for v in values], "end": len(b), "physical": physical}
    return s


def random_delta_values(rng, n, bits):
    """n values whose deltas need about `bits` bits (wrapping int64)"""
    v, out = s64(rng.getrandbits(64)), []
    for _ in range(n):
        out.append(v)
        v = s64(v + (rng.getrandbits(bits) if bits else 5))
    return out


def random_delta_stream(rng, name):
    bs, mb = rng.choice(((128, 1), (128, 2), (128, 4), (256, 8)))
    n = rng.choice((1, 2, bs // mb, bs // mb + 1, bs, bs + 1, 2 * bs + 3, 40))
    return delta_stream(random_delta_values(rng, n, rng.choice((0, 1, 7, 8, 20, 33, 63, 64))), bs, mb, name)


# ---- Parquet PLAIN BYTE_ARRAY -------------------------------------------------------------------------------------------------------------------
def byte_array_stream(values, name):
    b, le32, at = P.plain_encode(P.BYTE_ARRAY, values), [], 0
    for v in values:
        le32.append(at)
        at += 4 + len(v)
    header = [o + k for o in le32 for k in range(4)]
    s = Stream("byte_arrays", b, name, count=len(values), header=header, le32=le32, total=len(values))
    s.meta = {"values": [bytes(v) for v in values]}
    return s


def random_byte_array_stream(rng, name):
    n = rng.choice((1, 2, 5, 20))
    return byte_array_stream([bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 3, 40, 300)))) for _ in range(n)], name)


# ---- base streams: a few dozen random compositions per walker ----------------------------------------------------------------------------------
def base_streams(walker, seed=20240):
    rng = random.Random("%s-%d" % (walker, seed))
    out = []
    for i in range(28):
        name = "%s/base%02d" % (walker, i)
        if walker == "rle_v2":
            signed = bool(i & 1)
            out.append(compose(walker, [random_v2_piece(rng, signed) for _ in range(rng.randrange(1, 7))], name, signed=signed))
        elif walker == "rle_v1":
            signed = bool(i & 1)
            out.append(compose(walker, [random_v1_piece(rng, signed) for _ in range(rng.randrange(1, 7))], name, signed=signed))
        elif walker == "byte_rle":
            out.append(compose(walker, [random_byte_piece(rng) for _ in range(rng.randrange(1, 9))], name))
        elif walker == "hybrid":
            out.append(random_hybrid_stream(rng, name))
        elif walker == "delta":
            out.append(random_delta_stream(rng, name))
        else:
            out.append(random_byte_array_stream(rng, name))
    return out


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------
def cut_lengths(s):
    """at most MAX_CUTS lengths < len(data): every cut inside a header first (a cut at length p + 1 ends the stream behind header byte p, a cut
    at p in front of it), the rest spread evenly.  A stream with more header bytes than MAX_CUTS / 2 keeps all of those cuts."""
    n = len(s.data)
    inside = sorted({c for p in s.header for c in (p, p + 1) if c < n})
    rest = [c for c in range(n) if c not in set(inside)]
    room = max(MAX_CUTS - len(inside), 0)
    step = max(len(rest) // room, 1) if room else 0
    return sorted(set(inside) | set(rest[::step][:room] if room else []))


def mutants(s, rng, n_random=0):
    """the mutants of one base stream (Streams with total None: nobody knows what they hold)"""
    d = s.data
    for c in cut_lengths(s):
        yield s.with_data(d[:c], "%s/cut%d" % (s.name, c))
    for p in s.header:
        for v in HEADER_BYTES:
            yield s.with_data(d[:p] + bytes([v]) + d[p + 1:], "%s/byte%d=%02x" % (s.name, p, v))
    for a, b in s.varints:
        for v in VARINT_VALUES:
            yield s.with_data(d[:a] + uleb(v) + d[b:], "%s/varint%d=%x" % (s.name, a, v))
    for a in s.le32:
        for v in VARINT_VALUES:
            yield s.with_data(d[:a] + struct.pack("<I", v & 0xffffffff) + d[a + 4:], "%s/length%d=%x" % (s.name, a, v))
    for p in s.widths:
        for v in WIDTH_BYTES:
            yield s.with_data(d[:p] + bytes([v]) + d[p + 1:], "%s/width%d=%d" % (s.name, p, v))
    if s.walker == "hybrid":          # the width byte of a dictionary page / the level width: a scalar argument of the walk
        for v in WIDTH_BYTES:
            yield s.with_data(d, "%s/bit_width=%d" % (s.name, v), bit_width=v)


def random_streams(walker, count=300, seed=7):
    rng = random.Random("%s-random-%d" % (walker, seed))
    for i in range(count):
        data = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 48)))
        yield Stream(walker, data, "%s/random%03d" % (walker, i), signed=bool(i & 1), bit_width=rng.randrange(1, 33), want=rng.choice((1, 2, 8, 64, 300)) if walker in ("hybrid", "delta") else 0,
                     count=rng.choice((1, 2, 5)) if walker == "byte_arrays" else 0)


def corpus(walker):
    """(base streams, mutants) of one walker"""
    rng = random.Random("%s-mutants" % walker)
    base = base_streams(walker)
    return base, [m for s in base for m in mutants(s, rng)] + list(random_streams(walker))


# ---- MALFORMED: refused by the walker, before anything is uploaded ------------------------------------------------------------------------------
def _delta_header(block_size, miniblocks, total, first=0):
    return uleb(block_size) + uleb(miniblocks) + uleb(total) + P.zigzag_uleb(first)


def malformed():
    rng = random.Random(3)
    big = byte_array_stream([b"abc"], "x").data
    return [
        # mini * width overflows int64 to 0: the old check passed and the kernel would have read ~`want` bytes behind the page
        Stream("delta", _delta_header(1 << 61, 1, 1000) + uleb(0) + bytes([8]) + bytes(64), "delta/block_size_2^61_width_8", want=1000),
        # mini is negative as int64: the old walk moved backwards and read bytes[-...] on the host
        Stream("delta", _delta_header(1 << 63, 1, 1000) + uleb(0) + bytes([8]) + bytes(64), "delta/block_size_2^63", want=1000),
        Stream("delta", _delta_header(128, 4, 100) + uleb(0) + bytes([65, 0, 0, 0]) + bytes(600), "delta/width_byte_65", want=100),
        Stream("hybrid", P.hybrid_packed_run([1] * 8, 32), "hybrid/bit_width_33", bit_width=33, want=8),
        Stream("hybrid", bytes([0x81] * 5 + [0x80, 0x00]) + bytes(64), "hybrid/run_header_of_six_continuation_bytes", bit_width=8, want=8),
        # PATCHED_BASE: patch width 64 (code 31) + gap width 1
        Stream("rle_v2", bytes([0x80 | (7 << 1), 3, 31, (0 << 5) | 1, 0]) + bytes(4) + bytes(16), "rle_v2/patch_width_plus_gap_width_65", signed=True),
        Stream("rle_v2", bytes([0xc0 | (3 << 1), 0]) + uleb(5) + uleb(2), "rle_v2/delta_with_a_width_and_length_0", signed=True),
        Stream("rle_v2", O.rle_v2_direct([rng.getrandbits(13) for _ in range(100)], False, width=13)[:-1], "rle_v2/direct_run_one_byte_short", signed=True),
        Stream("byte_rle", byte_literals(b"abcdefg").data[:-1], "byte_rle/literal_group_one_byte_short"),
        Stream("byte_arrays", struct.pack("<I", 0x80000000) + big, "byte_arrays/length_0x80000000", count=1),
    ]


# ---- ODD_BUT_LEGAL: accepted by the walker, never emitted by a writer; `values` = what the reference's reader produces ---------------------------
def odd_but_legal():
    rng = random.Random(5)
    out = []
    # DELTA of 2 values with a packed width: first, first + delta base; nothing is packed (LongInputStreamV2.java:117-121: length becomes 0, :127 does not loop)
    s = compose("rle_v2", [v2_delta(-7, [1000], True, width=13)], "rle_v2/delta_of_2_values_with_a_width", signed=True)
    s.meta = {"values": [-7, 993], "says": "lib/trino-orc/src/main/java/io/trino/orc/stream/LongInputStreamV2.java:117-137"}
    out.append(s)
    # a patch whose position lies behind the run's last value: `i == actualGap` never holds (LongInputStreamV2.java:216-217), the values stay unpatched
    p, vals = v2_patched(rng, 40, 500, 8, 12, [10, 200])
    s = compose("rle_v2", [p], "rle_v2/patch_behind_the_last_value", signed=True)
    s.meta = {"values": vals, "says": "lib/trino-orc/src/main/java/io/trino/orc/stream/LongInputStreamV2.java:216-217"}
    out.append(s)
    # a (255, 0) continuation as the last patch entry, behind a patch the loop never reaches (position 255 of 200 values): the entry is never
    # loaded (LongInputStreamV2.java:227-240 runs only inside `i == actualGap`), every value is base + unpacked (:250)
    p, vals = v2_patched(rng, 200, -3, 5, 7, [255, 510], gap_width=8, patch_values=[9, 0])
    s = compose("rle_v2", [p], "rle_v2/continuation_as_the_last_patch_entry", signed=True)
    s.meta = {"values": vals, "says": "lib/trino-orc/src/main/java/io/trino/orc/stream/LongInputStreamV2.java:216-250"}
    out.append(s)
    # a bit-packed run whose last group is cut to the bytes its wanted values occupy (3 values of 9 bits: 4 bytes of the group's 9)
    vals = [rng.getrandbits(9) for _ in range(11)]
    full = hybrid_stream([h_packed(vals[:8], 9), h_packed(vals[8:], 9)], 9, "hybrid/last_group_cut_to_the_wanted_values")
    s = full.with_data(full.data[:-5], full.name, total=11, want=11)
    s.meta = {"values": vals, "says": "lib/trino-parquet/src/main/java/io/trino/parquet/ParquetEncoding.java:198-212 hands the stream to parquet-mr's RunLengthBitPackingHybridDecoder (not in the tree), "
                                      "whose readNext takes min(group bytes, bytes available)"}
    out.append(s)
    # a dictionary page of 3 entries whose id stream declares bit width 32
    ids = [rng.randrange(3) for _ in range(21)]
    s = hybrid_stream([h_packed(ids[:16], 32), h_rle(2, 5, 32)], 32, "hybrid/width_32_over_a_3_entry_dictionary")
    s.meta = {"values": ids[:16] + [2] * 5, "dictionary": 3, "says": "lib/trino-parquet/src/main/java/io/trino/parquet/ParquetEncoding.java:117-143 (the width is the page's first byte, "
                                                                       "whatever the dictionary's size)"}
    out.append(s)
    # the last block lists widths for miniblocks that are not written
    vals = random_delta_values(rng, 40, 11)
    s = delta_stream(vals, 128, 4, "delta/widths_listed_for_unwritten_miniblocks", tail_width=17)
    s.meta["says"] = "lib/trino-parquet/src/main/java/io/trino/parquet/ParquetEncoding.java:146-154 hands the section to parquet-mr's DeltaBinaryPackingValuesReader (not in the tree), " \
                     "which loads a miniblock only when a value of it is asked for"
    out.append(s)
    return out


# ---- coverage streams: well-formed, every shape at which the decode kernels take another path (at most 64 runs and 20 000 values each) ----------
DELTA_COUNTS = (2, 3, 9, 65, 511, 512)        # rle_v2_decode_kernel blocks the packed deltas 8 per lane
DELTA_SHAPES = ((128, 1), (128, 2), (128, 4), (256, 8), (1024, 32), (4096, 128))


def run_offsets(s):
    """the byte offset of every run of a composed RLEv2 stream (its first header byte)"""
    return [h for i, h in enumerate(s.header) if i == 0 or s.header[i - 1] != h - 1]


def coverage_rle_v2():
    """[Stream]: signed and unsigned RLEv2 streams; meta['values'] where the builder knows them (PATCHED_BASE)"""
    rng = random.Random(11)
    out = []
    for signed in (True, False):
        tag = "signed" if signed else "unsigned"
        counts = (1, 2, 63, 64, 65, 511, 512)
        # DIRECT at every width code (width 64 unsigned: values at or above 2^63)
        pieces = [Piece(O.rle_v2_direct([rng.getrandbits(w) | (1 << (w - 1)) for _ in range(counts[i % 7])], False, width=w), header=[0, 1], n=counts[i % 7])
                  for i, w in enumerate(ORC_WIDTHS)]
        out.append(compose("rle_v2", pieces, "rle_v2/direct_every_width_" + tag, signed=signed))
        # SHORT_REPEAT of 1..8 value bytes (8 bytes unsigned: at or above 2^63), 3 and 10 values
        pieces = []
        for size in range(1, 9):
            for count in (3, 10):
                u = rng.getrandbits(8 * size) | (1 << (8 * size - 1))
                pieces.append(Piece(bytes([((size - 1) << 3) | (count - 3)]) + u.to_bytes(size, "big"), header=[0], n=count))
        out.append(compose("rle_v2", pieces, "rle_v2/short_repeat_every_size_" + tag, signed=signed))
        # DELTA: every packed width in both directions, the counts of the kernel's 8-per-lane blocking
        for sign in (1, -1):
            pieces = []
            for i, w in enumerate(ORC_WIDTHS[1:]):
                n = DELTA_COUNTS[i % len(DELTA_COUNTS)]
                first = rng.getrandbits(62)
                deltas = [sign * rng.randrange(1, 1 << 30)] + [rng.getrandbits(w) | (1 << (w - 1)) for _ in range(n - 2)]
                pieces.append(v2_delta(first, deltas, signed, width=w))
            out.append(compose("rle_v2", pieces, "rle_v2/delta_every_width_%s_%s" % ("up" if sign > 0 else "down", tag), signed=signed))
        # DELTA whose sums wrap int64 as Java's do: a first value within one delta of the end, fixed and packed, every count
        pieces = []
        for n in DELTA_COUNTS:
            for first, sign in ((I64_MAX - 3, 1), (I64_MIN + 3, -1)):
                f = first if signed else first & M64
                pieces.append(v2_delta(f, [sign * 1000] * (n - 1), signed))
                pieces.append(v2_delta(f, [sign * 1000] + [rng.getrandbits(17) for _ in range(n - 2)], signed, width=17))
        out.append(compose("rle_v2", pieces, "rle_v2/delta_wraps_int64_" + tag, signed=signed))
    # PATCHED_BASE (signed: LongColumnReader; the base has its own sign bit): every value width, base widths of 1..8 bytes and negative bases,
    # 1 and 31 patches, a patch on value 0 and on the last value, patch + gap widths on each closest_fixed_bits step, 1 / 64 / 65 / 512 values
    for signed in (True, False):
        pieces, values = [], []
        steps = ((24, 1), (32, 1), (56, 1), (24, 8), (32, 8), (56, 8), (4, 3), (12, 8))
        for i, fb in enumerate(ORC_WIDTHS):
            n = (1, 64, 65, 512)[i % 4]
            pw, pgw = steps[i % len(steps)]
            bw = i % 8 + 1
            base = (rng.getrandbits(8 * bw - 1) | (1 << (8 * bw - 2) if bw > 1 else 1)) * (1 if i % 3 else -1)
            if pgw == 1:
                pos = [0] + ([1, 2] if n > 2 else [])
            elif i % 5 == 0 and n >= 64:
                pos = sorted({0, n - 1} | set(rng.sample(range(1, n - 1), 29)))      # 31 patches
                if any(b - a > (1 << pgw) - 1 for a, b in zip(pos, pos[1:])):
                    pos = list(range(0, 31 * (n // 32), n // 32))[:30] + [n - 1] if n // 32 <= (1 << pgw) - 1 else list(range(30)) + [min(n - 1, 30 + (1 << pgw) - 1)]
            else:
                pos = [n - 1] if n - 1 <= (1 << pgw) - 1 else [0, min(n - 1, (1 << pgw) - 1)]
            p, vals = v2_patched(rng, n, base, fb, pw, pos, base_width=bw, gap_width=pgw)
            pieces.append(p)
            values += vals
        s = compose("rle_v2", pieces, "rle_v2/patched_base_every_width_" + ("signed" if signed else "unsigned"), signed=signed)
        s.meta = {"values": values}
        out.append(s)
    # runs that start at every byte offset modulo 8 of the uploaded buffer
    pieces = []
    for k in range(1, 25):
        pieces.append(Piece(O.rle_v2_direct([rng.getrandbits(11) for _ in range(k)], False, width=11), header=[0, 1], n=k))
        pieces.append(v2_delta(rng.getrandbits(20 + k), [3] + [rng.getrandbits(5) for _ in range(k)], True, width=5))
        if k % 3 == 0:
            pieces.append(v2_patched(rng, 10 + k, -k, 3, 6, [k % 7])[0])
    s = compose("rle_v2", pieces[:64], "rle_v2/runs_at_every_byte_offset", signed=True)
    assert {o % 8 for o in run_offsets(s)} == set(range(8))
    out.append(s)
    return out


def small_unsigned_stream(walker, limit, n_runs, seed):
    """an unsigned RLEv2 / RLEv1 stream of values in [0, limit): string lengths, dictionary ids"""
    rng = random.Random("small-%s-%d" % (walker, seed))
    bits = max(limit.bit_length() - 1, 1)
    pieces = []
    for i in range(n_runs):
        n = rng.choice((1, 2, 9, 65, 130 if walker == "rle_v1" else 512))
        kind = i % 4
        if walker == "rle_v1":
            if kind < 2:      # a run of max(n, 3) values climbing by 1 (kind 0) or equal (kind 1): base + 130 stays below the limit
                pieces.append(v1_run(rng.randrange(limit - 130), 1 - kind, max(n, 3), False))
            else:
                pieces.append(v1_literals([rng.randrange(limit) for _ in range(min(n, 128))], False))
        elif kind == 0:
            pieces.append(v2_short_repeat(rng.randrange(limit), rng.randrange(3, 11), False))
        elif kind == 1:
            pieces.append(Piece(O.rle_v2_direct([rng.getrandbits(bits) for _ in range(n)], False, width=O.closest_fixed_bits(bits)), header=[0, 1], n=n))
        elif kind == 2:
            pieces.append(v2_delta(rng.randrange(limit), [0] * max(n - 1, 1), False))
        else:
            pieces.append(v2_patched(rng, max(n, 2), 0, max(bits - 2, 1), 1, [0])[0])
    return compose(walker, pieces, "%s/small_unsigned_%d" % (walker, seed), signed=False)


def coverage_hybrid():
    """[Stream] with meta['values']: every bit width 0..32 (ids below 5, the large widths over a small dictionary), RLE runs of 1 / 7 / 8 / 9 values,
    bit-packed runs of one and of many groups, the two kinds alternating; one stream with an RLE run of 2^20 values"""
    rng = random.Random(13)
    out = []
    for bw in range(1, 33):
        top = min(1 << bw, 5)
        pieces, vals = [], []
        for kind in ("r1", "p1", "r7", "r8", "p40", "r9", "p1", "r1", "p3", "r300"):
            if kind[0] == "r":
                v, n = rng.randrange(top), int(kind[1:])
                pieces.append(h_rle(v, n, bw))
                vals += [v] * n
            else:
                vs = [rng.randrange(top) for _ in range(8 * int(kind[1:]))]
                pieces.append(h_packed(vs, bw))
                vals += vs
        tail = [rng.randrange(top) for _ in range(3)]          # a last group of which 3 values are wanted
        pieces.append(h_packed(tail, bw))
        s = hybrid_stream(pieces, bw, "hybrid/every_run_kind_width_%d" % bw)
        s.meta = {"values": vals + tail}
        out.append(s)
    s = hybrid_stream([h_rle(1, 5, 1), h_rle(0, 1 << 20, 1), h_packed([1, 0, 1, 1, 0, 0, 1, 0], 1), h_rle(1, 9, 1)], 1, "hybrid/rle_run_of_2^20")
    s.meta = {"values": [1] * 5 + [0] * (1 << 20) + [1, 0, 1, 1, 0, 0, 1, 0] + [1] * 9}
    out.append(s)
    return out


def coverage_delta():
    """[Stream] (meta: values, end, physical = INT64 arithmetic): every block shape at every count edge; every width 0..64; min deltas at both int64 ends"""
    rng = random.Random(17)
    out = []
    for bs, mb in DELTA_SHAPES:
        mini = bs // mb
        for n in (1, 2, mini, mini + 1, bs, bs + 1, 2 * bs):
            out.append(delta_stream(random_delta_values(rng, n, rng.choice((3, 12, 31, 47))), bs, mb, "delta/shape_%d_%d_count_%d" % (bs, mb, n)))
    for w in range(65):
        bs, mb = DELTA_SHAPES[w % 4]
        n = bs + bs // mb + 2
        vals, v = [], s64(rng.getrandbits(64))
        for i in range(n):          # deltas 0 .. 2^w - 1 with both ends present in every miniblock: the miniblock's width is exactly w
            vals.append(v)
            d = 0 if i % 3 == 0 else ((1 << w) - 1 if i % 3 == 1 else rng.getrandbits(w) if w else 0)
            v = s64(v + d)
        s = delta_stream(vals, bs, mb, "delta/width_%d" % w)
        assert w in s.data[s.widths[0]:s.widths[0] + 1], (w, list(s.data[s.widths[0]:s.widths[0] + mb]))
        out.append(s)
    # min delta INT64_MIN (a block with a delta of -2^63 and larger ones: width 64), and INT64_MAX (every delta of the block: width 0)
    vals, v = [], 12345
    for d in [I64_MIN, I64_MAX, 0, -1, I64_MIN, 7] * 30:
        vals.append(v)
        v = s64(v + d)
    out.append(delta_stream(vals, 128, 4, "delta/min_delta_int64_min"))
    vals, v = [], -99
    for _ in range(200):
        vals.append(v)
        v = s64(v + I64_MAX)
    out.append(delta_stream(vals, 128, 2, "delta/min_delta_int64_max"))
    return out


def coverage(walker):
    if walker == "rle_v2":
        return coverage_rle_v2() + [small_unsigned_stream("rle_v2", 300, 40, k) for k in range(2)]
    if walker == "rle_v1":
        rng = random.Random(19)
        edges = [I64_MAX, I64_MIN, 0, -1, 1, I64_MAX - 1, I64_MIN + 1]
        return [compose("rle_v1", [v1_literals(edges, True), v1_run(I64_MAX - 100, 127, 130, True), v1_run(I64_MIN + 100, -128, 130, True), v1_literals([s64(rng.getrandbits(64)) for _ in range(128)], True)],
                        "rle_v1/int64_edges", signed=True)] + [small_unsigned_stream("rle_v1", 300, 40, k) for k in range(2)]
    if walker == "hybrid":
        return coverage_hybrid()
    if walker == "delta":
        return coverage_delta()
    return []

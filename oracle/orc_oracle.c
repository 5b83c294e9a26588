/*
 * orc_oracle.c -- CPU restatement of the reference's ORC integer / byte / boolean stream decoders (scan-side decode).
 * TEST INFRASTRUCTURE: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may call it; the product (presto-1_amd/) never does.
 *
 * Byte at a time, value at a time, like the Java classes it follows (paths under lib/trino-orc/src/main/java/io/trino/orc/stream/):
 *   o_orc_rle_v2        LongInputStreamV2.java:59-312   (readValues: SHORT_REPEAT / DIRECT / PATCHED_BASE / DELTA)
 *   o_orc_rle_v1        LongInputStreamV1.java:47-103
 *   o_orc_unpack        LongBitPacker.java:82-108       (unpackGeneric; the width-specialised unpackN of :110-351 are asserted equal to it
 *                                                        by lib/trino-orc/src/test/java/io/trino/orc/stream/TestLongBitPacker.java:41-60)
 *   o_orc_decode_bit_width / o_orc_closest_fixed_bits   LongDecode.java:47-115
 *   o_orc_read_vint / o_orc_write_vlong / zigzag        LongDecode.java:117-183
 *   o_orc_byte_rle      ByteInputStream.java:43-75
 *   o_orc_boolean       BooleanInputStream.java:36-58   (byte RLE, bits most significant first)
 * Pinned (tests/test_orc_oracle_cpu.py) on tests/golden/orc_streams.json: the stream bytes of the reference's own ORC test resources with the
 * WRITER's column statistics (count, min, max, sum) as known answers, and on the value lists of TestLongDecode.java:36-56.
 */
#include <stdint.h>
#include <string.h>

typedef struct {
    const uint8_t *p;
    int64_t len, at;
    int eof;
} in_t;

static int rd(in_t *in)   /* InputStream.read(): -1 at the end */
{
    if (in->at >= in->len) {
        in->eof = 1;
        return -1;
    }
    return in->p[in->at++];
}

int32_t o_orc_decode_bit_width(int32_t n)   /* LongDecode.java:47-76; FixedBitSizes ordinals: ONE = 0 .. TWENTY_FOUR = 23, 26 = 24, 28, 30, 32, 40, 48, 56, 64 = 31 */
{
    if (n >= 0 && n <= 23) return n + 1;
    switch (n) {
    case 24: return 26;
    case 25: return 28;
    case 26: return 30;
    case 27: return 32;
    case 28: return 40;
    case 29: return 48;
    case 30: return 56;
    default: return 64;
    }
}

int32_t o_orc_closest_fixed_bits(int32_t width)   /* LongDecode.java:81-115 */
{
    if (width == 0) return 1;
    if (width >= 1 && width <= 24) return width;
    if (width <= 26) return 26;
    if (width <= 28) return 28;
    if (width <= 30) return 30;
    if (width <= 32) return 32;
    if (width <= 40) return 40;
    if (width <= 48) return 48;
    if (width <= 56) return 56;
    return 64;
}

static int64_t zigzag_decode(uint64_t v) { return (int64_t)((v >> 1) ^ (uint64_t)(-(int64_t)(v & 1))); }   /* LongDecode.java:155-158 */

static uint64_t read_unsigned_vint(in_t *in)   /* LongDecode.java:124-140 */
{
    uint64_t result = 0;
    int offset = 0;
    int b;
    do {
        b = rd(in);
        if (b < 0) return result;
        if (offset < 64) result |= ((uint64_t)(b & 0x7f)) << offset;
        offset += 7;
    } while (b & 0x80);
    return result;
}
static int64_t read_vint(in_t *in, int is_signed) { const uint64_t u = read_unsigned_vint(in); return is_signed ? zigzag_decode(u) : (int64_t)u; }

int64_t o_orc_read_vint(const uint8_t *bytes, int64_t len, int32_t is_signed, int64_t *consumed)
{
    in_t in = {bytes, len, 0, 0};
    const int64_t v = read_vint(&in, is_signed);
    if (consumed) *consumed = in.eof ? -1 : in.at;
    return v;
}

int32_t o_orc_write_vlong(int64_t value, int32_t is_signed, uint8_t *out)   /* LongDecode.java:160-183 */
{
    uint64_t v = is_signed ? (((uint64_t)value << 1) ^ (uint64_t)(value >> 63)) : (uint64_t)value;
    int32_t n = 0;
    for (;;) {
        if ((v & ~(uint64_t)0x7f) == 0) {
            out[n++] = (uint8_t)v;
            return n;
        }
        out[n++] = (uint8_t)(0x80 | (v & 0x7f));
        v >>= 7;
    }
}

/* LongBitPacker.unpackGeneric (LongBitPacker.java:82-108): big-endian bit stream, every call starts at a byte boundary */
static void unpack_generic(in_t *in, int64_t *buffer, int64_t offset, int64_t len, int bit_size)
{
    int bits_left = 0;
    int current = 0;
    for (int64_t i = offset; i < offset + len; i++) {
        uint64_t result = 0;
        int to_read = bit_size;
        while (to_read > bits_left) {
            result <<= bits_left;
            result |= (uint64_t)(current & ((1 << bits_left) - 1));
            to_read -= bits_left;
            current = rd(in);
            if (current < 0) current = 0;
            bits_left = 8;
        }
        if (to_read > 0) {
            result <<= to_read;
            bits_left -= to_read;
            result |= (uint64_t)((current >> bits_left) & ((1 << to_read) - 1));
        }
        buffer[i] = (int64_t)result;
    }
}

int64_t o_orc_unpack(const uint8_t *bytes, int64_t len, int64_t count, int32_t bit_size, int64_t *out)
{
    in_t in = {bytes, len, 0, 0};
    unpack_generic(&in, out, 0, count, bit_size);
    return in.eof ? -1 : in.at;   /* bytes read */
}

static uint64_t bytes_to_long_be(in_t *in, int n)   /* LongInputStreamV2.java:296-309 */
{
    uint64_t out = 0;
    while (n > 0) {
        n--;
        int v = rd(in);
        if (v < 0) v = 0;
        out |= ((uint64_t)v) << (n * 8);
    }
    return out;
}

#define EMIT(v)                                  \
    do {                                         \
        if (n >= cap) return -2;                 \
        out[n++] = (int64_t)(v);                 \
    } while (0)

/* every value of the stream; returns their number, -1 = truncated / corrupt stream, -2 = more than `cap` values */
int64_t o_orc_rle_v2(const uint8_t *bytes, int64_t len, int32_t is_signed, int64_t *out, int64_t cap)
{
    in_t in = {bytes, len, 0, 0};
    int64_t n = 0;
    static int64_t unpacked[512], patch[32 + 4];
    while (in.at < in.len) {
        const int first = rd(&in);
        const int enc = (first >> 6) & 3;
        if (enc == 0) {   /* SHORT_REPEAT :255-282 */
            const int size = ((first >> 3) & 7) + 1;
            const int length = (first & 7) + 3;
            uint64_t val = bytes_to_long_be(&in, size);
            const int64_t v = is_signed ? zigzag_decode(val) : (int64_t)val;
            for (int i = 0; i < length; i++) EMIT(v);
        }
        else if (enc == 1) {   /* DIRECT :229-252 */
            const int fixed_bits = o_orc_decode_bit_width((first >> 1) & 0x1f);
            int length = (first & 1) << 8;
            length |= rd(&in);
            length += 1;
            unpack_generic(&in, unpacked, 0, length, fixed_bits);
            for (int i = 0; i < length; i++) EMIT(is_signed ? zigzag_decode((uint64_t)unpacked[i]) : unpacked[i]);
        }
        else if (enc == 2) {   /* PATCHED_BASE :135-226 */
            const int fb = o_orc_decode_bit_width((first >> 1) & 0x1f);
            int length = (first & 1) << 8;
            length |= rd(&in);
            length += 1;
            const int third = rd(&in);
            const int base_width = ((third >> 5) & 7) + 1;
            const int patch_width = o_orc_decode_bit_width(third & 0x1f);
            const int fourth = rd(&in);
            const int patch_gap_width = ((fourth >> 5) & 7) + 1;
            const int patch_list_length = fourth & 0x1f;
            /* (Java's long arithmetic wraps: every sum and shift below is done on uint64_t, shifts by the count modulo 64) */
            const uint64_t raw_base = bytes_to_long_be(&in, base_width);
            const uint64_t mask = (uint64_t)1 << ((base_width * 8) - 1);
            const uint64_t base = (raw_base & mask) != 0 ? ~(raw_base & ~mask) + 1 : raw_base;
            unpack_generic(&in, unpacked, 0, length, fb);
            if (patch_width + patch_gap_width > 64) return -1;   /* "Invalid RLEv2 encoded stream" */
            const int bit_size = o_orc_closest_fixed_bits(patch_width + patch_gap_width);
            memset(patch, 0, sizeof(patch));
            unpack_generic(&in, patch, 0, patch_list_length, bit_size);
            int patch_index = 0;
            const uint64_t patch_mask = patch_width >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << patch_width) - 1);
            uint64_t current_gap = patch_width >= 64 ? 0 : (uint64_t)patch[patch_index] >> patch_width;
            uint64_t current_patch = (uint64_t)patch[patch_index] & patch_mask;
            int64_t actual_gap = 0;
            while (current_gap == 255 && current_patch == 0 && patch_index + 1 < 36) {
                actual_gap += 255;
                patch_index++;
                current_gap = (uint64_t)patch[patch_index] >> patch_width;
                current_patch = (uint64_t)patch[patch_index] & patch_mask;
            }
            actual_gap += (int64_t)current_gap;
            for (int i = 0; i < length; i++) {
                if (i == actual_gap) {
                    const uint64_t patched = (uint64_t)unpacked[i] | (current_patch << (fb & 63));   /* :219 */
                    EMIT(base + patched);
                    patch_index++;
                    if (patch_index < patch_list_length) {
                        current_gap = (uint64_t)patch[patch_index] >> patch_width;
                        current_patch = (uint64_t)patch[patch_index] & patch_mask;
                        actual_gap = 0;
                        while (current_gap == 255 && current_patch == 0 && patch_index + 1 < 36) {
                            actual_gap += 255;
                            patch_index++;
                            current_gap = (uint64_t)patch[patch_index] >> patch_width;
                            current_patch = (uint64_t)patch[patch_index] & patch_mask;
                        }
                        actual_gap += (int64_t)current_gap;
                        actual_gap += i;
                    }
                }
                else EMIT(base + (uint64_t)unpacked[i]);
            }
        }
        else {   /* DELTA :82-132 */
            int fixed_bits = (first >> 1) & 0x1f;
            if (fixed_bits != 0) fixed_bits = o_orc_decode_bit_width(fixed_bits);
            int length = (first & 1) << 8;
            length |= rd(&in);
            const int64_t first_val = read_vint(&in, is_signed);
            EMIT(first_val);
            if (fixed_bits == 0) {
                const int64_t fixed_delta = zigzag_decode(read_unsigned_vint(&in));
                for (int i = 0; i < length; i++) {
                    const int64_t next = (int64_t)((uint64_t)out[n - 1] + (uint64_t)fixed_delta);
                    EMIT(next);
                }
            }
            else {
                const int64_t delta_base = zigzag_decode(read_unsigned_vint(&in));
                /* a packed width with no second value: :121 makes the length -1 and the width-specialised unpackers of LongBitPacker.java:110-351 are
                 * handed a negative count; no writer emits it, the library refuses it ("Invalid RLEv2 encoded stream") and so does the oracle */
                if (length < 1) return -1;
                EMIT((int64_t)((uint64_t)first_val + (uint64_t)delta_base));
                int64_t prev = out[n - 1];
                length -= 1;
                unpack_generic(&in, unpacked, 0, length, fixed_bits);
                for (int i = 0; i < length; i++) {
                    prev = delta_base < 0 ? (int64_t)((uint64_t)prev - (uint64_t)unpacked[i]) : (int64_t)((uint64_t)prev + (uint64_t)unpacked[i]);
                    EMIT(prev);
                }
            }
        }
        if (in.eof) return -1;
    }
    return n;
}

int64_t o_orc_rle_v1(const uint8_t *bytes, int64_t len, int32_t is_signed, int64_t *out, int64_t cap)   /* LongInputStreamV1.java:47-103 */
{
    in_t in = {bytes, len, 0, 0};
    int64_t n = 0;
    while (in.at < in.len) {
        const int control = rd(&in);
        if (control < 0x80) {
            const int count = control + 3;
            int delta = rd(&in);
            delta = (int8_t)delta;
            const int64_t base = read_vint(&in, is_signed);
            for (int i = 0; i < count; i++) EMIT((int64_t)((uint64_t)base + (uint64_t)((int64_t)i * delta)));
        }
        else {
            const int count = 0x100 - control;
            for (int i = 0; i < count; i++) EMIT(read_vint(&in, is_signed));
        }
        if (in.eof) return -1;
    }
    return n;
}
#undef EMIT

int64_t o_orc_byte_rle(const uint8_t *bytes, int64_t len, uint8_t *out, int64_t cap)   /* ByteInputStream.java:43-75 */
{
    in_t in = {bytes, len, 0, 0};
    int64_t n = 0;
    while (in.at < in.len) {
        const int control = rd(&in);
        if ((control & 0x80) == 0) {
            const int length = control + 3;
            const int value = rd(&in);
            if (value < 0) return -1;
            for (int i = 0; i < length; i++) {
                if (n >= cap) return -2;
                out[n++] = (uint8_t)value;
            }
        }
        else {
            const int length = 0x100 - control;
            for (int i = 0; i < length; i++) {
                const int v = rd(&in);
                if (v < 0) return -1;
                if (n >= cap) return -2;
                out[n++] = (uint8_t)v;
            }
        }
    }
    return n;
}

/* BooleanInputStream: `count` bits of the byte-RLE payload, high bit first; out[i] = 0 / 1.  Returns count, or <0 */
int64_t o_orc_boolean(const uint8_t *bytes, int64_t len, int64_t count, uint8_t *out)
{
    static uint8_t tmp[1 << 20];
    const int64_t need = (count + 7) / 8;
    if (need > (int64_t)sizeof(tmp)) return -2;
    const int64_t got = o_orc_byte_rle(bytes, len, tmp, sizeof(tmp));
    if (got < need) return -1;
    for (int64_t i = 0; i < count; i++) out[i] = (uint8_t)((tmp[i >> 3] >> (7 - (i & 7))) & 1);
    return count;
}

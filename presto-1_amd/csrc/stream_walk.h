// stream_walk.h -- the HOST side of the scan decoders (orc.hip, parquet.hip): the walks over the variable-length headers of an ORC RLEv2 / RLEv1 /
// byte-RLE stream, a Parquet RLE / bit-packed hybrid stream, a DELTA_BINARY_PACKED section and a PLAIN BYTE_ARRAY section, and the run
// directories they produce.  The kernels read `bytes + run.in_off + ...` without further checks: these walks are the whole bounds check, and
// this header is the contract between the two sides --
//   * the walkers refuse (WALK_FAIL) every stream whose directory would send a kernel outside the uploaded bytes plus their slack;
//   * the slack the uploads add and the reach of every device bit reader behind a value's first byte are the constants below;
//   * check_plan(...) states, per directory type, what the kernels rely on.  The walkers do not call it: tests/stream_walk/walk_main.cpp does, on
//     a fuzzed corpus under the host sanitizers (tests/test_stream_walk_cpu.py).
// Nothing of HIP and not common.h is included, so that program compiles it with a plain C++ compiler.  Errors go through WALK_FAIL(message):
// by default a standard exception; orc.hip and parquet.hip define it as ::tgpu::fail(TGPU_ERR_INVALID_ARGUMENT, message) before they include this.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#ifndef WALK_FAIL
#define WALK_FAIL(msg) throw std::invalid_argument(msg)
#endif

namespace tgpu {
namespace walk {

// ---- slack behind the uploaded bytes, and how far the device bit readers look behind the first byte of a value ------------------------------
constexpr int kOrcSlack = 32;            // orc.hip: upload_padded
constexpr int kParquetSlack = 16;        // parquet.hip: upload_padded
constexpr int kReadBitsReach = 9;        // orc.hip read_bits: 8 bytes, and a ninth when the value straddles them
constexpr int kHybridReach = 5;          // parquet.hip hybrid_decode_kernel: 32 bits at any bit offset span at most 5 bytes
constexpr int kDeltaUnpackReach = 9;     // parquet.hip delta_unpack_kernel: an 8-byte load, and a ninth byte when the value straddles it
// a value's first byte lies inside the stream (what the walkers check), so a reader reaches at most reach - 1 bytes into the slack
static_assert(kReadBitsReach <= kOrcSlack, "read_bits reads past the slack of the uploaded ORC stream");
static_assert(kHybridReach <= kParquetSlack, "hybrid_decode_kernel reads past the slack of the uploaded page");
static_assert(kDeltaUnpackReach <= kParquetSlack, "delta_unpack_kernel reads past the slack of the uploaded page");

// ---- ORC ---------------------------------------------------------------------------------------------------------------------------------------
enum RunKind : int32_t { SHORT_REPEAT = 0, DIRECT = 1, PATCHED_BASE = 2, DELTA = 3, V1_RUN = 4, V1_LITERALS = 5 };

struct OrcRun {
    int64_t in_off;       // first byte of the run's PACKED payload (behind the header fields the host has read)
    int64_t out_off;      // index of the run's first value
    int32_t kind, count;  // values of the run
    int32_t width;        // bit width of the packed values (0: DELTA with a fixed delta)
    int32_t patch_width, patch_gap_width, patch_count, patch_bits;   // PATCHED_BASE: patch list entries of patch_bits bits = gap | patch
    int64_t base;         // SHORT_REPEAT: the (zigzag-decoded) value; PATCHED_BASE: base; DELTA: first value
    int64_t delta;        // DELTA: fixed delta / delta base
    int64_t patch_off;    // PATCHED_BASE: first byte of the patch list
};

inline int decode_bit_width(int n)
{
    if (n >= 0 && n <= 23) return n + 1;
    static const int wide[8] = {26, 28, 30, 32, 40, 48, 56, 64};
    return wide[(n - 24) & 7];
}
inline int closest_fixed_bits(int w)
{
    if (w == 0) return 1;
    if (w <= 24) return w;
    if (w <= 26) return 26;
    if (w <= 28) return 28;
    if (w <= 30) return 30;
    if (w <= 32) return 32;
    if (w <= 40) return 40;
    if (w <= 48) return 48;
    if (w <= 56) return 56;
    return 64;
}

struct HostReader {
    const uint8_t *p;
    int64_t len, at = 0;
    int read()
    {
        if (at >= len) WALK_FAIL("ORC stream: read past the end of an RLE run");
        return p[at++];
    }
    uint64_t vint()
    {
        uint64_t r = 0;
        int off = 0, b;
        do {
            b = read();
            if (off < 64) r |= (uint64_t)(b & 0x7f) << off;
            off += 7;
        } while (b & 0x80);
        return r;
    }
    void skip(int64_t n)
    {
        if (n > len - at) WALK_FAIL("ORC stream: a run is longer than the stream");
        at += n;
    }
};
inline int64_t zigzag(uint64_t v) { return (int64_t)((v >> 1) ^ (~(v & 1) + 1)); }

// the run directory of an RLEv2 stream (LongInputStreamV2.readValues :59-80 and the four readers' header parsing)
inline std::vector<OrcRun> scan_rle_v2(const uint8_t *bytes, int64_t len, bool is_signed, int64_t &total)
{
    std::vector<OrcRun> runs;
    HostReader in{bytes, len};
    total = 0;
    while (in.at < in.len) {
        OrcRun r{};
        const int first = in.read();
        r.kind = (first >> 6) & 3;
        r.out_off = total;
        if (r.kind == SHORT_REPEAT) {   // :255-282
            const int size = ((first >> 3) & 7) + 1;
            r.count = (first & 7) + 3;
            uint64_t v = 0;
            for (int n = size; n > 0;) {
                n--;
                v |= (uint64_t)in.read() << (n * 8);
            }
            r.base = is_signed ? zigzag(v) : (int64_t)v;
            r.in_off = in.at;
        }
        else if (r.kind == DIRECT) {   // :229-252
            r.width = decode_bit_width((first >> 1) & 0x1f);
            r.count = (((first & 1) << 8) | in.read()) + 1;
            r.in_off = in.at;
            in.skip(((int64_t)r.count * r.width + 7) / 8);
        }
        else if (r.kind == PATCHED_BASE) {   // :135-226
            r.width = decode_bit_width((first >> 1) & 0x1f);
            r.count = (((first & 1) << 8) | in.read()) + 1;
            const int third = in.read();
            const int base_width = ((third >> 5) & 7) + 1;
            r.patch_width = decode_bit_width(third & 0x1f);
            const int fourth = in.read();
            r.patch_gap_width = ((fourth >> 5) & 7) + 1;
            r.patch_count = fourth & 0x1f;
            uint64_t b = 0;
            for (int n = base_width; n > 0;) {
                n--;
                b |= (uint64_t)in.read() << (n * 8);
            }
            const uint64_t mask = 1ull << (base_width * 8 - 1);
            r.base = (b & mask) ? (int64_t)(~(b & ~mask) + 1) : (int64_t)b;
            if (r.patch_width + r.patch_gap_width > 64) WALK_FAIL("Invalid RLEv2 encoded stream");
            r.patch_bits = closest_fixed_bits(r.patch_width + r.patch_gap_width);
            r.in_off = in.at;
            in.skip(((int64_t)r.count * r.width + 7) / 8);
            r.patch_off = in.at;
            in.skip(((int64_t)r.patch_count * r.patch_bits + 7) / 8);
        }
        else {   // DELTA :82-132
            int fixed_bits = (first >> 1) & 0x1f;
            if (fixed_bits != 0) fixed_bits = decode_bit_width(fixed_bits);
            const int length = ((first & 1) << 8) | in.read();
            const uint64_t fv = in.vint();
            r.base = is_signed ? zigzag(fv) : (int64_t)fv;
            r.delta = zigzag(in.vint());
            r.width = fixed_bits;
            r.count = length + 1;
            r.in_off = in.at;
            if (fixed_bits != 0) {
                if (length < 1) WALK_FAIL("Invalid RLEv2 encoded stream");
                in.skip(((int64_t)(length - 1) * fixed_bits + 7) / 8);
            }
        }
        total += r.count;
        runs.push_back(r);
    }
    return runs;
}

// RLEv1 (LongInputStreamV1.java:47-103; files written before Hive 0.12): a control byte < 0x80 = a run of control + 3 values base + i * delta
// (delta a signed byte, base a varint); else 0x100 - control literal varints.  The host reads the control bytes and walks the varints'
// continuation bits (it must, to find the next control byte).
inline std::vector<OrcRun> scan_rle_v1(const uint8_t *bytes, int64_t len, bool is_signed, int64_t &total)
{
    std::vector<OrcRun> runs;
    HostReader in{bytes, len};
    total = 0;
    while (in.at < in.len) {
        OrcRun r{};
        const int control = in.read();
        r.out_off = total;
        if (control < 0x80) {
            r.kind = V1_RUN;
            r.count = control + 3;
            r.delta = (int8_t)in.read();
            const uint64_t v = in.vint();
            r.base = is_signed ? zigzag(v) : (int64_t)v;
            r.in_off = in.at;
        } else {
            r.kind = V1_LITERALS;
            r.count = 0x100 - control;
            r.in_off = in.at;
            for (int i = 0; i < r.count; i++) (void)in.vint();
        }
        total += r.count;
        if (total > 0x7fffffffLL) WALK_FAIL("ORC stream holds more than 2^31 values");
        runs.push_back(r);
    }
    return runs;
}

struct ByteRun {
    int64_t in_off, out_off;
    int32_t count, repeat;   // repeat: one value byte at in_off; else `count` literal bytes
};

inline std::vector<ByteRun> scan_byte_rle(const uint8_t *bytes, int64_t len, int64_t &total)   // ByteInputStream.readNextBlock :43-75
{
    std::vector<ByteRun> runs;
    HostReader in{bytes, len};
    total = 0;
    while (in.at < in.len) {
        const int control = in.read();
        ByteRun r{};
        r.out_off = total;
        if ((control & 0x80) == 0) {
            r.count = control + 3;
            r.repeat = 1;
            r.in_off = in.at;
            in.skip(1);
        }
        else {
            r.count = 0x100 - control;
            r.in_off = in.at;
            in.skip(r.count);
        }
        total += r.count;
        runs.push_back(r);
    }
    return runs;
}

// ---- Parquet -----------------------------------------------------------------------------------------------------------------------------------
struct HybridRun {
    int64_t in_off;    // bit-packed run: first byte of the packed values
    int64_t out_off;   // index of the run's first value
    int32_t count;     // values of the run (the last bit-packed run is cut at the number of values wanted: its tail is padding)
    int32_t packed;    // 1 = bit-packed, 0 = RLE
    int64_t value;     // RLE: the repeated value
};

// the run directory of an RLE / bit-packed hybrid stream (Encodings.md; RunLengthBitPackingHybridDecoder.readNext): header = ULEB128;
// bit 0 set: (header >> 1) groups of 8 bit-packed values; clear: a run of header >> 1 copies of one value of ceil(bit_width / 8) bytes
inline std::vector<HybridRun> scan_hybrid(const uint8_t *bytes, int64_t len, int bit_width, int64_t want)
{
    if (!(bit_width >= 0 && bit_width <= 32)) WALK_FAIL("Parquet hybrid stream: bit width out of range");
    std::vector<HybridRun> runs;
    int64_t at = 0, total = 0;
    while (total < want) {
        if (at >= len) WALK_FAIL("Parquet hybrid stream ends before the page's values do");
        uint64_t header = 0;
        for (int shift = 0;; shift += 7) {
            if (at >= len || shift > 35) WALK_FAIL("Parquet hybrid stream: bad run header");
            const int b = bytes[at++];
            header |= (uint64_t)(b & 0x7f) << shift;
            if (!(b & 0x80)) break;
        }
        HybridRun r{};
        r.out_off = total;
        if (header & 1) {
            // (header < 2^42: neither product leaves int64)
            const int64_t values = (int64_t)(header >> 1) * 8, packed_bytes = (int64_t)(header >> 1) * bit_width;
            r.packed = 1;
            r.in_off = at;
            r.count = (int32_t)std::min<int64_t>(values, want - total);
            // (writers may cut the padding of the LAST group short: only the bytes the wanted values occupy must be there)
            if (((int64_t)r.count * bit_width + 7) / 8 > len - at) WALK_FAIL("Parquet hybrid stream: a bit-packed run is longer than the stream");
            at = packed_bytes > len - at ? len : at + packed_bytes;
        } else {
            const int64_t count = (int64_t)(header >> 1);
            const int width_bytes = (bit_width + 7) / 8;
            if (count == 0 || width_bytes > len - at) WALK_FAIL("Parquet hybrid stream: bad RLE run");
            uint64_t v = 0;
            for (int i = 0; i < width_bytes; i++) v |= (uint64_t)bytes[at++] << (8 * i);
            r.value = (int64_t)v;
            r.count = (int32_t)std::min<int64_t>(count, want - total);
        }
        total += r.count;
        runs.push_back(r);
    }
    return runs;
}

// PLAIN BYTE_ARRAY values: where each value's bytes start in `bytes` and how long it is (a 4-byte little-endian length in front of each)
inline void scan_byte_arrays(const uint8_t *bytes, int64_t len, int64_t count, std::vector<int32_t> &src_off, std::vector<int32_t> &lengths)
{
    src_off.clear();
    lengths.clear();
    int64_t at = 0;
    for (int64_t i = 0; i < count; i++) {
        if (4 > len - at) WALK_FAIL("Parquet PLAIN BYTE_ARRAY section ends inside a length");
        uint32_t l;
        memcpy(&l, bytes + at, 4);
        at += 4;
        if (l > 0x7fffffffu || (int64_t)l > len - at) WALK_FAIL("Parquet PLAIN BYTE_ARRAY value is longer than its section");
        if (at > 0x7fffffffLL) WALK_FAIL("Parquet PLAIN BYTE_ARRAY section is larger than 2 GB");
        src_off.push_back((int32_t)at);
        lengths.push_back((int32_t)l);
        at += l;
    }
}

inline bool read_uleb(const uint8_t *bytes, int64_t len, int64_t &at, uint64_t &out)
{
    uint64_t v = 0;
    for (int shift = 0;; shift += 7) {
        if (at >= len || shift > 63) return false;
        const int b = bytes[at++];
        v |= (uint64_t)(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
    }
    out = v;
    return true;
}

// DELTA_BINARY_PACKED (Encodings.md "Delta Encoding"): header: block size, miniblocks per block, total count (ULEB128), first value (zigzag);
// blocks: min delta (zigzag), one bit-width byte per miniblock, the miniblocks' (delta - min delta) bit-packed least significant bit first.
struct Mini {
    int64_t in_off;      // first byte of the miniblock's packed deltas
    int64_t out_off;     // index of the value its first delta produces (>= 1: value 0 is the header's first value)
    int64_t min_delta;
    int32_t count;       // deltas of the miniblock that are values of the page (the last one may be padded)
    int32_t width;
};
struct DeltaPlan {
    std::vector<Mini> minis;
    uint64_t first = 0;   // value 0
    int64_t end = 0;      // the bytes the section takes
};

// the header and block walk of `want` (>= 1) DELTA_BINARY_PACKED values.  The block shape is bounded by the bytes that are there, never by a
// product that could leave int64: values per miniblock fit int32 (Mini.count; a page holds at most 2^31 - 1 values), and a miniblock of
// width > 0 must fit the rest of the section BEFORE its size is multiplied out.
inline DeltaPlan scan_delta(const uint8_t *bytes, int64_t len, int64_t want)
{
    DeltaPlan plan;
    int64_t at = 0;
    uint64_t block_size, miniblocks, total, zz;
    if (!(read_uleb(bytes, len, at, block_size) && read_uleb(bytes, len, at, miniblocks) && read_uleb(bytes, len, at, total) && read_uleb(bytes, len, at, zz)))
        WALK_FAIL("Parquet DELTA_BINARY_PACKED header cut short");
    if (!(miniblocks > 0 && miniblocks <= 4096 && block_size > 0 && block_size % 128 == 0 && block_size % miniblocks == 0 && (block_size / miniblocks) % 32 == 0 &&
          block_size / miniblocks <= 0x7fffffffull))
        WALK_FAIL("Parquet DELTA_BINARY_PACKED block shape outside the specification");
    if (!(total <= 0x7fffffffffffffffull && (int64_t)total >= want)) WALK_FAIL("Parquet DELTA_BINARY_PACKED section holds fewer values than the page has non-null positions");
    const int64_t mini = (int64_t)(block_size / miniblocks);
    plan.first = (zz >> 1) ^ (~(zz & 1) + 1);
    for (int64_t done = 1; done < want;) {
        uint64_t zmin;
        if (!(read_uleb(bytes, len, at, zmin) && (int64_t)miniblocks <= len - at)) WALK_FAIL("Parquet DELTA_BINARY_PACKED block header cut short");
        const uint64_t min_delta = (zmin >> 1) ^ (~(zmin & 1) + 1);
        const uint8_t *widths = bytes + at;
        at += (int64_t)miniblocks;
        for (uint64_t m = 0; m < miniblocks && done < want; m++) {
            const int width = widths[m];
            // (mini is a multiple of 32, so mini * width is a whole number of bytes: this is `at + mini * width / 8 <= len` without the product)
            if (!(width <= 64 && (width == 0 || mini <= (len - at) * 8 / width))) WALK_FAIL("Parquet DELTA_BINARY_PACKED miniblock cut short");
            Mini mb;
            mb.in_off = at;
            mb.out_off = done;
            mb.min_delta = (int64_t)min_delta;
            mb.count = (int32_t)std::min<int64_t>(mini, want - done);
            mb.width = width;
            plan.minis.push_back(mb);
            done += mb.count;
            at += mini * width / 8;
        }
    }
    plan.end = at;
    return plan;
}

// ---- what the kernels rely on: nullptr, or the clause a directory breaks ---------------------------------------------------------------------
inline int64_t bytes_of(int64_t count, int64_t width) { return (count * width + 7) / 8; }

// RLEv2 / RLEv1 (rle_v2_decode_kernel, rle_v1_decode_kernel)
inline const char *check_plan(const std::vector<OrcRun> &runs, const uint8_t *bytes, int64_t len, int64_t total, bool v1)
{
    int64_t sum = 0;
    for (const OrcRun &r : runs) {
        if (r.count < 1 || r.count > (v1 ? 130 : 512)) return "count";
        if (r.width < 0 || r.width > 64) return "width";
        if (r.out_off != sum) return "out_off";
        if (r.in_off < 0 || r.in_off > len) return "in_off";
        if (v1 ? (r.kind != V1_RUN && r.kind != V1_LITERALS) : (r.kind < SHORT_REPEAT || r.kind > DELTA)) return "kind";
        if ((r.kind == DIRECT || r.kind == PATCHED_BASE) && (r.width < 1 || bytes_of(r.count, r.width) > len - r.in_off)) return "packed values past the stream";
        if (r.kind == DELTA && r.width > 0 && (r.count < 2 || bytes_of(r.count - 2, r.width) > len - r.in_off)) return "packed deltas past the stream";
        if (r.kind == PATCHED_BASE) {
            if (r.patch_count < 0 || r.patch_count > 31) return "patch_count";
            if (r.patch_width < 1 || r.patch_gap_width < 1 || r.patch_width + r.patch_gap_width > 64) return "patch_width + patch_gap_width";
            if (r.patch_bits < r.patch_width + r.patch_gap_width || r.patch_bits > 64) return "patch_bits";
            if (r.patch_off < 0 || r.patch_off > len || bytes_of(r.patch_count, r.patch_bits) > len - r.patch_off) return "patch list past the stream";
        }
        if (r.kind == V1_LITERALS) {
            int64_t at = r.in_off;
            for (int i = 0; i < r.count; i++) {
                do {
                    if (at >= len) return "literal varints past the stream";
                } while (bytes[at++] & 0x80);
            }
        }
        sum += r.count;
    }
    return sum == total ? nullptr : "total";
}

// byte-RLE (byte_rle_decode_kernel)
inline const char *check_plan(const std::vector<ByteRun> &runs, int64_t len, int64_t total)
{
    int64_t sum = 0;
    for (const ByteRun &r : runs) {
        if (r.count < 1 || r.count > 130) return "count";
        if (r.out_off != sum) return "out_off";
        if (r.in_off < 0 || (r.repeat ? 1 : r.count) > len - r.in_off) return "bytes past the stream";
        sum += r.count;
    }
    return sum == total ? nullptr : "total";
}

// Parquet hybrid (hybrid_decode_kernel): a bit-packed header of zero groups leaves a run of no values, which reads nothing
inline const char *check_plan(const std::vector<HybridRun> &runs, int64_t len, int bit_width, int64_t want)
{
    int64_t sum = 0;
    if (bit_width < 0 || bit_width > 32) return "bit_width";
    for (const HybridRun &r : runs) {
        if (r.count < 0 || (r.count == 0 && !r.packed)) return "count";
        if (r.out_off != sum) return "out_off";
        if (r.packed && (r.in_off < 0 || r.in_off > len || bytes_of(r.count, bit_width) > len - r.in_off)) return "packed values past the stream";
        sum += r.count;
    }
    if ((int64_t)runs.size() > len) return "more runs than bytes";
    return sum == want ? nullptr : "want";
}

// Parquet delta (delta_unpack_kernel, then the prefix sum over `want` slots)
inline const char *check_plan(const DeltaPlan &plan, int64_t len, int64_t want)
{
    int64_t next = 1;
    if (plan.end < 0 || plan.end > len) return "end";
    for (const Mini &m : plan.minis) {
        if (m.count < 1) return "count";
        if (m.width < 0 || m.width > 64) return "width";
        if (m.out_off < 1 || m.out_off != next || m.out_off + m.count > want) return "out_off";
        if (m.in_off < 0 || m.in_off > plan.end || bytes_of(m.count, m.width) > plan.end - m.in_off) return "packed deltas past the section";
        next += m.count;
    }
    return next == std::max<int64_t>(want, 1) ? nullptr : "want";
}

// PLAIN BYTE_ARRAY (copy_strings_kernel)
inline const char *check_plan(const std::vector<int32_t> &src_off, const std::vector<int32_t> &lengths, int64_t len, int64_t count)
{
    if ((int64_t)src_off.size() != count || (int64_t)lengths.size() != count) return "count";
    for (size_t i = 0; i < src_off.size(); i++)
        if (src_off[i] < 4 || lengths[i] < 0 || (int64_t)lengths[i] > len - src_off[i]) return "value past the section";
    return nullptr;
}

}  // namespace walk
}  // namespace tgpu

// walk_main.cpp -- the host walks of csrc/stream_walk.h as a stand-alone program, for tests/test_stream_walk_cpu.py to build with
// -fsanitize=address,undefined and run as an ordinary child process.
//
//   walk_main CASES
// CASES holds one case per line:  <walker> <is_signed> <bit_width> <want> <count> <hex of the stream, or - for no bytes>
//   walker: rle_v2 | rle_v1 | byte_rle | hybrid | delta | byte_arrays   (scalars a walker does not take are ignored)
// Every stream is copied into a heap buffer of exactly its length, so AddressSanitizer sees any read past it.  Per case one line:
//   <line number> reject | ok <runs> <total> | VIOLATION <clause of check_plan>     then     oracle_reject | oracle_ok <fnv-1a of the values>
// The oracle decoders (oracle/orc_oracle.c, oracle/parquet_oracle.c) decode on the CPU from the same exactly sized buffer: the sanitizers
// check their every read as well.  Exit status 0 = no sanitizer report (they abort the process).
#include "../../presto-1_amd/csrc/stream_walk.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

extern "C" {
int64_t o_orc_rle_v2(const uint8_t *bytes, int64_t len, int32_t is_signed, int64_t *out, int64_t cap);
int64_t o_orc_rle_v1(const uint8_t *bytes, int64_t len, int32_t is_signed, int64_t *out, int64_t cap);
int64_t o_orc_byte_rle(const uint8_t *bytes, int64_t len, uint8_t *out, int64_t cap);
int64_t o_pq_hybrid(const uint8_t *bytes, int64_t len, int32_t bit_width, int32_t *out, int64_t want);
int64_t o_pq_plain_byte_array(const uint8_t *bytes, int64_t len, int64_t count, int32_t *offsets, uint8_t *pool, int64_t pool_cap);
int64_t o_pq_delta_binary_packed(const uint8_t *bytes, int64_t len, int64_t want, int32_t bits, int64_t *out, int64_t *consumed);
}

using namespace tgpu::walk;

static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull)
{
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static int hex_digit(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: walk_main CASES\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    setvbuf(stdout, nullptr, _IOLBF, 0);   // (a sanitizer report ends the process: what was decided before it is on the pipe)
    std::string line;
    for (long number = 1; std::getline(in, line); number++) {
        std::istringstream fields(line);
        std::string walker, hex;
        long long is_signed = 0, bit_width = 0, want = 0, count = 0;
        if (!(fields >> walker >> is_signed >> bit_width >> want >> count >> hex)) {
            fprintf(stderr, "line %ld: malformed case\n", number);
            return 2;
        }
        if (hex == "-") hex.clear();
        const int64_t len = (int64_t)hex.size() / 2;
        // exactly `len` bytes on the heap (one byte for an empty stream, never read: every walker tests the length first)
        uint8_t *bytes = static_cast<uint8_t *>(malloc(len > 0 ? (size_t)len : 1));
        for (int64_t i = 0; i < len; i++) {
            const int hi = hex_digit(hex[2 * i]), lo = hex_digit(hex[2 * i + 1]);
            if (hi < 0 || lo < 0) {
                fprintf(stderr, "line %ld: malformed hex\n", number);
                return 2;
            }
            bytes[i] = (uint8_t)(hi * 16 + lo);
        }
        // what the library bounds before it walks (decode_data_page: n <= 2^31 - 1; dictionary_count >= 0)
        if (want < 0 || want > 0x7fffffffLL || count < 0 || count > 0x7fffffffLL) {
            fprintf(stderr, "line %ld: want / count outside what the library passes to a walker\n", number);
            return 2;
        }
        printf("%ld ", number);
        const char *broken = nullptr;
        bool ok = true;
        size_t runs = 0;
        int64_t total = 0;
        try {
            if (walker == "rle_v2" || walker == "rle_v1") {
                const bool v1 = walker == "rle_v1";
                std::vector<OrcRun> plan = v1 ? scan_rle_v1(bytes, len, is_signed != 0, total) : scan_rle_v2(bytes, len, is_signed != 0, total);
                broken = check_plan(plan, bytes, len, total, v1);
                runs = plan.size();
            }
            else if (walker == "byte_rle") {
                std::vector<ByteRun> plan = scan_byte_rle(bytes, len, total);
                broken = check_plan(plan, len, total);
                runs = plan.size();
            }
            else if (walker == "hybrid") {
                // parquet.hip decode_hybrid: no value wanted or a bit width of 0 (every id is 0; the stream may be empty) never walks
                if (want > 0 && bit_width != 0) {
                    std::vector<HybridRun> plan = scan_hybrid(bytes, len, (int)std::min<long long>(bit_width, 1000), want);
                    broken = check_plan(plan, len, (int)bit_width, want);
                    runs = plan.size();
                }
                total = want;
            }
            else if (walker == "delta") {
                if (want > 0) {   // (delta_column / delta_length_strings / delta_strings: a page without non-null values never walks)
                    DeltaPlan plan = scan_delta(bytes, len, want);
                    broken = check_plan(plan, len, want);
                    runs = plan.minis.size();
                }
                total = want;
            }
            else if (walker == "byte_arrays") {
                std::vector<int32_t> src_off, lengths;
                scan_byte_arrays(bytes, len, count, src_off, lengths);
                broken = check_plan(src_off, lengths, len, count);
                runs = src_off.size();
                total = count;
            }
            else {
                fprintf(stderr, "line %ld: unknown walker %s\n", number, walker.c_str());
                return 2;
            }
        }
        catch (const std::invalid_argument &) {
            ok = false;
        }
        if (!ok) printf("reject ");
        else if (broken) printf("VIOLATION %s ", broken);
        else printf("ok %zu %lld ", runs, (long long)total);

        // the oracle on the same bytes
        int64_t got = -1;
        uint64_t h = 0;
        if (walker == "rle_v2" || walker == "rle_v1") {
            const int64_t cap = 256 * len + 512;   // (no run yields more than 512 values, and none takes fewer than 2 bytes)
            std::unique_ptr<int64_t[]> out(new int64_t[(size_t)cap]);
            got = walker == "rle_v1" ? o_orc_rle_v1(bytes, len, (int32_t)is_signed, out.get(), cap) : o_orc_rle_v2(bytes, len, (int32_t)is_signed, out.get(), cap);
            if (got >= 0) h = fnv(out.get(), (size_t)got * 8);
        }
        else if (walker == "byte_rle") {
            const int64_t cap = 130 * (len + 1);
            std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)cap]);
            got = o_orc_byte_rle(bytes, len, out.get(), cap);
            if (got >= 0) h = fnv(out.get(), (size_t)got);
        }
        else if (walker == "hybrid") {
            std::vector<int32_t> out((size_t)std::max<long long>(want, 1));
            got = o_pq_hybrid(bytes, len, (int32_t)std::min<long long>(bit_width, 1000), out.data(), want);
            if (got >= 0) h = fnv(out.data(), (size_t)got * 4);
            if (got >= 0 && got != want) got = -1;
        }
        else if (walker == "delta") {
            std::vector<int64_t> out((size_t)std::max<long long>(want, 1));
            int64_t consumed = 0;
            got = want > 0 ? o_pq_delta_binary_packed(bytes, len, want, 64, out.data(), &consumed) : 0;
            if (got >= 0) h = fnv(out.data(), (size_t)got * 8);
            if (got >= 0 && got != want) got = -1;
        }
        else {
            std::vector<int32_t> offsets((size_t)count + 1);
            std::vector<uint8_t> pool((size_t)std::max<int64_t>(len, 1));
            got = o_pq_plain_byte_array(bytes, len, count, offsets.data(), pool.data(), len);
            if (got >= 0) h = fnv(pool.data(), (size_t)got, fnv(offsets.data(), offsets.size() * 4));
        }
        if (got < 0) printf("oracle_reject\n");
        else printf("oracle_ok %016llx\n", (unsigned long long)h);
        free(bytes);
    }
    return 0;
}

// Host driver for presto-1_amd/csrc/device_range_frame.h: the text the window kernels compile, compiled as it stands by a host compiler under the
// sanitizers (tests/test_window_range_cpu.py).  Reads partitions from a file and prints every row's frame.
//   P <rows> <start type> <end type> <nulls first>
//   <rows> lines:  <sort key is null> <start comparison code> <end comparison code> <start bound code> <end bound code> <peer start> <peer end>
// Codes are unsigned 64-bit decimals, already complemented for a descending sort.  Every array is allocated with exactly <rows> elements, so a read
// outside the partition is a heap overflow the sanitizer reports.  Output: one line "start end" per row (-1 -1 = empty).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../presto-1_amd/csrc/device_range_frame.h"

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: range_main <cases>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    long long n;
    int start_type, end_type, nulls_first;
    while (fscanf(f, " P %lld %d %d %d", &n, &start_type, &end_type, &nulls_first) == 4) {
        if (n <= 0) return 3;
        std::vector<unsigned long long> start_codes((size_t)n), end_codes((size_t)n), start_bounds((size_t)n), end_bounds((size_t)n);
        std::vector<long long> peer_s((size_t)n), peer_e((size_t)n);
        std::vector<int> key_null((size_t)n);
        for (long long i = 0; i < n; i++) {
            if (fscanf(f, "%d %llu %llu %llu %llu %lld %lld", &key_null[(size_t)i], &start_codes[(size_t)i], &end_codes[(size_t)i], &start_bounds[(size_t)i],
                       &end_bounds[(size_t)i], &peer_s[(size_t)i], &peer_e[(size_t)i]) != 7)
                return 3;
        }
        const long long ps = 0, pe = n - 1;
        long long lo, hi;
        tg_range_run(nulls_first, ps, pe, key_null[0], peer_e[0], key_null[(size_t)pe], peer_s[(size_t)pe], &lo, &hi);
        for (long long i = 0; i < n; i++) {
            long long s, e;
            tg_range_frame(start_type, end_type, i, ps, pe, peer_s[(size_t)i], peer_e[(size_t)i], key_null[(size_t)i], lo, hi, start_codes.data(), start_bounds[(size_t)i],
                           end_codes.data(), end_bounds[(size_t)i], &s, &e);
            printf("%lld %lld\n", s, e);
        }
    }
    fclose(f);
    return 0;
}

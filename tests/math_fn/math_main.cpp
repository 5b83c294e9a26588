// The math-function arithmetic of presto-1_amd/csrc/device_math.h on the CPU: the very text the generated kernels embed, compiled here for the
// host under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_math_functions_cpu.py and run as an ordinary process.
//
//   math_main CASES      one case per line, one result line per case; a double travels as the 16 hex digits of its bits
//     jround  X              Math.round(X) as a decimal long
//     round   X FACTOR       tg_round_double
//     iround  NUM D KIND     round over integers as the generator emits it for D < 0: KIND 0 BIGINT, 1 INTEGER; OVERFLOW for a failing row
//     pow     X Y            tg_pow
//     signum  X
//     trunc   X
#include <math.h>

#include <cstdio>
#include <cstring>

#include "../../presto-1_amd/csrc/device_math.h"

static double from_bits(unsigned long long b)
{
    double x;
    memcpy(&x, &b, 8);
    return x;
}

static void put(double x)
{
    unsigned long long b;
    memcpy(&b, &x, 8);
    printf("%016llx\n", b);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: math_main CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char line[256], op[32];
    long long cases = 0;
    while (fgets(line, sizeof line, f)) {
        cases++;
        unsigned long long a = 0, b = 0;
        long long num = 0;
        int d = 0, kind = 0;
        if (sscanf(line, "%31s", op) != 1) continue;
        if (!strcmp(op, "jround") && sscanf(line, "%*s %llx", &a) == 1) printf("%lld\n", tg_jround(from_bits(a)));
        else if (!strcmp(op, "round") && sscanf(line, "%*s %llx %llx", &a, &b) == 2) put(tg_round_double(from_bits(a), from_bits(b)));
        else if (!strcmp(op, "pow") && sscanf(line, "%*s %llx %llx", &a, &b) == 2) put(tg_pow(from_bits(a), from_bits(b)));
        else if (!strcmp(op, "signum") && sscanf(line, "%*s %llx", &a) == 1) put(tg_signum(from_bits(a)));
        else if (!strcmp(op, "trunc") && sscanf(line, "%*s %llx", &a) == 1) put(tg_truncate(from_bits(a)));
        else if (!strcmp(op, "iround") && sscanf(line, "%*s %lld %d %d", &num, &d, &kind) == 3 && d < 0) {
            int overflow = d < -18;   // checkedPow(10, -d) overflows
            long long r = 0;
            if (!overflow) {
                long long factor = 1;
                for (int k = 0; k < -d; k++) factor *= 10;
                r = tg_round_long(num, factor, &overflow);
                if (kind == 1 && (r > 2147483647LL || r < -2147483648LL)) overflow = 1;
            }
            if (overflow) printf("OVERFLOW\n");
            else printf("%lld\n", r);
        }
        else {
            fprintf(stderr, "case %lld: bad case %s", cases, line);
            return 2;
        }
    }
    fclose(f);
    fprintf(stderr, "%lld cases\n", cases);
    return 0;
}

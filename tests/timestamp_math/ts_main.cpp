// The TIMESTAMP arithmetic of presto-1_amd/csrc/device_timestamp.h (over device_date.h's calendar) on the CPU: the very text the generated
// kernels embed, compiled here for the host under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_timestamp_functions_cpu.py and
// run as an ordinary process.
//
//   ts_main CASES        one case per line: "<op> <k> <a> <b>", one result line per case
//     all        - t -        the thirteen integer unary functions of timestamp t in the order of the model's UNARY_NAMES, then the bits of
//                             to_unixtime(t) as a signed 64-bit integer
//     date_trunc U t -        U = 0 millisecond, 1 second, 2 minute, 3 hour, 4 day, 5 week, 6 month, 7 quarter, 8 year
//     date_add   U*8+P v t    P = the argument's precision, 0..6
//     date_diff  U t1 t2
//     cast       Q t -        CAST(timestamp AS timestamp(Q))
//     from_date  - d -        CAST(date AS timestamp)
//     to_date    - t -        CAST(timestamp AS date)
//   A result that is no int64 count of microseconds, or an amount outside int32, prints as OVERFLOW.
#include <cstdio>
#include <cstring>

#include "../../presto-1_amd/csrc/device_date.h"
#include "../../presto-1_amd/csrc/device_timestamp.h"

static void put(long long value, int overflow)
{
    if (overflow) printf("OVERFLOW\n");
    else printf("%lld\n", value);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: ts_main CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char op[32], k_text[32];
    long long a = 0, b = 0;
    long long cases = 0;
    while (fscanf(f, "%31s %31s %lld %lld", op, k_text, &a, &b) == 4) {
        cases++;
        int k = -1;
        if (strcmp(k_text, "-") != 0 && (sscanf(k_text, "%d", &k) != 1 || k < 0)) {
            fprintf(stderr, "case %lld: bad parameter %s\n", cases, k_text);
            return 2;
        }
        int overflow = 0;
        if (!strcmp(op, "all")) {
            const int d = tg_ts_date(a);
            const int last = tg_date_last_day_of_month(d, &overflow);
            const double unix_time = (double)a / 1000000.0;
            long long bits;
            memcpy(&bits, &unix_time, 8);
            printf("%lld %lld %lld %lld %lld %lld %lld %lld %d %lld %lld %lld %lld %lld\n", tg_date_year(d), tg_date_quarter(d), tg_date_month(d), tg_date_week(d),
                   tg_date_day(d), tg_date_day_of_week(d), tg_date_day_of_year(d), tg_date_year_of_week(d), last, tg_ts_hour(a), tg_ts_minute(a), tg_ts_second(a),
                   tg_ts_millisecond(a), bits);
            if (overflow) {
                fprintf(stderr, "case %lld: last_day_of_month of a timestamp overflowed\n", cases);
                return 2;
            }
        }
        else if (!strcmp(op, "date_trunc") && k >= 0 && k <= TG_TS_UNIT_YEAR) {
            const long long r = tg_ts_trunc(k, a, &overflow);
            put(r, overflow);
        }
        else if (!strcmp(op, "date_add") && k >= 0 && k / 8 <= TG_TS_UNIT_YEAR && k % 8 <= 6) {
            const long long r = tg_ts_add(k / 8, a, b, k % 8, &overflow);
            put(r, overflow);
        }
        else if (!strcmp(op, "date_diff") && k >= 0 && k <= TG_TS_UNIT_YEAR) put(tg_ts_diff(k, a, b), 0);
        else if (!strcmp(op, "cast") && k >= 0 && k <= 6) put(tg_ts_cast_precision(a, k), 0);
        else if (!strcmp(op, "from_date") && a >= -2147483648LL && a <= 2147483647LL) put(tg_ts_from_date((int)a), 0);
        else if (!strcmp(op, "to_date")) put(tg_ts_to_date(a), 0);
        else {
            fprintf(stderr, "case %lld: bad case %s %s %lld %lld\n", cases, op, k_text, a, b);
            return 2;
        }
    }
    fclose(f);
    fprintf(stderr, "%lld cases\n", cases);
    return 0;
}

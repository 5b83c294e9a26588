// The calendar arithmetic of presto-1_amd/csrc/device_date.h on the CPU: the very text the generated kernels embed, compiled here for the
// host under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_date_functions_cpu.py and run as an ordinary process.
//
//   date_main CASES      one case per line: "<op> <unit> <a> <b>", one result line per case
//     all        - d -        the nine unary functions of day d, in the order of the IR's op values (last_day_of_month last)
//     date_trunc U d -        U = 0 day, 1 week, 2 month, 3 quarter, 4 year
//     date_add   U v d
//     date_diff  U d1 d2
//   A result that is no int32 day count, or an amount outside int32, prints as OVERFLOW.
#include <cstdio>
#include <cstring>

#include "../../presto-1_amd/csrc/device_date.h"

static void put_date(int value, int overflow, const char *end)
{
    if (overflow) printf("OVERFLOW%s", end);
    else printf("%d%s", value, end);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: date_main CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char op[32], unit_text[32];
    long long a = 0, b = 0;
    long long cases = 0;
    while (fscanf(f, "%31s %31s %lld %lld", op, unit_text, &a, &b) == 4) {
        cases++;
        int unit = -1;
        if (strcmp(unit_text, "-") != 0 && (sscanf(unit_text, "%d", &unit) != 1 || unit < TG_DATE_UNIT_DAY || unit > TG_DATE_UNIT_YEAR)) {
            fprintf(stderr, "case %lld: bad unit %s\n", cases, unit_text);
            return 2;
        }
        const bool date_a = a >= -2147483648LL && a <= 2147483647LL, date_b = b >= -2147483648LL && b <= 2147483647LL;
        int overflow = 0;
        if (!strcmp(op, "all") && date_a) {
            const int d = (int)a;
            printf("%lld %lld %lld %lld %lld %lld %lld %lld ", tg_date_year(d), tg_date_quarter(d), tg_date_month(d), tg_date_week(d), tg_date_day(d),
                   tg_date_day_of_week(d), tg_date_day_of_year(d), tg_date_year_of_week(d));
            const int last = tg_date_last_day_of_month(d, &overflow);
            put_date(last, overflow, "\n");
        }
        else if (!strcmp(op, "date_trunc") && unit >= 0 && date_a) {
            const int r = tg_date_trunc(unit, (int)a, &overflow);
            put_date(r, overflow, "\n");
        }
        else if (!strcmp(op, "date_add") && unit >= 0 && date_b) {
            const int r = tg_date_add(unit, a, (int)b, &overflow);
            put_date(r, overflow, "\n");
        }
        else if (!strcmp(op, "date_diff") && unit >= 0 && date_a && date_b) printf("%lld\n", tg_date_diff(unit, (int)a, (int)b));
        else {
            fprintf(stderr, "case %lld: bad case %s %s %lld %lld\n", cases, op, unit_text, a, b);
            return 2;
        }
    }
    fclose(f);
    fprintf(stderr, "%lld cases\n", cases);
    return 0;
}

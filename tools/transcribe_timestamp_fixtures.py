#!/usr/bin/env python3
"""Transcribes the short-precision literals of the reference's timestamp tests into tests/golden/timestamp_function_vectors.json (data only: the SQL
text of each case, its pieces, its source line and the expected value).

Run in the build container (reads the reference as text; the reference is Java and is not executed):

    python tools/transcribe_timestamp_fixtures.py

Sources, under core/trino-main/src/test/java/io/trino/operator/scalar/timestamp: TestExtract.java, TestDateTrunc.java, TestTimestamp.java and
TestOperators.java.  A line is taken when it is `assertThat(assertions.expression("<sql>")).matches("<literal>")` (TestOperators: .isEqualTo(true /
false)), its SQL is one of the forms below and every timestamp in it has at most 6 fractional digits (timestamp(p), p <= 6: the type of the IR):

    EXTRACT(field FROM TIMESTAMP '..') / field(TIMESTAMP '..')     BIGINT literal          -> "extract"
    last_day_of_month(TIMESTAMP '..')                              DATE literal            -> "last_day_of_month"
    to_unixtime(TIMESTAMP '..')                                    DOUBLE literal          -> "to_unixtime"
    date_trunc('unit', TIMESTAMP '..')                             TIMESTAMP literal       -> "date_trunc"
    date_add('unit', n, TIMESTAMP '..')                            TIMESTAMP literal       -> "date_add" (precision = the literal's digits)
    date_diff('unit', TIMESTAMP '..', TIMESTAMP '..')              BIGINT literal          -> "date_diff"
    CAST(TIMESTAMP '..' AS TIMESTAMP(q)), q <= 6                   TIMESTAMP literal       -> "cast_precision"
    CAST(TIMESTAMP '..' AS DATE)                                   DATE literal            -> "to_date"
    CAST(DATE '..' AS TIMESTAMP(q)), q <= 6                        TIMESTAMP literal       -> "from_date"
    TIMESTAMP '..' <op> TIMESTAMP '..', BETWEEN                    true / false            -> "compare"

Timestamps are written as microseconds since 1970-01-01 00:00:00, days as days since 1970-01-01.  Every other assertion line of the four files
-- long timestamps, time zones, TIME, VARCHAR casts, formats, intervals -- is outside the IR: counted per file in "_comment", never guessed at."""
import datetime
import json
import os
import re

REF = "/root/reference/core/trino-main/src/test/java/io/trino/operator/scalar/timestamp/"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "timestamp_function_vectors.json")
EPOCH = datetime.datetime(1970, 1, 1)
ALIASES = {"day_of_month": "day", "dow": "day_of_week", "doy": "day_of_year", "week_of_year": "week", "yow": "year_of_week"}
FIELDS = ("year", "quarter", "month", "week", "day", "day_of_week", "day_of_year", "year_of_week", "hour", "minute", "second", "millisecond")
TS = r"TIMESTAMP '(\d{4}-\d\d-\d\d \d\d:\d\d:\d\d(?:\.\d+)?)'"
DATE = r"DATE '(\d{4}-\d\d-\d\d)'"
OPS = {"=": "EQUAL", "<>": "NOT_EQUAL", "!=": "NOT_EQUAL", "<": "LESS_THAN", "<=": "LESS_THAN_OR_EQUAL", ">": "GREATER_THAN", ">=": "GREATER_THAN_OR_EQUAL"}


class Long(Exception):
    """a timestamp of more than 6 fractional digits"""


def micros(text):
    """'YYYY-MM-DD HH:MM:SS[.f]' -> (microseconds, precision)"""
    head, _, frac = text.partition(".")
    if len(frac) > 6:
        raise Long(text)
    dt = datetime.datetime.strptime(head, "%Y-%m-%d %H:%M:%S")
    return (dt - EPOCH) // datetime.timedelta(microseconds=1) + int((frac + "000000")[:6]), len(frac)


def days(text):
    return (datetime.datetime.strptime(text, "%Y-%m-%d") - EPOCH).days


def read(sql, expected):
    """-> (group, case) or None"""
    f = re.fullmatch
    m = f(r"(?i)extract\((\w+) FROM " + TS + r"\)", sql) or f(r"(\w+)\(" + TS + r"\)", sql)
    if m:
        name = ALIASES.get(m.group(1).lower(), m.group(1).lower())
        us, p = micros(m.group(2))
        e = f(r"BIGINT '(-?\d+)'", expected)
        if name in FIELDS and e:
            return "extract", {"function": name, "us": us, "precision": p, "expected": int(e.group(1))}
        e = f(DATE, expected)
        if name == "last_day_of_month" and e:
            return "last_day_of_month", {"us": us, "precision": p, "expected": days(e.group(1))}
        e = f(r"(-?\d+(?:\.\d+)?)e0", expected)
        if name == "to_unixtime" and e:
            return "to_unixtime", {"us": us, "precision": p, "expected": float(e.group(1))}
        return None
    m = f(r"date_trunc\('(\w+)', " + TS + r"\)", sql)
    e = f(TS, expected)
    if m and e:
        us, p = micros(m.group(2))
        return "date_trunc", {"unit": m.group(1), "us": us, "precision": p, "expected": micros(e.group(1))[0]}
    m = f(r"date_add\('(\w+)', (-?\d+), " + TS + r"\)", sql)
    if m and e:
        us, p = micros(m.group(3))
        return "date_add", {"unit": m.group(1), "value": int(m.group(2)), "us": us, "precision": p, "expected": micros(e.group(1))[0]}
    m = f(r"date_diff\('(\w+)', " + TS + ", " + TS + r"\)", sql)
    b = f(r"BIGINT '(-?\d+)'", expected)
    if m and b:
        (us1, p1), (us2, p2) = micros(m.group(2)), micros(m.group(3))
        return "date_diff", {"unit": m.group(1), "us1": us1, "us2": us2, "precision": max(p1, p2), "expected": int(b.group(1))}
    m = f(r"CAST\(" + TS + r" AS TIMESTAMP\((\d+)\)\)", sql)
    if m and e:
        if int(m.group(2)) > 6:
            raise Long(sql)
        us, p = micros(m.group(1))
        return "cast_precision", {"us": us, "precision": p, "target": int(m.group(2)), "expected": micros(e.group(1))[0]}
    m = f(r"CAST\(" + TS + r" AS DATE\)", sql)
    d = f(DATE, expected)
    if m and d:
        us, p = micros(m.group(1))
        return "to_date", {"us": us, "precision": p, "expected": days(d.group(1))}
    m = f(r"CAST\(" + DATE + r" AS TIMESTAMP\((\d+)\)\)", sql)
    if m and e:
        if int(m.group(2)) > 6:
            raise Long(sql)
        return "from_date", {"day": days(m.group(1)), "target": int(m.group(2)), "expected": micros(e.group(1))[0]}
    m = f(TS + r" (=|<>|!=|<|<=|>|>=) " + TS, sql)
    if m and expected in ("true", "false"):
        return "compare", {"op": OPS[m.group(2)], "us1": micros(m.group(1))[0], "us2": micros(m.group(3))[0], "expected": expected == "true"}
    m = f(TS + " BETWEEN " + TS + " AND " + TS, sql)
    if m and expected in ("true", "false"):
        return "compare", {"op": "BETWEEN", "us1": micros(m.group(1))[0], "us2": micros(m.group(2))[0], "us3": micros(m.group(3))[0], "expected": expected == "true"}
    return None


def main():
    groups = {k: [] for k in ("extract", "last_day_of_month", "to_unixtime", "date_trunc", "date_add", "date_diff", "cast_precision", "to_date", "from_date", "compare")}
    outside = {}
    for name in ("TestExtract.java", "TestDateTrunc.java", "TestTimestamp.java", "TestOperators.java"):
        outside[name] = {"long_or_precision_above_6": 0, "other_forms": 0}
        for no, line in enumerate(open(REF + name).read().split("\n"), 1):
            m = re.search(r'assertions\.expression\("(.*)"\)\)\s*\.(?:matches\("(.*)"\)|isEqualTo\((true|false)\))', line)
            if not m:
                if "assertions." in line:
                    outside[name]["other_forms"] += 1
                continue
            sql, expected = m.group(1), m.group(2) if m.group(2) is not None else m.group(3)
            try:
                got = read(sql, expected)
            except Long:
                outside[name]["long_or_precision_above_6"] += 1
                continue
            except ValueError:
                got = None
            if got is None:
                outside[name]["other_forms"] += 1
                continue
            group, case = got
            groups[group].append(dict({"source": name, "line": no, "sql": sql}, **case))
    total_outside = sum(sum(v.values()) for v in outside.values())
    doc = {"_comment": "Transcribed by tools/transcribe_timestamp_fixtures.py from the reference's operator/scalar/timestamp tests: the lines whose timestamps are "
                       "timestamp(p), p <= 6.  Microseconds / days since 1970-01-01.  Assertion lines outside the IR, per file: " + json.dumps(outside, sort_keys=True),
           "lines_outside_the_ir": total_outside, "outside": outside}
    doc.update(groups)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in groups.items()}, outside)


if __name__ == "__main__":
    main()

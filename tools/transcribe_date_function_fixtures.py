#!/usr/bin/env python3
"""Transcribes the DATE cases of the reference's date-function tests into tests/golden/date_function_vectors.json (data only: the SQL text of
each case, its pieces, its source line and the expected value).

Run in the build container (reads the reference as text; the reference is Java and is not executed):

    python tools/transcribe_date_function_fixtures.py

Sources, under core/trino-main/src/test/java/io/trino/operator/scalar:
    date/TestExtract.java                      every case: EXTRACT(field FROM DATE '...') and field(DATE '...') with a BIGINT literal
    TestDateTimeFunctions.java
        testYearOfWeek       :426-434          the DATE lines (the TIMESTAMP lines are outside the IR: skipped and counted)
        testLastDayOfMonth   :440-444          the DATE lines
        testExtractFromDate  :516-538
        testTruncateDate     :652-668
        testAddFieldToDate   :698-705
        testDateDiffDate     :770-779
The first three groups state their expectation as a literal.  The last three compute it with Joda calls on the test's date
(DATE_LITERAL, :101); their expectation is worked out here with Python's datetime from the SQL text alone and the case names its source line,
where the reference's own expression can be read.  Day numbers count from 1970-01-01.  A line this script cannot read fully is skipped and
counted."""
import datetime
import json
import os
import re

REF = "/root/reference/core/trino-main/src/test/java/io/trino/operator/scalar/"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "date_function_vectors.json")
EPOCH = datetime.date(1970, 1, 1)
ALIASES = {"day_of_month": "day", "dow": "day_of_week", "doy": "day_of_year", "week_of_year": "week", "yow": "year_of_week"}
FIELDS = ("year", "quarter", "month", "week", "day", "day_of_week", "day_of_year", "year_of_week")
DATE_SQL = r"DATE '(\d{4})-(\d\d)-(\d\d)'"


def day_number(y, m, d):
    return (datetime.date(int(y), int(m), int(d)) - EPOCH).days


def lines(path, first=1, last=None):
    text = open(REF + path).read().split("\n")
    return [(i + 1, text[i]) for i in range(first - 1, len(text) if last is None else last)]


def extract_case(no, source, sql, expected):
    """EXTRACT(F FROM DATE '...') or f(DATE '...') -> a case, or None when the argument is no DATE literal"""
    m = re.fullmatch(r"(?i)extract\((\w+) FROM " + DATE_SQL + r"\)", sql) or re.fullmatch(r"(\w+)\(" + DATE_SQL + r"\)", sql)
    if not m:
        return None
    name = m.group(1).lower()
    fn = ALIASES.get(name, name)
    if fn not in FIELDS:
        return None
    return {"source": source, "line": no, "sql": sql, "function": fn, "date": "%s-%s-%s" % m.group(2, 3, 4), "day": day_number(*m.group(2, 3, 4)), "expected": int(expected)}


def add_months(date, n):
    k = date.year * 12 + date.month - 1 + n
    y, m = k // 12, k % 12 + 1
    for d in range(date.day, 0, -1):
        try:
            return datetime.date(y, m, d)
        except ValueError:
            continue


def main():
    main_file = "TestDateTimeFunctions.java"
    out = {"source": "core/trino-main/src/test/java/io/trino/operator/scalar/{date/TestExtract.java, TestDateTimeFunctions.java}",
           "extract": [], "last_day_of_month": [], "date_trunc": [], "date_add": [], "date_diff": []}
    skipped = 0
    for no, l in lines("date/TestExtract.java"):
        m = re.search(r'assertions\.expression\("([^"]*)"\)\)\.matches\("BIGINT \'(-?\d+)\'"\)', l)
        case = extract_case(no, "date/TestExtract.java", m.group(1), m.group(2)) if m else None
        if case:
            out["extract"].append(case)
        elif "assert" in l and "import" not in l:
            skipped += 1
    literal = None
    for no, l in lines(main_file, 95, 110):
        m = re.search(r'String DATE_LITERAL = "(' + DATE_SQL + ')";', l)
        if m:
            literal = m.group(1)
    base = datetime.date(*[int(x) for x in re.fullmatch(DATE_SQL, literal).groups()])
    base_day = (base - EPOCH).days

    def sql_of(l):
        """the SQL text of an assertFunction line, DATE_LITERAL spliced in"""
        m = re.search(r'assertFunction\("((?:[^"]|" \+ \w+ \+ ")*)", ', l)
        if not m:
            return None
        parts = re.split(r'" \+ (\w+) \+ "', m.group(1))
        for i in range(1, len(parts), 2):
            parts[i] = {"DATE_LITERAL": literal, "baseDateTimeLiteral": "DATE '1960-05-03'"}.get(parts[i])
            if parts[i] is None:
                return None
        return "".join(parts)

    for first, last in ((426, 434), (516, 538)):
        for no, l in lines(main_file, first, last):
            sql = sql_of(l)
            m = re.search(r", BIGINT, (-?\d+)L\);", l)
            case = extract_case(no, main_file, sql, m.group(1)) if sql and m else None
            if case:
                out["extract"].append(case)
            elif "assertFunction" in l:
                skipped += 1
    for no, l in lines(main_file, 440, 444):
        sql = sql_of(l)
        m = re.fullmatch(r"last_day_of_month\(" + DATE_SQL + r"\)", sql or "")
        lit = re.search(r"LocalDate\.of\((\d+), (\d+), (\d+)\)", l)
        if m:
            # the expectation: a LocalDate literal, or day 31 of the test date's month
            want = datetime.date(*[int(x) for x in lit.groups()]) if lit else base.replace(day=31)
            out["last_day_of_month"].append({"source": main_file, "line": no, "sql": sql, "date": "%s-%s-%s" % m.groups(), "day": day_number(*m.groups()),
                                             "expected_date": want.isoformat(), "expected": (want - EPOCH).days})
        elif "assertFunction" in l:
            skipped += 1
    for no, l in lines(main_file, 652, 668):
        sql = sql_of(l)
        m = re.fullmatch(r"date_trunc\('(\w+)', " + DATE_SQL + r"\)", sql or "")
        if m:
            u = m.group(1)
            want = {"day": base, "week": base - datetime.timedelta(days=base.weekday()), "month": base.replace(day=1),
                    "quarter": base.replace(month=(base.month - 1) // 3 * 3 + 1, day=1), "year": base.replace(month=1, day=1)}[u]
            out["date_trunc"].append({"source": main_file, "line": no, "sql": sql, "unit": u, "day": base_day, "expected_date": want.isoformat(), "expected": (want - EPOCH).days})
        elif "assertFunction" in l:
            skipped += 1
    months = {"month": 1, "quarter": 3, "year": 12}
    for no, l in lines(main_file, 698, 705):
        sql = sql_of(l)
        m = re.fullmatch(r"date_add\('(\w+)', (-?\d+), " + DATE_SQL + r"\)", sql or "")
        if m:
            u, v = m.group(1), int(m.group(2))
            want = base + datetime.timedelta(days=v * (7 if u == "week" else 1)) if u in ("day", "week") else add_months(base, v * months[u])
            out["date_add"].append({"source": main_file, "line": no, "sql": sql, "unit": u, "value": v, "day": base_day, "expected_date": want.isoformat(), "expected": (want - EPOCH).days})
        elif "assertFunction" in l:
            skipped += 1
    for no, l in lines(main_file, 770, 779):
        sql = sql_of(l)
        m = re.fullmatch(r"date_diff\('(\w+)', " + DATE_SQL + ", " + DATE_SQL + r"\)", sql or "")
        if m:
            u = m.group(1)
            a, b = datetime.date(*[int(x) for x in m.group(2, 3, 4)]), datetime.date(*[int(x) for x in m.group(5, 6, 7)])
            assert a <= b
            whole = (b.year - a.year) * 12 + b.month - a.month - (b.day < a.day)     # a.day <= 28 here: no clamping arises
            assert a.day <= 28
            want = (b - a).days // (7 if u == "week" else 1) if u in ("day", "week") else whole // months[u]
            out["date_diff"].append({"source": main_file, "line": no, "sql": sql, "unit": u, "day1": (a - EPOCH).days, "day2": (b - EPOCH).days, "expected": want})
        elif "assertFunction" in l:
            skipped += 1
    out["skipped_lines"] = skipped
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print({k: len(v) for k, v in out.items() if isinstance(v, list)}, "skipped", skipped)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Transcribes the cases of the reference's T/sql/query/TestWindowFrameRange.java into tests/golden/window_range_vectors.json: data only.

    python tools/transcribe_window_range_fixtures.py <reference checkout> [output.json]

Every assertThat(assertions.query(..)).matches(..) becomes one entry: the sort order, the partition column, the bounds, the input rows and the expected
row per output (array_agg as a list).  DATE values are ISO strings, INTERVAL YEAR TO MONTH values their month counts (key type BIGINT), decimal and
REAL values floats (key type DOUBLE).  The assertThatThrownBy cases of testInvalidOffset are listed with a "skip" reason: the check they are about is
the planner's, in front of the operator.  The avg(number) column of testMultipleWindowFunctions is marked skipped inside its entry."""
import json
import os
import re
import sys

DATE = re.compile(r"^\d{4}-\d{2}-\d{2}$")


def literals(text):
    """the concatenation of the Java string literals of `text`"""
    return "".join(m.group(1) for m in re.finditer(r'"((?:[^"\\]|\\.)*)"', text))


def split_top(text, sep=","):
    out, depth, quote, cur, i = [], 0, False, "", 0
    while i < len(text):
        c = text[i]
        if c == "'":
            quote = not quote
        if not quote and c in "([":
            depth += 1
        if not quote and c in ")]":
            depth -= 1
        if not quote and depth == 0 and text.startswith(sep, i):
            out.append(cur.strip())
            cur = ""
            i += len(sep)
            continue
        cur += c
        i += 1
    if cur.strip():
        out.append(cur.strip())
    return out


def item(text, seen):
    text = text.strip()
    if text.startswith("CAST("):
        return item(split_top(text[5:-1], " AS ")[0], seen)
    if text.startswith("ARRAY["):
        return [item(x, seen) for x in split_top(text[6:-1])]
    if text.startswith("("):
        return [item(x, seen) for x in split_top(text[1:-1])]
    if text == "null":
        return None
    m = re.match(r"^INTERVAL '(-?\d+)' (month|year)$", text, re.I)
    if m:
        seen.add("interval")
        return int(m.group(1)) * (12 if m.group(2).lower() == "year" else 1)
    m = re.match(r"^DATE '(.*)'$", text)
    if m:
        return m.group(1)
    m = re.match(r"^(REAL|DOUBLE) '(.*)'$", text)
    if m:
        return float(m.group(2))
    m = re.match(r"^(TINYINT|SMALLINT|INTEGER|BIGINT) '(.*)'$", text)
    if m:
        return int(m.group(2))
    if text.startswith("'"):
        return text[1:-1]
    return float(text) if re.search(r"[.e]", text) else int(text)


def bound(text, seen):
    text = text.strip()
    if text in ("UNBOUNDED PRECEDING", "UNBOUNDED FOLLOWING"):
        return {"type": text.replace(" ", "_")}
    if text == "CURRENT ROW":
        return {"type": "CURRENT_ROW"}
    expr, kind = text.rsplit(" ", 1)
    b = {"type": kind}
    m = re.match(r"^interval '(\d+)' (\w+)$", expr)
    if m:
        if "interval" in seen:    # an interval key: plain months
            b["value"] = int(m.group(1)) * (12 if m.group(2) == "year" else 1)
        else:
            b["value"], b["unit"] = int(m.group(1)), m.group(2)
        return b
    m = re.match(r"^(\w) ([*/]) ([\d.]+)$", expr)
    if m:
        b["column"], b["op"], b["by"] = m.group(1), m.group(2), float(m.group(3))
        return b
    b["value"] = item(expr, set())
    return b


def window(text, seen):
    m = re.match(r"^(?:PARTITION BY (\w+) )?ORDER BY (\w+)(?: (ASC|DESC))?(?: NULLS (FIRST|LAST))? RANGE (.*)$", text)
    partition, key, direction, nulls, frame = m.groups()
    m = re.match(r"^BETWEEN (.*) AND (.*)$", frame)
    start, end = (m.group(1), m.group(2)) if m else (frame, "CURRENT ROW")
    return {"partition": partition, "key": key, "order": "%s_NULLS_%s" % (direction or "ASC", nulls or "LAST"), "start": bound(start, seen), "end": bound(end, seen)}


def key_type(values, seen):
    present = [v for v in values if v is not None]
    if "interval" in seen:
        return "BIGINT"
    if any(isinstance(v, str) and DATE.match(v) for v in present):
        return "DATE"
    return "DOUBLE" if any(isinstance(v, float) for v in present) else "INTEGER"


def case(test, sql, values):
    seen = set()
    m = re.match(r"^SELECT (.*) FROM \(VALUES (.*)\) T\((.*)\)$", sql)
    select, rows, columns = split_top(m.group(1)), split_top(m.group(2)), [c.strip() for c in m.group(3).split(",")]
    rows = [item(r, seen) for r in rows]
    rows = [r if isinstance(r, list) else [r] for r in rows]
    outputs = []
    for s in select:
        m = re.match(r"^(\w+)\((\w+)\) OVER\((.*)\)$", s)
        if not m:
            outputs.append({"column": s})
            continue
        w = window(m.group(3), seen)
        w["function"], w["argument"] = m.group(1), m.group(2)
        if m.group(1) != "array_agg":
            w["skip"] = "window avg is refused (TGPU_ERR_NOT_SUPPORTED): the reference accumulates it in a double, left to right"
        outputs.append(w)
    expected = [item(r, seen) for r in split_top(values[len("VALUES "):])]
    if len(outputs) == 1:
        expected = [[e] for e in expected]
    keys = {o["key"] for o in outputs if "key" in o}
    assert len(keys) == 1
    key = keys.pop()
    return {"test": test, "sql": sql, "columns": columns, "key": key, "key_type": key_type([r[columns.index(key)] for r in rows], seen), "rows": rows, "outputs": outputs,
            "expected": expected}


def main():
    source = open(os.path.join(sys.argv[1], "core/trino-main/src/test/java/io/trino/sql/query/TestWindowFrameRange.java")).read()
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "window_range_vectors.json")
    cases = []
    for test in re.finditer(r"public void (test\w+)\(\)\s*\{(.*?)\n    \}", source, re.S):
        name, body = test.group(1), test.group(2)
        for m in re.finditer(r"assertThat\(assertions\.query\((.*?)\)\)\s*\.matches\((.*?)\);", body, re.S):
            cases.append(case(name, literals(m.group(1)), literals(m.group(2))))
        for m in re.finditer(r"assertThatThrownBy\(\(\) -> assertions\.query\((.*?)\)\)\s*\.hasMessage\((.*?)\);", body, re.S):
            cases.append({"test": name, "sql": literals(m.group(1)), "message": literals(m.group(2)),
                          "skip": "the offset check is the planner's fail() filter in front of the operator"})
    with open(out, "w") as f:
        json.dump({"source": "T/sql/query/TestWindowFrameRange.java", "cases": cases}, f, indent=1)
        f.write("\n")
    print(len(cases), "cases,", sum("skip" in c for c in cases), "skipped ->", out)


if __name__ == "__main__":
    main()

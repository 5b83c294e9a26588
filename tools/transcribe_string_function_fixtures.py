#!/usr/bin/env python3
"""Transcribes the literals of the reference's string-function tests into tests/golden/string_function_vectors.json (data only: the
arguments and the literal results, each with its source line).

Run in the build container (reads the reference as text; the reference is Java and is not executed):

    python tools/transcribe_string_function_fixtures.py

Source: core/trino-main/src/test/java/io/trino/operator/scalar/TestStringFunctions.java
    testConcat          :107-121  CONCAT(...) of literals, nested or n-ary (written as a tree: a string or {"concat": [args]}), and the
                                  one-argument failure with its message
    testLength          :132-141
    testStringPosition  :267-315  the two-argument STRPOS lines (through testStrPosAndPosition or direct) and the STARTS_WITH lines; the
                                  three-argument lines are outside the IR: skipped and counted
    testSubstring       :353-386  SUBSTR(v, start[, length]) and SUBSTRING(v FROM start [FOR length])
A line this script cannot read fully is skipped and counted."""
import json
import os
import re

REF = "/root/reference/core/trino-main/src/test/java/io/trino/operator/scalar/TestStringFunctions.java"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "string_function_vectors.json")
JSTR = r'"((?:[^"\\]|\\.)*)"'


class Skip(Exception):
    pass


def junescape(s):
    out, i = [], 0
    while i < len(s):
        c = s[i]
        if c != "\\":
            out.append(c)
            i += 1
            continue
        n = s[i + 1]
        if n == "\\":
            out.append("\\")
        elif n == "u":
            out.append(chr(int(s[i + 2:i + 6], 16)))
            i += 4
        else:
            raise Skip(s)
        i += 2
    return "".join(out).encode("utf-16", "surrogatepass").decode("utf-16")   # surrogate pairs -> one code point


def lines(first, last):
    text = open(REF).read().split("\n")
    return [(i + 1, text[i]) for i in range(first - 1, last)]


def sql_string(s):
    s = s.strip()
    if s == "NULL":
        return None
    if len(s) >= 2 and s[0] == "'" and s[-1] == "'" and "'" not in s[1:-1]:
        return s[1:-1]
    raise Skip(s)


def split_args(s):
    out, depth, quote, cur = [], 0, False, ""
    for c in s:
        if c == "'":
            quote = not quote
        if not quote and c == "(":
            depth += 1
        if not quote and c == ")":
            depth -= 1
        if not quote and depth == 0 and c == ",":
            out.append(cur)
            cur = ""
        else:
            cur += c
    out.append(cur)
    return [a.strip() for a in out]


def concat_tree(s):
    s = s.strip()
    m = re.fullmatch(r"CONCAT\((.*)\)", s)
    if m:
        return {"concat": [concat_tree(a) for a in split_args(m.group(1))]}
    return sql_string(s)


def main():
    out = {"source": "core/trino-main/src/test/java/io/trino/operator/scalar/TestStringFunctions.java", "concat": [], "concat_errors": [], "length": [],
           "strpos": [], "starts_with": [], "substr": []}
    skipped = 0
    for no, l in lines(107, 121):
        try:
            m = re.search(r"assertFunction\(" + JSTR + r", VARCHAR, " + JSTR + r"\);", l)
            e = re.search(r"assertInvalidFunction\(" + JSTR + ", " + JSTR + r"\);", l)
            if m:
                out["concat"].append({"line": no, "expr": concat_tree(junescape(m.group(1))), "expected": junescape(m.group(2))})
            elif e:
                out["concat_errors"].append({"line": no, "expr": concat_tree(junescape(e.group(1))), "message": junescape(e.group(2))})
            elif "assert" in l:
                raise Skip(l)
        except Skip:
            skipped += 1
    for no, l in lines(132, 141):
        m = re.search(r"assertFunction\(" + JSTR + r", BIGINT, (\d+)L\);", l)
        if m:
            v = re.fullmatch(r"LENGTH\((.*)\)", junescape(m.group(1)))
            out["length"].append({"line": no, "value": sql_string(v.group(1)), "expected": int(m.group(2))})
        elif "assert" in l:
            skipped += 1
    jarg = r"(null|" + JSTR + ")"
    for no, l in lines(267, 315):
        try:
            m = re.search(r"testStrPosAndPosition\(" + jarg + ", " + jarg + r", (null|\d+L)\);", l)
            s = re.search(r"assertFunction\(" + JSTR + r", (BIGINT|BOOLEAN), (null|true|false|\d+L)\);", l)
            if m:
                a = None if m.group(1) == "null" else junescape(m.group(2))
                b = None if m.group(3) == "null" else junescape(m.group(4))
                out["strpos"].append({"line": no, "value": a, "substring": b, "expected": None if m.group(5) == "null" else int(m.group(5)[:-1])})
            elif s:
                call = re.fullmatch(r"(STRPOS|STARTS_WITH)\((.*)\)", junescape(s.group(1)))
                args = split_args(call.group(2))
                if len(args) != 2:
                    raise Skip(l)
                want = {"null": None, "true": True, "false": False}.get(s.group(3), None if s.group(3) == "null" else 0)
                if s.group(3)[0].isdigit():
                    want = int(s.group(3)[:-1])
                key = "strpos" if call.group(1) == "STRPOS" else "starts_with"
                out[key].append({"line": no, "value": sql_string(args[0]), "substring" if key == "strpos" else "prefix": sql_string(args[1]), "expected": want})
            elif "assert" in l:
                raise Skip(l)
        except Skip:
            skipped += 1
    for no, l in lines(353, 386):
        try:
            m = re.search(r"assertFunction\(" + JSTR + r", createVarcharType\(\d+\), " + JSTR + r"\);", l)
            if not m:
                if "assert" in l:
                    raise Skip(l)
                continue
            sql = junescape(m.group(1))
            a = re.fullmatch(r"SUBSTR\((.*)\)", sql)
            b = re.fullmatch(r"SUBSTRING\((.*) FROM (-?\d+)(?: FOR (-?\d+))?\)", sql)
            if a:
                args = split_args(a.group(1))
                value, start, length = sql_string(args[0]), int(args[1]), int(args[2]) if len(args) == 3 else None
            elif b:
                value, start, length = sql_string(b.group(1)), int(b.group(2)), None if b.group(3) is None else int(b.group(3))
            else:
                raise Skip(l)
            out["substr"].append({"line": no, "value": value, "start": start, "length": length, "expected": junescape(m.group(2))})
        except Skip:
            skipped += 1
    out["skipped_lines"] = skipped
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print({k: len(v) for k, v in out.items() if isinstance(v, list)}, "skipped", skipped)


if __name__ == "__main__":
    main()

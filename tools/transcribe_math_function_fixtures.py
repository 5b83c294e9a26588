#!/usr/bin/env python3
"""Transcribes the math-function assertions of the reference's TestMathFunctions.java into tests/golden/math_function_vectors.json.

  python tools/transcribe_math_function_fixtures.py <reference checkout>

Kept: assertFunction / assertInvalidFunction lines of abs, ceil / ceiling, floor, truncate, round, sign, sqrt, cbrt, exp, ln, log2, log10, log,
power / pow, is_nan, is_finite, is_infinite, degrees and radians whose arguments are BIGINT, INTEGER or DOUBLE (the types the IR has).  The
loops over the file's value arrays are unrolled.  For a function that exists over DOUBLE only, an integer or decimal literal is the DOUBLE
the SQL coercion makes of it.  Each case keeps the function, the arguments (integers as numbers, doubles as a decimal string and a bit
pattern), the source line and the worked-out expected value -- data only, none of the reference's program text.  Where the reference's expected
value is a java.lang.Math call, the value stored is worked out here: exactly for sqrt / toDegrees / toRadians, and as the correctly rounded
result (tools/gen_math_function_ulp_corpus.py truth(), mpmath) for cbrt, exp, log, log10 and pow, which the JVM only pins to within 1 ulp.
Every other line of the test methods read is counted in skipped_lines with the reason."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import math_fn_expected as X   # noqa: E402
from gen_math_function_ulp_corpus import truth   # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "math_function_vectors.json")
SOURCE = "core/trino-main/src/test/java/io/trino/operator/scalar/TestMathFunctions.java"
FUNCTIONS = {"abs", "ceil", "ceiling", "floor", "truncate", "round", "sign", "sqrt", "cbrt", "exp", "ln", "log2", "log10", "log", "power", "pow", "is_nan", "is_finite",
             "is_infinite", "degrees", "radians"}
TYPED = {"abs", "ceil", "ceiling", "floor", "round", "sign"}          # functions with a signature per type: a literal keeps its type
TYPES = {"BIGINT": "bigint", "INTEGER": "integer", "DOUBLE": "double", "BOOLEAN": "boolean"}


class Skip(Exception):
    pass


def java_double(x):
    """Double.toString for the values of the file's arrays (plain decimals)"""
    return repr(float(x))


def split_top(text, sep):
    parts, depth, quote, cur = [], 0, False, ""
    for ch in text:
        if ch == '"':
            quote = not quote
        if not quote:
            depth += ch == "("
            depth -= ch == ")"
        if ch == sep and not quote and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


def java_value(expr, env):
    """a piece of a string concatenation or an argument of a Math call -> (kind, value)"""
    expr = expr.strip()
    m = re.fullmatch(r"(\w+) \* (\d+)L", expr)
    if m and m.group(1) in env:
        return env[m.group(1)][0], env[m.group(1)][1] * int(m.group(2))
    if expr in env:
        return env[expr]
    if expr == "Integer.MIN_VALUE":
        return "int", -2**31
    if expr == "GREATEST_DOUBLE_LESS_THAN_HALF":
        return "double", 0.49999999999999994
    raise Skip("a REAL argument" if expr.startswith("(float)") else "a Java expression outside the transcriber: " + re.split(r"\W", expr)[0])


def java_string(expr, env):
    """"..." + var + "..." or format("...%s...", var) -> the string"""
    m = re.fullmatch(r'format\((".*?"), (.*)\)', expr)
    if m:
        kind, v = java_value(m.group(2), env)
        return json.loads(m.group(1)).replace("%s", java_double(v) if kind == "double" else str(v))
    out = ""
    for piece in split_top(expr, "+"):
        if piece.startswith('"'):
            out += json.loads(piece)
        else:
            kind, v = java_value(piece, env)
            out += java_double(v) if kind == "double" else str(v)
    return out


def double_of(text):
    return {"text": repr(text) if isinstance(text, float) else text, "bits": "%016x" % X.bits(float(text))}


def sql_double(text):
    """a DOUBLE-valued SQL expression -> float"""
    text = text.strip()
    if " / " in text:
        a, b = text.split(" / ")
        return X._div(sql_double(a), sql_double(b))
    if text == "nan()":
        return X.NAN
    if text in ("infinity()", "-infinity()"):
        return X.INF if text[0] != "-" else -X.INF
    m = re.fullmatch(r"DOUBLE\s*'(.*)'", text)
    if m:
        return float(m.group(1))
    if re.fullmatch(r"-?\d+(\.\d+)?(E-?\d+)?", text):
        return float(text)
    raise Skip("an argument outside BIGINT / INTEGER / DOUBLE")


def sql_argument(text, function, position):
    text = text.strip()
    double_only = function not in TYPED or (function == "truncate")
    m = re.fullmatch(r"CAST\(NULL AS (\w+)\)", text, re.I)
    if m:
        if m.group(1).upper() not in ("BIGINT", "INTEGER", "DOUBLE"):
            raise Skip("an argument outside BIGINT / INTEGER / DOUBLE")
        return {"type": TYPES[m.group(1).upper()], "value": None}
    if text == "NULL":
        if not double_only:
            raise Skip("an untyped NULL")
        return {"type": "double", "value": None}
    if function == "round" and position == 1:
        if not re.fullmatch(r"-?\d+", text):
            raise Skip("decimals that are no integer literal")
        return {"type": "integer", "value": int(text)}
    m = re.fullmatch(r"(BIGINT|INTEGER)\s*'(-?\d+)'", text)
    if m or re.fullmatch(r"-?\d+", text):
        v = int(m.group(2) if m else text)
        t = m.group(1).lower() if m else ("integer" if -2**31 <= v < 2**31 else "bigint")
        return {"type": "double", "value": double_of(float(v))} if double_only else {"type": t, "value": v}
    if re.fullmatch(r"-?\d+\.\d+", text) and not double_only:
        raise Skip("a DECIMAL argument")
    return {"type": "double", "value": double_of(sql_double(text))}


def argument_value(a):
    return None if a["value"] is None else X.from_bits(int(a["value"]["bits"], 16)) if a["type"] == "double" else a["value"]


def expected_of(text, rtype, function, args, env):
    text = text.strip()
    if text == "null":
        return None
    if rtype == "boolean":
        if text in ("true", "false"):
            return text == "true"
        raise Skip("an expected value outside the transcriber")
    if re.match(r"Math\.", text):
        # the reference's expected value is what its JVM computes: worked out here from the case's own arguments
        name = {"ceil": "ceiling", "pow": "power"}.get(function, function)
        values = [argument_value(a) for a in args]
        if any(v is None for v in values):
            return None
        if name in X.BOUNDED:
            return double_of(truth(name, *values)[0])
        return double_of((X.UNARY.get(name) or X.BINARY[name])(*values))
    if rtype == "double":
        if text in ("Double.NaN", "Double.POSITIVE_INFINITY", "Double.NEGATIVE_INFINITY"):
            return double_of({"Double.NaN": X.NAN, "Double.POSITIVE_INFINITY": X.INF, "Double.NEGATIVE_INFINITY": -X.INF}[text])
        if re.fullmatch(r"-?\d+(\.\d+)?(E-?\d+)?", text):
            return double_of(float(text))
    elif re.fullmatch(r"-?\d+L?", text):
        return int(text.rstrip("L"))
    raise Skip("an expected value outside the transcriber")


def arrays_of(source):
    """the value arrays the loops run over: name -> (kind, values)"""
    out = {}
    for m in re.finditer(r"private static final (double|int|long)\[\] (\w+) = \{(.*?)\};", source):
        kind = "double" if m.group(1) == "double" else "int"
        out[m.group(2)] = (kind, [float(v) if kind == "double" else int(v) for v in m.group(3).split(",")])
    return out


def transcribe(root):
    source = open(os.path.join(root, SOURCE)).read()
    arrays = arrays_of(source)
    cases, skipped, loops = [], {}, []          # loops: (indent, variable, kind, values)
    for number, line in enumerate(source.split("\n"), 1):
        indent = len(line) - len(line.lstrip())
        body = line.strip()
        while loops and body == "}" and loops[-1][0] == indent:
            loops.pop()
        m = re.fullmatch(r"for \((double|int|long) (\w+) : (\w+)\) \{", body)
        if m and m.group(3) in arrays:
            kind = "double" if m.group(1) == "double" else "int"
            loops.append((indent, m.group(2), kind, [float(v) if kind == "double" else int(v) for v in arrays[m.group(3)][1]]))
            continue
        m = re.fullmatch(r"(assertFunction|assertInvalidFunction)\((.*)\);", body)
        if not m:
            continue
        parts = split_top(m.group(2), ",")
        name = re.match(r'(?:format\()?"\s*(\w+)', parts[0])
        if not name or name.group(1) not in FUNCTIONS:
            continue

        def bindings(at):
            if at == len(loops):
                yield {}
                return
            for v in loops[at][3]:
                for rest in bindings(at + 1):
                    yield dict(rest, **{loops[at][1]: (loops[at][2], v)})

        for env in bindings(0):
            try:
                first, rest = parts[0], parts[1:]
                sql = java_string(first, env).strip()
                call = re.fullmatch(r"(\w+)\(\s*(.*?)\s*\)", sql, re.S)
                if not call:
                    raise Skip("not a single call")
                function = call.group(1)
                args = [sql_argument(a, function, k) for k, a in enumerate(split_top(call.group(2), ","))]
                if function in TYPED and args[0]["type"] not in ("bigint", "integer", "double"):
                    raise Skip("an argument outside BIGINT / INTEGER / DOUBLE")
                case = {"function": function, "arguments": args, "line": number}
                if m.group(1) == "assertInvalidFunction":
                    if function not in ("abs", "round"):
                        raise Skip("an error case of another function")
                    case["error"] = rest[0]
                else:
                    if rest[0] not in TYPES:
                        raise Skip("a result type outside the IR")
                    case["type"] = TYPES[rest[0]]
                    case["expected"] = expected_of(rest[1], case["type"], function, args, env)
                if case not in cases:
                    cases.append(case)
            except Skip as e:
                skipped[str(e)] = skipped.get(str(e), 0) + 1
    return {"source": SOURCE, "cases": cases, "skipped_lines": skipped}


def text(gold):
    lines = ['{"source": %s,' % json.dumps(gold["source"]), ' "skipped_lines": %s,' % json.dumps(gold["skipped_lines"], sort_keys=True), ' "cases": [']
    lines += ["  %s%s" % (json.dumps(c, sort_keys=True), "," if i + 1 < len(gold["cases"]) else "") for i, c in enumerate(gold["cases"])]
    return "\n".join(lines + [" ]", "}"]) + "\n"


if __name__ == "__main__":
    gold = transcribe(sys.argv[1])
    with open(OUT, "w") as f:
        f.write(text(gold))
    by = {}
    for c in gold["cases"]:
        by[c["function"]] = by.get(c["function"], 0) + 1
    print(len(gold["cases"]), "cases", by, "skipped", gold["skipped_lines"])

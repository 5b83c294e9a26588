"""LIKE and IN without a GPU: the Python restatement on the reference's pinned literals, the IR layout, the generated source of every LIKE
shape and IN strategy (hiprtc compiles for gfx950 without a device), and the errors raised when the program is created."""
import re

import pytest

import like_in_cases as C
import like_in_expected as X


def test_in_restatement():
    nan = float("nan")
    assert X.in_list(None, [1]) is None and X.in_list(1, [2, 1]) is True and X.in_list(1, [2]) is False and X.in_list(1, [2, None]) is None
    assert X.in_list(1, [None, 1]) is True and X.in_list(nan, [nan]) is False and X.in_list(-0.0, [0.0]) is True and X.in_list(1.5, [nan, None]) is None


def test_flat_program_lays_the_list_out_consecutively(pkg):
    f = pkg.field
    prog = pkg.expressions.FlatProgram(pkg.in_(f(0, pkg.BIGINT) + 1, [3, None, 5]), [pkg.like(f(1, pkg.VARCHAR), "a%", "\\")])
    assert pkg.expressions.OPS["LIKE"] == 15 and pkg.expressions.FORMS["IN"] == 7
    node = prog.nodes[prog.filter_root]
    assert node["kind"] == 3 and node["op"] == 7 and len(node["args"]) == 1 and node["slen"] == 3
    items = prog.nodes[node["ival"]:node["ival"] + 3]
    assert [i["kind"] for i in items] == [1, 1, 1] and [i.get("is_null") for i in items] == [0, 1, 0] and items[2]["ival"] == 5
    like = prog.nodes[prog.projection_roots[0]]
    assert like["kind"] == 2 and like["op"] == 15 and len(like["args"]) == 3 and all(prog.nodes[a]["kind"] == 1 for a in like["args"][1:])


LIKE_SHAPES = ["abc", "", "%", "%%", "___", "_%", "abcdefghi%", "%abcdefghijklmnopq", "abcd%wxyz", "%special%requests%", "a_c", "_bc%", "%_b", "%a_c%d", "a%_é_%b%c_"]
NEW_HELPERS = ["tg_lk_", "tg_in_", "TG_LIKE_IN_HELPERS"]


def test_every_like_shape_and_in_strategy_compiles(pkg):
    f, V, B, D = pkg.field, pkg.VARCHAR, pkg.BIGINT, pkg.DOUBLE
    v = f(0, V)
    pkg.precompile_page_processor([V, B, D], pkg.like(v, "%ab%"), [pkg.like(v, p) for p in LIKE_SHAPES[:11]])
    pkg.precompile_page_processor([V, B, D], None, [pkg.like(v, p, "\\") for p in LIKE_SHAPES[11:]] + [
        pkg.in_(f(1, B), [1]), pkg.in_(f(1, B), list(range(C.IN_SMALL_LIST)) + [None]), pkg.in_(f(1, B), list(range(C.IN_SMALL_LIST + 1))),
        pkg.in_(f(2, D), [0.5 * i for i in range(40)]), pkg.in_(v, ["a", "bc", "bd"]), pkg.in_(v, ["s%d" % i for i in range(40)]), pkg.in_(v, [None])])
    src = pkg.page_processor_source([V, B, D], None, [pkg.like(v, "%special%requests%"), pkg.in_(f(1, B), list(range(40)))])
    assert "tg_lk_find_lit" in src and "tg_in_probe" in src
    # the threshold between the comparison chain and the table
    assert "tg_in_probe" not in pkg.page_processor_source([B], None, [pkg.in_(f(0, B), list(range(C.IN_SMALL_LIST)) + [3, None])])
    assert "tg_in_probe" in pkg.page_processor_source([B], None, [pkg.in_(f(0, B), list(range(C.IN_SMALL_LIST + 1)))])
    # anchored literals and plain equality need no helper at all
    for p in ("abc", "abc%", "%abc", "ab%yz", "%"):
        assert not any(h in pkg.page_processor_source([V], None, [pkg.like(f(0, V), p)]) for h in NEW_HELPERS), p


def test_programs_without_like_or_in_get_no_helper(pkg):
    import __graft_entry__ as entry
    for name, (types, filt, projs) in entry.bench_page_processors(pkg).items():
        src = pkg.page_processor_source(types, filt, projs)
        assert not any(h in src for h in NEW_HELPERS), name


def test_different_patterns_and_lists_generate_different_sources(pkg):
    """the kernel cache is keyed by the generated source: it covers the pattern bytes and the list items"""
    f, V, B = pkg.field, pkg.VARCHAR, pkg.BIGINT
    s = lambda e, t: pkg.page_processor_source([t], None, [e])
    assert s(pkg.like(f(0, V), "%abc%"), V) != s(pkg.like(f(0, V), "%abd%"), V)
    assert s(pkg.in_(f(0, B), list(range(40))), B) != s(pkg.in_(f(0, B), list(range(39)) + [77]), B)
    assert s(pkg.in_(f(0, V), ["a", "b"]), V) != s(pkg.in_(f(0, V), ["a", "c"]), V)


@pytest.mark.parametrize("pattern,escape,message", [("#", "#", X.ESCAPE_FOLLOW), ("abc#abc", "#", X.ESCAPE_FOLLOW), ("abc#", "#", X.ESCAPE_FOLLOW), ("abc", "##", X.ESCAPE_LENGTH)])
def test_bad_escapes_fail_when_the_program_is_created(pkg, pattern, escape, message):
    with pytest.raises(pkg.TgpuError) as e:
        pkg.precompile_page_processor([pkg.VARCHAR], pkg.like(pkg.field(0, pkg.VARCHAR), pattern, escape), [])
    assert e.value.code == -1 and message in str(e.value)


def test_ir_errors(pkg):
    f, V, B, E = pkg.field, pkg.VARCHAR, pkg.BIGINT, pkg.expressions
    with pytest.raises(pkg.TgpuError) as e:     # a pattern that is no constant
        pkg.precompile_page_processor([V, V], pkg.like(f(0, V), f(1, V)), [])
    assert e.value.code == -8

    def in_error(mutate, types=(B,)):
        prog = E.FlatProgram(pkg.in_(f(0, B), [1, 2]), [])
        mutate(prog)
        spec, keep = prog.to_c()
        import ctypes
        arr = (ctypes.c_int32 * len(types))(*types)
        return pkg._lib.lib().tgpu_precompile_page_processor(len(types), arr, ctypes.byref(spec))

    root = lambda p: p.nodes[p.filter_root]
    assert in_error(lambda p: None) == 0
    assert in_error(lambda p: root(p).update(slen=0)) == -1
    assert in_error(lambda p: root(p).update(ival=len(p.nodes) - 1)) == -1
    assert in_error(lambda p: p.nodes[root(p)["ival"]].update(kind=0, op=0)) == -1          # an item that is no constant
    assert in_error(lambda p: p.nodes[root(p)["ival"]].update(type=pkg.DOUBLE)) == -1       # an item of another type
    assert in_error(lambda p: root(p).update(slen=65537)) == -8


# ---- the reference's pinned literals (tests/golden/like_in_vectors.json, tools/transcribe_like_in_fixtures.py) ---------------------
import json
import os

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "like_in_vectors.json")))
TABLES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "expression_vectors.json")))["expression_compiler"]["value_tables"]


def gold_like_cases():
    return GOLD["interpreter_like"] + GOLD["like_functions"]["like"]


def test_restatement_against_the_golden_like_cases():
    assert len(gold_like_cases()) >= 60
    for c in gold_like_cases():
        value = bytes(c["value_bytes"]).decode("utf-8", "surrogateescape") if "value_bytes" in c else c["value"]   # testLikeInvalidUtf8Value: any byte-wise search
        assert X.like(value, c["pattern"], c["escape"], c["has_escape"]) is c["expected"], c
    for c in GOLD["like_functions"]["errors"]:
        fn = {"likePattern": X.like_regex, "isLikePattern": X.is_like_pattern, "patternConstantPrefixBytes": X.pattern_constant_prefix_bytes}[c["function"]]
        with pytest.raises(X.LikeError) as e:
            fn(c["pattern"], c["escape"])
        assert str(e.value) == c["message"], c
    for c in GOLD["like_functions"]["is_like_pattern"]:
        assert X.is_like_pattern(c["pattern"], c["escape"]) is c["expected"], c
    for c in GOLD["like_functions"]["pattern_constant_prefix_bytes"]:
        assert X.pattern_constant_prefix_bytes(c["pattern"], c["escape"]) == c["expected"], c
    for c in GOLD["like_functions"]["unescape"]:
        assert X.unescape_literal_like_pattern(c["pattern"], c["escape"]) == c["expected"], c
    for c in GOLD["interpreter_like_optimization"]:   # rewritten to an equality exactly when the pattern has no wildcard; then it matches that literal alone
        esc = c["escape"] if c["has_escape"] else None
        if c["pattern"] == "" and c["has_escape"]:
            continue                                   # :1270 stays a LIKE although it has no wildcard (the optimizer's choice, not semantics)
        assert (c["equals"] is not None) == (not X.is_like_pattern(c["pattern"], esc)), c
        if c["equals"] is not None:
            assert X.unescape_literal_like_pattern(c["pattern"], esc) == c["equals"]
            assert X.like(c["equals"], c["pattern"], esc) is True and X.like(c["equals"] + "x", c["pattern"], esc) is False


def test_restatement_against_the_golden_in_lists():
    tables = dict(TABLES, **{"smallInts+extremeInts": TABLES["smallInts"] + TABLES["extremeInts"]})
    assert len(GOLD["compiler_in"]) >= 20
    for c in GOLD["compiler_in"]:
        contains = [i for i in c["items"] if i is not None]
        for v in tables[c["values_table"]]:
            want = None if v is None else (True if v in contains else (None if None in c["items"] else False))   # the test's own expression (:1172-1286)
            assert X.in_list(v, c["items"]) is want, (c, v)
    for c in GOLD["compiler_huge_in"]:
        conv = {"integer": int, "bigint": int, "double": float, "varchar": str}[c["type"]]
        items = [conv(i) for i in range(*c["range"])]
        assert X.in_list(c["value"], [c["extra"]] + items) is c["expected_with_extra"] and X.in_list(c["value"], items) is c["expected_without"]


def test_java_glue_maps_in_and_like():
    """GpuRowExpressions against the reference's sources as text (no JDK here): the form, the function names and the regex accessor it relies on"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    glue = open(os.path.join(root, "java/io/trino/operator/gpu/GpuRowExpressions.java")).read()
    assert "SpecialForm.Form.IN" in glue and "LikeFunctions.LIKE_PATTERN_FUNCTION_NAME" in glue and ".pattern()" in glue
    assert re.search(r"OP_EQUAL = 7, OP_LIKE = 15, SF_OR = 2, SF_IN = 7", glue)
    header = open(os.path.join(root, "include/tgpu.h")).read()
    assert "TGPU_OP_LIKE = 15" in header and "TGPU_SF_IN = 7" in header
    ref = "/root/reference/core/trino-main/src/main/java/io/trino"
    if not os.path.isdir(ref):
        pytest.skip("needs a checkout of the reference sources")
    form = open(os.path.join(ref, "sql/relational/SpecialForm.java")).read()
    assert re.search(r"enum Form\s*\{[^}]*\bIN\b", form)
    like = open(os.path.join(ref, "type/LikeFunctions.java")).read()
    assert 'LIKE_PATTERN_FUNCTION_NAME = "$like_pattern"' in like and '@ScalarFunction(value = "like", hidden = true)' in like
    assert 'LIKE_FUNCTION_NAME = "like"' in glue
    joni = open(os.path.join(ref, "type/JoniRegexp.java")).read()
    assert re.search(r"public Slice pattern\(\)", joni) and "public final class JoniRegexp" in joni
    # the characters likePattern escapes are the ones the inversion un-escapes (:221-228)
    for ch in ("case '\\\\':", "case '^':", "case '$':", "case '.':", "case '*':"):
        assert ch in like, ch


def regex_of_like(pattern, escape):
    """LikeFunctions.likePattern's regex text (:198-241), for the inversion test"""
    out, escaped = ["^"], False
    esc = escape if escape is not None else None
    for ch in pattern:
        if esc is not None and not escaped and ch == esc:
            escaped = True
            continue
        if ch == "%":
            out.append("%" if escaped else ".*")
        elif ch == "_":
            out.append("_" if escaped else ".")
        else:
            out.append(("\\" if ch in "\\^$.*" else "") + ch)
        escaped = False
    return "".join(out) + "$"


def like_pattern_of_regex(regex):
    """GpuRowExpressions.likePatternOfRegex, line by line"""
    assert len(regex) >= 2 and regex[0] == "^" and regex[-1] == "$"
    out, i, end = [], 1, len(regex) - 1
    while i < end:
        c = regex[i]
        if c == ".":
            if i + 1 < end and regex[i + 1] == "*":
                out.append("%")
                i += 1
            else:
                out.append("_")
            i += 1
            continue
        if c == "\\":
            i += 1
            assert i < end
            c = regex[i]
        else:
            assert c not in "^$*"
        out.append(("\\" if c in "%_\\" else "") + c)
        i += 1
    return "".join(out)


def test_the_regex_inversion_gives_an_equivalent_pattern():
    """the Java method has no JVM to run on here: its Python transliteration is checked, and that the Java text has the same branches"""
    glue = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "java/io/trino/operator/gpu/GpuRowExpressions.java")).read()
    body = glue[glue.index("static String likePatternOfRegex"):glue.index("private static int addIn")]
    for must in ("regex.charAt(i + 1) == '*'", "like.append('%')", "like.append('_')", "c == '%' || c == '_' || c == '\\\\'", "c == '^' || c == '$' || c == '*'"):
        assert must in body, must
    values = C.random_values()[:128] + ["a.c", "a*c", "^a$", ".*", "a\\c"]
    pats = [(p, e) for p, e in C.random_patterns() + [("a.c%", None), ("%a*_", None), ("^%$", None), ("a\\%.*", "\\"), (".*", None), ("._*", None)]]
    checked = 0
    for p, e in pats:
        try:
            X.like_regex(p, e)
        except X.LikeError:
            continue
        back = like_pattern_of_regex(regex_of_like(p, e))
        assert X.like_column(values, back, "\\") == X.like_column(values, p, e), (p, e, back)
        checked += 1
    assert checked > 200

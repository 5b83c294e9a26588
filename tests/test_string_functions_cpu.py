"""The string functions and computed VARCHAR projections without a GPU: the Python restatement on the reference's pinned literals, the IR
layout, the generated source (hiprtc compiles for gfx950 without a device) and the errors raised when the program is created."""
import ctypes
import json
import os
import re

import pytest

import string_fn_cases as C
import string_fn_expected as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "string_function_vectors.json")))
NEW_HELPERS = ["fp_vwrite", "tg_vw_", "tg_cp_", "tg_str_find", "tg_digits", "TG_STRING_HELPERS", "TG_VW_COOP_MIN", "FvArgs"]


def enc(s):
    return None if s is None else s.encode()


def concat_value(tree):
    if isinstance(tree, dict):
        args = [concat_value(a) for a in tree["concat"]]
        if len(args) < 2:
            raise ValueError("There must be two or more concatenation arguments")
        out = args[0]
        for a in args[1:]:
            out = X.concat(out, a)
        return out
    return enc(tree)


def test_restatement_against_the_golden_cases():
    assert len(GOLD["concat"]) >= 10 and len(GOLD["length"]) >= 6 and len(GOLD["strpos"]) >= 25 and len(GOLD["starts_with"]) >= 10 and len(GOLD["substr"]) >= 25
    for c in GOLD["concat"]:
        assert concat_value(c["expr"]) == enc(c["expected"]), c
    for c in GOLD["concat_errors"]:
        with pytest.raises(ValueError) as e:
            concat_value(c["expr"])
        assert str(e.value) == c["message"]
    for c in GOLD["length"]:
        assert X.length(enc(c["value"])) == c["expected"], c
    for c in GOLD["strpos"]:
        assert X.strpos(enc(c["value"]), enc(c["substring"])) == c["expected"], c
    for c in GOLD["starts_with"]:
        assert X.starts_with(enc(c["value"]), enc(c["prefix"])) is c["expected"], c
    for c in GOLD["substr"]:
        assert X.substring(enc(c["value"]), c["start"], c["length"], c["length"] is not None) == enc(c["expected"]), c


def test_restatement_edges():
    v = "a名b".encode()
    assert X.substring(v, 2**63 - 1) == b"" and X.substring(v, -2**63) == b"" and X.substring(v, -3) == v and X.substring(v, -4) == b""
    assert X.substring(v, 2, 2**63 - 1, True) == "名b".encode() and X.substring(v, -2, 1, True) == "名".encode() and X.substring(v, 1, -2**63, True) == b""
    assert X.substring(None, 1) is None and X.substring(v, None) is None and X.substring(v, 1, None, True) is None
    assert X.substring(v, -1, 2**31 - 1, True) == b"b"          # the reference's int addition overflows here: the library gives the suffix
    assert X.cast_integer(-2**63) == b"-9223372036854775808" and X.cast_integer(0) == b"0" and X.cast_boolean(False) == b"false"
    assert X.length(b"\x80abc") == 3 and X.strpos("名名a".encode(), b"a") == 3 and X.strpos(b"abc", b"") == 1
    assert len(C.boundary_values()) > 70 and {len(v) for v in C.boundary_values() if v is not None} >= set(C.LENGTHS)
    assert len(C.substr_pairs()) > 300


def programs(pkg):
    """every op, every cast, IF / COALESCE over views and over built values, nested concat"""
    f, c, V, B, I, BO = pkg.field, pkg.constant, pkg.VARCHAR, pkg.BIGINT, pkg.INTEGER, pkg.BOOLEAN
    x, k, i, b = f(0, V), f(1, B), f(2, I), f(3, BO)
    types = [V, B, I, BO]
    projs = [pkg.length(x), pkg.substr(x, 1), pkg.substr(x, k, 2), pkg.concat("Customer#", pkg.cast(k, V)), pkg.strpos(x, "ab"), pkg.starts_with(x, "ab"),
             pkg.cast(k, V), pkg.cast(i, V), pkg.cast(b, V), pkg.cast(x, V), pkg.if_(b, c("a", V), c("bb", V)), pkg.coalesce(x, "n/a"),
             pkg.if_(b, pkg.concat(x, "-", x), pkg.cast(k, V)), pkg.coalesce(pkg.concat(x, "z"), x), pkg.concat(pkg.concat(x, "a"), pkg.concat("b", pkg.cast(i, V))),
             pkg.length(pkg.concat(x, pkg.cast(k, V)))]
    filt = pkg.and_(pkg.in_(pkg.substr(x, 1, 2), ["13", "31"]), pkg.length(pkg.substr(x, 2)) > 3)
    return types, filt, projs


def test_every_op_compiles_with_and_without_a_filter(pkg):
    """without the feature: TGPU_ERR_COMPILER, "computed VARCHAR projections are not supported" """
    types, filt, projs = programs(pkg)
    for part in (projs[:8], projs[8:]):      # at most 8 computed VARCHAR projections per processor
        pkg.precompile_page_processor(types, None, part)
        pkg.precompile_page_processor(types, filt, part)
    src = pkg.page_processor_source(types, filt, projs[:8])
    assert "fp_vwrite" in src and "tg_vw_copy_wave" in src and "tg_cp_count" in src and "tg_str_find" in src
    # views only, in a filter and a fixed-width projection: the helpers, but no write pass
    src = pkg.page_processor_source(types, filt, [pkg.length(pkg.field(0, pkg.VARCHAR))])
    assert "fp_vwrite" not in src and "tg_cp_offset" in src


def test_programs_without_varchar_projections_get_no_helper(pkg):
    import __graft_entry__ as entry
    for name, (types, filt, projs) in entry.bench_page_processors(pkg).items():
        src = pkg.page_processor_source(types, filt, projs)
        assert not any(h in src for h in NEW_HELPERS), name


def test_the_copy_threshold_is_part_of_the_source(pkg, monkeypatch):
    """TGPU_VW_COOP_MIN changes the generated source, hence the kernel cache key"""
    V = pkg.VARCHAR
    sources = []
    for value in ("0", "64", str(2**40)):
        monkeypatch.setenv("TGPU_VW_COOP_MIN", value)
        sources.append(pkg.page_processor_source([V], None, [pkg.substr(pkg.field(0, V), 1)]))
        assert "#define TG_VW_COOP_MIN %sLL" % value in sources[-1]
    assert len(set(sources)) == 3
    monkeypatch.delenv("TGPU_VW_COOP_MIN")
    default = pkg.page_processor_source([V], None, [pkg.substr(pkg.field(0, V), 1)])
    assert re.search(r"#define TG_VW_COOP_MIN \d+LL", default) and default not in sources[:1]


def raw_status(pkg, types, prog):
    spec, keep = prog.to_c()
    arr = (ctypes.c_int32 * len(types))(*types)
    return pkg._lib.lib().tgpu_precompile_page_processor(len(types), arr, ctypes.byref(spec))


def test_ir_errors(pkg):
    f, V, B, D, E = pkg.field, pkg.VARCHAR, pkg.BIGINT, pkg.DOUBLE, pkg.expressions
    x = f(0, V)
    built = pkg.concat(x, "a")
    for consumer in (built.eq("b"), pkg.like(built, "a%"), pkg.in_(built, ["a"]), pkg.substr(built, 1), pkg.strpos(built, "a"), pkg.strpos(x, built),
                     pkg.starts_with(built, "a"), pkg.substr(pkg.cast(f(1, B), V), 1), pkg.between(built, "a", "b")):
        with pytest.raises(pkg.TgpuError) as e:
            pkg.precompile_page_processor([V, B], None, [consumer])
        assert e.value.code == -8 and "built VARCHAR value" in str(e.value), str(e.value)
    # what a built value may feed
    pkg.precompile_page_processor([V, B], pkg.is_null(built), [pkg.length(built), pkg.concat(built, built), pkg.coalesce(built, x)])

    def status(expr, types=(V, B)):
        return raw_status(pkg, list(types), E.FlatProgram(None, [expr]))

    COMPILER = -4
    assert status(pkg.length(x)) == 0
    assert status(E.call("LENGTH", B, f(1, B))) == COMPILER                                  # wrong argument type
    assert status(E.call("SUBSTR", V, x, f(0, V))) == COMPILER
    assert status(E.call("CONCAT", V, x, f(1, B))) == COMPILER
    assert status(E.call("STRPOS", B, x, f(1, B))) == COMPILER
    assert status(E.call("STARTS_WITH", pkg.BOOLEAN, f(1, B), x)) == COMPILER
    assert status(E.call("LENGTH", V, x)) == COMPILER                                         # wrong result type
    assert status(E.call("SUBSTR", V, x)) == COMPILER and status(E.call("CONCAT", V, x)) == COMPILER      # wrong argument count
    assert status(E.call("LENGTH", B, x, x)) == COMPILER and status(E.call("STRPOS", B, x)) == COMPILER
    assert status(pkg.cast(f(1, D), V), (V, D)) == COMPILER and status(pkg.cast(f(1, pkg.DATE), V), (V, pkg.DATE)) == COMPILER
    # a ninth computed VARCHAR projection
    assert raw_status(pkg, [V], E.FlatProgram(None, [pkg.substr(x, i + 1) for i in range(8)])) == 0
    with pytest.raises(pkg.TgpuError) as e:
        pkg.precompile_page_processor([V], None, [pkg.substr(x, i + 1) for i in range(9)])
    assert e.value.code == COMPILER and "too many computed VARCHAR projections" in str(e.value)
    # 32 pieces at the most
    pkg.precompile_page_processor([V], None, [pkg.concat(*([x] * 32))])
    with pytest.raises(pkg.TgpuError) as e:
        pkg.precompile_page_processor([V], None, [pkg.concat(*([x] * 33))])
    assert e.value.code == -8 and "32 pieces" in str(e.value)
    with pytest.raises(ValueError) as e:
        pkg.concat(x)
    assert str(e.value) == "There must be two or more concatenation arguments" == GOLD["concat_errors"][0]["message"]


def test_fused_generators_keep_the_unfused_composition(pkg):
    """a computed VARCHAR group key, count(col) input or probe output is no error when the fused factory is created: it is just not fused"""
    f, V, B = pkg.field, pkg.VARCHAR, pkg.BIGINT
    key = pkg.substr(f(0, V), 1, 2)
    pkg.precompile_fused_aggregation([V, B], None, [key, f(1, B)], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)], [0])
    pkg.precompile_fused_aggregation([V, B], None, [pkg.concat(f(0, V), "x"), f(1, B)], [(pkg.COUNT_COLUMN, 0)], [1])
    pkg.precompile_fused_probe([V, B], None, [f(1, B), key, pkg.concat("#", pkg.cast(f(1, B), V))], 0, [0, 1, 2])
    # views inside the filter and a fixed-width projection stay fused: the generators compile them
    filt = pkg.and_(pkg.starts_with(f(0, V), "ab"), pkg.strpos(pkg.substr(f(0, V), 2), "b") > 0)
    pkg.precompile_fused_aggregation([V, B], filt, [f(1, B), pkg.length(f(0, V))], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)], [0])
    pkg.precompile_fused_probe([V, B], filt, [f(1, B), pkg.length(f(0, V))], 0, [0, 1])


def test_flat_program_layout(pkg):
    f, V, B, E = pkg.field, pkg.VARCHAR, pkg.BIGINT, pkg.expressions
    assert [E.OPS[n] for n in ("LENGTH", "SUBSTR", "CONCAT", "STRPOS", "STARTS_WITH")] == [16, 17, 18, 19, 20]
    prog = E.FlatProgram(None, [pkg.substr(f(0, V), 2, 3), pkg.concat(f(0, V), "b", f(0, V)), pkg.substr("abc", 1), pkg.cast(f(1, B), V)])
    sub = prog.nodes[prog.projection_roots[0]]
    assert sub["kind"] == 2 and sub["op"] == 17 and len(sub["args"]) == 3 and [prog.nodes[a]["type"] for a in sub["args"]] == [V, B, B]
    assert prog.nodes[sub["args"][1]]["ival"] == 2 and prog.nodes[sub["args"][2]]["ival"] == 3
    outer = prog.nodes[prog.projection_roots[1]]
    inner = prog.nodes[outer["args"][0]]
    assert outer["op"] == 18 and inner["op"] == 18 and len(outer["args"]) == 2 and len(inner["args"]) == 2 and prog.nodes[outer["args"][1]]["kind"] == 0
    assert prog.nodes[prog.nodes[prog.projection_roots[2]]["args"][0]]["kind"] == 1       # a Python str is wrapped as a constant
    cast = prog.nodes[prog.projection_roots[3]]
    assert cast["op"] == 14 and cast["type"] == V
    assert all(hasattr(pkg, n) for n in ("length", "substr", "concat", "strpos", "starts_with"))


def test_java_glue_maps_the_string_functions():
    """GpuRowExpressions against the reference's sources as text (no JDK here)"""
    glue = open(os.path.join(ROOT, "java/io/trino/operator/gpu/GpuRowExpressions.java")).read()
    assert "OP_CAST = 14, OP_LENGTH = 16, OP_SUBSTR = 17, OP_CONCAT = 18, OP_STRPOS = 19, OP_STARTS_WITH = 20" in glue
    for name in ("length", "substr", "substring", "concat", "strpos", "starts_with"):
        assert 'case "%s"' % name in glue, name
    assert "isUnbounded()" in glue and "bounded varchar(n)" in glue and 'CAST_OPERATOR = "$operator$CAST"' in glue
    header = open(os.path.join(ROOT, "include/tgpu.h")).read()
    for name, value in (("LENGTH", 16), ("SUBSTR", 17), ("CONCAT", 18), ("STRPOS", 19), ("STARTS_WITH", 20)):
        assert "TGPU_OP_%s = %d" % (name, value) in header
    for rule in ("parity unpinned", "Concatenated string is too large", "variable width block cannot exceed 2GB", "too many computed VARCHAR projections",
                 "Ints.saturatedCast", "IndexOutOfBoundsException", "Out of scope"):
        assert rule in header, rule
    ref = "/root/reference/core/trino-main/src/main/java/io/trino/operator/scalar"
    if not os.path.isdir(ref):
        pytest.skip("needs a checkout of the reference sources")
    fns = open(os.path.join(ref, "StringFunctions.java")).read()
    # a @ScalarFunction without a value is named after its method (startsWith -> starts_with)
    assert re.search(r'@ScalarFunction\n(\s+@\w+\([^\n]*\)\n)*\s+public static long length\(@SqlType\("varchar\(x\)"\)', fns)
    assert re.search(r'@ScalarFunction\("strpos"\)\n(\s+@\w+\([^\n]*\)\n)*\s+public static long stringPosition\(@SqlType\("varchar\(x\)"\) Slice string, @SqlType\("varchar\(y\)"\) Slice substring\)', fns)
    assert len(re.findall(r'@ScalarFunction\(alias = "substr"\)\n(?:\s+@\w+\([^\n]*\)\n)*\s+public static Slice substring\(', fns)) == 2
    assert re.search(r'@ScalarFunction\n(\s+@\w+\([^\n]*\)\n)*\s+public static boolean startsWith\(', fns)
    concat = open(os.path.join(ref, "ConcatFunction.java")).read()
    assert '"concat"' in concat and "There must be two or more concatenation arguments" in concat and "Concatenated string is too large" in concat

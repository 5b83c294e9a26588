"""The TIMESTAMP functions without a GPU: the expected-value evaluator (tests/timestamp_fn_expected.py) on the reference's pinned literals and
against datetime + timedelta; the kernels' arithmetic (presto-1_amd/csrc/device_timestamp.h over device_date.h) compiled for the host under
AddressSanitizer and UndefinedBehaviorSanitizer -- tests/timestamp_math/ts_main.cpp, built here at test time into an ignored directory and run
as an ordinary child process, nothing preloaded, nothing loaded into Python -- against the evaluator on the seeded corpus
(tests/timestamp_fn_cases.py); the generated programs compiled for gfx950; the errors raised when a program is created; the IR's layout."""
import ctypes
import datetime
import json
import os
import re
import subprocess

import pytest

import date_fn_expected as D
import timestamp_fn_cases as C
import timestamp_fn_expected as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "timestamp_function_vectors.json")))
SRC = os.path.join(ROOT, "tests", "timestamp_math", "ts_main.cpp")
OUT = os.path.join(ROOT, "tests", "timestamp_math", "build")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
EPOCH = datetime.datetime(1970, 1, 1)
OWN = ["HOUR", "MINUTE", "SECOND", "MILLISECOND", "TO_UNIXTIME"]


# ---- (a) the evaluator ----------------------------------------------------------------------------------------------------------------
def test_evaluator_against_the_golden_cases():
    assert len(GOLD["extract"]) >= 100 and len(GOLD["date_trunc"]) >= 50 and len(GOLD["date_add"]) >= 25 and len(GOLD["date_diff"]) >= 25 and len(GOLD["compare"]) >= 90
    assert len(GOLD["cast_precision"]) >= 40 and len(GOLD["to_date"]) >= 7 and len(GOLD["from_date"]) >= 7 and len(GOLD["last_day_of_month"]) >= 7
    assert {c["function"] for c in GOLD["extract"]} == set(X.UNARY_NAMES) - {"last_day_of_month"}
    for c in GOLD["extract"]:
        assert X.UNARY[c["function"]](c["us"]) == c["expected"], c
    for c in GOLD["last_day_of_month"]:
        assert X.last_day_of_month(c["us"]) == c["expected"], c
    for c in GOLD["to_unixtime"]:
        assert X.to_unixtime(c["us"]) == c["expected"], c
    for c in GOLD["date_trunc"]:
        assert X.date_trunc(c["unit"], c["us"]) == c["expected"], c
    for c in GOLD["date_add"]:
        assert X.date_add(c["unit"], c["value"], c["us"], c["precision"]) == c["expected"], c
    for c in GOLD["date_diff"]:
        assert X.date_diff(c["unit"], c["us1"], c["us2"]) == c["expected"], c
    for c in GOLD["cast_precision"]:
        assert X.cast_precision(c["us"], c["target"]) == c["expected"], c
    for c in GOLD["to_date"]:
        assert X.to_date(c["us"]) == c["expected"], c
    for c in GOLD["from_date"]:
        assert X.from_date(c["day"]) == c["expected"], c
    assert "_comment" in GOLD and GOLD["lines_outside_the_ir"] > 0


def test_evaluator_against_datetime_and_timedelta():
    """years 1 .. 9999: instants spread over every year, the last and first microsecond of each, and timedelta arithmetic for the precise units"""
    micro = datetime.timedelta(microseconds=1)
    checked = 0
    for y in range(1, 10000):
        for dt in (datetime.datetime(y, 1, 1), datetime.datetime(y, 12, 31, 23, 59, 59, 999_999), datetime.datetime(y, 2, 28, 13, 7, 11, 123_456),
                   datetime.datetime(y, 3, 1, 0, 0, 0, 1), datetime.datetime(y, 1 + y % 12, 1 + y % 28, y % 24, y % 60, (y * 7) % 60, (y * 104_729) % 1_000_000)):
            us = (dt - EPOCH) // micro
            assert us == C.at(dt.year, dt.month, dt.day, dt.hour, dt.minute, dt.second, dt.microsecond)
            iso = dt.isocalendar()
            got = X.unary_row(us)
            want = (dt.year, (dt.month - 1) // 3 + 1, dt.month, iso[1], dt.day, iso[2], dt.timetuple().tm_yday, iso[0])
            assert got[:8] == want and got[9:] == (dt.hour, dt.minute, dt.second, dt.microsecond // 1000), dt
            assert X.to_date(us) == dt.toordinal() - EPOCH.toordinal() and X.from_date(X.to_date(us)) == (datetime.datetime(dt.year, dt.month, dt.day) - EPOCH) // micro
            assert X.date_trunc("hour", us) == (dt.replace(minute=0, second=0, microsecond=0) - EPOCH) // micro
            assert X.date_trunc("month", us) == (datetime.datetime(dt.year, dt.month, 1) - EPOCH) // micro
            assert X.date_trunc("week", us) == (datetime.datetime.fromordinal(dt.toordinal() - dt.weekday()) - EPOCH) // micro
            if 2 <= y <= 9998:
                for unit, delta in (("second", datetime.timedelta(seconds=1)), ("minute", datetime.timedelta(minutes=1)), ("hour", datetime.timedelta(hours=1)),
                                    ("day", datetime.timedelta(days=1)), ("week", datetime.timedelta(weeks=1)), ("millisecond", datetime.timedelta(milliseconds=1))):
                    v = (y % 97) - 48
                    later = ((dt + v * delta) - EPOCH) // micro
                    assert X.date_add(unit, v, us) == later, (dt, unit, v)
                    assert X.date_diff(unit, us, later) == v and X.date_diff(unit, later, us) == -v
            checked += 1
    assert checked == 9999 * 5
    assert X.to_unixtime(1_500_000) == 1.5 and X.to_unixtime(-1) == -1e-06 and X.double_bits(X.to_unixtime(0)) == 0


def test_evaluator_edges():
    at = C.at
    assert X.split(-1) == (-1, 86_399_999, 999) and X.split(999) == (0, 0, 999) and X.split(-1000) == (-1, 86_399_999, 0) and X.split(-1001) == (-1, 86_399_998, 999)
    assert X.hour(-1) == 23 and X.minute(-1) == 59 and X.second(-1) == 59 and X.millisecond(-1) == 999 and X.year(-1) == 1969
    assert X.split(X.INT64_MAX)[0] == C.MAX_DAY == 106751991 and X.split(X.INT64_MIN)[0] == C.MIN_DAY == -106751992
    assert X.year(X.INT64_MAX) == 294247 and X.year(X.INT64_MIN) == -290308
    # months keep the time of day and clamp the day of the month
    assert X.date_add("month", 1, at(2001, 1, 31, 12, 30, 0, 5)) == at(2001, 2, 28, 12, 30, 0, 5) and X.date_add("year", 1, at(2000, 2, 29, 23)) == at(2001, 2, 28, 23)
    assert X.date_diff("month", at(2001, 1, 31, 12), at(2001, 2, 28, 11)) == 0 and X.date_diff("month", at(2001, 1, 31, 12), at(2001, 2, 28, 12)) == 1
    # backwards: the negated count the other way (Jan 31 12:00 + 1 month = Feb 28 12:00 is reached)
    assert X.date_diff("month", at(2001, 2, 28, 12), at(2001, 1, 31, 12)) == -1 and X.date_diff("month", at(2001, 2, 28, 11), at(2001, 1, 31, 12)) == 0
    assert X.date_diff("second", 999_999, 0) == 0 and X.date_diff("second", -1, 1_000_000) == 1 and X.date_diff("second", -1_000_001, 1_000_000) == 2 and X.date_diff("millisecond", -1, 0) == 1
    # rounding as DateTimes.roundDiv writes it; Java's wrap at the ends
    assert X.cast_precision(1500, 3) == 2000 and X.cast_precision(-1501, 3) == -2000 and X.cast_precision(1499, 3) == 1000 and X.cast_precision(-1499, 3) == -1000
    assert X.cast_precision(-1500, 3) == -1000      # roundDiv as written: (value + 1 - factor / 2) / factor sends a negative tie toward zero
    assert X.cast_precision(X.INT64_MAX, 6) == X.INT64_MAX and X.cast_precision(X.INT64_MAX, 0) == X.wrap64(X.round_div(X.INT64_MAX, 10**6) * 10**6)
    assert X.round_div(X.INT64_MAX, 1000) == X.wrap64(X.INT64_MAX + 500) // 1000 + 1 < 0      # the addition wrapped: a negative quotient, truncated toward zero
    assert X.date_add("day", 1, at(2020, 1, 1, 0, 0, 0, 500_000), 0) == at(2020, 1, 2, 0, 0, 1) and X.date_add("day", 1, at(2020, 1, 1, 0, 0, 0, 499_000), 0) == at(2020, 1, 2)
    assert X.date_add("millisecond", 5, 1_234_567, 2) == 1_240_567 and X.date_add("millisecond", 5, 1_234_567, 4) == 1_239_567
    # saturation and overflow
    assert X.from_date(106751991) == 106751991 * X.US_PER_DAY and X.from_date(106751992) == X.INT64_MAX and X.from_date(-106751991) == -106751991 * X.US_PER_DAY
    assert X.from_date(-106751992) == X.INT64_MIN and X.from_date(D.INT32_MIN) == X.INT64_MIN and X.from_date(D.INT32_MAX) == X.INT64_MAX
    for call in (lambda: X.date_trunc("second", X.INT64_MIN), lambda: X.date_trunc("year", X.INT64_MIN), lambda: X.date_add("day", 2**31, 0), lambda: X.date_add("day", -2**31 - 1, 0),
                 lambda: X.date_add("millisecond", 1, X.INT64_MAX), lambda: X.date_add("year", 2**31 - 1, 0), lambda: X.date_add("week", -2**31, 0)):
        with pytest.raises(X.OutOfRange):
            call()
    assert X.date_trunc("millisecond", X.INT64_MAX) == X.INT64_MAX - 807 and X.date_add("millisecond", 0, X.INT64_MAX) == X.INT64_MAX
    assert X.date_trunc(None, 5) is None and X.date_add("day", None, 5) is None and X.date_diff("day", 1, None) is None and X.date_trunc("HoUr", 3_600_000_001) == 3_600_000_000
    with pytest.raises(ValueError) as e:
        X.date_trunc("fortnight", 0)
    assert str(e.value) == "'fortnight' is not a valid Timestamp field"
    xs = C.edge_instants()
    assert len(xs) > 300 and xs[0] == X.INT64_MIN and xs[-1] == X.INT64_MAX and {-1, 0, 999, 1000, -1000} <= set(xs)


# ---- (b) the kernels' arithmetic on the host, under the sanitizers ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ts_main():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ts_main")
    deps = [SRC] + [os.path.join(ROOT, "presto-1_amd", "csrc", h) for h in ("device_date.h", "device_timestamp.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-std=c++17"] + SANITIZE + ["-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def run(exe, lines, tmp_path, name):
    path = str(tmp_path / (name + ".cases"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    # (the time limit only catches a program that does not end: the cases take a second or two)
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    done = p.stdout.decode().splitlines()
    assert p.returncode == 0, "sanitizer report or crash (exit %d) behind case %d:\n%s" % (p.returncode, len(done), p.stderr.decode()[-3000:])
    assert len(done) == len(lines)
    return done


def checked(call):
    try:
        return str(call())
    except X.OutOfRange:
        return "OVERFLOW"


def test_host_unary_and_casts(ts_main, tmp_path):
    xs = C.instants()
    got = run(ts_main, ["all - %d 0" % t for t in xs], tmp_path, "unary")
    for t, g in zip(xs, got):
        assert g == " ".join(str(v) for v in X.unary_row(t) + (X.double_bits(X.to_unixtime(t)),)), t
    lines = ["cast %d %d 0" % (q, t) for q in C.PRECISIONS for t in xs] + ["to_date - %d 0" % t for t in xs] + ["from_date - %d 0" % d for d in C.DATE_CAST_DAYS]
    want = [str(X.cast_precision(t, q)) for q in C.PRECISIONS for t in xs] + [str(X.to_date(t)) for t in xs] + [str(X.from_date(d)) for d in C.DATE_CAST_DAYS]
    got = run(ts_main, lines, tmp_path, "casts")
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:10]


def test_host_trunc_add_diff(ts_main, tmp_path):
    xs, lines, want = C.edge_instants() + C.random_instants(300, seed=32), [], []
    for u in X.UNITS:
        k = C.UNIT_CODES[u]
        for i, t in enumerate(xs):
            lines.append("date_trunc %d %d 0" % (k, t))
            want.append(checked(lambda: X.date_trunc(u, t)))
            for j, v in enumerate(C.AMOUNTS):
                p = (i + j) % 7                                                      # every precision with every unit and amount, spread over the instants
                lines.append("date_add %d %d %d" % (k * 8 + p, v, t))
                want.append(checked(lambda: X.date_add(u, v, t, p)))
        for a, b in C.diff_pairs():
            lines.append("date_diff %d %d %d" % (k, a, b))
            want.append(str(X.date_diff(u, a, b)))
    for t in C.edge_instants()[::5]:                                                 # every p in 0..6 on the same instant
        for p in C.PRECISIONS:
            for u, v in (("millisecond", 1), ("second", -1), ("month", 1), ("day", 0)):
                lines.append("date_add %d %d %d" % (C.UNIT_CODES[u] * 8 + p, v, t))
                want.append(checked(lambda: X.date_add(u, v, t, p)))
    got = run(ts_main, lines, tmp_path, "binary")
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:10]
    assert 1000 < want.count("OVERFLOW") < len(want) // 2


# ---- (c) the generated programs compile for gfx950 ---------------------------------------------------------------------------------------
def unary_exprs(pkg, t):
    return [pkg.year(t), pkg.quarter(t), pkg.month(t), pkg.week(t), pkg.day(t), pkg.day_of_week(t), pkg.day_of_year(t), pkg.year_of_week(t), pkg.last_day_of_month(t),
            pkg.hour(t), pkg.minute(t), pkg.second(t), pkg.millisecond(t), pkg.to_unixtime(t)]


def test_every_op_compiles(pkg):
    f, T, B, D_ = pkg.field, pkg.TIMESTAMP, pkg.BIGINT, pkg.DATE
    t, k, e, d = f(0, T), f(1, B), f(2, T), f(3, D_)
    types = [T, B, T, D_]
    pkg.precompile_page_processor(types, None, unary_exprs(pkg, t))
    projs = [g(u, *a) for u in X.UNITS for g, a in ((pkg.date_trunc, (t,)), (pkg.date_add, (k, t, 3)), (pkg.date_diff, (t, e)))]
    projs += [pkg.cast(t, T, q) for q in range(7)] + [pkg.cast(t, D_), pkg.cast(d, T)]
    filt = pkg.and_(pkg.and_(pkg.year(t).eq(1995), pkg.in_(t, [0, 1, None])), pkg.between(t, 0, pkg.constant(10**15, T)))
    for at in range(0, len(projs), 8):                                   # (a page processor takes a limited number of computed projections)
        pkg.precompile_page_processor(types, filt, projs[at:at + 8])
    src = "".join(pkg.page_processor_source(types, filt, projs[at:at + 8]) for at in (0, 24, 32))   # hour and year units, the casts
    assert src.count("#define TG_TIMESTAMP_HELPERS") == 3 and src.count("#define TG_DATE_HELPERS") == 3 and src.index("#define TG_DATE_HELPERS") < src.index("#define TG_TIMESTAMP_HELPERS")
    assert "tg_ts_add(8, " in src and "tg_ts_diff(8, " in src and "tg_ts_trunc(0, " in src and "TG_RAISE(TG_E_RANGE)" in src and "tg_ts_cast_precision(" in src
    # the helper text is the header itself, and only a program with a TIMESTAMP function gets it
    header = open(os.path.join(ROOT, "presto-1_amd", "csrc", "device_timestamp.h")).read()
    assert header in src and not re.search(r"^\s*#\s*include", header, re.M)
    plain = pkg.page_processor_source(types, t < e, [k + 1, pkg.if_(pkg.is_null(t), e, t), pkg.coalesce(t, e), pkg.cast(t, T, 6), pkg.to_unixtime(t)])
    assert "tg_ts" not in plain and "tg_date" not in plain and "/ 1000000.0" in plain
    assert "tg_ts" not in pkg.page_processor_source(types, None, [pkg.date_trunc(None, t), pkg.date_add(None, k, t)])


def test_fused_generators_take_timestamp_functions(pkg):
    f, T, B = pkg.field, pkg.TIMESTAMP, pkg.BIGINT
    aggs = [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1), (pkg.MIN_TIMESTAMP, 2), (pkg.MAX_TIMESTAMP, 2)]
    pkg.precompile_fused_aggregation([T, B], pkg.hour(f(0, T)) < 12, [f(0, T), pkg.minute(f(0, T)), pkg.date_trunc("hour", f(0, T))], aggs, [0])
    pkg.precompile_fused_probe([T, B], pkg.year(f(0, T)).eq(1995), [pkg.date_trunc("day", f(0, T)), f(1, B)], 0, [0, 1])


# ---- (d) errors when the program is created ---------------------------------------------------------------------------------------------
def raw_status(pkg, types, prog):
    spec, keep = prog.to_c()
    arr = (ctypes.c_int32 * len(types))(*types)
    return pkg._lib.lib().tgpu_precompile_page_processor(len(types), arr, ctypes.byref(spec))


def test_ir_errors(pkg):
    f, c, T, B, V, I, D_, DBL, E = pkg.field, pkg.constant, pkg.TIMESTAMP, pkg.BIGINT, pkg.VARCHAR, pkg.INTEGER, pkg.DATE, pkg.DOUBLE, pkg.expressions
    types = [T, B, V, I, D_]
    t, k, v, i, d = f(0, T), f(1, B), f(2, V), f(3, I), f(4, D_)
    month = c("month", V)

    def status(expr):
        return raw_status(pkg, types, E.FlatProgram(None, [expr]))

    COMPILER, NOT_SUPPORTED = -4, -8
    for name in ("YEAR", "QUARTER", "MONTH", "WEEK", "DAY", "DAY_OF_WEEK", "DAY_OF_YEAR", "YEAR_OF_WEEK", "LAST_DAY_OF_MONTH") + tuple(OWN):
        result = D_ if name == "LAST_DAY_OF_MONTH" else DBL if name == "TO_UNIXTIME" else B
        assert status(E.call(name, result, t)) == 0, name
        assert status(E.call(name, T, t)) == COMPILER and status(E.call(name, I, t)) == COMPILER, name                  # wrong result type
        assert status(E.call(name, result, t, t)) == COMPILER, name                                                     # wrong argument count
    for name in OWN:
        result = DBL if name == "TO_UNIXTIME" else B
        assert status(E.call(name, result, k)) == COMPILER and status(E.call(name, result, d)) == COMPILER, name        # no DATE / BIGINT flavour
    assert status(E.call("DATE_TRUNC", T, month, t)) == 0 and status(E.call("DATE_TRUNC", D_, month, t)) == COMPILER and status(E.call("DATE_TRUNC", T, month, d)) == COMPILER
    assert status(E.CallExpression("DATE_ADD", T, [month, k, t], ival=3)) == 0 and status(E.CallExpression("DATE_ADD", T, [month, k, t], ival=7)) == COMPILER
    assert status(E.CallExpression("DATE_ADD", T, [month, k, t], ival=-1)) == COMPILER and status(E.call("DATE_ADD", T, month, i, t)) == COMPILER
    assert status(E.call("DATE_ADD", D_, month, k, t)) == COMPILER and status(E.call("DATE_DIFF", B, month, t, d)) == COMPILER and status(E.call("DATE_DIFF", B, month, d, t)) == COMPILER
    assert status(E.call("DATE_DIFF", T, month, t, t)) == COMPILER and status(E.call("DATE_DIFF", B, month, t, t)) == 0
    # casts: DATE <-> TIMESTAMP and TIMESTAMP -> TIMESTAMP(q) only
    assert status(pkg.cast(t, D_)) == 0 and status(pkg.cast(d, T)) == 0 and all(status(pkg.cast(t, T, q)) == 0 for q in range(7))
    assert status(pkg.cast(t, T, 7)) == COMPILER and status(pkg.cast(t, T, -1)) == COMPILER
    for other in (B, I, DBL, V, pkg.BOOLEAN):
        assert status(pkg.cast(t, other)) == COMPILER, other
    for src in (k, i, v):
        assert status(pkg.cast(src, T)) == COMPILER
    # arithmetic on TIMESTAMP is outside the IR (timestamp +- interval)
    assert status(E.call("ADD", T, t, t)) == COMPILER and status(E.call("SUBTRACT", T, t, t)) == COMPILER and status(E.call("NEGATE", T, t)) == COMPILER
    assert status(E.call("LESS_THAN", pkg.BOOLEAN, t, k)) == COMPILER and status(t < t) == 0
    # the unit: a constant, one of nine, in any case
    for expr in (pkg.date_trunc(v, t), pkg.date_add(v, k, t), pkg.date_diff(pkg.substr(v, 1), t, t)):
        with pytest.raises(pkg.TgpuError) as e:
            pkg.precompile_page_processor(types, None, [expr])
        assert e.value.code == NOT_SUPPORTED and "the unit must be a VARCHAR constant" in str(e.value)
    for unit, lowered in (("fortnight", "fortnight"), ("MICROSECOND", "microsecond"), ("", ""), ("months", "months"), ("Ho ur", "ho ur")):
        for expr in (pkg.date_trunc(unit, t), pkg.date_add(unit, k, t), pkg.date_diff(unit, t, t)):
            with pytest.raises(pkg.TgpuError) as e:
                pkg.precompile_page_processor(types, None, [expr])
            assert e.value.code == -1 and ("'%s' is not a valid Timestamp field" % lowered) in str(e.value), str(e.value)
    sources = [pkg.page_processor_source(types, None, [pkg.date_trunc(u, t), pkg.date_add(u, k, t)]) for u in ("hour", "HOUR", "hOuR")]
    assert sources[0] == sources[1] == sources[2] and "tg_ts_trunc(3, " in sources[0]


# ---- (e) the IR's layout and the header ------------------------------------------------------------------------------------------------------
def test_flat_program_layout_and_header(pkg):
    f, T, B, V, E = pkg.field, pkg.TIMESTAMP, pkg.BIGINT, pkg.VARCHAR, pkg.expressions
    assert T == 7 and [E.OPS[n] for n in OWN] == list(range(52, 57)) and all(hasattr(pkg, n.lower()) for n in OWN)
    assert (pkg.MIN_TIMESTAMP, pkg.MAX_TIMESTAMP) == (17, 18)
    prog = E.FlatProgram(None, [pkg.date_add("month", 3, f(0, T), 2), pkg.date_diff("year", f(0, T), 11556), pkg.cast(f(0, T), T, 3), pkg.date_add("month", 3, f(0, pkg.DATE))])
    add = prog.nodes[prog.projection_roots[0]]
    assert add["op"] == 31 and add["type"] == T and add["ival"] == 2 and [prog.nodes[a]["type"] for a in add["args"]] == [V, B, T]
    diff = prog.nodes[prog.projection_roots[1]]
    assert diff["op"] == 32 and diff["type"] == B and prog.nodes[diff["args"][2]]["type"] == T and prog.nodes[diff["args"][2]]["ival"] == 11556
    assert prog.nodes[prog.projection_roots[2]]["ival"] == 3 and prog.nodes[prog.projection_roots[3]]["ival"] == 0 and prog.nodes[prog.projection_roots[3]]["type"] == pkg.DATE
    header = open(os.path.join(ROOT, "include/tgpu.h")).read()
    for name, value in zip(OWN, range(52, 57)):
        assert "TGPU_OP_%s = %d" % (name, value) in header
    for rule in ("TGPU_TIMESTAMP = 7", "ShortTimestampType.java:128-161", "AbstractLongType.java:126-166", "TGPU_AGG_MIN_TIMESTAMP = 17", "TGPU_AGG_MAX_TIMESTAMP = 18",
                 "is not a valid Timestamp field", "SATURATES", "wraparound included", "from_unixtime", "date_format / date_parse / to_iso8601"):
        assert rule in header, rule
    block = pkg.Block(T, [1, None, -5])
    assert block.values.dtype.name == "int64" and pkg.Page(block).rows() == [(1,), (None,), (-5,)] and pkg.spi.TYPE_NAMES[T] == "timestamp"

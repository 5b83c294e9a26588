"""The Java glue's TIMESTAMP mapping against the header and, where a checkout of the reference is at hand, against the reference's declarations, as
text (there is no JDK here): the type code and its block class, the function names of operator/scalar/timestamp/, the precision handed over for
date_add and the timestamp -> timestamp cast, and what keeps the Java operator."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/core/"
strip = lambda t: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))


def read(path):
    return open(os.path.join(ROOT, path)).read()


def test_type_code_and_block_class():
    pages, header = read("java/io/trino/operator/gpu/GpuPages.java"), read("include/tgpu.h")
    assert "TGPU_TIMESTAMP = 7" in header and re.search(r"T_VARCHAR = 6, T_TIMESTAMP = 7;", pages)
    code = strip(pages)
    assert re.search(r"type instanceof io\.trino\.spi\.type\.TimestampType && \(\(io\.trino\.spi\.type\.TimestampType\) type\)\.isShort\(\)\) return T_TIMESTAMP;", code)
    assert "TimestampWithTimeZone" not in code                                   # falls through to "type not supported": the plan node keeps the Java operator
    assert code.index("isShort()") < code.index('throw new IllegalArgumentException("type not supported by the GPU operators')
    assert re.search(r"case T_BIGINT: case T_DOUBLE: case T_TIMESTAMP: values\[ch\] = new long\[positions\];", code)
    assert re.search(r"case T_BIGINT: case T_DOUBLE: case T_TIMESTAMP: blocks\[ch\] = new LongArrayBlock\(", code)
    shim = read("jni/tgpu_jni.c")
    assert "t == TGPU_BIGINT || t == TGPU_DOUBLE || t == TGPU_TIMESTAMP ? 8" in shim
    factories = strip(read("java/io/trino/operator/gpu/GpuOperatorFactories.java"))
    assert factories.count("codes = windowTypeCodes(sourceTypes);") == 3 and "code == GpuPages.T_TIMESTAMP" in factories      # window nodes with a timestamp channel keep the Java operator


def test_function_names_and_precision():
    glue = read("java/io/trino/operator/gpu/GpuRowExpressions.java")
    header = read("include/tgpu.h")
    for name, value in (("HOUR", 52), ("MINUTE", 53), ("SECOND", 54), ("MILLISECOND", 55), ("TO_UNIXTIME", 56)):
        assert re.search(r"\bOP_%s = %d[,;]" % (name, value), glue) and "TGPU_OP_%s = %d" % (name, value) in header, name
    code = strip(glue)
    table = code[code.index("private static int timestampFunction("):code.index("private static boolean isShortTimestamp(")]
    assert re.findall(r'case "(\w+)":', table) == ["hour", "minute", "second", "millisecond", "to_unixtime"]
    # the date-function names serve both flavours: the DATE one is tried first, the short-timestamp one next, with p on date_add's node
    assert "int timestampOp = dateOp != 0 ? dateOp : timestampFunction(name, call.getArguments().size());" in code
    assert "timestampOp == OP_DATE_ADD ? ((TimestampType) call.getArguments().get(2).getType()).getPrecision() : 0" in code
    assert "return emit(p, CALL, type, timestampOp, args, false, precision, 0, 0);" in code
    # casts: date <-> timestamp and timestamp -> timestamp with the target precision when it narrows; nothing else passes the generic operator loop
    assert "precision = source <= target ? 6 : target;" in code and "return emit(p, CALL, type, OP_CAST, new int[] {add(p, argument)}, false, precision, 0, 0);" in code
    assert '"date".equalsIgnoreCase(name)' in code and "is not in the GPU IR" in code[code.index("op == OP_CAST && (type == T_TIMESTAMP"):][:400]
    assert "((TimestampType) type).isShort()" in code
    # the shim hands every node's long to ival, whatever the node's kind
    assert "o->ival = iv[i]; o->dval = dv[i];" in read("jni/tgpu_jni.c")


def test_names_against_the_reference():
    base = REF + "trino-main/src/main/java/io/trino/operator/scalar/timestamp/"
    if not os.path.isdir(base):
        pytest.skip("needs a checkout of the reference sources")
    code = strip(read("java/io/trino/operator/gpu/GpuRowExpressions.java"))
    date_table = code[code.index("private static int dateFunction("):code.index("private static boolean overDates(")]
    own_table = code[code.index("private static int timestampFunction("):code.index("private static boolean isShortTimestamp(")]
    labels = set(re.findall(r'case "(\w+)":', date_table + own_table))
    names = set()
    for f in ("ExtractDay", "ExtractDayOfWeek", "ExtractDayOfYear", "ExtractHour", "ExtractMillisecond", "ExtractMinute", "ExtractMonth", "ExtractQuarter", "ExtractSecond",
              "ExtractWeekOfYear", "ExtractYear", "ExtractYearOfWeek", "LastDayOfMonth", "DateAdd", "DateDiff", "DateTrunc", "ToUnixTime"):
        text = open(base + f + ".java").read()
        m = re.search(r"@ScalarFunction\((.*?)\)", text)
        assert m and '@SqlType("timestamp(p)") long' in text, f                    # each has a short-timestamp flavour
        names.update(re.findall(r'"(\w+)"', m.group(1)))
    assert names == labels, names ^ labels
    assert '@ScalarFunction("date")' in open(base + "TimestampToDateCast.java").read()
    assert "round(epochMicros, (int) (MAX_SHORT_PRECISION - targetPrecision))" in open(base + "TimestampToTimestampCast.java").read()
    assert "if (precision <= 3) {" in open(base + "DateAdd.java").read()
    spi = REF + "trino-spi/src/main/java/io/trino/spi/type/"
    short, abstract_long = open(spi + "ShortTimestampType.java").read().split("\n"), open(spi + "AbstractLongType.java").read().split("\n")
    # the citation next to the enum: the same operator bodies in both classes
    for op, body in (("EQUAL", "return left == right;"), ("XX_HASH_64", "return XxHash64.hash(value);"), ("COMPARISON", "return Long.compare(left, right);")):
        for lines, span in ((short, (127, 161)), (abstract_long, (125, 166))):
            at = [i for i in range(*span) if "@ScalarOperator(%s)" % op in lines[i]]
            assert len(at) == 1 and body in "".join(lines[at[0]:at[0] + 5]), (op, span)
    assert "return AbstractLongType.hash(value);" in "".join(short[127:161])
    assert "public final boolean isShort()" in open(spi + "TimestampType.java").read()

package io.trino.operator.gpu;

import io.airlift.slice.Slice;
import io.trino.spi.type.BigintType;
import io.trino.spi.type.DateType;
import io.trino.spi.type.DoubleType;
import io.trino.spi.type.IntegerType;
import io.trino.spi.type.TimestampType;
import io.trino.spi.type.Type;
import io.trino.spi.type.VarcharType;
import io.trino.sql.relational.CallExpression;
import io.trino.sql.relational.ConstantExpression;
import io.trino.sql.relational.InputReferenceExpression;
import io.trino.sql.relational.RowExpression;
import io.trino.sql.relational.SpecialForm;
import io.trino.type.JoniRegexp;
import io.trino.type.LikeFunctions;

import java.io.ByteArrayOutputStream;
import java.util.ArrayList;
import java.util.List;
import java.util.Optional;

/**
 * RowExpression (core/trino-main/src/main/java/io/trino/sql/relational) -> the tgpu_expr_node array of tgpu_page_processor_spec: what the
 * reference hands to ExpressionCompiler.compilePageProcessor (sql/gen/ExpressionCompiler.java:94-122) goes to the library's own compiler
 * (hiprtc, gfx950) instead.  An expression outside the library's IR makes {@link #serialize} return empty: the planner then keeps the Java operator.
 */
public final class GpuRowExpressions
{
    // tgpu_expr_kind / tgpu_expr_op / tgpu_special_form (include/tgpu.h)
    private static final int INPUT = 0, CONST = 1, CALL = 2, SPECIAL = 3;
    private static final String[] OPERATORS = {null, "$operator$ADD", "$operator$SUBTRACT", "$operator$MULTIPLY", "$operator$DIVIDE", "$operator$MODULUS", "$operator$NEGATION",
            "$operator$EQUAL", "$operator$NOT_EQUAL", "$operator$LESS_THAN", "$operator$LESS_THAN_OR_EQUAL", "$operator$GREATER_THAN", "$operator$GREATER_THAN_OR_EQUAL", "not",
            "$operator$CAST"};
    private static final int OP_EQUAL = 7, OP_LIKE = 15, SF_OR = 2, SF_IN = 7;   // TGPU_OP_EQUAL, TGPU_OP_LIKE, TGPU_SF_OR, TGPU_SF_IN
    private static final String LIKE_FUNCTION_NAME = "like";                    // LikeFunctions.likeVarchar (type/LikeFunctions.java:71-74)
    // TGPU_OP_LENGTH .. TGPU_OP_STARTS_WITH: operator/scalar/StringFunctions.java (length :94, strpos :205, substring / alias substr :274 and
    // :321, starts_with :909) and operator/scalar/ConcatFunction.java ("concat"), over varchar arguments
    private static final int OP_CAST = 14, OP_LENGTH = 16, OP_SUBSTR = 17, OP_CONCAT = 18, OP_STRPOS = 19, OP_STARTS_WITH = 20;
    private static final String CAST_OPERATOR = "$operator$CAST";
    // TGPU_OP_YEAR .. TGPU_OP_DATE_DIFF: operator/scalar/DateTimeFunctions.java over DATE (truncateDate :260, addFieldValueDate :270, diffDate :280,
    // dayOfWeekFromDate :436 ... yearFromDate :517)
    private static final int OP_YEAR = 21, OP_QUARTER = 22, OP_MONTH = 23, OP_WEEK = 24, OP_DAY = 25, OP_DAY_OF_WEEK = 26, OP_DAY_OF_YEAR = 27, OP_YEAR_OF_WEEK = 28;
    private static final int OP_LAST_DAY_OF_MONTH = 29, OP_DATE_TRUNC = 30, OP_DATE_ADD = 31, OP_DATE_DIFF = 32;
    // TGPU_OP_ABS .. TGPU_OP_RADIANS: operator/scalar/MathFunctions.java over BIGINT, INTEGER and DOUBLE (abs :127-148, ceiling :245-264, truncate :317,
    // floor :390-409, log :473, power :561, round :724-833, sign :1085-1125)
    private static final int OP_MODULUS = 5, OP_ABS = 33, OP_SIGN = 34, OP_FLOOR = 35, OP_CEILING = 36, OP_TRUNCATE = 37, OP_ROUND = 38, OP_SQRT = 39, OP_CBRT = 40, OP_EXP = 41;
    private static final int OP_LN = 42, OP_LOG2 = 43, OP_LOG10 = 44, OP_LOG = 45, OP_POWER = 46, OP_IS_NAN = 47, OP_IS_FINITE = 48, OP_IS_INFINITE = 49, OP_DEGREES = 50, OP_RADIANS = 51;
    // TGPU_OP_HOUR .. TGPU_OP_TO_UNIXTIME and the timestamp flavours of TGPU_OP_YEAR .. TGPU_OP_DATE_DIFF: operator/scalar/timestamp/ (ExtractHour.java,
    // ExtractMinute.java, ExtractSecond.java, ExtractMillisecond.java, ToUnixTime.java; DateTrunc.java, DateAdd.java, DateDiff.java ...), over a short timestamp(p)
    private static final int OP_HOUR = 52, OP_MINUTE = 53, OP_SECOND = 54, OP_MILLISECOND = 55, OP_TO_UNIXTIME = 56;
    private static final int T_TIMESTAMP = GpuPages.T_TIMESTAMP;

    public static final class Program
    {
        public final List<int[]> nodes = new ArrayList<>();      // {kind, type, op, n_args, arg0, arg1, arg2, is_null, slen}
        public final List<Long> longValues = new ArrayList<>();
        public final List<Double> doubleValues = new ArrayList<>();
        public final ByteArrayOutputStream stringPool = new ByteArrayOutputStream();
        public int filterRoot = -1;
        public int[] projectionRoots = new int[0];

        public int[][] nodeArray()
        {
            return nodes.toArray(new int[0][]);
        }

        public long[] longArray()
        {
            return longValues.stream().mapToLong(Long::longValue).toArray();
        }

        public double[] doubleArray()
        {
            return doubleValues.stream().mapToDouble(Double::doubleValue).toArray();
        }
    }

    private GpuRowExpressions() {}

    public static Optional<Program> serialize(Optional<RowExpression> filter, List<RowExpression> projections)
    {
        try {
            Program program = new Program();
            if (filter.isPresent()) {
                program.filterRoot = add(program, filter.get());
            }
            program.projectionRoots = projections.stream().mapToInt(p -> add(program, p)).toArray();
            return Optional.of(program);
        }
        catch (IllegalArgumentException unsupported) {
            return Optional.empty();
        }
    }

    private static int emit(Program p, int kind, int type, int op, int[] args, boolean isNull, long longValue, double doubleValue, int stringLength)
    {
        int[] node = {kind, type, op, args.length, args.length > 0 ? args[0] : 0, args.length > 1 ? args[1] : 0, args.length > 2 ? args[2] : 0, isNull ? 1 : 0, stringLength};
        p.nodes.add(node);
        p.longValues.add(longValue);
        p.doubleValues.add(doubleValue);
        return p.nodes.size() - 1;
    }

    private static int add(Program p, RowExpression e)
    {
        int type = GpuPages.typeCode(e.getType());
        if (e instanceof InputReferenceExpression) {
            return emit(p, INPUT, type, ((InputReferenceExpression) e).getField(), new int[0], false, 0, 0, 0);
        }
        if (e instanceof ConstantExpression) {
            Object value = ((ConstantExpression) e).getValue();
            if (value == null) {
                return emit(p, CONST, type, 0, new int[0], true, 0, 0, 0);
            }
            if (value instanceof Slice) {
                byte[] bytes = ((Slice) value).getBytes();
                int at = p.stringPool.size();
                p.stringPool.write(bytes, 0, bytes.length);
                return emit(p, CONST, type, 0, new int[0], false, at, 0, bytes.length);
            }
            if (value instanceof Double) {
                return emit(p, CONST, type, 0, new int[0], false, 0, (Double) value, 0);
            }
            if (value instanceof Boolean) {
                return emit(p, CONST, type, 0, new int[0], false, (Boolean) value ? 1 : 0, 0, 0);
            }
            return emit(p, CONST, type, 0, new int[0], false, ((Number) value).longValue(), 0, 0);
        }
        if (e instanceof CallExpression) {
            CallExpression call = (CallExpression) e;
            String name = call.getResolvedFunction().getSignature().getName();
            if (CAST_OPERATOR.equalsIgnoreCase(name) && call.getType() instanceof VarcharType) {
                return addCastToVarchar(p, type, call);
            }
            int stringOp = stringFunction(name, call.getArguments().size());
            if (stringOp != 0) {
                return addStringFunction(p, type, stringOp, call.getArguments());
            }
            int dateOp = dateFunction(name, call.getArguments().size());
            if (dateOp != 0 && overDates(dateOp, call.getArguments())) {
                int[] args = call.getArguments().stream().mapToInt(a -> add(p, a)).toArray();
                return emit(p, CALL, type, dateOp, args, false, 0, 0, 0);
            }
            int timestampOp = dateOp != 0 ? dateOp : timestampFunction(name, call.getArguments().size());
            if (timestampOp != 0 && overTimestamps(timestampOp, call.getArguments())) {
                int[] args = call.getArguments().stream().mapToInt(a -> add(p, a)).toArray();
                // date_add rounds its millisecond result to the argument's precision when that is 3 or less (DateAdd.java:50-52): the node carries p
                long precision = timestampOp == OP_DATE_ADD ? ((TimestampType) call.getArguments().get(2).getType()).getPrecision() : 0;
                return emit(p, CALL, type, timestampOp, args, false, precision, 0, 0);
            }
            if (isTimestampCast(name, call)) {
                return addTimestampCast(p, type, call);
            }
            if (call.getArguments().isEmpty() && call.getType() instanceof DoubleType) {
                Double constant = mathConstant(name);
                if (constant != null) {
                    return emit(p, CONST, type, 0, new int[0], false, 0, constant, 0);
                }
            }
            int mathOp = mathFunction(name, call.getArguments().size());
            if (mathOp != 0 && overNumbers(mathOp, call.getType(), call.getArguments())) {
                int[] args = call.getArguments().stream().mapToInt(a -> add(p, a)).toArray();
                return emit(p, CALL, type, mathOp, args, false, 0, 0, 0);
            }
            for (int op = 1; op < OPERATORS.length; op++) {
                if (OPERATORS[op].equalsIgnoreCase(name)) {
                    if (op == OP_CAST && (type == T_TIMESTAMP || call.getArguments().stream().anyMatch(a -> isShortTimestamp(a.getType())))) {
                        throw new IllegalArgumentException("CAST between timestamp and " + call.getType() + " is not in the GPU IR");   // (date and timestamp(p): above)
                    }
                    int[] args = call.getArguments().stream().mapToInt(a -> add(p, a)).toArray();
                    return emit(p, CALL, type, op, args, false, 0, 0, 0);
                }
            }
            if (LIKE_FUNCTION_NAME.equalsIgnoreCase(name) && call.getArguments().size() == 2) {
                return addLike(p, type, call.getArguments().get(0), call.getArguments().get(1));
            }
            throw new IllegalArgumentException("function not in the GPU IR: " + name);
        }
        if (e instanceof SpecialForm) {
            SpecialForm form = (SpecialForm) e;
            if (form.getForm() == SpecialForm.Form.IN) {
                return addIn(p, type, form.getArguments());
            }
            int op;
            switch (form.getForm()) {
                case AND: op = 1; break;
                case OR: op = 2; break;
                case IF: op = 3; break;
                case IS_NULL: op = 4; break;
                case COALESCE: op = 5; break;
                case BETWEEN: op = 6; break;
                default: throw new IllegalArgumentException("special form not in the GPU IR: " + form.getForm());
            }
            List<RowExpression> arguments = form.getArguments();
            if (arguments.size() > 3) {
                throw new IllegalArgumentException("special form with more than 3 arguments");
            }
            int[] args = arguments.stream().mapToInt(a -> add(p, a)).toArray();
            return emit(p, SPECIAL, type, op, args, false, 0, 0, 0);
        }
        throw new IllegalArgumentException("expression not in the GPU IR: " + e);
    }

    private static int stringFunction(String name, int arguments)
    {
        switch (name.toLowerCase(java.util.Locale.ENGLISH)) {
            case "length": return arguments == 1 ? OP_LENGTH : 0;
            case "substr":
            case "substring": return arguments == 2 || arguments == 3 ? OP_SUBSTR : 0;
            case "concat": return arguments >= 2 ? OP_CONCAT : 0;
            case "strpos": return arguments == 2 ? OP_STRPOS : 0;   // the three-argument form (instance) is not in the IR
            case "starts_with": return arguments == 2 ? OP_STARTS_WITH : 0;
            default: return 0;
        }
    }

    /**
     * The names and aliases of DateTimeFunctions.java's DATE functions -> TGPU_OP_YEAR .. TGPU_OP_DATE_DIFF.  EXTRACT(field FROM d) arrives
     * as these function names.  d + INTERVAL arrives as an interval operator, which is outside the IR: a planner that wants it on the device
     * folds a constant interval into date_add first.
     */
    private static int dateFunction(String name, int arguments)
    {
        switch (name.toLowerCase(java.util.Locale.ENGLISH)) {
            case "year": return arguments == 1 ? OP_YEAR : 0;
            case "quarter": return arguments == 1 ? OP_QUARTER : 0;
            case "month": return arguments == 1 ? OP_MONTH : 0;
            case "week":
            case "week_of_year": return arguments == 1 ? OP_WEEK : 0;
            case "day":
            case "day_of_month": return arguments == 1 ? OP_DAY : 0;
            case "day_of_week":
            case "dow": return arguments == 1 ? OP_DAY_OF_WEEK : 0;
            case "day_of_year":
            case "doy": return arguments == 1 ? OP_DAY_OF_YEAR : 0;
            case "year_of_week":
            case "yow": return arguments == 1 ? OP_YEAR_OF_WEEK : 0;
            case "last_day_of_month": return arguments == 1 ? OP_LAST_DAY_OF_MONTH : 0;
            case "date_trunc": return arguments == 2 ? OP_DATE_TRUNC : 0;
            case "date_add": return arguments == 3 ? OP_DATE_ADD : 0;
            case "date_diff": return arguments == 3 ? OP_DATE_DIFF : 0;
            default: return 0;
        }
    }

    /**
     * The same names exist over timestamps, times and intervals: the DATE flavour is decided here, the short-timestamp flavour by
     * overTimestamps, every other one falls through to "function not in the GPU IR".  The unit of date_trunc / date_add / date_diff is a varchar, which the library wants constant.
     */
    private static boolean overDates(int op, List<RowExpression> arguments)
    {
        if (op < OP_DATE_TRUNC) {
            return arguments.get(0).getType() instanceof DateType;
        }
        if (!(arguments.get(0).getType() instanceof VarcharType)) {
            return false;
        }
        boolean dates = arguments.get(arguments.size() - 1).getType() instanceof DateType;
        return op == OP_DATE_DIFF ? dates && arguments.get(1).getType() instanceof DateType : dates;
    }

    /** the functions that exist over timestamps only (operator/scalar/timestamp/ExtractHour.java ... ToUnixTime.java) */
    private static int timestampFunction(String name, int arguments)
    {
        switch (name.toLowerCase(java.util.Locale.ENGLISH)) {
            case "hour": return arguments == 1 ? OP_HOUR : 0;
            case "minute": return arguments == 1 ? OP_MINUTE : 0;
            case "second": return arguments == 1 ? OP_SECOND : 0;
            case "millisecond": return arguments == 1 ? OP_MILLISECOND : 0;
            case "to_unixtime": return arguments == 1 ? OP_TO_UNIXTIME : 0;
            default: return 0;
        }
    }

    /** timestamp(p) with p <= 6: epoch microseconds in a long.  timestamp(p > 6) and timestamp with time zone are outside the IR */
    private static boolean isShortTimestamp(io.trino.spi.type.Type type)
    {
        return type instanceof TimestampType && ((TimestampType) type).isShort();
    }

    /** the timestamp flavour of a date / time function: its last argument (date_diff: its last two) is a short timestamp; the unit is a varchar */
    private static boolean overTimestamps(int op, List<RowExpression> arguments)
    {
        if (op < OP_DATE_TRUNC || op >= OP_HOUR) {
            return isShortTimestamp(arguments.get(0).getType());
        }
        if (!(arguments.get(0).getType() instanceof VarcharType)) {
            return false;
        }
        boolean timestamps = isShortTimestamp(arguments.get(arguments.size() - 1).getType());
        return op == OP_DATE_DIFF ? timestamps && isShortTimestamp(arguments.get(1).getType()) : timestamps;
    }

    /**
     * CAST(date AS timestamp(p)) (DateToTimestampCast.java), CAST(timestamp(p) AS date) and its function name date(t) (TimestampToDateCast.java) and
     * CAST(timestamp(p) AS timestamp(q)) (TimestampToTimestampCast.java), short timestamps only
     */
    private static boolean isTimestampCast(String name, CallExpression call)
    {
        if (call.getArguments().size() != 1) {
            return false;
        }
        io.trino.spi.type.Type from = call.getArguments().get(0).getType();
        io.trino.spi.type.Type to = call.getType();
        if ("date".equalsIgnoreCase(name)) {
            return isShortTimestamp(from) && to instanceof DateType;
        }
        if (!CAST_OPERATOR.equalsIgnoreCase(name)) {
            return false;
        }
        return (isShortTimestamp(from) && (to instanceof DateType || isShortTimestamp(to))) || (from instanceof DateType && isShortTimestamp(to));
    }

    /**
     * The CAST node's long is the target precision of a timestamp -> timestamp cast that narrows: the library rounds to it as shortToShort does
     * (TimestampToTimestampCast.java:37-49).  A widening cast returns its argument there, which is the node's 6
     */
    private static int addTimestampCast(Program p, int type, CallExpression call)
    {
        RowExpression argument = call.getArguments().get(0);
        long precision = 0;
        if (isShortTimestamp(argument.getType()) && isShortTimestamp(call.getType())) {
            int source = ((TimestampType) argument.getType()).getPrecision();
            int target = ((TimestampType) call.getType()).getPrecision();
            precision = source <= target ? 6 : target;
        }
        return emit(p, CALL, type, OP_CAST, new int[] {add(p, argument)}, false, precision, 0, 0);
    }

    /**
     * The names and aliases of MathFunctions.java -> TGPU_OP_ABS .. TGPU_OP_RADIANS.  mod(a, b) is the IR's MODULUS, with one difference: a zero
     * integer divisor is DIVISION_BY_ZERO here, where the reference's function lets the raw ArithmeticException through (mod :513-524 has
     * no check; the % operator's has).  The trigonometric and hyperbolic functions, width_bucket, random, the bases, the CDFs and the
     * bitwise functions are outside the IR.
     */
    private static int mathFunction(String name, int arguments)
    {
        switch (name.toLowerCase(java.util.Locale.ENGLISH)) {
            case "abs": return arguments == 1 ? OP_ABS : 0;
            case "sign": return arguments == 1 ? OP_SIGN : 0;
            case "floor": return arguments == 1 ? OP_FLOOR : 0;
            case "ceil":
            case "ceiling": return arguments == 1 ? OP_CEILING : 0;
            case "truncate": return arguments == 1 ? OP_TRUNCATE : 0;   // truncate(x, n) exists over decimals only
            case "round": return arguments == 1 || arguments == 2 ? OP_ROUND : 0;
            case "sqrt": return arguments == 1 ? OP_SQRT : 0;
            case "cbrt": return arguments == 1 ? OP_CBRT : 0;
            case "exp": return arguments == 1 ? OP_EXP : 0;
            case "ln": return arguments == 1 ? OP_LN : 0;
            case "log2": return arguments == 1 ? OP_LOG2 : 0;
            case "log10": return arguments == 1 ? OP_LOG10 : 0;
            case "log": return arguments == 2 ? OP_LOG : 0;
            case "pow":
            case "power": return arguments == 2 ? OP_POWER : 0;
            case "is_nan": return arguments == 1 ? OP_IS_NAN : 0;
            case "is_finite": return arguments == 1 ? OP_IS_FINITE : 0;
            case "is_infinite": return arguments == 1 ? OP_IS_INFINITE : 0;
            case "degrees": return arguments == 1 ? OP_DEGREES : 0;
            case "radians": return arguments == 1 ? OP_RADIANS : 0;
            case "mod": return arguments == 2 ? OP_MODULUS : 0;
            default: return 0;
        }
    }

    /**
     * The same names exist over tinyint, smallint, real and decimal: only the BIGINT / INTEGER / DOUBLE flavours are in the IR, every other one
     * falls through to "function not in the GPU IR".  abs, sign, floor, ceiling, round and mod keep their argument's type; everything else
     * is over double.  The number of decimals of round is an integer, which the library wants constant.
     */
    private static boolean overNumbers(int op, Type result, List<RowExpression> arguments)
    {
        Type first = arguments.get(0).getType();
        boolean integer = first instanceof BigintType || first instanceof IntegerType;
        boolean typed = op == OP_ABS || op == OP_SIGN || op == OP_FLOOR || op == OP_CEILING || op == OP_ROUND || op == OP_MODULUS;
        if (!(first instanceof DoubleType) && !(typed && integer)) {
            return false;
        }
        if (op == OP_ROUND) {
            return result.equals(first) && (arguments.size() == 1 || arguments.get(1).getType() instanceof IntegerType);
        }
        if (op == OP_IS_NAN || op == OP_IS_FINITE || op == OP_IS_INFINITE) {
            return true;
        }
        return result.equals(first) && arguments.stream().allMatch(a -> a.getType().equals(first));
    }

    /** pi(), e(), nan() and infinity() fold to DOUBLE constants (MathFunctions.java :358, :553, :1189, :1197) */
    private static Double mathConstant(String name)
    {
        switch (name.toLowerCase(java.util.Locale.ENGLISH)) {
            case "pi": return Math.PI;
            case "e": return Math.E;
            case "nan": return Double.NaN;
            case "infinity": return Double.POSITIVE_INFINITY;
            default: return null;
        }
    }

    /**
     * length / substr / concat / strpos / starts_with over varchar -> TGPU_OP_LENGTH .. TGPU_OP_STARTS_WITH.  The same names exist over
     * char(x), varbinary and arrays: those are outside the IR.  concat(a, b, c, ...) is folded to the left, as the IR's CONCAT takes two.
     */
    private static int addStringFunction(Program p, int type, int op, List<RowExpression> arguments)
    {
        int strings = op == OP_LENGTH || op == OP_SUBSTR ? 1 : arguments.size();
        for (int i = 0; i < strings; i++) {
            if (!(arguments.get(i).getType() instanceof VarcharType)) {
                throw new IllegalArgumentException("string function over a type that is not varchar");
            }
        }
        int[] args = arguments.stream().mapToInt(a -> add(p, a)).toArray();
        if (op != OP_CONCAT) {
            return emit(p, CALL, type, op, args, false, 0, 0, 0);
        }
        int result = args[0];
        for (int i = 1; i < args.length; i++) {
            result = emit(p, CALL, type, OP_CONCAT, new int[] {result, args[i]}, false, 0, 0, 0);
        }
        return result;
    }

    /**
     * CAST(x AS varchar) from bigint / integer (String.valueOf), boolean and varchar.  The IR's VARCHAR has no length: a bounded varchar(n)
     * target, whose cast checks the length, is refused.
     */
    private static int addCastToVarchar(Program p, int type, CallExpression call)
    {
        if (!((VarcharType) call.getType()).isUnbounded()) {
            throw new IllegalArgumentException("CAST to a bounded varchar(n) is not in the GPU IR");
        }
        RowExpression argument = call.getArguments().get(0);
        String from = argument.getType().getTypeSignature().getBase();
        boolean unboundedVarchar = argument.getType() instanceof VarcharType && ((VarcharType) argument.getType()).isUnbounded();
        if (!(from.equals("bigint") || from.equals("integer") || from.equals("boolean") || unboundedVarchar)) {
            throw new IllegalArgumentException("CAST to varchar from " + from + " is not in the GPU IR");
        }
        return emit(p, CALL, type, OP_CAST, new int[] {add(p, argument)}, false, 0, 0, 0);
    }

    private static int addStringConstant(Program p, int type, byte[] bytes)
    {
        if (bytes == null) {
            return emit(p, CONST, type, 0, new int[0], true, 0, 0, 0);
        }
        int at = p.stringPool.size();
        p.stringPool.write(bytes, 0, bytes.length);
        return emit(p, CONST, type, 0, new int[0], false, at, 0, bytes.length);
    }

    private static byte[] constantBytes(RowExpression e)
    {
        if (!(e instanceof ConstantExpression)) {
            throw new IllegalArgumentException("LIKE pattern / escape is not a constant");
        }
        Object value = ((ConstantExpression) e).getValue();
        if (value != null && !(value instanceof Slice)) {
            throw new IllegalArgumentException("LIKE pattern / escape is not a varchar constant");
        }
        return value == null ? null : ((Slice) value).getBytes();
    }

    /**
     * value LIKE pattern -> TGPU_OP_LIKE(value, pattern constant [, escape constant]).  The pattern argument is either the call
     * $like_pattern(pattern [, escape]) over constants, or what the optimizer folded it to: a ConstantExpression holding the JoniRegexp
     * that LikeFunctions.likePattern built (type/LikeFunctions.java:198-241).  Anything else is outside the IR.
     */
    private static int addLike(Program p, int type, RowExpression value, RowExpression pattern)
    {
        int varchar = GpuPages.typeCode(value.getType());
        int valueNode = add(p, value);
        if (pattern instanceof CallExpression) {
            CallExpression call = (CallExpression) pattern;
            List<RowExpression> arguments = call.getArguments();
            if (!LikeFunctions.LIKE_PATTERN_FUNCTION_NAME.equalsIgnoreCase(call.getResolvedFunction().getSignature().getName()) || arguments.isEmpty() || arguments.size() > 2) {
                throw new IllegalArgumentException("LIKE pattern is not a $like_pattern call");
            }
            for (RowExpression argument : arguments) {
                if (GpuPages.typeCode(argument.getType()) != varchar) {   // the char(x) flavour pads the pattern: not in the IR
                    throw new IllegalArgumentException("LIKE pattern is not a varchar");
                }
            }
            int patternNode = addStringConstant(p, varchar, constantBytes(arguments.get(0)));
            if (arguments.size() == 1) {
                return emit(p, CALL, type, OP_LIKE, new int[] {valueNode, patternNode}, false, 0, 0, 0);
            }
            int escapeNode = addStringConstant(p, varchar, constantBytes(arguments.get(1)));
            return emit(p, CALL, type, OP_LIKE, new int[] {valueNode, patternNode, escapeNode}, false, 0, 0, 0);
        }
        if (pattern instanceof ConstantExpression) {
            Object folded = ((ConstantExpression) pattern).getValue();
            if (folded == null) {
                int patternNode = addStringConstant(p, varchar, null);
                return emit(p, CALL, type, OP_LIKE, new int[] {valueNode, patternNode}, false, 0, 0, 0);
            }
            if (folded instanceof JoniRegexp) {
                byte[] like = likePatternOfRegex(((JoniRegexp) folded).pattern().toStringUtf8()).getBytes(java.nio.charset.StandardCharsets.UTF_8);
                int patternNode = addStringConstant(p, varchar, like);
                int escapeNode = addStringConstant(p, varchar, new byte[] {'\\'});
                return emit(p, CALL, type, OP_LIKE, new int[] {valueNode, patternNode, escapeNode}, false, 0, 0, 0);
            }
        }
        throw new IllegalArgumentException("LIKE pattern is not a constant");
    }

    /**
     * The inverse of LikeFunctions.likePattern's translation: '^', then ".*" for '%', "." for '_', a backslash in front of each of
     * \ ^ $ . * and every other character (an escaped '%' or '_' among them) as itself, then '$'.  The translation is injective, so
     * the regex text gives back a LIKE pattern, written here with the escape character backslash.
     */
    static String likePatternOfRegex(String regex)
    {
        if (regex.length() < 2 || regex.charAt(0) != '^' || regex.charAt(regex.length() - 1) != '$') {
            throw new IllegalArgumentException("not a regex written by LikeFunctions.likePattern");
        }
        StringBuilder like = new StringBuilder();
        for (int i = 1; i < regex.length() - 1; i++) {
            char c = regex.charAt(i);
            if (c == '.') {
                if (i + 1 < regex.length() - 1 && regex.charAt(i + 1) == '*') {
                    like.append('%');
                    i++;
                }
                else {
                    like.append('_');
                }
                continue;
            }
            if (c == '\\') {
                i++;
                if (i >= regex.length() - 1) {
                    throw new IllegalArgumentException("not a regex written by LikeFunctions.likePattern");
                }
                c = regex.charAt(i);
            }
            else if (c == '^' || c == '$' || c == '*') {
                throw new IllegalArgumentException("not a regex written by LikeFunctions.likePattern");
            }
            if (c == '%' || c == '_' || c == '\\') {
                like.append('\\');
            }
            like.append(c);
        }
        return like.toString();
    }

    /**
     * value IN (items) (SpecialForm.Form.IN, sql/gen/InCodeGenerator.java:92-121) -> TGPU_SF_IN over the constant items, laid out as
     * consecutive CONST nodes named by (ival, slen) of the IN node.  Items that are not constants become "OR value = item", which is the
     * same in three-valued logic.
     */
    private static int addIn(Program p, int type, List<RowExpression> arguments)
    {
        if (arguments.size() < 2) {
            throw new IllegalArgumentException("IN without items");
        }
        int valueType = GpuPages.typeCode(arguments.get(0).getType());
        int valueNode = add(p, arguments.get(0));
        List<RowExpression> constants = new ArrayList<>();
        List<RowExpression> others = new ArrayList<>();
        for (RowExpression item : arguments.subList(1, arguments.size())) {
            if (GpuPages.typeCode(item.getType()) != valueType) {
                throw new IllegalArgumentException("IN item of another type");
            }
            (item instanceof ConstantExpression ? constants : others).add(item);
        }
        int[] otherNodes = others.stream().mapToInt(item -> add(p, item)).toArray();
        int result = -1;
        if (!constants.isEmpty()) {
            int first = p.nodes.size();
            for (RowExpression item : constants) {
                add(p, item);   // one CONST node each: the list stays consecutive
            }
            result = emit(p, SPECIAL, type, SF_IN, new int[] {valueNode}, false, first, 0, constants.size());
        }
        for (int itemNode : otherNodes) {
            int equal = emit(p, CALL, type, OP_EQUAL, new int[] {valueNode, itemNode}, false, 0, 0, 0);
            result = result < 0 ? equal : emit(p, SPECIAL, type, SF_OR, new int[] {result, equal}, false, 0, 0, 0);
        }
        return result;
    }
}

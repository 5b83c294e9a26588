/*
 * tgpu.h -- C ABI of the MI355X-native operator hot path (libtgpu.so).
 *
 * This is the drop-in boundary: exactly what a JNI shim for core/trino-main would bind (INTEGRATION.md shows
 * that shim).  Plain C: opaque handles, plain pointers and sizes, int32 status codes.  No torch / HIP types.
 *
 * Reference interfaces replaced (paths relative to the reference root;
 * M/ = core/trino-main/src/main/java/io/trino/ , S/ = core/trino-spi/src/main/java/io/trino/spi/):
 *   - tgpu_operator_*            <-> M/operator/Operator.java:20-102
 *   - tgpu_operator_factory_*    <-> M/operator/OperatorFactory.java:18-50
 *   - tgpu_block / tgpu_page     <-> S/Page.java:33-73, S/block/LongArrayBlock.java:38-75, IntArrayBlock.java,
 *                                    ByteArrayBlock.java, VariableWidthBlock.java:38-83, DictionaryBlock.java:40-100,
 *                                    RunLengthEncodedBlock.java:30-70
 *   - tgpu_filter_project_*      <-> M/operator/FilterAndProjectOperator.java:73-88 + M/sql/gen/ExpressionCompiler.java:94-122
 *   - tgpu_hash_aggregation_*    <-> M/operator/HashAggregationOperator.java:54-262
 *   - tgpu_hash_builder_* / tgpu_lookup_join_* <-> M/operator/HashBuilderOperator.java:54-152,
 *                                    M/operator/LookupJoinOperatorFactory.java:40-113, LookupJoinOperators.java:30-63
 *   - tgpu_group_by_hash_*       <-> M/operator/GroupByHash.java:45-99
 *   - tgpu_hash_page             <-> M/operator/InterpretedHashGenerator.java:56-70
 *   - tgpu_partition_page        <-> M/operator/PartitionedOutputOperator.java:406-426 + HashGenerator.java:24-35
 *   - tgpu_partitioned_output_*  <-> M/operator/PartitionedOutputOperator.java:46-486 (operator + PagePartitioner)
 *   - tgpu_top_n_* / tgpu_order_by_* <-> M/operator/TopNOperator.java:47-225, OrderByOperator.java:48-300
 *   - tgpu_lookup_outer_*        <-> M/operator/LookupOuterOperator.java:32-235, OuterLookupSource.java:146-190
 *   - tgpu_merge_pages_*         <-> M/operator/project/MergePages.java:64-190
 *   - tgpu_dynamic_filter_source_* <-> M/operator/DynamicFilterSourceOperator.java:74-425
 *   - tgpu_nested_loop_* / tgpu_filter_project_nested_loop_join_* <-> M/operator/NestedLoopBuildOperator.java, NestedLoopJoinPagesBuilder.java, NestedLoopJoinOperator.java
 *   - tgpu_set_builder_* / tgpu_hash_semi_join_* <-> M/operator/SetBuilderOperator.java:39-233, HashSemiJoinOperator.java:44-218, ChannelSet.java:62-108
 *   - tgpu_mark_distinct_* / tgpu_distinct_limit_* <-> M/operator/MarkDistinctOperator.java:37-203, MarkDistinctHash.java:31-87, DistinctLimitOperator.java:40-263
 *   - tgpu_row_number_* / tgpu_limit_* <-> M/operator/RowNumberOperator.java:43-364, LimitOperator.java:25-120
 *   - tgpu_top_n_ranking_*       <-> M/operator/TopNRankingOperator.java:42-310, GroupedTopNRowNumberBuilder.java:99-188, GroupedTopNRankBuilder.java
 *   - tgpu_window_*              <-> M/operator/WindowOperator.java:205-310,844-855, M/operator/window/WindowPartition.java:184-345, the function classes of M/operator/window
 *   - tgpu_serialize_page / tgpu_deserialize_page <-> M/execution/buffer/PagesSerde.java:64-160, PagesSerdeUtil.java:45-71,
 *                                    S/block/{LongArray,IntArray,ByteArray,VariableWidth,RunLength,Dictionary}BlockEncoding.java, EncoderUtil.java:33-118
 *   - tgpu_exchange_*            <-> M/operator/PartitionedOutputOperator.java:406-476 -> M/operator/ExchangeOperator.java (the hop between
 *                                    the stages of a FIXED_HASH / FIXED_BROADCAST distribution), over RCCL / xGMI instead of HTTP
 *   - tgpu_operator_add_input_output_page: Operator.addInput with a page that never left the device (no reference counterpart:
 *                                    on the JVM the Page object itself is what travels between operators)
 *
 * Threading rule = the reference's (M/operator/Driver.java:55-62): one caller at a time per handle; distinct
 * handles are independent, also when they belong to one context (their kernels then share its stream and execute in issue
 * order; the context serialises its staging buffers; the per-kernel profile assumes a single driver thread); a built lookup
 * source is immutable and shared read-only by probe operators (outer joins mark visited build positions with idempotent stores).
 * Ownership rule: input buffers are only read during the call (the library copies/uploads what it keeps), with one exception: a
 * TGPU_DEVICE block whose arrays all lie inside live buffers of the SAME context (the blocks of a tgpu_output_page, or regions of
 * them) is recognised at ingest and shares those buffers' owners -- an operator that keeps its rows keeps a reference, not a copy,
 * and the memory outlives tgpu_output_page_release for as long as that reference does.  Library buffers are immutable once they
 * have left in an output page: nobody, the caller included, writes them.  Device memory of the embedding or of another context is
 * never recognised and keeps the copy (or, under tgpu_context_set_device_input_stable, the promise below).  A recognised block
 * saves copies only: the operators that defer their launches to a later call (fused aggregation, fused join) do that for pages of
 * TGPU_DEVICE blocks under the promise alone.
 * Output pages are owned by the library until tgpu_output_page_release.
 */
#ifndef TGPU_H
#define TGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: 0 ok, >0 informational, <0 error mirroring io.trino.spi.StandardErrorCode ---- */
#define TGPU_OK 0
#define TGPU_WOULD_BLOCK 1                          /* tgpu_operator_get_output: no page yet and the operator's isBlocked() future is not done */
#define TGPU_ERR_INVALID_ARGUMENT (-1)              /* GENERIC_INTERNAL_ERROR / IllegalArgumentException */
#define TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE (-2)    /* M/type/BigintOperators.java:47-79 */
#define TGPU_ERR_INSUFFICIENT_RESOURCES (-3)        /* GENERIC_INSUFFICIENT_RESOURCES: BigintGroupByHash.java:264-267, PagesIndex.java:234-236 */
#define TGPU_ERR_COMPILER (-4)                      /* COMPILER_ERROR: M/sql/gen/PageFunctionCompiler.java:199-205 */
#define TGPU_ERR_INTERNAL (-5)                      /* GENERIC_INTERNAL_ERROR (illegal operator state etc.) */
#define TGPU_ERR_DEVICE (-6)                        /* no HIP device / HIP runtime failure: the library never falls back to CPU */
#define TGPU_ERR_DIVISION_BY_ZERO (-7)              /* DIVISION_BY_ZERO */
#define TGPU_ERR_NOT_SUPPORTED (-8)                 /* NOT_SUPPORTED */
#define TGPU_ERR_INVALID_CAST_ARGUMENT (-9)         /* INVALID_CAST_ARGUMENT: M/type/DoubleOperators.java:108-163 */

/* ---- types (S/type): storage is what the reference's flat blocks hold ---- */
typedef enum tgpu_type {
    TGPU_BIGINT = 1,   /* int64   LongArrayBlock */
    TGPU_INTEGER = 2,  /* int32   IntArrayBlock */
    TGPU_DATE = 3,     /* int32   IntArrayBlock (days) */
    TGPU_DOUBLE = 4,   /* IEEE double, LongArrayBlock bits */
    TGPU_BOOLEAN = 5,  /* 1 byte  ByteArrayBlock */
    TGPU_VARCHAR = 6,  /* VariableWidthBlock: byte pool + int32 offsets[n+1] */
    /* timestamp(p), 0 <= p <= 6, without time zone: int64 microseconds since 1970-01-01 00:00:00 UTC in a LongArrayBlock
     * (S/type/ShortTimestampType.java:48-75).  The precision is not part of the type code: a timestamp(p) value is a multiple of 10^(6-p) by
     * construction, the library neither checks nor needs that, and the two functions whose result depends on p receive it on their node.
     * BIGINT's twin wherever a value is carried, compared, hashed or ordered: ShortTimestampType.java:128-161 declares EQUAL (left == right),
     * HASH_CODE (AbstractLongType.hash), XX_HASH_64 (XxHash64.hash), COMPARISON (Long.compare), LESS_THAN and LESS_THAN_OR_EQUAL, each with
     * the body AbstractLongType.java:126-166 gives BIGINT (BigintType extends AbstractLongType and declares none of its own); neither declares
     * IS_DISTINCT_FROM, which TypeOperators derives from EQUAL for both.  timestamp(p > 6) (LongTimestampType, a 12-byte Fixed12Block) and
     * timestamp with time zone are not this type. */
    TGPU_TIMESTAMP = 7
} tgpu_type;

typedef enum tgpu_encoding {
    TGPU_FLAT = 0, TGPU_DICTIONARY = 1, TGPU_RLE = 2,
    TGPU_LAZY = 3   /* S/block/LazyBlock.java: not loaded yet; only in pages a tgpu_page_source hands out (loaded through its load_block) */
} tgpu_encoding;
typedef enum tgpu_memory { TGPU_HOST = 0, TGPU_DEVICE = 1 } tgpu_memory;

/* One Block.  All pointers of one block live in the same memory space (`memory`). */
typedef struct tgpu_block {
    int32_t type;            /* tgpu_type */
    int32_t encoding;        /* tgpu_encoding */
    int32_t memory;          /* tgpu_memory */
    int32_t position_count;
    const void *values;      /* FLAT fixed width: position_count elements (arrayOffset already applied); VARCHAR: byte pool */
    const uint8_t *nulls;    /* FLAT: one byte per position (Java boolean[] valueIsNull), NULL = no nulls */
    const int32_t *offsets;  /* FLAT VARCHAR: position_count + 1 */
    const int32_t *ids;      /* DICTIONARY: position_count ids into `dictionary` */
    const struct tgpu_block *dictionary; /* DICTIONARY: the dictionary; RLE: the single-position value block */
} tgpu_block;

typedef struct tgpu_page {
    int32_t position_count;
    int32_t channel_count;
    const tgpu_block *blocks;
} tgpu_page;

typedef struct tgpu_context tgpu_context;
typedef struct tgpu_operator_factory tgpu_operator_factory;
typedef struct tgpu_operator tgpu_operator;
typedef struct tgpu_lookup_source_factory tgpu_lookup_source_factory;
typedef struct tgpu_set_supplier tgpu_set_supplier;            /* SetBuilderOperator.SetSupplier */
typedef struct tgpu_nested_loop_bridge tgpu_nested_loop_bridge; /* NestedLoopJoinBridge / NestedLoopJoinPagesSupplier */
typedef struct tgpu_group_by_hash tgpu_group_by_hash;
typedef struct tgpu_output_page tgpu_output_page;

/* ---- context: one HIP device + one stream; all handles created from it launch on that stream ---- */
int32_t tgpu_context_create(int32_t device, void *hip_stream /* hipStream_t or NULL = null stream */, tgpu_context **out);
void tgpu_context_destroy(tgpu_context *ctx);
int32_t tgpu_context_synchronize(tgpu_context *ctx);
/* last error message of the calling thread (messages mirror the reference's, e.g. "bigint multiplication overflow: 3 * 4") */
const char *tgpu_last_error(void);
const char *tgpu_version(void);
/* directory holding the JIT kernel sources/cache (defaults to the directory of libtgpu.so) */
int32_t tgpu_set_resource_dir(const char *dir);

/* Order in which sum(double) / avg(double) add their rows (DESIGN.md "DOUBLE aggregate policy"), for operators created afterwards:
 *   EXACT (default): few groups -> the correctly rounded exact sum (order independent; equals the Java result whenever that is itself
 *                    exact, else differs from it by the Java order's own rounding error); many groups -> rows added in row order;
 *   JAVA:            always in row order, one group's rows after another -- the loop of DoubleSumAggregation.java:34-38 /
 *                    AccumulatorCompiler.java:487-566, bit-identical to the Java operator for any input, at the price of a
 *                    sequential chain per group (meant for page-sized inputs and strict-parity runs). */
/* Output page size.  The reference's operators cut their output at PageBuilder.isFull (1 MB, S/block/PageBuilderStatus.java:49-60;
 * LookupJoinPageBuilder.java:51-56, OrderByOperator.java:270-296); the GPU operators produce one page per call, which is what downstream
 * GPU operators want.  In front of Java operators set limits: tgpu_operator_get_output then hands a larger page out as consecutive
 * zero-copy regions of at most max_rows rows and about max_bytes bytes (Java block accounting); 0 = no limit (the default). */
int32_t tgpu_context_set_max_output_page(tgpu_context *ctx, int64_t max_bytes, int64_t max_rows);

/* A promise about borrowed TGPU_DEVICE input (hosts that keep their own HBM buffers; library-owned pages and host pages need none): the
 * blocks of a page stay valid and UNCHANGED until the operator they were handed to is finished (tgpu_operator_is_finished) or closed,
 * instead of "until overwritten in stream order".  It lets the operators that keep input BY REFERENCE do so with such pages: the fused
 * aggregation collects small pages for one launch and re-runs a page whose launch met a new group, the fused join keeps two probe pages in
 * flight (DESIGN.md "Page granularity").  Java pages are immutable and referenced by the operator for as long as it needs them
 * (Operator.addInput transfers a reference, SURVEY.md 8b "Ownership"): this is the device-memory counterpart of that rule.  Default off:
 * borrowed device pages then take the synchronous protocol. */
int32_t tgpu_context_set_device_input_stable(tgpu_context *ctx, int32_t stable);

typedef enum tgpu_double_sum_order { TGPU_SUM_ORDER_EXACT = 0, TGPU_SUM_ORDER_JAVA = 1 } tgpu_double_sum_order;
int32_t tgpu_context_set_double_sum_order(tgpu_context *ctx, int32_t order);

/* Pinned (page-locked) host memory for hosts that fill their own receive buffers (an exchange client, a file reader): blocks whose arrays
 * live in such memory are transferred by asynchronous DMA.  Every tgpu_operator_add_input of a host page stages its arrays through a
 * double-buffered ring on a second HIP stream, so the transfer of page i + 1 runs under the kernels of page i (DESIGN.md "Ingest"). */
int32_t tgpu_pinned_alloc(tgpu_context *ctx, int64_t bytes, void **out);
int32_t tgpu_pinned_free(tgpu_context *ctx, void *ptr);

/* per-kernel HIP-event timing on the context's stream (bench.py's roofline leg) */
int32_t tgpu_profile_enable(tgpu_context *ctx, int32_t enabled);
int32_t tgpu_profile_reset(tgpu_context *ctx);
/* writes a JSON object {"kernel": {"count": n, "total_ms": t, "min_ms": a, "max_ms": b}, ...}; returns needed length */
int64_t tgpu_profile_dump(tgpu_context *ctx, char *buf, int64_t buf_len);

/* ---- RowExpression IR (M/sql/relational/{CallExpression,ConstantExpression,InputReferenceExpression,SpecialForm}.java) ---- */
typedef enum tgpu_expr_kind { TGPU_EX_INPUT = 0, TGPU_EX_CONST = 1, TGPU_EX_CALL = 2, TGPU_EX_SPECIAL = 3 } tgpu_expr_kind;
typedef enum tgpu_expr_op {
    TGPU_OP_ADD = 1, TGPU_OP_SUBTRACT, TGPU_OP_MULTIPLY, TGPU_OP_DIVIDE, TGPU_OP_MODULUS, TGPU_OP_NEGATE,
    TGPU_OP_EQUAL, TGPU_OP_NOT_EQUAL, TGPU_OP_LESS_THAN, TGPU_OP_LESS_THAN_OR_EQUAL, TGPU_OP_GREATER_THAN,
    TGPU_OP_GREATER_THAN_OR_EQUAL, TGPU_OP_NOT, TGPU_OP_CAST,
    /* value LIKE pattern [ESCAPE escape] (M/type/LikeFunctions.java:62-118 likeVarchar / likePattern, :198-255 the pattern translation and
     * getEscapeChar).  Result BOOLEAN, n_args 2 or 3: args[0] any VARCHAR expression, args[1] the pattern, args[2] the optional escape.  Pattern and
     * escape must be TGPU_EX_CONST VARCHAR nodes (TGPU_ERR_NOT_SUPPORTED otherwise): the generator reads them, they are never evaluated as
     * values.  '%' matches any run of bytes, '_' exactly one code point, everything else is a literal and the whole value must match.  Without an
     * escape argument nothing escapes; an empty escape disables escaping; one character escapes '%', '_' and itself.  A longer escape fails with
     * "Escape string must be a single character", an escape character followed by anything else (or ending the pattern) with "Escape character
     * must be followed by '%', '_' or the escape character itself": both TGPU_ERR_INVALID_ARGUMENT when the factory is created.  A null value,
     * pattern or escape gives NULL.  LIKE raises no per-row error. */
    TGPU_OP_LIKE = 15,
    /* String functions (M/operator/scalar/StringFunctions.java, ConcatFunction.java) and CAST(... AS VARCHAR).
     *
     * Arguments and nulls.  Every argument is an ordinary expression, not only a constant, and the usual call convention holds: the first null
     * argument gives NULL and the arguments after it are not evaluated.
     *
     * Code-point rule.  A code point starts at every byte b with (b & 0xC0) != 0x80.  LENGTH counts those bytes; SUBSTR counts its positions in
     * them, and its result begins at such a byte and ends in front of one or at the end of the value (bytes in front of the value's first start
     * byte belong to no code point).  On well-formed UTF-8 that is the reference's result.  On malformed bytes the reference's result depends on
     * airlift's SliceUtf8: parity unpinned; the library guarantees the rule above and that no byte outside the value is read.
     *
     *   TGPU_OP_LENGTH       (VARCHAR) -> BIGINT                    length :94-100: the number of code points.
     *   TGPU_OP_SUBSTR       (VARCHAR, BIGINT start [, BIGINT length]) -> VARCHAR     substring :274-309 and :321-367.  start and length are
     *                        saturated to int32 (Ints.saturatedCast).  start == 0, length <= 0 and an empty value each give ''.  start > 0 counts
     *                        from the front (1 = the first code point), a start past the end gives ''.  start < 0 counts from the end (-1 = the
     *                        last code point), a start before the beginning gives ''.  A length that reaches past the end gives the suffix.
     *                        Deviation: the reference's negative-start branch adds two ints (startCodePoint + lengthCodePoints, :359); for
     *                        lengths near 2^31 that add overflows and the reference ends in an internal IndexOutOfBoundsException.  The library
     *                        returns the suffix there.
     *   TGPU_OP_CONCAT       (VARCHAR, VARCHAR) -> VARCHAR          ConcatFunction.java (n-ary there; the builders nest it left to right).  A
     *                        result row longer than 2^31 - 1 bytes fails with TGPU_ERR_INVALID_ARGUMENT, "Concatenated string is too large"
     *                        (the reference's INVALID_FUNCTION_ARGUMENT), at the first such row.
     *   TGPU_OP_STRPOS       (VARCHAR, VARCHAR substring) -> BIGINT stringPosition :205-247, the two-argument form only.  A byte search
     *                        (Slice.indexOf); the result is the 1-based code-point index of the first match, 0 when the substring is absent,
     *                        1 for an empty substring.  The three-argument form (instance) is not part of the IR.
     *   TGPU_OP_STARTS_WITH  (VARCHAR, VARCHAR prefix) -> BOOLEAN   startsWith :909-915: the value's first bytes equal the prefix.
     *
     * TGPU_OP_CAST with a VARCHAR result: from BIGINT and INTEGER the decimal digits of String.valueOf (BigintOperators.java:198-205,
     * IntegerOperators.java:170), from BOOLEAN 'true' / 'false' (BooleanOperators.java:82), from VARCHAR the value itself.  VARCHAR is the
     * unbounded varchar: the IR has no length parameter, so the varchar(x) overflow checks of those casts do not arise.  Casts from DOUBLE and
     * DATE to VARCHAR are not supported (TGPU_ERR_COMPILER).
     *
     * IF and COALESCE accept VARCHAR operands and give a VARCHAR result.
     *
     * Views and built values.  A VARCHAR expression is a view -- (pointer, length) into an input block or a constant: INPUT, CONST, SUBSTR of a
     * view, CAST(boolean), IF / COALESCE over views -- or a built value, a list of up to 32 pieces that exists only while a row is evaluated:
     * CONCAT, CAST(BIGINT / INTEGER AS VARCHAR), IF / COALESCE with a built branch.  Views feed every consumer.  Built values feed a
     * projection root, CONCAT, LENGTH, IF / COALESCE branches and IS_NULL; under a comparison, BETWEEN, LIKE, IN, SUBSTR, STRPOS or
     * STARTS_WITH, and with more than 32 pieces, the factory fails with TGPU_ERR_NOT_SUPPORTED naming the consumer.
     *
     * Computed VARCHAR projections: at most 8 per page processor ("too many computed VARCHAR projections", TGPU_ERR_COMPILER).  An output
     * column of more than 2^31 - 1 bytes fails with TGPU_ERR_INSUFFICIENT_RESOURCES, "variable width block cannot exceed 2GB".
     *
     * Out of scope: lower / upper (Java's case tables), trim / ltrim / rtrim (airlift's whitespace set), replace, reverse, lpad / rpad and
     * CHAR(n). */
    TGPU_OP_LENGTH = 16,
    TGPU_OP_SUBSTR = 17,
    TGPU_OP_CONCAT = 18,
    TGPU_OP_STRPOS = 19,
    TGPU_OP_STARTS_WITH = 20,
    /* DATE functions (M/operator/scalar/DateTimeFunctions.java), over TGPU_DATE = int32 days since 1970-01-01.
     *
     * Calendar.  The proleptic Gregorian (ISO) calendar in UTC with astronomical year numbering -- year 0 exists, negative years are allowed --
     * which is what Joda's ISOChronology.getInstanceUTC() gives.  It holds for every int32 day count: day -2147483648 is -5877641-06-23, a
     * Tuesday, and day 2147483647 is 5881580-07-11, a Friday.  No extraction raises an error.
     *
     *   TGPU_OP_YEAR              (DATE) -> BIGINT   yearFromDate :517-523
     *   TGPU_OP_QUARTER           (DATE) -> BIGINT   quarterFromDate :509-515: (month - 1) / 3 + 1
     *   TGPU_OP_MONTH             (DATE) -> BIGINT   monthFromDate :493-499
     *   TGPU_OP_WEEK              (DATE) -> BIGINT   weekFromDate :477-483: the ISO-8601 week of the week-year.  With thu = days - (day_of_week - 1) + 3,
     *                             the Thursday of the value's week: week = (day_of_year(thu) - 1) / 7 + 1
     *   TGPU_OP_DAY               (DATE) -> BIGINT   dayFromDate :444-450: the day of the month
     *   TGPU_OP_DAY_OF_WEEK       (DATE) -> BIGINT   dayOfWeekFromDate :436-442: floormod(days + 3, 7) + 1, Monday = 1 ... Sunday = 7
     *   TGPU_OP_DAY_OF_YEAR       (DATE) -> BIGINT   dayOfYearFromDate :469-475
     *   TGPU_OP_YEAR_OF_WEEK      (DATE) -> BIGINT   yearOfWeekFromDate :485-491: year(thu)
     *   TGPU_OP_LAST_DAY_OF_MONTH (DATE) -> DATE     lastDayOfMonthFromDate :460-467: same year and month, last day
     *   TGPU_OP_DATE_TRUNC        (VARCHAR unit, DATE) -> DATE                truncateDate :260-268.  day: the value itself; week: the Monday on or
     *                             before it; month, quarter, year: the first day of the period
     *   TGPU_OP_DATE_ADD          (VARCHAR unit, BIGINT value, DATE) -> DATE  addFieldValueDate :270-278.  day: d + v; week: d + 7v; month: the
     *                             (year, month) moves by v months and the day of the month is clamped to the target month's length (Jan 31 + 1
     *                             month = Feb 28 or Feb 29); quarter: 3v months; year: 12v months (Feb 29 + 1 year = Feb 28)
     *   TGPU_OP_DATE_DIFF         (VARCHAR unit, DATE d1, DATE d2) -> BIGINT  diffDate :280-287.  For d2 >= d1 the largest n >= 0 with
     *                             date_add(unit, n, d1) <= d2 (date_add unbounded here); for d2 < d1 it is -date_diff(unit, d2, d1).  day and week
     *                             reduce to (d2 - d1) / {1, 7} truncated toward zero
     *
     * Units.  The unit is 'day', 'week', 'month', 'quarter' or 'year', matched after ASCII lower-casing (getDateField :289-305 uses
     * toLowerCase(ENGLISH)).  It must be a TGPU_EX_CONST VARCHAR node (TGPU_ERR_NOT_SUPPORTED otherwise): the generator reads it, it is never
     * evaluated as a value.  Any other string fails when the factory is created with TGPU_ERR_INVALID_ARGUMENT and the reference's message
     * "'<lower-cased unit>' is not a valid DATE field".  A null unit constant gives NULL for every row and the other arguments are not evaluated:
     * the usual first-null-argument rule, which holds for the other arguments too.  Wrong argument types, result type or argument count:
     * TGPU_ERR_COMPILER.
     *
     * Deviation (int32 DATE).  The reference does toIntExact(value), computes in a long and fails only when a too-large day count is written
     * to an int block (S/type/AbstractIntType.java:85-95).  The library's DATE is int32 everywhere: a row fails with
     * TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE when date_add's value lies outside int32 or when the DATE result of date_add, date_trunc or
     * last_day_of_month lies outside int32 days (date_trunc in the range's first year, whose first days lie before it; last_day_of_month in its last 11 days).  It
     * fails like the checked arithmetic ops do, with the same rule for which error of a page wins.  No intermediate value overflows silently.
     *
     * Deviation (date_diff).  The rule above was compared with a restatement of Joda's getDifferenceAsLong (BasicMonthOfYearDateTimeField,
     * getYearDifference) on 300,000 date pairs biased to month ends and leap days without a mismatch for month, quarter and year, but Joda's
     * source is not part of the reference tree: beyond the reference's test literals Joda parity unpinned; the rule above is what the library
     * guarantees.
     *
     * Out of the IR: CAST between DATE and any other type but TIMESTAMP (TGPU_ERR_COMPILER), the TIME / INTERVAL variants of these functions
     * (the TIMESTAMP variants: below, at TGPU_OP_HOUR),
     * date_format / date_parse / to_iso8601 / current_date and the date + interval operators (a planner folds constant intervals into
     * date_add). */
    TGPU_OP_YEAR = 21,
    TGPU_OP_QUARTER = 22,
    TGPU_OP_MONTH = 23,
    TGPU_OP_WEEK = 24,
    TGPU_OP_DAY = 25,
    TGPU_OP_DAY_OF_WEEK = 26,
    TGPU_OP_DAY_OF_YEAR = 27,
    TGPU_OP_YEAR_OF_WEEK = 28,
    TGPU_OP_LAST_DAY_OF_MONTH = 29,
    TGPU_OP_DATE_TRUNC = 30,
    TGPU_OP_DATE_ADD = 31,
    TGPU_OP_DATE_DIFF = 32,
    /* Math functions (M/operator/scalar/MathFunctions.java) over BIGINT, INTEGER and DOUBLE.  The usual call convention: arguments left to
     * right, the first NULL argument gives NULL and the arguments after it are not evaluated.  A wrong argument count, argument type or
     * result type: TGPU_ERR_COMPILER when the factory is created.
     *
     * Exact group: the result is pinned bit for bit, except that a NaN result may be any NaN (JDK versions differ on the sign and payload
     * Math.abs leaves).
     *
     *   TGPU_OP_ABS       (BIGINT) -> BIGINT, (INTEGER) -> INTEGER, (DOUBLE) -> DOUBLE   :127-148.  The integer minimum fails with
     *                     TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE and the reference's message, "Value -9223372036854775808 is out of range for
     *                     abs(bigint)" / "Value -2147483648 is out of range for abs(integer)".  DOUBLE: the sign bit cleared.
     *   TGPU_OP_SIGN      (BIGINT) -> BIGINT, (INTEGER) -> INTEGER, (DOUBLE) -> DOUBLE   :1085-1125.  -1, 0 or 1; DOUBLE is Math.signum: NaN
     *                     gives NaN, a zero keeps its sign.
     *   TGPU_OP_FLOOR     BIGINT / INTEGER: the identity; (DOUBLE) -> DOUBLE             :390-409, Math.floor
     *   TGPU_OP_CEILING   BIGINT / INTEGER: the identity; (DOUBLE) -> DOUBLE             :245-264, Math.ceil: ceiling(-0.5) is -0.0
     *   TGPU_OP_TRUNCATE  (DOUBLE) -> DOUBLE   :315-320: signum(x) * floor(abs(x)).  -0.5 gives -0.0; NaN and the infinities pass through.
     *   TGPU_OP_ROUND     one argument: BIGINT / INTEGER the identity (:724-735), (DOUBLE) -> DOUBLE = round(x, 0) (:805-808).
     *                     Two arguments: (BIGINT | INTEGER | DOUBLE, INTEGER decimals) -> the first argument's type.  decimals must be a
     *                     TGPU_EX_CONST INTEGER node: TGPU_ERR_NOT_SUPPORTED otherwise, "the number of decimals must be an INTEGER constant".
     *                     A null constant gives NULL for every row and evaluates nothing.
     *                     Integers (roundLong :787-800): d >= 0 is the identity.  -18 <= d < 0: q = num / 10^-d rounded half away from zero
     *                     (RoundingMode.HALF_UP), then q * 10^-d with the overflow checked.  d <= -19 fails for every non-null row:
     *                     checkedPow overflows before num is looked at.  Every failure is TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE,
     *                     "numerical overflow: " + num.  Deviation: INTEGER fails in the same way when the rounded value leaves int32; the
     *                     reference's toIntExact there throws an ArithmeticException that escapes its own catch (:770-776).
     *                     DOUBLE (:821-833): NaN and the infinities as they are.  Otherwise, with factor = 10^d, jround(x * factor) / factor
     *                     for x >= 0 and -(jround(-x * factor) / factor) for x < 0, where jround is Math.round: the exact floor(x + 1/2) as a
     *                     long, saturated at the int64 ends, 0 for NaN, converted back to double before the division.  factor is the
     *                     correctly rounded decimal 1e<d>: equal to Math.pow(10, d) for 0 <= d <= 22, where the power is exact; outside of
     *                     that the correctly rounded power, JVM parity unpinned.  d > 308 (factor +inf) gives +-0.0 and d < -323 (factor 0)
     *                     gives NaN for every finite x: what the formula gives.
     *   TGPU_OP_SQRT      (DOUBLE) -> DOUBLE   :1141: the correctly rounded IEEE square root.  Negative gives NaN, -0.0 gives -0.0.
     *   TGPU_OP_IS_NAN, TGPU_OP_IS_FINITE, TGPU_OP_IS_INFINITE   (DOUBLE) -> BOOLEAN   :1165-1184
     *   TGPU_OP_DEGREES, TGPU_OP_RADIANS   (DOUBLE) -> DOUBLE   :350, :569: one multiplication by 57.29577951308232, resp.
     *                     0.017453292519943295.  That is Math.toDegrees / toRadians since JDK 9 (JDK 8 multiplied by 180 and divided by pi);
     *                     the reference needs Java 11.
     *
     * Bounded group: (DOUBLE) -> DOUBLE, never fails.  The JVM promises "within 1 ulp of the exact result" for these, so there is no bit
     * parity to keep: a finite result lies within 1 ulp of the correctly rounded one for CBRT, EXP, LN, LOG10 and POWER, and within the
     * interval bound of the quotient (tests/golden/math_function_ulp_corpus.json "bounds") for LOG2 and LOG.
     *
     *   TGPU_OP_CBRT :221, TGPU_OP_EXP :366, TGPU_OP_LN :465, TGPU_OP_LOG10 :489   Math.cbrt / exp / log / log10
     *   TGPU_OP_LOG2      :481: ln(x) / ln(2)
     *   TGPU_OP_LOG       (DOUBLE base, DOUBLE x) -> DOUBLE   :473: ln(x) / ln(base), the base first
     *   TGPU_OP_POWER     (DOUBLE x, DOUBLE y) -> DOUBLE      :561, Math.pow
     *
     * Special cases are Java's: a negative argument of a logarithm gives NaN, ln(+-0) is -inf, exp overflows to +inf.  POWER follows
     * Math.pow's list, which differs from C's pow twice: pow(1, NaN) is NaN and pow(+-1, +-inf) is NaN; pow(x, +-0) is 1 even for a NaN x.
     * Where the mathematical value of x ^ y for an integral y with |y| <= 1024 is a double (power(2, 10), power(10, 22), power(-3, 3)), the
     * result is that value.
     *
     * Out of the IR: the trigonometric and hyperbolic functions, width_bucket, random, to_base / from_base, the CDF functions,
     * cosine_similarity, greatest / least, the bitwise functions, the TINYINT / SMALLINT / REAL / DECIMAL flavours and a decimals argument
     * that is no constant.  mod(a, b) is TGPU_OP_MODULUS. */
    TGPU_OP_ABS = 33,
    TGPU_OP_SIGN = 34,
    TGPU_OP_FLOOR = 35,
    TGPU_OP_CEILING = 36,
    TGPU_OP_TRUNCATE = 37,
    TGPU_OP_ROUND = 38,
    TGPU_OP_SQRT = 39,
    TGPU_OP_CBRT = 40,
    TGPU_OP_EXP = 41,
    TGPU_OP_LN = 42,
    TGPU_OP_LOG2 = 43,
    TGPU_OP_LOG10 = 44,
    TGPU_OP_LOG = 45,
    TGPU_OP_POWER = 46,
    TGPU_OP_IS_NAN = 47,
    TGPU_OP_IS_FINITE = 48,
    TGPU_OP_IS_INFINITE = 49,
    TGPU_OP_DEGREES = 50,
    TGPU_OP_RADIANS = 51,
    /* TIMESTAMP functions (M/operator/scalar/timestamp/), over TGPU_TIMESTAMP = int64 microseconds since 1970-01-01 00:00:00 UTC, precision
     * p <= 6.  INPUT and CONST nodes of type TIMESTAMP carry microseconds (CONST: ival).  The six comparisons, BETWEEN, IN, IS_NULL, IF and
     * COALESCE take TIMESTAMP exactly as they take BIGINT.
     *
     * Throughout: ms = floordiv(us, 1000) (DateTimes.scaleEpochMicrosToMillis), day = floordiv(ms, 86 400 000), tod = ms - day * 86 400 000.
     * day always fits int32 (|day| <= 106 751 992); the calendar is the DATE functions' (csrc/device_date.h), the arithmetic around it is
     * csrc/device_timestamp.h.
     *
     *   TGPU_OP_YEAR .. TGPU_OP_YEAR_OF_WEEK  (TIMESTAMP) -> BIGINT   the DATE function of `day` (ExtractYear.java etc.: the Joda field of
     *                             scaleEpochMicrosToMillis)
     *   TGPU_OP_LAST_DAY_OF_MONTH (TIMESTAMP) -> DATE       the DATE function of `day` (LastDayOfMonth.java); cannot leave int32 here
     *   TGPU_OP_HOUR, TGPU_OP_MINUTE, TGPU_OP_SECOND, TGPU_OP_MILLISECOND   (TIMESTAMP) -> BIGINT   tod / 3 600 000, tod / 60 000 % 60,
     *                             tod / 1000 % 60, tod % 1000 (ExtractHour.java ...)
     *   TGPU_OP_TO_UNIXTIME       (TIMESTAMP) -> DOUBLE     (double) us / 1000000.0: one int64 -> double conversion and one IEEE division,
     *                             bit for bit (ToUnixTime.java)
     *   TGPU_OP_DATE_TRUNC        (VARCHAR unit, TIMESTAMP) -> TIMESTAMP   DateTrunc.java: ms floored to the unit (week: Monday 00:00), then
     *                             x 1000; the sub-millisecond part is dropped
     *   TGPU_OP_DATE_ADD          (VARCHAR unit, BIGINT value, TIMESTAMP) -> TIMESTAMP   DateAdd.java:41-57.  The node's ival is the argument's
     *                             precision p (0..6).  value must fit int32 (toIntExact).  The precise units add value * unit_ms to ms; month /
     *                             quarter / year move the (year, month) of `day` with the day of the month clamped and keep tod.  For p <= 3
     *                             the millisecond result is rounded with DateTimes.round(ms, 3 - p).  Result ms' * 1000 + floormod(us, 1000)
     *   TGPU_OP_DATE_DIFF         (VARCHAR unit, TIMESTAMP t1, TIMESTAMP t2) -> BIGINT   DateDiff.java, on ms1 and ms2.  Precise units:
     *                             (ms2 - ms1) / unit_ms truncated toward zero.  month: for t2 >= t1 the largest n >= 0 with
     *                             add_months(ms1, n) <= ms2, else the negated count the other way; quarter = months / 3, year = months / 12
     *   TGPU_OP_CAST              (DATE) -> TIMESTAMP       TimeUnit.DAYS.toMicros (DateToTimestampCast.java), which SATURATES at the int64 ends
     *                             for days beyond +-106 751 991.  No error
     *                             (TIMESTAMP) -> DATE       floordiv(us, 86 400 000 000) (TimestampToDateCast.java)
     *                             (TIMESTAMP) -> TIMESTAMP  the node's ival is the target precision q (0..6): roundDiv(us, 10^(6-q)) * 10^(6-q)
     *                             with roundDiv as M/type/DateTimes.java:104-117 writes it -- (v + f/2) / f for v >= 0, (v + 1 - f/2) / f for v < 0,
     *                             Java's truncating division: to the nearest, a positive tie up and a negative tie toward zero -- in 64-bit
     *                             two's-complement arithmetic, wraparound included.  q = 6 is the identity
     *
     * Units.  'millisecond', 'second', 'minute', 'hour', 'day', 'week', 'month', 'quarter' or 'year' (getTimestampField,
     * DateTimeFunctions.java:323-347), a TGPU_EX_CONST VARCHAR node matched after ASCII lower-casing; TGPU_ERR_NOT_SUPPORTED when it is no
     * constant.  Any other string fails when the factory is created with TGPU_ERR_INVALID_ARGUMENT and the reference's message
     * "'<lower-cased unit>' is not a valid Timestamp field".  Nulls: the usual first-null-argument rule, the unit included.
     *
     * Errors.  A row fails with TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE when date_add's value lies outside int32 or when a date_trunc / date_add
     * result is not an int64 count of microseconds (where the reference's toIntExact / multiplyExact throw; the library also fails where the
     * reference's last addition of the microseconds of the millisecond would wrap).  The rule for which error of a page wins is the checked
     * arithmetic's.  No intermediate value overflows silently; the months index is kept in 64 bits.  Wrong argument types, counts, result
     * types or a precision outside 0..6: TGPU_ERR_COMPILER.
     *
     * date_diff in months, quarters and years: as for DATE, Joda's source is not part of the reference tree; beyond the reference's test
     * literals Joda parity is unpinned and the rule above is what the library guarantees.
     *
     * Out of the IR: CAST between TIMESTAMP and VARCHAR (and any type but DATE), date_format / date_parse / to_iso8601, from_unixtime (its
     * result carries a zone), the timestamp +- interval operators, TIME, timestamp(p > 6) and timestamp with time zone. */
    TGPU_OP_HOUR = 52,
    TGPU_OP_MINUTE = 53,
    TGPU_OP_SECOND = 54,
    TGPU_OP_MILLISECOND = 55,
    TGPU_OP_TO_UNIXTIME = 56
} tgpu_expr_op;
typedef enum tgpu_special_form { /* M/sql/relational/SpecialForm.java:137-152 */
    TGPU_SF_AND = 1, TGPU_SF_OR, TGPU_SF_IF, TGPU_SF_IS_NULL, TGPU_SF_COALESCE, TGPU_SF_BETWEEN,
    /* value IN (item, ...) (M/sql/gen/InCodeGenerator.java:92-121; equality is the type's EQUAL operator).  Result BOOLEAN, n_args = 1: args[0]
     * is the value, of any of the six types.  The list is `slen` consecutive nodes starting at node index `ival` (fields that are otherwise
     * read on CONST nodes only: every walker over args[0 .. n_args) stays correct, list items reference no channel).  Each item is a
     * TGPU_EX_CONST of the value's type; a null item is allowed.  slen < 1, a range outside the node array, a non-constant item or an item of
     * another type: TGPU_ERR_INVALID_ARGUMENT; more than 65,536 items: TGPU_ERR_NOT_SUPPORTED.  A null value gives NULL; otherwise TRUE when
     * a non-null item equals the value; otherwise NULL when the list holds a null item, else FALSE.  DOUBLE compares with == (NaN matches
     * nothing, -0.0 matches +0.0), VARCHAR by bytes. */
    TGPU_SF_IN = 7
} tgpu_special_form;

typedef struct tgpu_expr_node {
    int32_t kind;      /* tgpu_expr_kind */
    int32_t type;      /* result tgpu_type */
    int32_t op;        /* CALL: tgpu_expr_op; SPECIAL: tgpu_special_form; INPUT: channel */
    int32_t n_args;
    int32_t args[3];   /* indices into the node array */
    int32_t is_null;   /* CONST: null literal */
    int64_t ival;      /* CONST BIGINT/INTEGER/DATE/BOOLEAN/TIMESTAMP value; VARCHAR: offset into string_pool; DATE_ADD / CAST over TIMESTAMP: precision */
    double dval;       /* CONST DOUBLE */
    int32_t slen;      /* CONST VARCHAR length */
    int32_t pad;
} tgpu_expr_node;

/* A page processor = optional filter + projections over one shared node array (ExpressionCompiler.compilePageProcessor) */
typedef struct tgpu_page_processor_spec {
    const tgpu_expr_node *nodes;
    int32_t node_count;
    const char *string_pool;
    int32_t string_pool_len;
    int32_t filter_root;            /* -1 = no filter */
    int32_t projection_count;
    const int32_t *projection_roots;
} tgpu_page_processor_spec;

/* ---- operator factories ---- */
/* FilterAndProjectOperator.createOperatorFactory (M/operator/FilterAndProjectOperator.java:73-88).  The expressions are
 * compiled to one fused gfx950 kernel (the GPU counterpart of M/sql/gen/PageFunctionCompiler.java). */
int32_t tgpu_filter_project_factory_create(tgpu_context *ctx, int32_t operator_id,
                                           int32_t input_type_count, const int32_t *input_types,
                                           const tgpu_page_processor_spec *spec,
                                           tgpu_operator_factory **out);

typedef enum tgpu_agg_function {
    TGPU_AGG_COUNT_ALL = 1,     /* count(*)        M/operator/aggregation/CountAggregation.java:34-56 */
    TGPU_AGG_COUNT_COLUMN = 2,  /* count(col)      CountColumn.java */
    TGPU_AGG_SUM_BIGINT = 3,    /* sum(bigint)     LongSumAggregation.java:34-63 */
    TGPU_AGG_SUM_DOUBLE = 4,    /* sum(double)     DoubleSumAggregation.java:34-63 */
    TGPU_AGG_AVG_BIGINT = 5,    /* avg(bigint)     AverageAggregations.java:35-80 */
    TGPU_AGG_AVG_DOUBLE = 6,    /* avg(double)     AverageAggregations.java:42-80 */
    TGPU_AGG_MIN_BIGINT = 7,    /* min(bigint)     AbstractMinMaxAggregationFunction.java:233-289 (LONG_INPUT / LONG_COMBINE, NullableLongState) */
    TGPU_AGG_MAX_BIGINT = 8,    /* max(bigint)     the same with the comparison turned round (MaxAggregationFunction.java) */
    TGPU_AGG_MIN_DOUBLE = 9,    /* min(double)     :227-230,291-306 with Double.compare (DoubleType.java:194-198): -0.0 < +0.0, NaN above +inf */
    TGPU_AGG_MAX_DOUBLE = 10,   /* max(double)     M/util/MinMaxCompare.java maxDouble: value > state || isNaN(state).  A NaN result is the canonical NaN; among
                                 *                 zeros of both signs as the maximum +0.0 is returned (the reference: the one that came first) */
    /* IntegerType and DateType are long.class types, so AbstractMinMaxAggregationFunction.java:118-128,160-190 picks NullableLongState and the
     * LONG_INPUT / LONG_COMBINE methods for them as for BIGINT: signed 32-bit order, the intermediate value is BIGINT.  Hash aggregation (spilled
     * or not), the fused filter/project aggregation and the streaming aggregation take them; window aggregates do not. */
    TGPU_AGG_MIN_INTEGER = 11,  /* min(integer)    one INTEGER channel; output INTEGER */
    TGPU_AGG_MAX_INTEGER = 12,  /* max(integer) */
    TGPU_AGG_MIN_DATE = 13,     /* min(date)       one DATE channel (days since the epoch, int32); output DATE */
    TGPU_AGG_MAX_DATE = 14,     /* max(date) */
    /* VARCHAR is a Slice type: the state is the BlockPositionState of :118-128,160-190, whose input / combine keep the position the
     * comparison prefers (:245,269,325) -- Slice.compareTo: unsigned bytes left to right, a proper prefix sorts first; '' is a value, not
     * NULL; equal strings are byte-identical, so which one is kept cannot be observed.  Plain hash aggregation only (grouped or global,
     * SINGLE / PARTIAL / FINAL, masks): tgpu_hash_aggregation_factory_set_spill_enabled(1) fails with TGPU_ERR_NOT_SUPPORTED, "min / max
     * over VARCHAR cannot spill" (the factory stays usable unspilled), and the fused and the streaming aggregation factories fail with
     * TGPU_ERR_NOT_SUPPORTED at creation.  A result channel of more than 2^31 - 1 bytes fails with TGPU_ERR_INSUFFICIENT_RESOURCES,
     * "variable width block cannot exceed 2GB". */
    TGPU_AGG_MIN_VARCHAR = 15,  /* min(varchar)    one VARCHAR channel; output VARCHAR */
    TGPU_AGG_MAX_VARCHAR = 16,  /* max(varchar) */
    /* ShortTimestampType is a long.class type as well: NullableLongState and LONG_INPUT / LONG_COMBINE over the int64 microseconds, which is
     * min / max(bigint) on the same values (nothing is narrowed).  PARTIAL gives min(bigint)'s layout (count BIGINT, extreme BIGINT), SINGLE /
     * FINAL one TIMESTAMP channel.  Hash aggregation (spilled or not), the fused filter / project aggregation and the streaming aggregation
     * take them; window aggregates do not.  sum / avg over a TIMESTAMP channel: TGPU_ERR_INVALID_ARGUMENT like any wrong input type. */
    TGPU_AGG_MIN_TIMESTAMP = 17, /* min(timestamp(p)), p <= 6   one TIMESTAMP channel; output TIMESTAMP */
    TGPU_AGG_MAX_TIMESTAMP = 18  /* max(timestamp(p)) */
} tgpu_agg_function;

typedef struct tgpu_agg_spec {
    int32_t function;       /* tgpu_agg_function */
    int32_t input_channel;  /* -1 for count(*) */
    int32_t mask_channel;   /* BOOLEAN channel or -1 (AccumulatorCompiler.java:487-566 mask handling) */
} tgpu_agg_spec;

typedef enum tgpu_agg_step { TGPU_STEP_SINGLE = 0, TGPU_STEP_PARTIAL = 1, TGPU_STEP_FINAL = 2 } tgpu_agg_step;

/* HashAggregationOperatorFactory (M/operator/HashAggregationOperator.java:54-262).  Output channels: group-by keys,
 * [hash channel if hash_channel >= 0], then one channel per aggregate (PARTIAL: two channels per sum / avg / min / max = count BIGINT,
 * sum DOUBLE|BIGINT or the extreme BIGINT -- the flattened LongDoubleState / LongLongState / NullableLongState, count 0 = null state;
 * FINAL consumes that layout).  min / max over INTEGER and DATE: SINGLE / FINAL give one channel of the input's own type (int32
 * storage), NULL for a group without an unmasked non-null row; PARTIAL gives count BIGINT, extreme BIGINT (the sign-extended value, 0
 * where the count is 0) -- min(bigint)'s layout, the reference's intermediate type is BIGINT too -- and FINAL narrows it again.
 * min / max over VARCHAR: SINGLE / FINAL give one VARCHAR channel, NULL for a group without an unmasked non-null row; PARTIAL gives
 * count BIGINT, value VARCHAR, the cell NULL and empty where the count is 0; FINAL ignores the value cell of a row whose count is 0,
 * whatever its null flag, and adds the counts.  A raw input channel of another type than the function's fails the first add_input with
 * TGPU_ERR_INVALID_ARGUMENT. */
int32_t tgpu_hash_aggregation_factory_create(tgpu_context *ctx, int32_t operator_id,
                                             int32_t group_by_count, const int32_t *group_by_types, const int32_t *group_by_channels,
                                             int32_t hash_channel /* -1 = none */, int32_t step,
                                             int32_t agg_count, const tgpu_agg_spec *aggs,
                                             int32_t expected_groups, int32_t produce_default_output,
                                             tgpu_operator_factory **out);

/* StreamingAggregationOperator.createOperatorFactory (M/operator/StreamingAggregationOperator.java:50-69; process / processInput :216-347):
 * the aggregation the planner chooses when its input is already grouped on the keys (M/sql/planner/LocalExecutionPlanner.java:3022-3031).
 * `types` are the source types; the group-by types are those of `group_by_channels`.
 *   Groups        a group is a maximal run of consecutive rows of the stream whose key rows are NOT DISTINCT from each other
 *                 (rowNotDistinctFromRow: null equals null, any NaN equals any NaN, -0.0 equals +0.0, VARCHAR by bytes), across any
 *                 number of pages.  No order among the groups is needed or checked; a key that comes back later is a new group.
 *   Output        channels: the group-by keys, then the aggregates in the layouts of tgpu_hash_aggregation_factory_create (SINGLE /
 *                 PARTIAL / FINAL); no hash channel.  One row per group, in stream order.  A group leaves with the add_input whose
 *                 page holds the first row of the NEXT group, the last one with finish.
 *   Key cells     those of the row the reference reads (:283-305,317-324), bit for bit (NaN payload, sign of zero): a group that ends
 *                 inside page P takes the first row of its segment in P -- row 0 of P when it began on an earlier page; a group whose
 *                 last row is the last row of P (flushed by the next page's first row or by finish) takes that last row of P.
 *   Sums          DOUBLE sums and averages are the sequential additions of the group's rows in row order (the Java loop), always:
 *                 tgpu_context_set_double_sum_order does not apply.  FINAL combines its intermediate rows in row order, too.
 *                 sum(bigint): 128-bit accumulation, the total decides, as on the hash aggregation's paths.  An overflow fails the call
 *                 that completes the group -- that add_input, or finish for the last group -- with TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE;
 *                 no row of that page is emitted, pages handed out earlier stay valid.
 *   Protocol      needs_input until finish, except while an output page waits to be fetched (:237-242); a page without rows is a
 *                 no-op; no input, no output; is_finished once finish was called and the output is drained.
 *   memory_bytes  the accumulator states of one page's groups, the carried key row and the pending output page: independent of the
 *                 length of the stream.
 * group_by_count == 0 is TGPU_ERR_INVALID_ARGUMENT (the planner streams only on non-empty pre-grouped keys; the global aggregation stays
 * with the hash operator); more than 16 aggregates, unknown functions, channels out of range: TGPU_ERR_INVALID_ARGUMENT. */
int32_t tgpu_streaming_aggregation_factory_create(tgpu_context *ctx, int32_t operator_id,
                                                  int32_t type_count, const int32_t *types,
                                                  int32_t group_by_count, const int32_t *group_by_channels, int32_t step,
                                                  int32_t agg_count, const tgpu_agg_spec *aggs,
                                                  tgpu_operator_factory **out);

/* HashBuilderOperatorFactory + its JoinBridge (M/operator/HashBuilderOperator.java:54-152;
 * PartitionedLookupSourceFactory.java:110-124 with one partition per GPU). */
int32_t tgpu_hash_builder_factory_create(tgpu_context *ctx, int32_t operator_id,
                                         int32_t type_count, const int32_t *types,
                                         int32_t output_channel_count, const int32_t *output_channels,
                                         int32_t hash_channel_count, const int32_t *hash_channels /* join key channels */,
                                         int32_t precomputed_hash_channel /* -1 = none */, int32_t expected_positions,
                                         tgpu_lookup_source_factory **bridge_out, tgpu_operator_factory **out);
/* The build side as `partition_count` HashBuilderOperators (PartitionedLookupSourceFactory.java:110-124: one per build driver; each receives
 * the rows a LocalExchange with the LocalPartitionGenerator function -- TGPU_PARTITION_LOCAL below -- routes to its partition).
 * tgpu_operator_factory_create_operator may then be called partition_count times; the probes stay blocked until every build operator has
 * finished (lendPartitionLookupSource).  The partitions are concatenated in partition order into ONE table in HBM (the reference keeps P
 * tables to parallelise a CPU build); results equal PartitionedLookupSource's (PartitionedLookupSource.java:87-153): a key's matches
 * newest -> oldest within its partition, unmatched outer rows partition by partition (:233-262).  partition_count: a power of two. */
int32_t tgpu_partitioned_hash_builder_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                                     int32_t output_channel_count, const int32_t *output_channels, int32_t hash_channel_count,
                                                     const int32_t *hash_channels, int32_t precomputed_hash_channel, int32_t expected_positions,
                                                     int32_t partition_count, tgpu_lookup_source_factory **bridge_out, tgpu_operator_factory **out);
/* PartitionedLookupSource's join-position encoding (PartitionedLookupSource.java:212-226): (joinPosition << shiftSize) | partition with
 * shiftSize = numberOfTrailingZeros(partitionCount) + 1; for shims that must hand such positions to Java code.  encode returns
 * TGPU_ERR_INVALID_ARGUMENT (negative, never a position) unless partition_count is a power of two, 0 <= partition < partition_count and
 * join_position >= 0 */
int64_t tgpu_partitioned_join_position_encode(int32_t partition, int32_t join_position, int32_t partition_count);
int32_t tgpu_partitioned_join_position_decode(int64_t partitioned_join_position, int32_t partition_count, int32_t *partition, int32_t *join_position);
void tgpu_lookup_source_factory_destroy(tgpu_lookup_source_factory *bridge);
/* JoinFilterFunction (M/operator/JoinHash.java:44-47,82-130; M/sql/gen/JoinFilterFunctionCompiler.java; handed to the build side like
 * JoinHashSupplier.java:54-70): a predicate over (build row, probe row) that a join position must pass besides key equality.  `spec`'s
 * filter expression is that predicate (its projections are ignored); its input channels [0, build type count) are the build side's
 * channels (the hash builder's `types`), channel build-type-count + k is probe channel k.  A key's chain is walked newest -> oldest and
 * rejected positions are skipped; a PROBE_OUTER / FULL_OUTER row all of whose candidates are rejected comes out with a null build side.
 * Call before the probe operators are created. */
int32_t tgpu_lookup_source_factory_set_join_filter(tgpu_lookup_source_factory *bridge, int32_t probe_type_count, const int32_t *probe_types,
                                                   const tgpu_page_processor_spec *spec);
/* statistics of the built table (valid once the build operator finished): positions, table slots, position links */
int32_t tgpu_lookup_source_stats(tgpu_lookup_source_factory *bridge, int64_t *positions, int64_t *hash_size, int64_t *link_count);

/* LookupJoinOperators.JoinType ordinals (M/operator/LookupJoinOperators.java:30-36).  LOOKUP_OUTER / FULL_OUTER probes also record the
 * build positions they matched; the unmatched build rows come out of the LookupOuterOperator (tgpu_lookup_outer_factory_create) */
typedef enum tgpu_join_type { TGPU_JOIN_INNER = 0, TGPU_JOIN_PROBE_OUTER = 1, TGPU_JOIN_LOOKUP_OUTER = 2, TGPU_JOIN_FULL_OUTER = 3 } tgpu_join_type;

/* LookupJoinOperators.innerJoin / probeOuterJoin (M/operator/LookupJoinOperators.java:30-63).  Output page = probe output
 * channels then the build side's output channels (M/operator/LookupJoinPageBuilder.java:101-131). */
int32_t tgpu_lookup_join_factory_create(tgpu_context *ctx, int32_t operator_id, tgpu_lookup_source_factory *bridge,
                                        int32_t probe_type_count, const int32_t *probe_types,
                                        int32_t probe_join_channel_count, const int32_t *probe_join_channels,
                                        int32_t probe_hash_channel /* -1 = none */,
                                        int32_t probe_output_channel_count, const int32_t *probe_output_channels,
                                        int32_t join_type, tgpu_operator_factory **out);

/* Operator fusion by codegen: FilterAndProjectOperator feeding LookupJoinOperator compiled into one kernel (what
 * LocalExecutionPlanner.visitJoin would construct when the probe source is a filter/project node, M/sql/planner/
 * LocalExecutionPlanner.java:1742,2284-2311).  Behaves exactly like the two reference operators back to back:
 * `spec`'s projections form the probe page, and probe_join_channels / probe_hash_channel / probe_output_channels index
 * those projections.  Configurations the fused kernel does not cover run the two steps unfused inside the operator.
 * Pages the operator may keep (library-owned pages, host pages, borrowed device pages under tgpu_context_set_device_input_stable) of up to
 * 2^25 rows are probed asynchronously: pages below 2^22 rows are collected until 2^24 rows or 64 pages share one launch (one output page,
 * rows in input order), and two launches are kept in flight.  tgpu_operator_get_output returns no page for an input page until that has
 * happened, tgpu_operator_finish was called or get_output is polled twice without input in between (Operator.getOutput may return null,
 * M/operator/Operator.java:53-79); an expression error of such a page is returned by the call that completes its launch. */
int32_t tgpu_filter_project_lookup_join_factory_create(tgpu_context *ctx, int32_t operator_id, tgpu_lookup_source_factory *bridge,
                                                       int32_t input_type_count, const int32_t *input_types,
                                                       const tgpu_page_processor_spec *spec,
                                                       int32_t probe_join_channel_count, const int32_t *probe_join_channels,
                                                       int32_t probe_hash_channel /* -1 = none */,
                                                       int32_t probe_output_channel_count, const int32_t *probe_output_channels,
                                                       int32_t join_type, tgpu_operator_factory **out);

/* LookupOuterOperator.LookupOuterOperatorFactory (M/operator/LookupOuterOperator.java:35-110; created by LookupJoinOperatorFactory for
 * LOOKUP_OUTER / FULL_OUTER joins, LookupJoinOperatorFactory.java:88-103): a source operator that, once every probe operator of the join
 * has finished (is_blocked until then), emits the build rows no probe matched, in build-position order: `probe_output_types` channels of
 * nulls followed by the build output channels. */
int32_t tgpu_lookup_outer_factory_create(tgpu_context *ctx, int32_t operator_id, tgpu_lookup_source_factory *bridge, int32_t probe_output_type_count,
                                         const int32_t *probe_output_types, tgpu_operator_factory **out);

/* ---- semi join (LocalExecutionPlanner.visitSemiJoin, M/sql/planner/LocalExecutionPlanner.java:2326-2412): x IN (SELECT ...) ---- */
/* SetBuilderOperatorFactory (M/operator/SetBuilderOperator.java:92-135) + its SetSupplier (:39-90): a sink on the build pipeline that
 * collects channel `set_channel` of every page into a set in HBM (ChannelSet.java:62-108: null keys are inserted too; containsNull = a null
 * key was seen) and publishes it to every probe operator at finish().  hash_channel (-1 = none) is accepted and not read: the set hashes
 * its keys itself.  expected_positions is a sizing hint only.  The factory cannot be duplicated (TGPU_ERR_NOT_SUPPORTED). */
int32_t tgpu_set_builder_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                        int32_t set_channel, int32_t hash_channel /* -1 = none */, int32_t expected_positions,
                                        tgpu_set_supplier **supplier_out, tgpu_operator_factory **out);
/* HashSemiJoinOperator.HashSemiJoinOperatorFactory (M/operator/HashSemiJoinOperator.java:44-118, :166-218): output page = the input
 * page's channels unchanged (a probe hash channel included), then one BOOLEAN channel; one output page per input page, rows in input
 * order.  Per row: null probe key -> false if the set is empty, else null; key in the set -> true; else null if the set contains a null,
 * else false.  Membership is GroupByHash.contains (ChannelSet.java:70-78): DOUBLE NaN / -0.0 as the group-by hash, VARCHAR bytewise.
 * The probe key type must be the set's type (TGPU_ERR_INVALID_ARGUMENT otherwise).  Like the LookupJoinOperator: is_blocked = 1 and
 * needs_input = 0 until the set builder has finished; a probe finished before that ends without output.  duplicate() shares the set. */
int32_t tgpu_hash_semi_join_factory_create(tgpu_context *ctx, int32_t operator_id, tgpu_set_supplier *supplier,
                                           int32_t probe_type_count, const int32_t *probe_types, int32_t probe_join_channel,
                                           int32_t probe_hash_channel /* -1 = none */, tgpu_operator_factory **out);
/* valid once the builder finished: distinct keys (a null counts, as in ChannelSet.size), containsNull, HBM bytes, layout (0 bitmap,
 * 1 hash, 2 generic) */
int32_t tgpu_set_supplier_stats(tgpu_set_supplier *supplier, int64_t *size, int32_t *contains_null, int64_t *bytes, int32_t *layout);
void tgpu_set_supplier_destroy(tgpu_set_supplier *supplier);

/* ---- nested loop join (LocalExecutionPlanner.visitJoin for a node without equi-criteria: cross join, scalar subquery comparison, band and
 * inequality joins; M/operator/NestedLoopBuildOperator.java, NestedLoopJoinPagesBuilder.java, NestedLoopJoinOperator.java).  INNER only,
 * as in the reference.
 *
 * The sequence every operator below produces: one probe page (p rows) against each build page (b rows) in turn, in build order.  The
 * LARGE side of such a pair is the build page iff b > p (a tie makes the probe page large; with an empty probe channel list and a non-empty
 * build channel list a tie makes the build page large, NestedLoopJoinOperator.java:265-267).  The reference emits one page per row of the
 * small side, in row order, each holding every row of the large side in order with the small row repeated; channels = probe_channels then
 * build_channels.  The device operators produce THE ROWS OF THOSE PAGES IN THAT ORDER and cut the sequence into output pages of their
 * own size.  Without any output channel only position counts come out and only their sum is defined. ---- */
/* NestedLoopBuildOperatorFactory (NestedLoopBuildOperator.java:33-94) + the bridge to the probes (NestedLoopJoinPagesSupplier).  A sink:
 * get_output is always null.  The pages are kept in HBM as delivered -- page boundaries decide which side of a pair is large -- except
 * that empty pages are dropped and, when type_count = 0, pages are only counted and re-cut into pages of 8192 positions plus a remainder
 * (NestedLoopJoinPagesBuilder.java:64-76,100-105).  memory_bytes = the retained size.  finish() publishes the pages; a second build
 * operator finishing on the same bridge fails with TGPU_ERR_INTERNAL "pagesFuture already set".  After finish() the operator is blocked,
 * and not finished, until every probe operator of the bridge has closed and every probe factory has had no_more_operators (as the hash
 * builder).  The factory cannot be duplicated (TGPU_ERR_NOT_SUPPORTED). */
int32_t tgpu_nested_loop_build_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                              tgpu_nested_loop_bridge **bridge_out, tgpu_operator_factory **out);
/* valid once the build operator finished: kept pages (after the re-cut), their positions, their bytes in HBM */
int32_t tgpu_nested_loop_bridge_stats(tgpu_nested_loop_bridge *bridge, int64_t *pages, int64_t *positions, int64_t *bytes);
void tgpu_nested_loop_bridge_destroy(tgpu_nested_loop_bridge *bridge);
/* NestedLoopJoinOperatorFactory (NestedLoopJoinOperator.java:44-108).  is_blocked = 1 and needs_input = 0 until the build operator has
 * finished; needs_input = 0 while a probe page still has output to give; an empty probe page, or an empty build side, produces nothing;
 * finish() with output still to give keeps is_finished = 0 until it has been drained; close() at any time is clean; duplicate() shares the
 * bridge.  Every get_output returns the next piece of the sequence: at most max_output_rows rows (0 = the default: 4,194,304 rows; 2^31 - 1
 * when both channel lists are empty), and fewer where a VARCHAR channel's pool would otherwise reach 2^31 bytes.  A probe page's product may
 * exceed 2^31 rows: it comes out piece by piece.  Channels may repeat and come in any order. */
int32_t tgpu_nested_loop_join_factory_create(tgpu_context *ctx, int32_t operator_id, tgpu_nested_loop_bridge *bridge,
                                             int32_t probe_type_count, const int32_t *probe_types,
                                             int32_t probe_channel_count, const int32_t *probe_channels,
                                             int32_t build_channel_count, const int32_t *build_channels,
                                             int64_t max_output_rows /* 0 = default */, tgpu_operator_factory **out);
/* NestedLoopJoin(all probe channels, all build channels) feeding FilterAndProjectOperator(spec), as one operator.  Input channel
 * k < probe_type_count of `spec` is probe channel k, channel probe_type_count + j is build channel j: PROBE FIRST, the order of the join's
 * output page -- NOT the build-first order of tgpu_lookup_source_factory_set_join_filter.  Output = the filtered and projected sequence.  At
 * most max_product_rows pairs (0 = the default: 67,108,864) are evaluated per get_output; a step without survivors returns null and the
 * operator goes on.  A filter over BIGINT / INTEGER / DATE / DOUBLE / BOOLEAN values that cannot raise is evaluated over the virtual
 * product, only the surviving pairs are written; any other spec (no filter, a filter that can raise, VARCHAR in the filter) runs as product
 * pieces of the channels it reads followed by the page processor -- same output.  The operator fails with the error the reference
 * composition throws first: the first reference page that fails, within it the filter before projection 0 before projection 1 ..., then
 * the first row (found by re-running the failing piece one reference page at a time). */
int32_t tgpu_filter_project_nested_loop_join_factory_create(tgpu_context *ctx, int32_t operator_id, tgpu_nested_loop_bridge *bridge,
                                                            int32_t probe_type_count, const int32_t *probe_types,
                                                            const tgpu_page_processor_spec *spec,
                                                            int64_t max_product_rows /* 0 = default */, tgpu_operator_factory **out);

/* ---- count(DISTINCT x) and SELECT DISTINCT ... LIMIT n (LocalExecutionPlanner.visitMarkDistinct / visitDistinctLimit) ---- */
/* MarkDistinctOperator.MarkDistinctOperatorFactory (M/operator/MarkDistinctOperator.java:39-92, :94-203; MarkDistinctHash.java:52-69): output
 * page = the input page's channels unchanged, then one BOOLEAN channel without nulls that is true on the first row of every value of the
 * mark channels the operator has not seen before (a null key is a value like any other); one output page per input page.  The marker is
 * what tgpu_agg_spec.mask_channel reads for count(DISTINCT x).  mark_channels: non-empty, any order, at most 8, each in [0, type_count);
 * hash_channel: -1 or a BIGINT channel holding the precomputed raw hash of the mark channels.  TGPU_ERR_INVALID_ARGUMENT otherwise.
 * One GroupByHash per operator (expected size 10 000, MarkDistinctHash.java:39); memory_bytes = its estimated size. */
int32_t tgpu_mark_distinct_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                          int32_t mark_channel_count, const int32_t *mark_channels, int32_t hash_channel /* -1 = none */,
                                          tgpu_operator_factory **out);
/* DistinctLimitOperator.DistinctLimitOperatorFactory (M/operator/DistinctLimitOperator.java:42-99, :101-263): output page = the distinct
 * channels in the given order, then the hash channel if there is one (:125-128), flat; it holds the rows of the input page that start
 * a new value of the distinct channels, in row order, cut at the remaining limit (:189-202).  No output page for an input page that
 * contributes no row.  needs_input = not finishing, limit not reached, no page pending; is_finished = no page pending and (finishing
 * or limit reached): with limit 0 at once.  Arguments as tgpu_mark_distinct_factory_create; limit < 0 is TGPU_ERR_INVALID_ARGUMENT (:70). */
int32_t tgpu_distinct_limit_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                           int32_t distinct_channel_count, const int32_t *distinct_channels, int64_t limit,
                                           int32_t hash_channel /* -1 = none */, tgpu_operator_factory **out);

/* ---- row_number() OVER (PARTITION BY k) [<= n] and LIMIT n (LocalExecutionPlanner.visitRowNumber / visitLimit) ---- */
/* RowNumberOperator.RowNumberOperatorFactory (M/operator/RowNumberOperator.java:43-119, :121-364): output page = the output channels in
 * the given order, then one BIGINT channel without nulls: the row's number inside its partition (the rows that agree on the partition
 * channels; a null key is a value like any other), counted from 1 in arrival order across all pages.  Always output_channel_count + 1
 * channels.  max_rows_per_partition = -1: one output page per input page, every row.  >= 0: only the rows whose number is <= the limit,
 * in row order; no output page for an input page that keeps no row; 0 is legal and keeps nothing.  partition_channel_count = 0: one
 * partition; with a limit the operator is finished (and needs no input) once it has numbered `limit` rows.  A partitioned operator
 * never finishes early.  One page at a time: needs_input is false while a page's output is pending.  The partition types are taken
 * from `types`; at most 8 partition channels.  hash_channel: -1 or a BIGINT channel holding the precomputed raw hash of the partition
 * channels.  max_rows_per_partition < -1 or > 2^31 - 1 (the reference's limit is a Java int), expected_positions <= 0, a channel out of range or a hash channel without partition channels:
 * TGPU_ERR_INVALID_ARGUMENT.  memory_bytes = the hash's estimated size + the per-partition counts (:266). */
int32_t tgpu_row_number_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                       int32_t output_channel_count, const int32_t *output_channels, int32_t partition_channel_count,
                                       const int32_t *partition_channels, int64_t max_rows_per_partition /* -1 = none */,
                                       int32_t hash_channel /* -1 = none */, int32_t expected_positions, tgpu_operator_factory **out);
/* LimitOperator.LimitOperatorFactory (M/operator/LimitOperator.java:27-60, :62-119): whole pages pass through untouched while they fit
 * into the remaining limit, the page that crosses it is cut to a region of its first rows, finish() zeroes the remainder.
 * needs_input = remaining > 0 and no page pending; is_finished = remaining == 0 and no page pending: with limit 0 at once.
 * limit < 0 is TGPU_ERR_INVALID_ARGUMENT (:70). */
int32_t tgpu_limit_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types, int64_t limit,
                                  tgpu_operator_factory **out);

/* ---- row_number() / rank() OVER (PARTITION BY k ORDER BY x) <= n (LocalExecutionPlanner.visitTopNRanking) ---- */
/* TopNRankingOperator.TopNRankingOperatorFactory (M/operator/TopNRankingOperator.java:42-156, :170-310; GroupedTopNRowNumberBuilder.java:99-188,
 * GroupedTopNRankBuilder.java; row order = SimplePageWithPositionComparator.java:58-79, sort_orders as for tgpu_top_n_factory_create): the
 * operator consumes pages until finish() (needs_input = not finishing) and then hands out ONE page, none for empty input: the output
 * channels in the given order, then -- unless `partial` (generateRanking = !partial, :99) -- one BIGINT channel without nulls, the ranking.
 * Partitions (the rows that agree on the partition channels; a null key is a value like any other; no partition channel = one partition,
 * no hash) come out in the order of their keys' first arrival, the rows of a partition in the order of the sort channels, rows that
 * compare equal in arrival order across all pages.  TGPU_RANKING_ROW_NUMBER keeps the first max_rank_per_partition rows of every
 * partition in that order, numbered from 1.  TGPU_RANKING_RANK keeps every row whose rank (1 + the rows of its partition that sort
 * strictly before it) is <= max_rank_per_partition: ties at the boundary are all kept, peers (rows the comparator calls equal: null =
 * null, NaN = NaN, -0.0 before +0.0) carry the same rank.  TGPU_RANKING_DENSE_RANK (UnsupportedOperationException, :235-236), an unknown
 * ranking type, max_rank_per_partition <= 0 or > 2^31 - 1 (a Java int, :96), expected_positions <= 0 (:98), no sort channel or more
 * than 8, more than 8 partition channels, a channel or sort order out of range, a hash channel that is not BIGINT or comes without
 * partition channels: TGPU_ERR_INVALID_ARGUMENT.  memory_bytes = the hash's estimated size + the candidate rows held (within a
 * constant factor of partitions x max_rank_per_partition, plus one page), their group ids and one cutoff per partition. */
typedef enum tgpu_ranking_type { TGPU_RANKING_ROW_NUMBER = 0, TGPU_RANKING_RANK = 1, TGPU_RANKING_DENSE_RANK = 2 } tgpu_ranking_type;
int32_t tgpu_top_n_ranking_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t ranking_type,
                                          int32_t type_count, const int32_t *types,
                                          int32_t output_channel_count, const int32_t *output_channels,
                                          int32_t partition_channel_count, const int32_t *partition_channels,
                                          int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                          int64_t max_rank_per_partition, int32_t partial,
                                          int32_t hash_channel /* -1 = none */, int32_t expected_positions, tgpu_operator_factory **out);

/* ---- window functions: f(..) OVER (PARTITION BY k ORDER BY x <frame>) (LocalExecutionPlanner.visitWindow) ---- */
/* WindowOperator.WindowOperatorFactory (M/operator/WindowOperator.java:205-310; the row loop of M/operator/window/WindowPartition.java:184-214).
 * The operator consumes pages until finish() (needs_input = not finishing) and then hands out ONE page, none for empty input: the output
 * channels in the given order, then one channel per window function in the given order.
 * ROW ORDER.  With at least one partition or sort channel the rows come out in PagesIndex.sort order (sortPagesIndexIfNecessary, :844-855): sort keys
 * = the partition channels, each ASC_NULLS_LAST, then the sort channels with their sort orders (:254); rows that compare equal on all of them keep
 * their arrival order across pages (the reference's quicksort leaves it open; OrderBy, TopN and TopNRanking fix it the same way here).  With neither,
 * nothing is sorted: the input is one partition in arrival order and every row is a peer of every other.  Partition + sort channels: at most 8.
 * PARTITIONS AND PEERS are maximal runs of ADJACENT rows of that order that are NOT DISTINCT on the partition channels / on the sort channels
 * (updatePeerGroup, WindowPartition.java:238-247; PagesIndex.positionNotDistinctFromPosition): null = null, NaN = NaN and -0.0 = +0.0, although
 * the sort puts -0.0 first -- not the comparator's "== 0" that tgpu_top_n_ranking_factory_create uses.  A partition head is also a peer head.
 * FRAMES (WindowPartition.java:281-345), the three that need no offset (frames with offsets: tgpu_window_factory_create_framed below); the frame of every one of them starts at the partition's first row:
 *   TGPU_FRAME_PARTITION          UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING (RANGE or ROWS): ends at the partition's last row (default without ORDER BY)
 *   TGPU_FRAME_RANGE_TO_CURRENT   RANGE UNBOUNDED PRECEDING .. CURRENT ROW: ends at the last peer of the current row (default with ORDER BY)
 *   TGPU_FRAME_ROWS_TO_CURRENT    ROWS UNBOUNDED PRECEDING .. CURRENT ROW: ends at the current row
 * FUNCTIONS (the classes of M/operator/window).  The ranking functions and lag / lead ignore the frame.
 *   ROW_NUMBER, RANK, DENSE_RANK  BIGINT, never null (RowNumberFunction, RankFunction, DenseRankFunction); no argument
 *   PERCENT_RANK                  DOUBLE: 0.0 in a partition of one row, else (double) (rank - 1) / (partition rows - 1) (PercentRankFunction.java)
 *   CUME_DIST                     DOUBLE: (double) (rows up to the current row's last peer) / (partition rows) (CumulativeDistributionFunction.java)
 *   LAG, LEAD                     1 to 3 argument channels: the value (any type), a BIGINT offset, a default of the value's type (LagFunction.java,
 *                                 LeadFunction.java).  A null offset gives null; no offset channel means 1; p = current -/+ offset in Java long
 *                                 arithmetic, in partition-relative positions; lag takes the value at p if 0 <= p <= current, lead if 0 <= p <
 *                                 partition rows; otherwise the default channel's cell of the CURRENT row, or null.  A negative offset fails
 *                                 get_output with TGPU_ERR_INVALID_ARGUMENT, "Offset must be at least 0".
 *   FIRST_VALUE, LAST_VALUE       one value channel of any type: the cell at the frame's first / last row (FirstValueFunction.java, LastValueFunction.java)
 *   AGGREGATE                     agg_function over the frame (AggregateWindowFunction.java): COUNT_ALL (no argument), COUNT_COLUMN (one channel of any
 *                                 type), SUM_BIGINT / MIN_BIGINT / MAX_BIGINT (one BIGINT channel), MIN_DOUBLE / MAX_DOUBLE (one DOUBLE channel); values
 *                                 as tgpu_agg_function documents them.  Counts are never null; sum / min / max are null while the frame holds no
 *                                 non-null input.  sum(bigint): the reference adds the partition's non-null values left to right with addExact over a
 *                                 frame that only ever grows, so get_output fails with TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE, "bigint addition overflow",
 *                                 exactly when some prefix of a partition's non-null values in sorted order leaves the int64 range.
 * TGPU_ERR_NOT_SUPPORTED: ignore_nulls != 0; SUM_DOUBLE / AVG_* (the reference accumulates them in a double left to right: a parallel scan cannot
 * give its bits).  TGPU_ERR_INVALID_ARGUMENT: an unknown function, frame or aggregate, a wrong argument count or type, a default whose type differs
 * from the value's, a channel or sort order out of range, more than 8 key channels, no function or more than 16, expected_positions <= 0.
 * preGroupedChannels / preSortedChannelPrefix are not part of the signature.  memory_bytes = the pages index, and once get_output ran
 * the positions and scan arrays it took. */
typedef enum tgpu_window_function {
    TGPU_WINDOW_ROW_NUMBER = 0, TGPU_WINDOW_RANK = 1, TGPU_WINDOW_DENSE_RANK = 2, TGPU_WINDOW_PERCENT_RANK = 3, TGPU_WINDOW_CUME_DIST = 4,
    TGPU_WINDOW_LAG = 5, TGPU_WINDOW_LEAD = 6, TGPU_WINDOW_FIRST_VALUE = 7, TGPU_WINDOW_LAST_VALUE = 8, TGPU_WINDOW_AGGREGATE = 9,
    TGPU_WINDOW_NTH_VALUE = 10, TGPU_WINDOW_NTILE = 11   /* tgpu_window_factory_create_framed only */
} tgpu_window_function;
typedef enum tgpu_window_frame { TGPU_FRAME_PARTITION = 0, TGPU_FRAME_RANGE_TO_CURRENT = 1, TGPU_FRAME_ROWS_TO_CURRENT = 2 } tgpu_window_frame;
#define TGPU_WINDOW_MAX_FUNCTIONS 16
typedef struct tgpu_window_function_spec {
    int32_t function;              /* tgpu_window_function */
    int32_t agg_function;          /* tgpu_agg_function, read for TGPU_WINDOW_AGGREGATE only */
    int32_t frame;                 /* tgpu_window_frame */
    int32_t argument_count;        /* 0 .. 3 */
    int32_t argument_channels[3];
    int32_t ignore_nulls;          /* must be 0 */
} tgpu_window_function_spec;
int32_t tgpu_window_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                   int32_t output_channel_count, const int32_t *output_channels,
                                   int32_t function_count, const tgpu_window_function_spec *functions,
                                   int32_t partition_channel_count, const int32_t *partition_channels,
                                   int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                   int32_t expected_positions, tgpu_operator_factory **out);

/* The same operator with the frames of M/operator/window/FrameInfo.java: ROWS / GROUPS with k PRECEDING / k FOLLOWING bounds, and the functions
 * nth_value and ntile.  The arguments are those of tgpu_window_factory_create plus frames[function_count] behind `functions`; the `frame` field
 * of a function spec is NOT read, frames[f] is function f's frame.  tgpu_window_factory_create is this entry point with TGPU_FRAME_PARTITION =
 * RANGE UNBOUNDED_PRECEDING .. UNBOUNDED_FOLLOWING, TGPU_FRAME_RANGE_TO_CURRENT = RANGE UNBOUNDED_PRECEDING .. CURRENT_ROW, TGPU_FRAME_ROWS_TO_CURRENT =
 * ROWS UNBOUNDED_PRECEDING .. CURRENT_ROW, and those three frames given here take the same path and give the same page, errors included.
 * BOUNDS.  start is UNBOUNDED_PRECEDING, PRECEDING, CURRENT_ROW or FOLLOWING; end is PRECEDING, CURRENT_ROW, FOLLOWING or UNBOUNDED_FOLLOWING; a CURRENT_ROW
 * start does not end PRECEDING, a FOLLOWING start ends FOLLOWING or UNBOUNDED_FOLLOWING (the analyzer's rules); anything else is
 * TGPU_ERR_INVALID_ARGUMENT.  start_channel / end_channel are read for a PRECEDING / FOLLOWING bound only: a BIGINT or INTEGER source channel whose cell
 * in the CURRENT row is the offset (getFrameValue, WindowPartition.java:591-607).  A null offset in any row fails get_output with
 * TGPU_ERR_INVALID_ARGUMENT, "Window frame starting offset must not be null" / "Window frame ending offset must not be null", a negative one with
 * "Window frame offset must not be negative" (the value is left out of the message), before any other error of the page.
 * FRAMES, with r = the row's position in its partition, E = the partition's last position, G = the row's peer group in its partition, L = the last:
 *   ROWS    WindowPartition.java:281-323.  a PRECEDING = max(r - a, 0), a FOLLOWING = min(r + a, E), for every int64 a >= 0.  Empty (:541-573) for
 *           UNBOUNDED_PRECEDING .. b PRECEDING with b > r; a FOLLOWING .. UNBOUNDED_FOLLOWING with a > E - r; both PRECEDING with a < b, or a > r and
 *           b > r; both FOLLOWING with a > b or a > E - r.
 *   GROUPS  :609-694.  start: the first row of group G - a (the partition's first row below group 0) / of group G + a (behind the partition above
 *           L) / of G; end: the last row of group G - b (-1 below group 0) / of G + b (E above L) / of G.  Empty when start > end, start > E or
 *           end < 0.  An offset of 2^31 or more is "beyond every group" (the reference's toIntExact throws there).
 *   RANGE   by peers only (:327-344): the four combinations of UNBOUNDED_PRECEDING / CURRENT_ROW with CURRENT_ROW / UNBOUNDED_FOLLOWING.  RANGE with a
 *           PRECEDING / FOLLOWING bound is TGPU_ERR_NOT_SUPPORTED: it needs the planner's computed comparison channels and a value search.
 * FUNCTIONS under a frame [s, e].  The ranking functions, lag, lead and ntile ignore it.
 *   FIRST_VALUE, LAST_VALUE   the cell at s / at e; null for an empty frame
 *   NTH_VALUE                 two channels, the value (any type) and a BIGINT offset (NthValueFunction.java:41-77): null for an empty frame or a null
 *                             offset, else the cell at s + offset - 1 if that is <= e, else null; an offset < 1 in a row with a frame fails get_output
 *                             with TGPU_ERR_INVALID_ARGUMENT, "Offset must be at least 1"
 *   NTILE                     one BIGINT channel, the buckets (NTileFunction.java:45-74): BIGINT; null for null buckets; buckets <= 0 fail with
 *                             TGPU_ERR_INVALID_ARGUMENT, "Buckets must be greater than 0"; else the bucket number from 1, the partition's remainder
 *                             rows going to the first buckets one each; more buckets than rows: the row's position + 1
 *   AGGREGATE                 the seven aggregates of tgpu_window_factory_create.  Counts over an empty frame are 0; sum / min / max are null over an
 *                             empty frame or one without a non-null input.  sum(bigint) is the exact sum of the frame; get_output fails with
 *                             TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE, "bigint addition overflow", exactly when some row's frame sum leaves int64 (a
 *                             partition prefix may).  The reference slides one accumulator from frame to frame with addExact / subtractExact and can
 *                             also throw on an intermediate that depends on the path between two frames: not reproduced.
 * TGPU_ERR_NOT_SUPPORTED as before: ignore_nulls != 0 (nth_value too), SUM_DOUBLE / AVG_*.  memory_bytes also counts the frame arrays and the
 * range-extreme index of min / max. */
typedef enum tgpu_frame_type { TGPU_FRAME_TYPE_RANGE = 0, TGPU_FRAME_TYPE_ROWS = 1, TGPU_FRAME_TYPE_GROUPS = 2 } tgpu_frame_type;   /* sql/tree/WindowFrame.Type ordinals */
typedef enum tgpu_frame_bound {
    TGPU_BOUND_UNBOUNDED_PRECEDING = 0, TGPU_BOUND_PRECEDING = 1, TGPU_BOUND_CURRENT_ROW = 2, TGPU_BOUND_FOLLOWING = 3, TGPU_BOUND_UNBOUNDED_FOLLOWING = 4
} tgpu_frame_bound;                                                                                                                  /* sql/tree/FrameBound.Type ordinals */
typedef struct tgpu_window_frame_spec { int32_t type, start_type, start_channel, end_type, end_channel; } tgpu_window_frame_spec;   /* M/operator/window/FrameInfo.java */
int32_t tgpu_window_factory_create_framed(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                          int32_t output_channel_count, const int32_t *output_channels,
                                          int32_t function_count, const tgpu_window_function_spec *functions, const tgpu_window_frame_spec *frames,
                                          int32_t partition_channel_count, const int32_t *partition_channels,
                                          int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                          int32_t expected_positions, tgpu_operator_factory **out);

/* The same operator with RANGE BETWEEN x PRECEDING / FOLLOWING AND y PRECEDING / FOLLOWING as well: "the rows whose sort key lies within x of mine"
 * (getFrameRange / seek, M/operator/window/WindowPartition.java:325-521; FrameInfo.java; WindowOperator.createFrameBoundComparators :420-443).  The
 * arguments are those of tgpu_window_factory_create_framed with frames of tgpu_window_range_frame_spec.  A frame of any other kind -- ROWS, GROUPS,
 * RANGE by peers -- behaves exactly as through tgpu_window_factory_create_framed, errors included; the two sort key fields are not read for it.
 * RANGE with a PRECEDING / FOLLOWING bound.  The operator has exactly ONE sort channel.  start_channel / end_channel do not hold an offset: they hold
 * the bound VALUE per row, sort key - / + offset, computed in front of the operator (ASC: PRECEDING = key - offset, FOLLOWING = key + offset; DESC the
 * other way round; the offset is checked there to be non-negative and not null).  start_sort_key_channel / end_sort_key_channel hold the sort key
 * coerced to the bound's type (FrameInfo.sortKeyChannelForStartComparison / ...EndComparison; the sort channel itself where no coercion is needed).
 * Bound and comparison key are of one type, BIGINT, INTEGER, DATE or DOUBLE, compared with the type's comparison operator (DOUBLE: -0.0 < +0.0, NaN
 * above +inf, as the sort has it).  TGPU_ERR_INVALID_ARGUMENT when the factory is created: not exactly one sort channel, a channel out of range, a
 * bound and its comparison key of different types, another type.  The analyzer's bound combinations are checked as before.
 * THE FRAME.  [lo, hi] = the partition's run of rows with a non-null sort key, K = the comparison key in sorted order, B = the current row's bound,
 * "K[p] <~ B" = K[p] <= B under ASC and K[p] >= B under DESC.
 *   a row whose sort key is null       its peer group (the partition's nulls), from the partition's first row for an UNBOUNDED_PRECEDING start and to
 *                                      its last row for an UNBOUNDED_FOLLOWING end.  Its bounds are never read.
 *   a row whose sort key is not null   start with a value: the first p in [lo, hi] with B <~ K[p], else hi + 1.  end with a value: the last p in [lo, hi]
 *                                      with K[p] <~ B, else lo - 1.  CURRENT_ROW: the peer group's first / last row.  UNBOUNDED_*: the partition's
 *                                      first / last row.  Nulls enter such a frame through UNBOUNDED_* only -- and as hi + 1 / lo - 1 where that is
 *                                      the block of nulls (1 FOLLOWING .. UNBOUNDED_FOLLOWING with nulls last: the largest key's frame is the nulls).
 *   empty                              start > end, start behind the partition, end in front of it (emptyFrame, :523-528)
 * These are the reference's frames whenever the bounds are what a planner produces (key -/+ a non-negative finite offset, without overflow).  For any
 * other bound (inf - inf, a bound on the wrong side of the row's key) the reference's walk leaves the partition; the library gives the closed form
 * above and reads nothing outside the partition.  A comparison key that is NOT monotone in the sort key gives an unspecified frame inside the
 * partition (the search bisects).
 * get_output fails with TGPU_ERR_INVALID_ARGUMENT, before any other error of the page: "Window frame starting offset must not be null" / "Window frame
 * ending offset must not be null" for a null bound in a row whose sort key is not null; "Window frame comparison key must not be null where the sort
 * key is not null" for a null comparison key in such a row.  memory_bytes also counts the search arrays: 8 bytes per row and distinct comparison key
 * channel, and one byte per row. */
typedef struct tgpu_window_range_frame_spec {
    int32_t type, start_type, start_channel, end_type, end_channel;
    int32_t start_sort_key_channel, end_sort_key_channel;   /* FrameInfo.sortKeyChannelForStartComparison / sortKeyChannelForEndComparison */
} tgpu_window_range_frame_spec;
int32_t tgpu_window_factory_create_ranged(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                          int32_t output_channel_count, const int32_t *output_channels,
                                          int32_t function_count, const tgpu_window_function_spec *functions, const tgpu_window_range_frame_spec *frames,
                                          int32_t partition_channel_count, const int32_t *partition_channels,
                                          int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                          int32_t expected_positions, tgpu_operator_factory **out);

/* FilterAndProjectOperator feeding HashAggregationOperator as one fused pipeline (what LocalExecutionPlanner.visitAggregation,
 * M/sql/planner/LocalExecutionPlanner.java:1198,2965-3056, would construct over a filter/project source; the shape of
 * testing/trino-benchmark HandTpchQuery1.java:60-133).  Same results as the two reference operators back to back.  `spec`'s
 * projections form the aggregation's input page: group_by_channels, hash_channel and the aggregates' input / mask channels
 * index those projections.  step is SINGLE or PARTIAL. */
int32_t tgpu_filter_project_hash_aggregation_factory_create(tgpu_context *ctx, int32_t operator_id,
                                                            int32_t input_type_count, const int32_t *input_types,
                                                            const tgpu_page_processor_spec *spec,
                                                            int32_t group_by_count, const int32_t *group_by_types, const int32_t *group_by_channels,
                                                            int32_t hash_channel /* -1 = none */, int32_t step,
                                                            int32_t agg_count, const tgpu_agg_spec *aggs,
                                                            int32_t expected_groups, tgpu_operator_factory **out);

/* TopNOperator.createOperatorFactory (M/operator/TopNOperator.java:47-62; TopNProcessor.java:45-66): the n first rows of the input
 * in the order of the sort channels (S/connector/SortOrder.java:18-21; row order = SimplePageWithPositionComparator.java:58-79:
 * nulls placed by the sort order, values by the type's COMPARISON operator, negated for DESC).  Rows that compare equal on every
 * sort channel come out in input order (the reference's heap leaves their order unspecified).  n == 0: no output, finished at
 * once (TopNOperator.java:154-156). */
typedef enum tgpu_sort_order {
    TGPU_SORT_ASC_NULLS_FIRST = 0, TGPU_SORT_ASC_NULLS_LAST = 1, TGPU_SORT_DESC_NULLS_FIRST = 2, TGPU_SORT_DESC_NULLS_LAST = 3
} tgpu_sort_order;
int32_t tgpu_top_n_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types, int64_t n,
                                  int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                  tgpu_operator_factory **out);

/* OrderByOperator.OrderByOperatorFactory (M/operator/OrderByOperator.java:48-131): every input row, in the order of the sort channels
 * (PagesIndex.sort, M/operator/PagesIndex.java:386-394, with the same row order as TopN above); output_channels selects the channels
 * of the output page.  Rows that compare equal come out in input order (the reference's quicksort leaves their order unspecified).
 * The sorted rows are emitted as one page (the reference cuts them into <= 1 MB pages, :270-296). */
int32_t tgpu_order_by_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                     int32_t output_channel_count, const int32_t *output_channels, int32_t expected_positions,
                                     int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                     tgpu_operator_factory **out);

/* ---- ScanFilterAndProjectOperator (M/operator/ScanFilterAndProjectOperator.java:66-447): a SOURCE operator that pulls pages from the split's
 * ConnectorPageSource (S/connector/ConnectorPageSource.java; here callbacks) and runs the page processor over them ---- */
typedef struct tgpu_page_source {
    void *user;
    /* ConnectorPageSource.getNextPage: 1 = *page filled (its arrays stay valid until the next call on this source), 0 = no page right now, < 0 error.
     * Channels may be TGPU_LAZY blocks (only type and position_count set). */
    int32_t (*get_next_page)(void *user, tgpu_page *page);
    int32_t (*is_finished)(void *user);                                        /* ConnectorPageSource.isFinished */
    int32_t (*is_blocked)(void *user);                                         /* isBlocked() future not done; NULL = never blocked */
    /* LazyBlock.getLoadedBlock for channel `channel` of the page get_next_page returned last: fills *block with a FLAT / DICTIONARY / RLE block.
     * Called at most once per channel and page, only for channels the filter reads and -- when the filter selected at least one row -- the
     * channels the projections read (PageProcessor.java:111-137; T/operator/project/TestPageProcessor.java:156-184,219-253). */
    int32_t (*load_block)(void *user, int32_t channel, tgpu_block *block);
    void (*close)(void *user);                                                 /* ConnectorPageSource.close; NULL = nothing to do */
} tgpu_page_source;
/* ScanFilterAndProjectOperatorFactory (:449-560) over the page-source flavour (processPageSource :275-287); `types` = the channels the
 * page source produces.  The operator takes no input: tgpu_operator_add_input fails. */
int32_t tgpu_scan_filter_project_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                                const tgpu_page_processor_spec *spec, tgpu_operator_factory **out);
/* SourceOperator.addSplit (:232-263: the split's page source; one at a time, the next one after the current is finished) / noMoreSplits */
int32_t tgpu_scan_operator_add_page_source(tgpu_operator *op, const tgpu_page_source *source);
int32_t tgpu_scan_operator_no_more_splits(tgpu_operator *op);
/* The record-cursor flavour (processColumnSource / RecordCursorToPages, :267-273,290-351; S/connector/RecordCursor.java): the split's source
 * is a row cursor.  The reference runs a compiled CursorProcessor over it row by row into a PageBuilder; here the rows are read through the
 * callbacks into host columns, up to 65 536 rows at a time (what RecordPageSource does, S/connector/RecordPageSource.java:70-135), and take
 * the page path from there -- the same rows in the same order, cut into other pages (page cuts are not part of the contract).  `types` =
 * the cursor's fields: BIGINT / INTEGER / DATE fields are read with get_long, DOUBLE with get_double, BOOLEAN with get_boolean, VARCHAR
 * with get_slice (bytes valid until the next advance).  close may be NULL. */
typedef struct tgpu_record_cursor {
    void *user;
    int32_t (*advance_next_position)(void *user);      /* RecordCursor.advanceNextPosition: 1 = positioned on a row, 0 = no more rows, < 0 error */
    int32_t (*is_null)(void *user, int32_t field);
    int32_t (*get_boolean)(void *user, int32_t field);
    int64_t (*get_long)(void *user, int32_t field);
    double (*get_double)(void *user, int32_t field);
    int32_t (*get_slice)(void *user, int32_t field, const void **bytes, int32_t *length);   /* 0 = ok, < 0 error */
    int64_t (*completed_bytes)(void *user);            /* RecordCursor.getCompletedBytes; NULL = not tracked */
    void (*close)(void *user);
} tgpu_record_cursor;
int32_t tgpu_scan_operator_add_record_cursor(tgpu_operator *op, const tgpu_record_cursor *cursor, int32_t type_count, const int32_t *types);
/* OperatorStats the scan side feeds (:354-397): positions pulled from the page sources, lazy blocks loaded / skipped */
int32_t tgpu_scan_operator_stats(tgpu_operator *op, int64_t *processed_positions, int64_t *lazy_blocks_loaded, int64_t *lazy_blocks_skipped);

/* ---- MergeOperator (M/operator/MergeOperator.java:44-256; the same routine behind LocalMergeSourceOperator, M/operator/exchange/
 * LocalMergeSourceOperator.java:39-): a SOURCE operator that merges k sorted page streams into one sorted stream, MergeSortedPages
 * (M/util/MergeSortedPages.java:41-142, WorkProcessorUtils.java:110-152).  `types` = the channels of every stream's pages,
 * output_channels the channels of the output page, sort channels / orders as for TopN above.  A stream is a tgpu_page_source
 * (tgpu_merge_operator_add_page_source = addSplit :155-177; load_block is never called: TGPU_LAZY blocks are refused); its pages
 * may be host or device memory, FLAT / DICTIONARY / RLE.  The source's arrays are valid until the next call on that source: a
 * pulled page is ingested (host), copied or owner-shared (device) at once.
 *   Source operator  needs_input is 0; tgpu_operator_add_input fails with TGPU_ERR_NOT_SUPPORTED (:222-231).
 *   Blocked          is_blocked is 1 until no_more_splits (blockedOnSplits, :208-219).  Afterwards it is 1 while some stream has no
 *                    buffered row, is not finished and its get_next_page last returned 0.  Like the reference, which blocks on its
 *                    sources one after the other, the operator waits on the FIRST such stream in split order: where that source has
 *                    an is_blocked callback the operator is unblocked as soon as the callback returns 0 (the next get_output pulls
 *                    again); without a callback it stays blocked until the next get_output has pulled.  get_output returns a NULL
 *                    page with TGPU_WOULD_BLOCK while the operator is blocked.
 *   Splits           add_page_source after no_more_splits fails ("noMoreSplits has been called already", :159).  No split at all
 *                    followed by no_more_splits: a finished operator without output.
 *   finish           is close (:196-199): the operator is finished at once and emits nothing further.
 *   close callbacks  every source's close is called exactly once: when its stream ends, or when the operator closes or finishes.
 *   Pulling          get_output pulls from every unfinished stream that holds fewer than half an internal read-ahead of rows, until
 *                    the source returns 0, is finished or the read-ahead is reached.  A negative return of get_next_page fails the
 *                    call with that value as its error code.  A page whose channel count or types differ from `types`:
 *                    TGPU_ERR_INVALID_ARGUMENT.  After such a failure the operator is still usable: the pages pulled before the
 *                    failing one stay buffered, only the failing page is lost, and the next get_output pulls again.
 *   Rounds           one get_output runs at most one round and returns at most one page (cut by tgpu_context_set_max_output_page as
 *                    for every operator; page cuts are not part of the contract).  Let B be the smallest (last buffered row, stream
 *                    index) over the unfinished streams -- rows compare with the comparator, then by stream index -- and t_B its
 *                    stream.  A buffered row (r, s) is SETTLED when (r, s) <= (B, t_B); with every stream finished every buffered
 *                    row is.  A round emits exactly the settled rows, merged.  With a stream that is unfinished and empty there is
 *                    no round (blocked, or the source yielded).
 *   Order            SimplePageWithPositionComparator (as TopN above).  Rows that compare equal come out lower stream first (in
 *                    add_page_source order) and, inside a stream, in arrival order; the reference's binary heap leaves the order of
 *                    cross-stream ties unspecified.
 *   Unsorted input   is not detected (neither does the reference).  Which row comes out where is then unspecified -- a row may come out
 *                    twice and another not at all; the row count is kept -- and nothing else is: no kernel reads outside its buffers
 *                    or loops without bound.
 *   Limits           more than 2^31 - 1 settled rows: the round is cut and the rest comes out of the next.  A VARCHAR output
 *                    channel over 2 GB fails with "variable width block cannot exceed 2GB".
 *   memory_bytes     the streams' buffered input rows (no page is ever pending: a round's page leaves with the get_output that built
 *                    it); 0 once the operator is finished. */
int32_t tgpu_merge_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types,
                                  int32_t output_channel_count, const int32_t *output_channels,
                                  int32_t sort_channel_count, const int32_t *sort_channels, const int32_t *sort_orders,
                                  tgpu_operator_factory **out);
int32_t tgpu_merge_operator_add_page_source(tgpu_operator *op, const tgpu_page_source *source);   /* addSplit: one sorted stream */
int32_t tgpu_merge_operator_no_more_splits(tgpu_operator *op);

/* OperatorFactory.createOperator / noMoreOperators (M/operator/OperatorFactory.java:18-50) */
int32_t tgpu_operator_factory_create_operator(tgpu_operator_factory *factory, tgpu_operator **out);
int32_t tgpu_operator_factory_no_more_operators(tgpu_operator_factory *factory);
/* OperatorFactory.duplicate() (M/operator/OperatorFactory.java:49): another factory of the same operator; probe-side join factories share
 * the join bridge (the probes are complete once EVERY duplicate has seen noMoreOperators); a hash builder cannot be duplicated
 * (TGPU_ERR_NOT_SUPPORTED, HashBuilderOperator.java:150-152) */
int32_t tgpu_operator_factory_duplicate(tgpu_operator_factory *factory, tgpu_operator_factory **out);
void tgpu_operator_factory_destroy(tgpu_operator_factory *factory);

/* ---- Operator (M/operator/Operator.java:20-102).  Boolean queries return 1/0, or <0 on error. ---- */
int32_t tgpu_operator_needs_input(tgpu_operator *op);
/* Lifetime of `page`: TGPU_HOST arrays have been consumed when the call returns (Java heap arrays are only pinned for the JNI call).
 * TGPU_DEVICE arrays are read by kernels on the context's stream, some of which may still be queued when the call returns (the
 * aggregation's accumulate launch is enqueued behind its group-by probe and not waited for): the caller may overwrite or free them in
 * STREAM ORDER -- by work on that stream, hipFreeAsync on it, hipFree (which synchronises), or after tgpu_context_synchronize -- the
 * rule of any stream-ordered device buffer.  An operator that keeps rows beyond the call copies them or shares the owner: the owner
 * of a page handed over with tgpu_operator_add_input_output_page, and the owners of TGPU_DEVICE blocks that lie inside live buffers of
 * this context (the blocks of an output page; see "Ownership rule" above) -- such blocks are never written by the caller. */
int32_t tgpu_operator_add_input(tgpu_operator *op, const tgpu_page *page);
/* *out = NULL when no page is available (Operator.getOutput() == null); returns TGPU_WOULD_BLOCK instead of TGPU_OK when, in addition,
 * the operator is blocked (a probe waiting for its build side, the outer operator waiting for the probes): the driver should park the
 * pipeline on tgpu_operator_is_blocked instead of spinning (Operator.java:32-35, Driver.java:367-400) */
int32_t tgpu_operator_get_output(tgpu_operator *op, tgpu_output_page **out);
/* Operator.startMemoryRevoke() / finishMemoryRevoke() (M/operator/Operator.java:53-79).  Only a spill-enabled SINGLE / FINAL hash
 * aggregation holds revocable memory: startMemoryRevoke moves its groups out of HBM (below) and has finished when it returns (the
 * reference's future is done); for every other operator state is user memory (tgpu_operator_memory_bytes) and both calls do nothing. */
int32_t tgpu_operator_start_memory_revoke(tgpu_operator *op);
int32_t tgpu_operator_finish_memory_revoke(tgpu_operator *op);
/* OperatorContext.getReservedRevocableBytes(): what startMemoryRevoke would free (the driver revokes while this is > 0,
 * T/operator/OperatorAssertion.java:150-156) */
int64_t tgpu_operator_revocable_memory_bytes(tgpu_operator *op);
/* HashAggregationOperatorFactory(..., spillEnabled, ...) (M/operator/HashAggregationOperator.java:133-154,389-425;
 * M/operator/aggregation/builder/SpillableHashAggregationBuilder.java:47-351), for operators created afterwards, SINGLE and FINAL steps:
 * startMemoryRevoke parks the builder's groups -- keys, raw hashes and the exact accumulator state -- in host memory as one run and
 * starts an empty builder (spillToDisk :283-299); when the output is built the runs are merged through a fresh group-by table, their
 * states added exactly (mergeFromDisk :229-240), and the groups come out in raw-hash order like the reference's merged result
 * (M/operator/MergeHashSort.java).  Accepted by tgpu_hash_aggregation_factory_create and
 * tgpu_filter_project_hash_aggregation_factory_create factories, TGPU_ERR_NOT_SUPPORTED otherwise. */
int32_t tgpu_hash_aggregation_factory_set_spill_enabled(tgpu_operator_factory *factory, int32_t enabled);
/* maxPartialMemory of HashAggregationOperatorFactory (M/operator/HashAggregationOperator.java:128-131; default 16 MB =
 * TaskManagerConfig max_partial_aggregation_memory), for operators created afterwards: a PARTIAL aggregation whose builder is full stops
 * taking input and flushes its groups as an intermediate page (:367-378, :494-497; InMemoryHashAggregationBuilder.isFull :208-215) */
int32_t tgpu_hash_aggregation_factory_set_max_partial_memory(tgpu_operator_factory *factory, int64_t bytes);
/* spills so far (DummySpillerFactory.getSpillsCount in the reference's tests) and the host bytes they hold or held */
int32_t tgpu_operator_spill_stats(tgpu_operator *op, int64_t *spill_count, int64_t *spilled_bytes);
int32_t tgpu_operator_finish(tgpu_operator *op);
int32_t tgpu_operator_is_finished(tgpu_operator *op);
/* addInput with a page another operator of this library produced: the buffers are shared (reference counted), so an operator that keeps
 * or forwards the page (MergePages passing a big page through) does not copy it; `page` may be released right after the call */
int32_t tgpu_operator_add_input_output_page(tgpu_operator *op, const tgpu_output_page *page);
int32_t tgpu_operator_is_blocked(tgpu_operator *op);    /* 1 = isBlocked() future not done (probe waiting for the build) */
int64_t tgpu_operator_memory_bytes(tgpu_operator *op);  /* what the shim reports to LocalMemoryContext.setBytes */
void tgpu_operator_close(tgpu_operator *op);            /* Operator.close(); also frees the handle */

/* ---- output pages (device resident, library owned) ---- */
int32_t tgpu_output_page_position_count(const tgpu_output_page *page);
int32_t tgpu_output_page_channel_count(const tgpu_output_page *page);
/* the page as device-memory blocks (valid until release); lets a downstream GPU operator consume it without a copy */
int32_t tgpu_output_page_as_page(const tgpu_output_page *page, tgpu_page *out);
/* sizes needed to host-materialise channel `ch`: value bytes (VARCHAR: byte-pool size) and whether it may hold nulls */
int32_t tgpu_output_page_block_info(const tgpu_output_page *page, int32_t ch, int32_t *type, int64_t *value_bytes, int32_t *may_have_nulls);
/* D2H copy of one channel into caller buffers: values (value_bytes), nulls (position_count bytes, may be NULL),
 * offsets ((position_count+1) int32, VARCHAR only) */
int32_t tgpu_output_page_copy_block(const tgpu_output_page *page, int32_t ch, void *values, uint8_t *nulls, int32_t *offsets);
/* the same for ALL channels at once (arrays indexed by channel, entries as for copy_block): every transfer is queued through
 * pinned staging and the stream is synchronised once (twice with VARCHAR channels: offsets first, then the bytes) instead of once
 * per buffer -- what the JNI shim uses to turn a GPU output page into heap blocks (S/Page.java:33-73) */
int32_t tgpu_output_page_copy_blocks(const tgpu_output_page *page, int32_t channel_count, void *const *values, uint8_t *const *nulls,
                                     int32_t *const *offsets);
void tgpu_output_page_release(tgpu_output_page *page);

/* ---- GroupByHash (M/operator/GroupByHash.java:45-99; BigintGroupByHash / MultiChannelGroupByHash semantics) ---- */
int32_t tgpu_group_by_hash_create(tgpu_context *ctx, int32_t type_count, const int32_t *types, const int32_t *hash_channels,
                                  int32_t input_hash_channel /* -1 = none */, int32_t expected_size, tgpu_group_by_hash **out);
void tgpu_group_by_hash_destroy(tgpu_group_by_hash *gbh);
int32_t tgpu_group_by_hash_add_page(tgpu_group_by_hash *gbh, const tgpu_page *page);
/* group id of every position (first-seen order, bit-exact with the Java classes) into group_ids[position_count] (host) */
int32_t tgpu_group_by_hash_get_group_ids(tgpu_group_by_hash *gbh, const tgpu_page *page, int64_t *group_ids, int64_t *group_count);
int32_t tgpu_group_by_hash_contains(tgpu_group_by_hash *gbh, int32_t position, const tgpu_page *page, int32_t *result);
int64_t tgpu_group_by_hash_group_count(tgpu_group_by_hash *gbh);
int32_t tgpu_group_by_hash_capacity(tgpu_group_by_hash *gbh);   /* the Java table's capacity for this many groups */
int64_t tgpu_group_by_hash_estimated_size(tgpu_group_by_hash *gbh);
/* appendValuesTo for group ids [0, group_count): key channels (+ raw hash channel when input_hash_channel >= 0) */
int32_t tgpu_group_by_hash_append_values(tgpu_group_by_hash *gbh, tgpu_output_page **out);

/* ---- hash / partition kernels exposed for parity tests and the exchange ---- */
/* InterpretedHashGenerator.hashPosition for every row: hashes[position_count] (host) */
int32_t tgpu_hash_page(tgpu_context *ctx, const tgpu_page *page, int32_t channel_count, const int32_t *channels, int64_t *hashes);
/* PagePartitioner.partitionPage: rows of `page` scattered into `partition_count` contiguous segments, ordered by partition
 * then by input position.  hash_channel >= 0 uses the precomputed raw hash, else the key channels are hashed.
 * partition = (rawHash & 0x7fff...) % partition_count (HashGenerator.java:24-35).  counts[partition_count] (host). */
int32_t tgpu_partition_page(tgpu_context *ctx, const tgpu_page *page, int32_t key_channel_count, const int32_t *key_channels,
                            int32_t hash_channel, int32_t partition_count, int64_t *counts, tgpu_output_page **out);

/* ---- DynamicFilterSourceOperator ---- */
/* M/operator/DynamicFilterSourceOperator.java:74-143 (factory), :145-425 (operator): a pass-through operator on the build side of a join
 * that collects, for every `channels[k]`, what the probe side's scan may be narrowed to: the distinct values while no channel has more
 * than max_distinct_values of them and the collected blocks stay within max_filter_size_in_bytes, else a [min, max] range per orderable
 * channel other than DOUBLE (BIGINT / INTEGER / DATE / BOOLEAN / VARCHAR, :187-190) while at most min_max_collection_limit rows have been
 * seen, else nothing ("all").  Sizes are the reference's block accounting, not TypedSet's JVM retained size (a superset at worst, which an
 * advisory filter allows). */
int32_t tgpu_dynamic_filter_source_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types, int32_t channel_count,
                                                  const int32_t *channels, int32_t max_distinct_values, int64_t max_filter_size_in_bytes,
                                                  int32_t min_max_collection_limit, tgpu_operator_factory **out);
typedef enum tgpu_dynamic_filter_kind { TGPU_DF_ALL = 0, TGPU_DF_VALUES = 1, TGPU_DF_RANGE = 2, TGPU_DF_NONE = 3 } tgpu_dynamic_filter_kind;
/* after finish(): the Domain of filter channel k that DynamicFilterSourceOperator.finish() hands to its consumer (:383-424):
 * VALUES -> *values = a one-channel page of the distinct non-null, non-NaN values (first-seen order; release it as usual);
 * RANGE -> [*min, *max] (BOOLEAN as 0 / 1); a VARCHAR channel's range comes as *values = a one-channel page of two rows, min then max;
 * NONE -> the channel only saw nulls; ALL -> no constraint */
int32_t tgpu_dynamic_filter_source_result(tgpu_operator *op, int32_t filter_channel, int32_t *kind, tgpu_output_page **values, int64_t *min, int64_t *max);

/* ---- MergePages as an operator: page coalescing in HBM ---- */
/* M/operator/project/MergePages.java:64-190 (MergePagesTransformation.process): a page with >= min_row_count rows or >= min_page_size_in_bytes
 * bytes passes through as it is, after the buffered rows; smaller pages are appended to a device buffer that is flushed when it reaches
 * max_page_size_in_bytes (PageBuilder.isFull) or at finish().  Sizes follow the reference's accounting ((width + 1) bytes per fixed-width
 * cell, length + 5 per VARCHAR cell).  The GPU operators want pages of tens of MB and more (DESIGN.md "Page granularity"): put this
 * operator in front of them with large thresholds; the reference's 1 MB cap on min_page_size_in_bytes (MergePages.java:58) is not enforced. */
int32_t tgpu_merge_pages_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types, int64_t min_page_size_in_bytes,
                                        int32_t min_row_count, int64_t max_page_size_in_bytes, tgpu_operator_factory **out);

/* ---- PartitionedOutputOperator: the shuffle producer behind the Operator API ---- */
/* M/operator/PartitionedOutputOperator.java:46-300, PagePartitioner :308-486.  A sink operator (getOutput() returns nothing, :303-306):
 * addInput groups the page's rows by partition = (rawHash & 0x7fff...) % partition_count (HashGenerator.java:24-35) of `hash_channel`
 * (>= 0: the precomputed raw hash) or of the `partition_channels` (InterpretedHashGenerator), rows in input order inside each
 * partition; a row goes to EVERY partition when `null_channel` >= 0 is null there, and so does the first row ever seen when
 * `replicates_any_row` is set (:411-418).  Constant partitioning arguments (:433-448): TGPU_ERR_NOT_SUPPORTED. */
typedef enum tgpu_partition_function {
    TGPU_PARTITION_HASH_MODULO = 0, /* remote exchanges: (rawHash & 0x7fff...) % partition_count, M/operator/HashGenerator.java:24-35 */
    TGPU_PARTITION_LOCAL = 1        /* LocalExchange (M/operator/exchange/PartitioningExchanger.java): (int) XxHash64.hash(Long.reverse(rawHash)) &
                                     * (partition_count - 1), partition_count a power of two, M/operator/exchange/LocalPartitionGenerator.java:45-65 */
} tgpu_partition_function;
int32_t tgpu_partitioned_output_factory_create(tgpu_context *ctx, int32_t operator_id, int32_t type_count, const int32_t *types, int32_t partition_channel_count,
                                               const int32_t *partition_channels, int32_t hash_channel /* -1 = hash the channels */, int32_t partition_count,
                                               int32_t replicates_any_row, int32_t null_channel /* -1 = none */, int32_t partition_function,
                                               tgpu_operator_factory **out);
/* what the reference enqueues into its OutputBuffer (PagePartitioner.flush :451-470: outputBuffer.enqueue(partition, pages)): the next
 * pending (partition, page) pair in enqueue order, device resident (serialize it with tgpu_serialize_page or hand it to a GPU
 * exchange); *out = NULL when nothing is pending */
int32_t tgpu_partitioned_output_poll(tgpu_operator *op, int32_t *partition, tgpu_output_page **out);
/* PartitionedOutputInfo (:396-399) */
int32_t tgpu_partitioned_output_info(tgpu_operator *op, int64_t *rows_added, int64_t *pages_added);

/* ---- SerializedPage <-> HBM: the reference's exchange / spill page format as the ingest / egress format ---- */
/* PagesSerde.serialize + PagesSerdeUtil.writeSerializedPage (M/execution/buffer/PagesSerde.java:64-115, PagesSerdeUtil.java:45-71;
 * block bodies: S/block/LongArrayBlockEncoding.java:37-61, IntArrayBlockEncoding, ByteArrayBlockEncoding, VariableWidthBlockEncoding.java:37-61,
 * null bits S/block/EncoderUtil.java:33-71) of `page` into `out` (host memory, `capacity` bytes): positionCount | markers (none) |
 * uncompressedSize | sizeInBytes | payload, byte for byte what the Java serde writes for the same flat blocks (one representation
 * detail aside: a null vector that holds no null is dropped at ingest, so such a block is written with mayHaveNull = 0 where Java
 * keeps the flag of an all-false valueIsNull array -- both decode to equal blocks).  *out_len = bytes
 * written.  out == NULL: *out_len = an upper bound of the size (nothing is computed), for sizing the buffer. */
int32_t tgpu_serialize_page(tgpu_context *ctx, const tgpu_page *page, void *out, int64_t capacity, int64_t *out_len);
/* PagesSerde.deserialize (PagesSerde.java:117-160) of one uncompressed, unencrypted SerializedPage in host memory, straight into a
 * device-resident page: LONG_ARRAY / INT_ARRAY / BYTE_ARRAY / VARIABLE_WIDTH blocks, RLE and DICTIONARY (RunLengthBlockEncoding.java:31-53,
 * DictionaryBlockEncoding.java:33-80) flattened on the device.  `types` = the tgpu_type of every channel (the encodings do not tell
 * BIGINT from DOUBLE, INTEGER from DATE).  A COMPRESSED page (exchange.compression-enabled: one LZ4 block, PagesSerde.java:73-93,153-165) is
 * inflated on the device first; ENCRYPTED: TGPU_ERR_NOT_SUPPORTED.  (tgpu_serialize_page always writes uncompressed pages, which every reader accepts.) */
int32_t tgpu_deserialize_page(tgpu_context *ctx, const void *bytes, int64_t len, int32_t type_count, const int32_t *types, tgpu_output_page **out);

/* ---- scan-side decode, first slice: ORC stripe streams -> device-resident blocks ---- */
/* What an ORC page source does per column and stripe / row group (lib/trino-orc/src/main/java/io/trino/orc/reader/LongColumnReader.java:100-230,
 * BooleanColumnReader.java, SliceDictionaryColumnReader.java:120-330 over stream/LongInputStreamV2.java:59-312, LongBitPacker.java:82-108,
 * ByteInputStream.java:43-75, BooleanInputStream.java:36-58), on the device: the streams are handed over DECOMPRESSED in host memory (the
 * chunk framing and its codecs stay with the file reader), `present` = the PRESENT stream or NULL (no nulls); *out = a one-channel page.
 * `encoding` = the column's ColumnEncoding kind: the integer streams of DIRECT / DICTIONARY columns (files written before Hive 0.12) are RLEv1
 * (stream/LongInputStreamV1.java:47-103), those of DIRECT_V2 / DICTIONARY_V2 columns RLEv2. */
typedef enum tgpu_orc_encoding { TGPU_ORC_DIRECT = 0, TGPU_ORC_DICTIONARY = 1, TGPU_ORC_DIRECT_V2 = 2, TGPU_ORC_DICTIONARY_V2 = 3 } tgpu_orc_encoding;
/* SHORT / INT / LONG / DATE columns: DATA = signed RLEv2; type = TGPU_BIGINT, TGPU_INTEGER or TGPU_DATE (32-bit types check the range like
 * LongInputStreamV2.next(int[]) :356-364) */
int32_t tgpu_orc_decode_long_column(tgpu_context *ctx, int32_t type, int32_t encoding, int32_t position_count, const void *present, int64_t present_len,
                                    const void *data, int64_t data_len, tgpu_output_page **out);
/* BOOLEAN columns: DATA = a boolean stream */
int32_t tgpu_orc_decode_boolean_column(tgpu_context *ctx, int32_t position_count, const void *present, int64_t present_len, const void *data, int64_t data_len,
                                       tgpu_output_page **out);
/* DOUBLE columns (reader/DoubleColumnReader.java:92-175): DATA = the non-null rows' doubles, 8 little-endian bytes each */
int32_t tgpu_orc_decode_double_column(tgpu_context *ctx, int32_t position_count, const void *present, int64_t present_len, const void *data, int64_t data_len,
                                      tgpu_output_page **out);
/* STRING / VARCHAR / CHAR columns in DICTIONARY_V2 encoding: DATA = unsigned RLEv2 ids, LENGTH = unsigned RLEv2 lengths of the dictionary_size
 * entries, DICTIONARY_DATA = their bytes; the result is a flat VARCHAR block */
int32_t tgpu_orc_decode_dictionary_string_column(tgpu_context *ctx, int32_t encoding, int32_t position_count, const void *present, int64_t present_len,
                                                 const void *data, int64_t data_len, int32_t dictionary_size, const void *length_stream, int64_t length_len,
                                                 const void *dictionary_data, int64_t dictionary_data_len, tgpu_output_page **out);

/* STRING / VARCHAR / CHAR columns in DIRECT_V2 encoding (reader/SliceDirectColumnReader.java:100-232): LENGTH = unsigned RLEv2 lengths of the
 * non-null rows, DATA = their bytes back to back; the result is a flat VARCHAR block */
int32_t tgpu_orc_decode_direct_string_column(tgpu_context *ctx, int32_t encoding, int32_t position_count, const void *present, int64_t present_len,
                                             const void *data, int64_t data_len, const void *length_stream, int64_t length_len, tgpu_output_page **out);

/* ---- scan-side decode, the second columnar format: Parquet data pages -> device-resident blocks ---- */
/* What a Parquet page source does per data page of a FLAT column (lib/trino-parquet/src/main/java/io/trino/parquet/reader/PrimitiveColumnReader.java
 * readPageV1 / readPageV2 / initDataReader, LevelRLEReader.java, ParquetEncoding.java, the dictionary package, reader/{Int,Long,Double,Boolean,Binary}ColumnReader.java;
 * the byte-level decoders are parquet-mr's, restated from the Parquet format specification), on the device.  The page arrives DECOMPRESSED and
 * taken apart by the file reader (thrift page headers and codecs stay there): `definition_levels` = the levels' RLE / bit-packed hybrid of bit
 * width 1 WITHOUT the 4-byte length a V1 page carries in front of it, NULL for a required column; `values` = the value section;
 * `dictionary` / `dictionary_count` = the column chunk's PLAIN dictionary page for the dictionary encodings, else NULL / 0.
 * `physical` = parquet.thrift Type (0 BOOLEAN, 1 INT32, 2 INT64, 5 DOUBLE, 6 BYTE_ARRAY) with `type` INTEGER / DATE, BIGINT, DOUBLE, BOOLEAN, VARCHAR;
 * `encoding` = parquet.thrift Encoding (0 PLAIN, 2 PLAIN_DICTIONARY, 8 RLE_DICTIONARY; 3 RLE for BOOLEAN values; 5 DELTA_BINARY_PACKED for INT32 and INT64, 6 DELTA_LENGTH_BYTE_ARRAY and 7 DELTA_BYTE_ARRAY for BYTE_ARRAY); anything else: TGPU_ERR_NOT_SUPPORTED.  *out = a one-channel page. */
int32_t tgpu_parquet_decode_data_page(tgpu_context *ctx, int32_t type, int32_t physical, int32_t encoding, int32_t position_count, const void *definition_levels,
                                      int64_t definition_levels_len, const void *values, int64_t values_len, const void *dictionary, int64_t dictionary_len,
                                      int32_t dictionary_count, tgpu_output_page **out);

/* ---- exchange between the GPUs of one node ---- */
/* What replaces PartitionedOutputOperator -> OutputBuffer -> HTTP -> ExchangeOperator (M/operator/PartitionedOutputOperator.java:406-476,
 * M/operator/ExchangeOperator.java) when the consumers of a FIXED_HASH_DISTRIBUTION / FIXED_BROADCAST_DISTRIBUTION stage
 * (M/sql/planner/SystemPartitioningHandle.java:59-60) are the GPUs of one node, one rank (process, context) per GPU: pages stay in HBM
 * and travel over xGMI.  One header all-to-all per page (row counts, null-vector flags, VARCHAR byte counts), then ONE grouped RCCL
 * ncclSend / ncclRecv exchange carrying every buffer of every channel to every peer.  Every call is collective: all ranks of the
 * exchange make the same calls in the same order (as the stages of one query do). */
typedef struct tgpu_exchange tgpu_exchange;
#define TGPU_EXCHANGE_ID_BYTES 128
/* rank 0 creates the id and hands it to the other ranks out of band (in the engine: with the task's exchange locations) */
int32_t tgpu_exchange_unique_id(void *id_out /* TGPU_EXCHANGE_ID_BYTES */);
int32_t tgpu_exchange_create(tgpu_context *ctx, const void *unique_id, int32_t rank, int32_t world, tgpu_exchange **out);
/* The same exchange over a transport of the caller's (rehearsals of several ranks on one GPU -- RCCL refuses two ranks on one device --
 * and tests).  all_to_all_meta: host int64 values, per_rank of them per destination / source.  all_to_all_v: device buffers; entry
 * [t * world + r] of the four arrays describes what goes to / comes from rank r in transfer t; the library has synchronised its stream
 * before the call and expects the bytes in place when it returns.  Entries for the caller's own rank are zero (handled inside). */
typedef struct tgpu_exchange_transport {
    void *user;
    int32_t (*all_to_all_meta)(void *user, const int64_t *send, int64_t *recv, int32_t per_rank);
    int32_t (*all_to_all_v)(void *user, int32_t transfers, const void *const *send_ptr, const int64_t *send_bytes, void *const *recv_ptr, const int64_t *recv_bytes);
} tgpu_exchange_transport;
int32_t tgpu_exchange_create_with_transport(tgpu_context *ctx, int32_t rank, int32_t world, const tgpu_exchange_transport *transport, tgpu_exchange **out);
void tgpu_exchange_destroy(tgpu_exchange *ex);
/* hash repartition of `page`: rows go to rank (rawHash & 0x7fff...) % world (M/operator/HashGenerator.java:24-35) of the key channels
 * (hash_channel >= 0: of that precomputed raw hash); *out = the rows this rank owns, grouped by source rank, input order kept */
int32_t tgpu_exchange_repartition(tgpu_exchange *ex, const tgpu_page *page, int32_t key_channel_count, const int32_t *key_channels, int32_t hash_channel,
                                  tgpu_output_page **out);
/* the pages a PartitionedOutputOperator with partition_count == world has pending (tgpu_partitioned_output_poll) shuffled to their
 * ranks: the shuffle producer and the exchange back to back without leaving the library */
int32_t tgpu_exchange_partitioned_output(tgpu_exchange *ex, tgpu_operator *partitioned_output_operator, int32_t type_count, const int32_t *types,
                                         tgpu_output_page **out);
/* broadcast (replicated join build side): every rank receives the pages of all ranks, concatenated in rank order */
int32_t tgpu_exchange_all_gather(tgpu_exchange *ex, const tgpu_page *page, tgpu_output_page **out);
/* bytes this rank has sent to OTHER ranks so far (xGMI traffic; bench.py's exchange_bytes_sent_per_step) */
int64_t tgpu_exchange_bytes_sent(tgpu_exchange *ex);

#ifdef __cplusplus
}
#endif
#endif /* TGPU_H */

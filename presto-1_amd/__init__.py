"""MI355X-native operator hot path for Trino (filter/project, hash aggregation, hash join) behind the C ABI in
include/tgpu.h.  The package directory name is not a Python identifier: import it with
importlib.import_module("presto-1_amd").  There is no CPU fallback: importing works anywhere, but every compute call
needs libtgpu.so (built by __graft_entry__.build()) and a HIP device.
"""
from . import _lib, expressions, operators, spi
from ._lib import SO_PATH, TgpuError, build
from .expressions import (and_, between, call, cast, coalesce, concat, constant, field, if_, in_, is_null, length, like, not_, or_, starts_with, strpos, substr,
                          date_add, date_diff, date_trunc, day, day_of_week, day_of_year, last_day_of_month, month, quarter, week, year, year_of_week,
                          abs_, sign, floor, ceiling, ceil, truncate, round_, sqrt, cbrt, exp, ln, log2, log10, log, power, pow_, is_nan, is_finite, is_infinite,
                          degrees, radians, hour, minute, second, millisecond, to_unixtime)
from .operators import (ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST, DynamicFilterSourceOperatorFactory, MergePagesOperatorFactory, OrderByOperatorFactory, PartitionedOutputOperator, PartitionedOutputOperatorFactory, TopNOperatorFactory, AVG_BIGINT, AVG_DOUBLE, MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE, SUM_ORDER_EXACT, SUM_ORDER_JAVA, COUNT_ALL, COUNT_COLUMN, FINAL, FULL_OUTER, INNER, LOOKUP_OUTER, PARTIAL, PROBE_OUTER, SINGLE, SUM_BIGINT, SUM_DOUBLE,
                        Context, FilterAndProjectOperatorFactory, ScanFilterAndProjectOperatorFactory, PageSource, RecordCursor, FilterProjectHashAggregationOperatorFactory, FilterProjectLookupJoinOperatorFactory, GroupByHash, HashAggregationOperatorFactory, HashBuilderOperatorFactory,
                        LookupJoinOperatorFactory, LookupOuterOperatorFactory, Operator, OperatorFactory, page_processor_source, fused_probe_launch_counts, fused_probe_depth_counts, precompile_fused_aggregation, precompile_fused_probe, precompile_page_processor, to_pages,
                        SET_BITMAP, SET_GENERIC, SET_HASH, HashSemiJoinOperatorFactory, SetBuilderOperatorFactory, SetSupplier,
                        NestedLoopBridge, NestedLoopBuildOperatorFactory, NestedLoopJoinOperatorFactory, FilterProjectNestedLoopJoinOperatorFactory,
                        precompile_nested_loop_filter, nested_loop_filter_source,
                        DistinctLimitOperatorFactory, MarkDistinctOperatorFactory,
                        LimitOperatorFactory, RowNumberOperatorFactory,
                        MergeOperator, MergeOperatorFactory,
                        StreamingAggregationOperatorFactory,
                        MIN_INTEGER, MAX_INTEGER, MIN_DATE, MAX_DATE, MIN_VARCHAR, MAX_VARCHAR, MIN_TIMESTAMP, MAX_TIMESTAMP,
                        DENSE_RANK, RANK, ROW_NUMBER, TopNRankingOperatorFactory,
                        FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT, WINDOW_AGGREGATE, WINDOW_CUME_DIST, WINDOW_DENSE_RANK, WINDOW_FIRST_VALUE,
                        WINDOW_LAG, WINDOW_LAST_VALUE, WINDOW_LEAD, WINDOW_PERCENT_RANK, WINDOW_RANK, WINDOW_ROW_NUMBER, WindowFunction, WindowOperatorFactory,
                        WINDOW_NTH_VALUE, WINDOW_NTILE, FRAME_TYPE_RANGE, FRAME_TYPE_ROWS, FRAME_TYPE_GROUPS, BOUND_UNBOUNDED_PRECEDING, BOUND_PRECEDING, BOUND_CURRENT_ROW,
                        BOUND_FOLLOWING, BOUND_UNBOUNDED_FOLLOWING, WindowFrame, WindowRangeFrame, window_range_bound)
from .spi import (BIGINT, BOOLEAN, DATE, DOUBLE, INTEGER, TIMESTAMP, VARCHAR, Block, DeviceBlock, DictionaryBlock, LazyBlock, OutputPage, Page, RunLengthEncodedBlock)

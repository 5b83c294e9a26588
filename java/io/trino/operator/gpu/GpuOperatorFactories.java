package io.trino.operator.gpu;

import io.airlift.units.DataSize;
import io.trino.metadata.Split;
import io.trino.operator.LookupJoinOperators.JoinType;
import io.trino.operator.OperatorFactory;
import io.trino.operator.SourceOperatorFactory;
import io.trino.operator.window.FrameInfo;
import io.trino.spi.connector.ConnectorPageSource;
import io.trino.spi.connector.SortOrder;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.AggregationNode.Step;
import io.trino.sql.planner.plan.PlanNodeId;
import io.trino.sql.planner.plan.TopNRankingNode.RankingType;
import io.trino.sql.relational.RowExpression;

import java.util.List;
import java.util.Optional;
import java.util.OptionalInt;
import java.util.concurrent.ScheduledExecutorService;
import java.util.function.Function;

/**
 * What LocalExecutionPlanner constructs instead of the Java factories when the session enables the GPU operators
 * (core/trino-main/src/main/java/io/trino/sql/planner/LocalExecutionPlanner.java:1235-1384 filter/project, :2965-3056 aggregation,
 * :2104-2311 join build + probe).  Every method returns Optional.empty() when the plan node is outside what the library covers
 * (a type, function or aggregate it does not have): the planner keeps the Java operator for that node -- the fallback is at the
 * planner, never inside the library.
 */
public final class GpuOperatorFactories
{
    private final long context;                         // tgpu_context*: one per worker and GPU
    private final ScheduledExecutorService poller;

    public GpuOperatorFactories(int device, ScheduledExecutorService poller)
    {
        this.context = GpuNative.createContext(device);
        this.poller = poller;
    }

    public long context()
    {
        return context;
    }

    /** operators in front of Java operators: output cut at PageBuilder.isFull granularity (S/block/PageBuilderStatus.java:49-60); 0 = one page per call */
    public void setMaxOutputPage(long maxBytes, long maxRows)
    {
        GpuNative.setMaxOutputPage(context, maxBytes, maxRows);
    }

    /** strict parity runs: sum(double) / avg(double) in the Java row order (DESIGN.md "DOUBLE aggregate policy") */
    public void setJavaDoubleSumOrder(boolean javaOrder)
    {
        GpuNative.setDoubleSumOrder(context, javaOrder ? 1 : 0);
    }

    /**
     * The promise that device blocks this embedding passes to addInput stay untouched until the operator that took them has finished
     * (a device-resident connector whose stripes live as long as the split): lets the fused aggregation / join keep such pages by reference.
     * Pages of the library itself (DevicePageHandle) never need it.
     */
    public void setDeviceInputStable(boolean stable)
    {
        GpuNative.setDeviceInputStable(context, stable);
    }

    private static int[] ints(List<Integer> values)
    {
        return values.stream().mapToInt(Integer::intValue).toArray();
    }

    private static int stepCode(Step step)
    {
        return step == Step.SINGLE ? 0 : step == Step.PARTIAL ? 1 : step == Step.FINAL ? 2 : -1;     // INTERMEDIATE: not built
    }

    /** FilterAndProjectOperator.createOperatorFactory (operator/FilterAndProjectOperator.java:73-88) */
    public Optional<OperatorFactory> filterAndProject(int operatorId, PlanNodeId planNodeId, List<Type> inputTypes, Optional<RowExpression> filter, List<RowExpression> projections)
    {
        int[] types;
        Optional<GpuRowExpressions.Program> program;
        try {
            types = GpuPages.typeCodes(inputTypes);
            program = GpuRowExpressions.serialize(filter, projections);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        if (program.isEmpty()) {
            return Optional.empty();
        }
        GpuRowExpressions.Program p = program.get();
        long factory = GpuNative.createFilterProjectFactory(context, operatorId, types, p.nodeArray(), p.longArray(), p.doubleArray(), p.stringPool.toByteArray(), p.filterRoot,
                p.projectionRoots);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuFilterAndProjectOperator", inputTypes, poller, factory));
    }

    /**
     * ScanFilterAndProjectOperatorFactory (operator/ScanFilterAndProjectOperator.java:449-560; LocalExecutionPlanner.java:1343-1384): the page-source flavour;
     * `pageSourceForSplit` = pageSourceProvider.createPageSource(session, split, table, columns, dynamicFilter) bound by the planner
     */
    public Optional<SourceOperatorFactory> scanFilterAndProject(int operatorId, PlanNodeId planNodeId, PlanNodeId sourceId, List<Type> sourceTypes,
            Function<Split, ConnectorPageSource> pageSourceForSplit, Optional<RowExpression> filter, List<RowExpression> projections)
    {
        int[] types;
        Optional<GpuRowExpressions.Program> program;
        try {
            types = GpuPages.typeCodes(sourceTypes);
            program = GpuRowExpressions.serialize(filter, projections);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        if (program.isEmpty()) {
            return Optional.empty();
        }
        GpuRowExpressions.Program p = program.get();
        long factory = GpuNative.createScanFilterProjectFactory(context, operatorId, types, p.nodeArray(), p.longArray(), p.doubleArray(), p.stringPool.toByteArray(), p.filterRoot,
                p.projectionRoots);
        return Optional.of(new GpuScanOperatorFactory(operatorId, planNodeId, sourceId, sourceTypes, pageSourceForSplit, poller, factory));
    }

    /**
     * HashAggregationOperatorFactory (operator/HashAggregationOperator.java:54-262).  aggregates: {tgpu_agg_function, input channel, mask channel} triples
     * resolved by the caller from the AccumulatorFactories' bound signatures (count / sum / avg over BIGINT and DOUBLE, min / max over BIGINT, DOUBLE, INTEGER, DATE, VARCHAR and short timestamps (TGPU_AGG_MIN_TIMESTAMP = 17 / TGPU_AGG_MAX_TIMESTAMP = 18); anything else -> Optional.empty()).
     * min / max over VARCHAR cannot spill: with spillEnabled such a plan keeps the Java operator.
     */
    public Optional<OperatorFactory> hashAggregation(int operatorId, PlanNodeId planNodeId, List<Type> inputTypes, List<Type> groupByTypes, List<Integer> groupByChannels, Step step,
            Optional<int[]> aggregates, Optional<Integer> hashChannel, int expectedGroups, boolean produceDefaultOutput, Optional<DataSize> maxPartialMemory, boolean spillEnabled)
    {
        if (aggregates.isEmpty() || stepCode(step) < 0) {
            return Optional.empty();
        }
        int[] keyTypes;
        try {
            GpuPages.typeCodes(inputTypes);
            keyTypes = GpuPages.typeCodes(groupByTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        if (spillEnabled && hasVarcharExtreme(aggregates.get())) {
            return Optional.empty();
        }
        long factory = GpuNative.createHashAggregationFactory(context, operatorId, keyTypes, ints(groupByChannels), hashChannel.orElse(-1), stepCode(step), aggregates.get(),
                expectedGroups, produceDefaultOutput);
        // HashAggregationOperatorFactory(..., maxPartialMemory, spillEnabled, ...) (operator/HashAggregationOperator.java:128-154)
        maxPartialMemory.ifPresent(limit -> GpuNative.setMaxPartialMemory(factory, limit.toBytes()));
        if (spillEnabled) {
            GpuNative.setSpillEnabled(factory, true);
        }
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuHashAggregationOperator", inputTypes, poller, factory));
    }

    /**
     * StreamingAggregationOperator.createOperatorFactory (operator/StreamingAggregationOperator.java:50-69), which the planner chooses when the input is
     * already grouped on the keys (sql/planner/LocalExecutionPlanner.java:3022-3031).  The arguments are the reference's -- the AccumulatorFactories as the
     * {tgpu_agg_function, input channel, mask channel} triples of hashAggregation, no JoinCompiler -- and the operator runs through the generic GpuOperator.
     * No group-by channel, an unsupported type, an aggregate the caller could not resolve or min / max over VARCHAR (hash aggregation only) ->
     * Optional.empty() (the Java operator stays).
     */
    public Optional<OperatorFactory> streamingAggregation(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Type> groupByTypes, List<Integer> groupByChannels, Step step,
            Optional<int[]> aggregates)
    {
        if (aggregates.isEmpty() || stepCode(step) < 0 || groupByChannels.isEmpty() || groupByTypes.size() != groupByChannels.size() || hasVarcharExtreme(aggregates.get())) {
            return Optional.empty();
        }
        int[] types;
        try {
            types = GpuPages.typeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createStreamingAggregationFactory(context, operatorId, types, ints(groupByChannels), stepCode(step), aggregates.get());
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuStreamingAggregationOperator", sourceTypes, poller, factory));
    }

    /**
     * A FilterNode / ProjectNode directly under an AggregationNode (LocalExecutionPlanner.visitAggregation over a filter/project source, :1198,2965-3056) as ONE
     * fused pipeline: tgpu_filter_project_hash_aggregation_factory_create, the operator bench.py's Q1 line times.  groupByChannels, hashChannel and the
     * aggregates' channels index the PROJECTIONS.  Same results as filterAndProject(...) feeding hashAggregation(...); SINGLE and PARTIAL steps.
     * min / max over VARCHAR is not fused: Optional.empty(), and the caller composes filterAndProject(...) and hashAggregation(...).
     */
    public Optional<OperatorFactory> filterProjectHashAggregation(int operatorId, PlanNodeId planNodeId, List<Type> inputTypes, Optional<RowExpression> filter,
            List<RowExpression> projections, List<Type> groupByTypes, List<Integer> groupByChannels, Step step, Optional<int[]> aggregates, Optional<Integer> hashChannel,
            int expectedGroups, Optional<DataSize> maxPartialMemory, boolean spillEnabled)
    {
        if (aggregates.isEmpty() || (step != Step.SINGLE && step != Step.PARTIAL) || hasVarcharExtreme(aggregates.get())) {
            return Optional.empty();
        }
        int[] types;
        int[] keyTypes;
        Optional<GpuRowExpressions.Program> program;
        try {
            types = GpuPages.typeCodes(inputTypes);
            keyTypes = GpuPages.typeCodes(groupByTypes);
            program = GpuRowExpressions.serialize(filter, projections);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        if (program.isEmpty()) {
            return Optional.empty();
        }
        GpuRowExpressions.Program p = program.get();
        long factory = GpuNative.createFilterProjectHashAggregationFactory(context, operatorId, types, p.nodeArray(), p.longArray(), p.doubleArray(), p.stringPool.toByteArray(),
                p.filterRoot, p.projectionRoots, keyTypes, ints(groupByChannels), hashChannel.orElse(-1), stepCode(step), aggregates.get(), expectedGroups);
        maxPartialMemory.ifPresent(limit -> GpuNative.setMaxPartialMemory(factory, limit.toBytes()));
        if (spillEnabled) {
            GpuNative.setSpillEnabled(factory, true);
        }
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuFilterProjectHashAggregationOperator", inputTypes, poller, factory));
    }

    /** TGPU_AGG_MIN_VARCHAR = 15 / TGPU_AGG_MAX_VARCHAR = 16 among the {function, input channel, mask channel} triples (include/tgpu.h) */
    private static boolean hasVarcharExtreme(int[] aggregates)
    {
        for (int i = 0; i + 2 < aggregates.length; i += 3) {
            if (aggregates[i] == 15 || aggregates[i] == 16) {
                return true;
            }
        }
        return false;
    }

    /** the join bridge handle (tgpu_lookup_source_factory*) plays the JoinBridgeManager's role (operator/PartitionedLookupSourceFactory.java:146-205) */
    public static final class JoinBuild
    {
        public final OperatorFactory buildFactory;
        public final long bridge;
        public final List<Type> buildTypes;

        JoinBuild(OperatorFactory buildFactory, long bridge, List<Type> buildTypes)
        {
            this.buildFactory = buildFactory;
            this.bridge = bridge;
            this.buildTypes = buildTypes;
        }

        /** {positions, table slots, position links} of the built table */
        public long[] stats()
        {
            long[] out = new long[3];
            GpuNative.lookupSourceStats(bridge, out);
            return out;
        }

        public void destroy()
        {
            GpuNative.destroyBridge(bridge);
        }
    }

    /**
     * HashBuilderOperatorFactory (operator/HashBuilderOperator.java:54-152; LocalExecutionPlanner.java:2104-2214).  partitionCount = the build side's driver
     * count (PartitionedLookupSourceFactory.java:110-124): 1 = one HashBuilderOperator, else one per local-exchange partition (a power of two).
     */
    public Optional<JoinBuild> hashBuilder(int operatorId, PlanNodeId planNodeId, List<Type> types, List<Integer> outputChannels, List<Integer> hashChannels,
            OptionalInt preComputedHashChannel, int expectedPositions, int partitionCount)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long[] handles = GpuNative.createHashBuilderFactory(context, operatorId, codes, ints(outputChannels), ints(hashChannels), preComputedHashChannel.orElse(-1), expectedPositions,
                partitionCount);
        return Optional.of(new JoinBuild(new GpuOperatorFactory(operatorId, planNodeId, "GpuHashBuilderOperator", types, poller, handles[0]), handles[1], types));
    }

    /**
     * JoinFilterFunction (operator/JoinHash.java:44-47; sql/gen/JoinFilterFunctionCompiler.java; handed to the build side like JoinHashSupplier.java:54-70): `filter`
     * reads build channels [0, buildTypes) and probe channel k as channel buildTypes + k.  Before the probe factories are created; false = outside the IR.
     */
    public boolean joinFilter(JoinBuild build, List<Type> probeTypes, RowExpression filter)
    {
        Optional<GpuRowExpressions.Program> program = GpuRowExpressions.serialize(Optional.of(filter), List.of());
        if (program.isEmpty()) {
            return false;
        }
        GpuRowExpressions.Program p = program.get();
        GpuNative.setJoinFilter(build.bridge, GpuPages.typeCodes(probeTypes), p.nodeArray(), p.longArray(), p.doubleArray(), p.stringPool.toByteArray(), p.filterRoot, p.projectionRoots);
        return true;
    }

    /** LookupJoinOperators.innerJoin / probeOuterJoin / lookupOuterJoin / fullOuterJoin (operator/LookupJoinOperators.java:30-63; LocalExecutionPlanner.java:2284-2311) */
    public Optional<OperatorFactory> lookupJoin(int operatorId, PlanNodeId planNodeId, JoinBuild build, List<Type> probeTypes, List<Integer> probeJoinChannels,
            OptionalInt probeHashChannel, List<Integer> probeOutputChannels, JoinType joinType)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(probeTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createLookupJoinFactory(context, operatorId, build.bridge, codes, ints(probeJoinChannels), probeHashChannel.orElse(-1), ints(probeOutputChannels),
                joinType.ordinal());
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuLookupJoinOperator", probeTypes, poller, factory));
    }

    /**
     * A FilterNode / ProjectNode directly under the probe side of a JoinNode as ONE fused pipeline (tgpu_filter_project_lookup_join_factory_create, the operator
     * bench.py's headline times): the projections form the probe page; probeJoinChannels / probeHashChannel / probeOutputChannels index them.
     */
    public Optional<OperatorFactory> filterProjectLookupJoin(int operatorId, PlanNodeId planNodeId, JoinBuild build, List<Type> inputTypes, Optional<RowExpression> filter,
            List<RowExpression> projections, List<Integer> probeJoinChannels, OptionalInt probeHashChannel, List<Integer> probeOutputChannels, JoinType joinType)
    {
        int[] types;
        Optional<GpuRowExpressions.Program> program;
        try {
            types = GpuPages.typeCodes(inputTypes);
            program = GpuRowExpressions.serialize(filter, projections);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        if (program.isEmpty()) {
            return Optional.empty();
        }
        GpuRowExpressions.Program p = program.get();
        long factory = GpuNative.createFilterProjectLookupJoinFactory(context, operatorId, build.bridge, types, p.nodeArray(), p.longArray(), p.doubleArray(),
                p.stringPool.toByteArray(), p.filterRoot, p.projectionRoots, ints(probeJoinChannels), probeHashChannel.orElse(-1), ints(probeOutputChannels), joinType.ordinal());
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuFilterProjectLookupJoinOperator", inputTypes, poller, factory));
    }

    /** LookupJoinOperatorFactory.createOuterOperatorFactory (operator/LookupJoinOperatorFactory.java:88-103,141-146) */
    public OperatorFactory lookupOuter(int operatorId, PlanNodeId planNodeId, JoinBuild build, List<Type> probeOutputTypes)
    {
        int[] codes = GpuPages.typeCodes(probeOutputTypes);
        return new GpuOperatorFactory(operatorId, planNodeId, "GpuLookupOuterOperator", List.of(), poller, GpuNative.createLookupOuterFactory(context, operatorId, build.bridge, codes));
    }

    /** the semi join's SetSupplier handle (tgpu_set_supplier*) between the set builder and the probes (operator/SetBuilderOperator.java:39-90) */
    public static final class SetBuild
    {
        public final OperatorFactory factory;
        public final long supplier;

        SetBuild(OperatorFactory factory, long supplier)
        {
            this.factory = factory;
            this.supplier = supplier;
        }

        /** {distinct keys (a null counted, ChannelSet.size), containsNull 0 / 1, HBM bytes, layout 0 bitmap | 1 hash | 2 generic} of the built set */
        public long[] stats()
        {
            long[] out = new long[4];
            GpuNative.setSupplierStats(supplier, out);
            return out;
        }

        public void destroy()
        {
            GpuNative.destroySetSupplier(supplier);
        }
    }

    /**
     * SetBuilderOperatorFactory (operator/SetBuilderOperator.java:92-135; LocalExecutionPlanner.visitSemiJoin :2326-2412).  A DynamicFilterSourceOperator
     * in front of it is {@link #dynamicFilterSource}.
     */
    public Optional<SetBuild> setBuilder(int operatorId, PlanNodeId planNodeId, List<Type> types, int setChannel, OptionalInt hashChannel, int expectedPositions)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long[] handles = GpuNative.createSetBuilderFactory(context, operatorId, codes, setChannel, hashChannel.orElse(-1), expectedPositions);
        return Optional.of(new SetBuild(new GpuSetBuilderOperatorFactory(operatorId, planNodeId, types, poller, handles[0], handles[1]), handles[1]));
    }

    /** HashSemiJoinOperator.HashSemiJoinOperatorFactory (operator/HashSemiJoinOperator.java:44-118): the probe page + one BOOLEAN channel */
    public Optional<OperatorFactory> hashSemiJoin(int operatorId, PlanNodeId planNodeId, SetBuild build, List<Type> probeTypes, int probeJoinChannel,
            OptionalInt probeHashChannel)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(probeTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createHashSemiJoinFactory(context, operatorId, build.supplier, codes, probeJoinChannel, probeHashChannel.orElse(-1));
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuHashSemiJoinOperator", probeTypes, poller, factory));
    }

    /** the nested loop join's bridge handle (tgpu_nested_loop_bridge*) between the build operator and the probes (operator/NestedLoopJoinPagesSupplier.java) */
    public static final class NestedLoopBuild
    {
        public final OperatorFactory factory;
        public final long bridge;
        final List<Type> buildTypes;

        NestedLoopBuild(OperatorFactory factory, long bridge, List<Type> buildTypes)
        {
            this.factory = factory;
            this.bridge = bridge;
            this.buildTypes = buildTypes;
        }

        /** {kept pages (zero-channel pages re-cut to 8192 positions), positions, HBM bytes} of the published build side */
        public long[] stats()
        {
            long[] out = new long[3];
            GpuNative.nestedLoopBridgeStats(bridge, out);
            return out;
        }

        public void destroy()
        {
            GpuNative.destroyNestedLoopBridge(bridge);
        }
    }

    /**
     * NestedLoopBuildOperatorFactory (operator/NestedLoopBuildOperator.java:33-94; LocalExecutionPlanner.visitJoin for a JoinNode without equi-criteria).
     * An empty type list is a build side without channels: its pages are only counted.
     */
    public Optional<NestedLoopBuild> nestedLoopBuild(int operatorId, PlanNodeId planNodeId, List<Type> types)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long[] handles = GpuNative.createNestedLoopBuildFactory(context, operatorId, codes);
        return Optional.of(new NestedLoopBuild(new GpuNestedLoopBuildOperatorFactory(operatorId, planNodeId, types, poller, handles[0]), handles[1], types));
    }

    /** NestedLoopJoinOperator.NestedLoopJoinOperatorFactory (operator/NestedLoopJoinOperator.java:44-108): probeChannels then buildChannels; maxOutputRows 0 = the default */
    public Optional<OperatorFactory> nestedLoopJoin(int operatorId, PlanNodeId planNodeId, NestedLoopBuild build, List<Type> probeTypes, List<Integer> probeChannels,
            List<Integer> buildChannels, long maxOutputRows)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(probeTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createNestedLoopJoinFactory(context, operatorId, build.bridge, codes, ints(probeChannels), ints(buildChannels), maxOutputRows);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuNestedLoopJoinOperator", probeTypes, poller, factory));
    }

    /**
     * The FilterNode / ProjectNode above a JoinNode without equi-criteria fused into the join (tgpu_filter_project_nested_loop_join_factory_create): the
     * expressions address the join's output page, probe channels first, then the build channels.
     */
    public Optional<OperatorFactory> filterProjectNestedLoopJoin(int operatorId, PlanNodeId planNodeId, NestedLoopBuild build, List<Type> probeTypes,
            Optional<RowExpression> filter, List<RowExpression> projections, long maxProductRows)
    {
        int[] codes;
        Optional<GpuRowExpressions.Program> program;
        try {
            codes = GpuPages.typeCodes(probeTypes);
            program = GpuRowExpressions.serialize(filter, projections);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        if (program.isEmpty()) {
            return Optional.empty();
        }
        GpuRowExpressions.Program p = program.get();
        long factory = GpuNative.createFilterProjectNestedLoopJoinFactory(context, operatorId, build.bridge, codes, p.nodeArray(), p.longArray(), p.doubleArray(),
                p.stringPool.toByteArray(), p.filterRoot, p.projectionRoots, maxProductRows);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuFilterProjectNestedLoopJoinOperator", probeTypes, poller, factory));
    }

    /**
     * MarkDistinctOperator.MarkDistinctOperatorFactory (operator/MarkDistinctOperator.java:51-71; LocalExecutionPlanner.visitMarkDistinct): the source page plus one
     * BOOLEAN channel that is true on the first row of every value of the mark channels; the aggregation reads it as its mask channel.
     */
    public Optional<OperatorFactory> markDistinct(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> markDistinctChannels, OptionalInt hashChannel)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createMarkDistinctFactory(context, operatorId, codes, ints(markDistinctChannels), hashChannel.orElse(-1));
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuMarkDistinctOperator", sourceTypes, poller, factory));
    }

    /** DistinctLimitOperator.DistinctLimitOperatorFactory (operator/DistinctLimitOperator.java:55-75; LocalExecutionPlanner.visitDistinctLimit) */
    public Optional<OperatorFactory> distinctLimit(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> distinctChannels, long limit,
            OptionalInt hashChannel)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createDistinctLimitFactory(context, operatorId, codes, ints(distinctChannels), limit, hashChannel.orElse(-1));
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuDistinctLimitOperator", sourceTypes, poller, factory));
    }

    /**
     * RowNumberOperator.RowNumberOperatorFactory (operator/RowNumberOperator.java:61-84; LocalExecutionPlanner.visitRowNumber): the output channels, then the BIGINT
     * number of the row inside its partition; with maxRowsPerPartition only the rows numbered up to it.  The partition types are those of the partition channels.
     */
    public Optional<OperatorFactory> rowNumber(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels, List<Integer> partitionChannels,
            Optional<Integer> maxRowsPerPartition, OptionalInt hashChannel, int expectedPositions)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createRowNumberFactory(context, operatorId, codes, ints(outputChannels), ints(partitionChannels),
                maxRowsPerPartition.map(Integer::longValue).orElse(-1L), hashChannel.orElse(-1), expectedPositions);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuRowNumberOperator", sourceTypes, poller, factory));
    }

    /**
     * TopNRankingOperator.TopNRankingOperatorFactory (operator/TopNRankingOperator.java:67-104; LocalExecutionPlanner.visitTopNRanking): row_number() / rank() OVER
     * (PARTITION BY .. ORDER BY ..) <= maxRankPerPartition.  The output channels, then (unless partial) the BIGINT ranking.  DENSE_RANK stays with the reference's
     * operator, which throws UnsupportedOperationException for it (:235-236).
     */
    public Optional<OperatorFactory> topNRanking(int operatorId, PlanNodeId planNodeId, RankingType rankingType, List<Type> sourceTypes, List<Integer> outputChannels,
            List<Integer> partitionChannels, List<Integer> sortChannels, List<SortOrder> sortOrders, int maxRankPerPartition, boolean partial, OptionalInt hashChannel,
            int expectedPositions)
    {
        if (rankingType == RankingType.DENSE_RANK) {
            return Optional.empty();
        }
        int[] codes;
        try {
            codes = GpuPages.typeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createTopNRankingFactory(context, operatorId, rankingType.ordinal(), codes, ints(outputChannels), ints(partitionChannels), ints(sortChannels),
                sortOrders.stream().mapToInt(SortOrder::ordinal).toArray(), maxRankPerPartition, partial, hashChannel.orElse(-1), expectedPositions);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuTopNRankingOperator", sourceTypes, poller, factory));
    }

    /** tgpu_window_function / tgpu_window_frame (include/tgpu.h) */
    public static final int WINDOW_ROW_NUMBER = 0;
    public static final int WINDOW_RANK = 1;
    public static final int WINDOW_DENSE_RANK = 2;
    public static final int WINDOW_PERCENT_RANK = 3;
    public static final int WINDOW_CUME_DIST = 4;
    public static final int WINDOW_LAG = 5;
    public static final int WINDOW_LEAD = 6;
    public static final int WINDOW_FIRST_VALUE = 7;
    public static final int WINDOW_LAST_VALUE = 8;
    public static final int WINDOW_AGGREGATE = 9;
    public static final int FRAME_PARTITION = 0;
    public static final int FRAME_RANGE_TO_CURRENT = 1;
    public static final int FRAME_ROWS_TO_CURRENT = 2;
    /** framedWindow(..) only: two more functions, tgpu_frame_type = WindowFrame.Type's ordinal, tgpu_frame_bound = FrameBound.Type's ordinal */
    public static final int WINDOW_NTH_VALUE = 10;
    public static final int WINDOW_NTILE = 11;
    public static final int FRAME_TYPE_RANGE = 0;
    public static final int FRAME_TYPE_ROWS = 1;
    public static final int FRAME_TYPE_GROUPS = 2;
    public static final int BOUND_UNBOUNDED_PRECEDING = 0;
    public static final int BOUND_PRECEDING = 1;
    public static final int BOUND_CURRENT_ROW = 2;
    public static final int BOUND_FOLLOWING = 3;
    public static final int BOUND_UNBOUNDED_FOLLOWING = 4;

    /** one window function as the eight ints of tgpu_window_function_spec; aggFunction is read for WINDOW_AGGREGATE only (the codes of aggregateSpecs) */
    public static int[] windowFunction(int function, int aggFunction, int frame, boolean ignoreNulls, List<Integer> argumentChannels)
    {
        if (argumentChannels.size() > 3) {
            throw new IllegalArgumentException("a window function takes at most 3 argument channels");
        }
        int[] spec = new int[8];
        spec[0] = function;
        spec[1] = aggFunction;
        spec[2] = frame;
        spec[3] = argumentChannels.size();
        for (int i = 0; i < argumentChannels.size(); i++) {
            spec[4 + i] = argumentChannels.get(i);
        }
        spec[7] = ignoreNulls ? 1 : 0;
        return spec;
    }

    /**
     * WindowOperator.WindowOperatorFactory (operator/WindowOperator.java:70-203; LocalExecutionPlanner.visitWindow): the window functions OVER (PARTITION BY ..
     * ORDER BY ..).  The output channels, then one channel per function.  functions: one windowFunction(..) per WindowFunctionDefinition; the caller returns
     * Optional.empty() itself for what include/tgpu.h rules out (IGNORE NULLS, DOUBLE sums and averages), and calls framedWindow(..) for frames with offsets, ntile and nth_value.  A node with
     * preGroupedChannels / preSortedChannelPrefix is handed over as if it had none: the result differs in the order of the partitions only.
     */
    public Optional<OperatorFactory> window(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels, List<int[]> functions,
            List<Integer> partitionChannels, List<Integer> sortChannels, List<SortOrder> sortOrders, int expectedPositions)
    {
        int[] codes;
        try {
            codes = windowTypeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        int[] flat = new int[functions.size() * 8];
        for (int i = 0; i < functions.size(); i++) {
            System.arraycopy(functions.get(i), 0, flat, i * 8, 8);
        }
        long factory = GpuNative.createWindowFactory(context, operatorId, codes, ints(outputChannels), flat, ints(partitionChannels), ints(sortChannels),
                sortOrders.stream().mapToInt(SortOrder::ordinal).toArray(), expectedPositions);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuWindowOperator", sourceTypes, poller, factory));
    }

    /**
     * the type codes of a window node's source channels.  The native window entry points take the codes 1..6: a node with a timestamp channel keeps the
     * Java operator (the library's own window factories take TGPU_TIMESTAMP channels, include/tgpu.h)
     */
    private static int[] windowTypeCodes(List<Type> sourceTypes)
    {
        int[] codes = GpuPages.typeCodes(sourceTypes);
        for (int code : codes) {
            if (code == GpuPages.T_TIMESTAMP) {
                throw new IllegalArgumentException("timestamp channels are not handed to the native window factories");
            }
        }
        return codes;
    }

    /** one frame as the five ints of tgpu_window_frame_spec, from the fields of a FrameInfo (operator/window/FrameInfo.java); the channels are read for PRECEDING / FOLLOWING bounds only */
    public static int[] windowFrame(FrameInfo frame)
    {
        return new int[] {frame.getType().ordinal(), frame.getStartType().ordinal(), frame.getStartChannel(), frame.getEndType().ordinal(), frame.getEndChannel()};
    }

    private static boolean hasOffset(int bound)
    {
        return bound == BOUND_PRECEDING || bound == BOUND_FOLLOWING;
    }

    /**
     * window(..) with the frames of FrameInfo: ROWS / GROUPS frames with k PRECEDING / k FOLLOWING bounds, RANGE frames by peers, and the functions nth_value and
     * ntile.  functions: one windowFunction(..) per WindowFunctionDefinition (its frame int is not read); frames: one windowFrame(..) per function.
     * Optional.empty() for what the library refuses: a type without a code, and RANGE with a PRECEDING / FOLLOWING bound; the caller returns it itself for
     * IGNORE NULLS and DOUBLE sums and averages, as for window(..).
     */
    public Optional<OperatorFactory> framedWindow(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels, List<int[]> functions,
            List<int[]> frames, List<Integer> partitionChannels, List<Integer> sortChannels, List<SortOrder> sortOrders, int expectedPositions)
    {
        if (frames.size() != functions.size()) {
            throw new IllegalArgumentException("one frame per window function");
        }
        int[] codes;
        try {
            codes = windowTypeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        int[] flat = new int[functions.size() * 8];
        int[] flatFrames = new int[frames.size() * 5];
        for (int i = 0; i < functions.size(); i++) {
            System.arraycopy(functions.get(i), 0, flat, i * 8, 8);
            int[] frame = frames.get(i);
            if (frame[0] == FRAME_TYPE_RANGE && (hasOffset(frame[1]) || hasOffset(frame[3]))) {
                return Optional.empty();
            }
            System.arraycopy(frame, 0, flatFrames, i * 5, 5);
        }
        long factory = GpuNative.createFramedWindowFactory(context, operatorId, codes, ints(outputChannels), flat, flatFrames, ints(partitionChannels), ints(sortChannels),
                sortOrders.stream().mapToInt(SortOrder::ordinal).toArray(), expectedPositions);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuWindowOperator", sourceTypes, poller, factory));
    }

    /**
     * one frame as the seven ints of tgpu_window_range_frame_spec: windowFrame(..) plus FrameInfo's two comparison key channels.  For a RANGE frame with a
     * PRECEDING / FOLLOWING bound the start / end channel holds the bound's VALUE (sort key -/+ offset, QueryPlanner.planFrameBound), not an offset
     */
    public static int[] windowRangeFrame(FrameInfo frame)
    {
        return new int[] {frame.getType().ordinal(), frame.getStartType().ordinal(), frame.getStartChannel(), frame.getEndType().ordinal(), frame.getEndChannel(),
                frame.getSortKeyChannelForStartComparison(), frame.getSortKeyChannelForEndComparison()};
    }

    /**
     * framedWindow(..) with RANGE BETWEEN x PRECEDING / FOLLOWING AND y PRECEDING / FOLLOWING as well (tgpu_window_factory_create_ranged).  functions: one
     * windowFunction(..) per WindowFunctionDefinition; frames: its FrameInfo.  Optional.empty() for a type without a code, and for a RANGE frame with a value
     * bound unless FrameInfo.getSortKeyChannel() is the node's single sort channel and getOrdering() agrees with its sort order; the caller returns it itself for
     * IGNORE NULLS and DOUBLE sums and averages, as for window(..).
     */
    public Optional<OperatorFactory> rangeWindow(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels, List<int[]> functions,
            List<FrameInfo> frames, List<Integer> partitionChannels, List<Integer> sortChannels, List<SortOrder> sortOrders, int expectedPositions)
    {
        if (frames.size() != functions.size()) {
            throw new IllegalArgumentException("one frame per window function");
        }
        int[] codes;
        try {
            codes = windowTypeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        int[] flat = new int[functions.size() * 8];
        int[] flatFrames = new int[frames.size() * 7];
        for (int i = 0; i < functions.size(); i++) {
            System.arraycopy(functions.get(i), 0, flat, i * 8, 8);
            FrameInfo info = frames.get(i);
            int[] frame = windowRangeFrame(info);
            if (frame[0] == FRAME_TYPE_RANGE && (hasOffset(frame[1]) || hasOffset(frame[3]))) {
                if (sortChannels.size() != 1 || sortOrders.size() != 1 || info.getSortKeyChannel() != sortChannels.get(0) || info.getOrdering().isEmpty()) {
                    return Optional.empty();
                }
                boolean ascending = info.getOrdering().get() == io.trino.sql.tree.SortItem.Ordering.ASCENDING;
                if (ascending != sortOrders.get(0).isAscending()) {
                    return Optional.empty();
                }
            }
            System.arraycopy(frame, 0, flatFrames, i * 7, 7);
        }
        long factory = GpuNative.createRangeWindowFactory(context, operatorId, codes, ints(outputChannels), flat, flatFrames, ints(partitionChannels), ints(sortChannels),
                sortOrders.stream().mapToInt(SortOrder::ordinal).toArray(), expectedPositions);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuWindowOperator", sourceTypes, poller, factory));
    }

    /** LimitOperator.LimitOperatorFactory (operator/LimitOperator.java:34-39; LocalExecutionPlanner.visitLimit) */
    public Optional<OperatorFactory> limit(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, long limit)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(sourceTypes);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createLimitFactory(context, operatorId, codes, limit);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuLimitOperator", sourceTypes, poller, factory));
    }

    /** TopNOperator.createOperatorFactory (operator/TopNOperator.java:47-62; LocalExecutionPlanner.visitTopN) */
    public Optional<OperatorFactory> topN(int operatorId, PlanNodeId planNodeId, List<Type> types, long n, List<Integer> sortChannels, List<SortOrder> sortOrders)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createTopNFactory(context, operatorId, codes, n, ints(sortChannels), sortOrders.stream().mapToInt(SortOrder::ordinal).toArray());
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuTopNOperator", types, poller, factory));
    }

    /** OrderByOperator.OrderByOperatorFactory (operator/OrderByOperator.java:48-131; LocalExecutionPlanner.visitSort) */
    public Optional<OperatorFactory> orderBy(int operatorId, PlanNodeId planNodeId, List<Type> types, List<Integer> outputChannels, int expectedPositions,
            List<Integer> sortChannels, List<SortOrder> sortOrders)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createOrderByFactory(context, operatorId, codes, ints(outputChannels), expectedPositions, ints(sortChannels),
                sortOrders.stream().mapToInt(SortOrder::ordinal).toArray());
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuOrderByOperator", types, poller, factory));
    }

    /**
     * MergeOperator.MergeOperatorFactory (operator/MergeOperator.java:47-107; LocalExecutionPlanner.java:783) and, with local sources behind
     * `pageSourceForSplit`, LocalMergeSourceOperator (operator/exchange/LocalMergeSourceOperator.java:39-; LocalExecutionPlanner.java:2687): the k-way merge
     * of sorted streams.  Every split added to the operator is one stream.
     */
    public Optional<SourceOperatorFactory> merge(int operatorId, PlanNodeId planNodeId, PlanNodeId sourceId, List<Type> types, List<Integer> outputChannels,
            List<Integer> sortChannels, List<SortOrder> sortOrders, Function<Split, ConnectorPageSource> pageSourceForSplit)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createMergeFactory(context, operatorId, codes, ints(outputChannels), ints(sortChannels), sortOrders.stream().mapToInt(SortOrder::ordinal).toArray());
        List<Type> outputTypes = outputChannels.stream().map(types::get).collect(java.util.stream.Collectors.toList());
        return Optional.of(new GpuMergeOperatorFactory(operatorId, planNodeId, sourceId, types, outputTypes, pageSourceForSplit, poller, factory));
    }

    /** MergePages (operator/project/MergePages.java:64-190) as an operator in front of GPU operators that want large pages (DESIGN.md "Page granularity") */
    public OperatorFactory mergePages(int operatorId, PlanNodeId planNodeId, List<Type> types, DataSize minPageSize, int minRowCount, DataSize maxPageSize)
    {
        long factory = GpuNative.createMergePagesFactory(context, operatorId, GpuPages.typeCodes(types), minPageSize.toBytes(), minRowCount, maxPageSize.toBytes());
        return new GpuOperatorFactory(operatorId, planNodeId, "GpuMergePagesOperator", types, poller, factory);
    }

    /**
     * PartitionedOutputOperator (operator/PartitionedOutputOperator.java:46-300): the shuffle producer.  The pending (partition, page) pairs are taken with
     * {@link #pollPartitionedOutput} (what PagePartitioner.flush hands to outputBuffer.enqueue, :451-470) or sent to the other GPUs by {@link GpuExchange}.
     * localPartitionFunction: the LocalPartitionGenerator function of local exchanges instead of (rawHash & 0x7fff...) % partitionCount.
     */
    public Optional<OperatorFactory> partitionedOutput(int operatorId, PlanNodeId planNodeId, List<Type> types, List<Integer> partitionChannels, OptionalInt hashChannel,
            int partitionCount, boolean replicatesAnyRow, OptionalInt nullChannel, boolean localPartitionFunction)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createPartitionedOutputFactory(context, operatorId, codes, ints(partitionChannels), hashChannel.orElse(-1), partitionCount, replicatesAnyRow,
                nullChannel.orElse(-1), localPartitionFunction ? 1 : 0);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuPartitionedOutputOperator", types, poller, factory));
    }

    /** the next pending page of a partitioned-output operator as a device-resident Page, partition[0] = its partition; null when nothing is pending */
    public static io.trino.spi.Page pollPartitionedOutput(GpuOperator operator, int[] partition)
    {
        long page = GpuNative.partitionedOutputPoll(operator.nativeHandle(), partition);
        return page == 0 ? null : GpuPages.deviceResident(page);
    }

    /** DynamicFilterSourceOperatorFactory (operator/DynamicFilterSourceOperator.java:74-143; LocalExecutionPlanner.java:2216-2260) */
    public Optional<OperatorFactory> dynamicFilterSource(int operatorId, PlanNodeId planNodeId, List<Type> types, List<Integer> channels, int maxDistinctValues,
            DataSize maxFilterSize, int minMaxCollectionLimit)
    {
        int[] codes;
        try {
            codes = GpuPages.typeCodes(types);
        }
        catch (IllegalArgumentException unsupportedType) {
            return Optional.empty();
        }
        long factory = GpuNative.createDynamicFilterSourceFactory(context, operatorId, codes, ints(channels), maxDistinctValues, maxFilterSize.toBytes(), minMaxCollectionLimit);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuDynamicFilterSourceOperator", types, poller, factory));
    }

    /** the Domain of filter channel k after finish() (DynamicFilterSourceOperator.java:383-424): kindMinMax = {ALL 0 | VALUES 1 | RANGE 2 | NONE 3, min, max}; the values / VARCHAR range page or null */
    public static io.trino.spi.Page dynamicFilterResult(GpuOperator operator, int filterChannel, long[] kindMinMax)
    {
        long page = GpuNative.dynamicFilterSourceResult(operator.nativeHandle(), filterChannel, kindMinMax);
        return page == 0 ? null : GpuPages.deviceResident(page);
    }

    /**
     * The hop between two stages whose tasks are the GPUs of one node (tgpu_exchange_*: K10 partition kernels + one grouped RCCL all-to-all-v over xGMI)
     * instead of PartitionedOutputOperator -> OutputBuffer -> HTTP -> ExchangeOperator.  Collective: every rank makes the same calls in the same order.
     */
    public static final class GpuExchange
    {
        private final long exchange;

        /** rank 0 creates the id ({@link #uniqueId}) and ships it with the task's exchange locations */
        public GpuExchange(GpuOperatorFactories factories, byte[] uniqueId, int rank, int world)
        {
            this.exchange = GpuNative.createExchange(factories.context, uniqueId, rank, world);
        }

        public static byte[] uniqueId()
        {
            return GpuNative.exchangeUniqueId();
        }

        private static long handleOf(io.trino.spi.Page page)
        {
            GpuPages.DevicePageHandle handle = GpuPages.deviceHandle(page);
            if (handle == null) {
                throw new IllegalArgumentException("the GPU exchange moves device-resident pages");
            }
            return handle.handle;
        }

        /** FIXED_HASH_DISTRIBUTION: this rank's rows of every rank's page */
        public io.trino.spi.Page repartition(io.trino.spi.Page page, List<Integer> keyChannels, OptionalInt hashChannel)
        {
            return GpuPages.deviceResident(GpuNative.exchangeRepartition(exchange, handleOf(page), ints(keyChannels), hashChannel.orElse(-1)));
        }

        /** what a partitioned-output operator (partitionCount == world) has pending after one addInput, shuffled to its ranks */
        public io.trino.spi.Page partitionedOutput(GpuOperator partitionedOutputOperator, List<Type> types)
        {
            return GpuPages.deviceResident(GpuNative.exchangePartitionedOutput(exchange, partitionedOutputOperator.nativeHandle(), GpuPages.typeCodes(types)));
        }

        /** FIXED_BROADCAST_DISTRIBUTION (a replicated join build side) */
        public io.trino.spi.Page allGather(io.trino.spi.Page page)
        {
            return GpuPages.deviceResident(GpuNative.exchangeAllGather(exchange, handleOf(page)));
        }

        public long bytesSent()
        {
            return GpuNative.exchangeBytesSent(exchange);
        }

        public void close()
        {
            GpuNative.destroyExchange(exchange);
        }
    }
}

package io.trino.operator.gpu;

import io.trino.metadata.Split;
import io.trino.operator.OperatorContext;
import io.trino.operator.SourceOperator;
import io.trino.spi.Page;
import io.trino.spi.connector.ConnectorPageSource;
import io.trino.spi.connector.UpdatablePageSource;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.List;
import java.util.Optional;
import java.util.concurrent.ScheduledExecutorService;
import java.util.function.Function;
import java.util.function.Supplier;

/**
 * MergeOperator (core/trino-main/src/main/java/io/trino/operator/MergeOperator.java:44-256): a SourceOperator (SourceOperator.java:24-33) that merges
 * the sorted page streams of its splits.  Every split is one stream: `pageSourceForSplit` wraps the split's pages (the reference reads a RemoteSplit
 * through an exchange client, :155-177) as a ConnectorPageSource, which the library pulls through {@link GpuPageSource}.  `sourceTypes` are the channels
 * of the streams' pages, `outputTypes` those of the merged page.
 */
public class GpuMergeOperator
        extends GpuOperator
        implements SourceOperator
{
    private final PlanNodeId sourceId;
    private final List<Type> sourceTypes;
    private final Function<Split, ConnectorPageSource> pageSourceForSplit;

    public GpuMergeOperator(OperatorContext operatorContext, long handle, PlanNodeId sourceId, List<Type> sourceTypes, List<Type> outputTypes,
            Function<Split, ConnectorPageSource> pageSourceForSplit, ScheduledExecutorService poller)
    {
        super(operatorContext, handle, outputTypes, poller);
        this.sourceId = sourceId;
        this.sourceTypes = sourceTypes;
        this.pageSourceForSplit = pageSourceForSplit;
    }

    @Override
    public PlanNodeId getSourceId()
    {
        return sourceId;
    }

    @Override
    public Supplier<Optional<UpdatablePageSource>> addSplit(Split split)
    {
        ConnectorPageSource source = pageSourceForSplit.apply(split);
        try {
            GpuNative.mergeAddPageSource(handle, new GpuPageSource(source, sourceTypes), GpuPages.typeCodes(sourceTypes));
        }
        catch (GpuNative.NativeError e) {
            throw GpuNative.toTrinoException(e);
        }
        return Optional::empty;      // MergeOperator.java:176
    }

    @Override
    public void noMoreSplits()
    {
        try {
            GpuNative.mergeNoMoreSplits(handle);
        }
        catch (GpuNative.NativeError e) {
            throw GpuNative.toTrinoException(e);
        }
    }

    // a source operator never sees addInput, where GpuOperator reports its memory: the buffered rows of the streams change with every pull
    @Override
    public Page getOutput()
    {
        Page page = super.getOutput();
        updateMemory();
        return page;
    }

    @Override
    public boolean needsInput()
    {
        return false;      // MergeOperator.java:222-225
    }

    @Override
    public void addInput(Page page)
    {
        throw new UnsupportedOperationException(getClass().getName() + " cannot take input");
    }
}

package io.trino.operator.gpu;

import io.trino.operator.DriverContext;
import io.trino.operator.Operator;
import io.trino.operator.OperatorContext;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.List;
import java.util.concurrent.ScheduledExecutorService;

/**
 * SetBuilderOperatorFactory (core/trino-main/src/main/java/io/trino/operator/SetBuilderOperator.java:92-135) over a tgpu_operator_factory handle:
 * its operators record the built set as their output once they have finished, as SetBuilderOperator.finish does (:172-183).
 */
public class GpuSetBuilderOperatorFactory
        extends GpuOperatorFactory
{
    private final long supplier;                       // tgpu_set_supplier*

    GpuSetBuilderOperatorFactory(int operatorId, PlanNodeId planNodeId, List<Type> inputTypes, ScheduledExecutorService poller, long factory, long supplier)
    {
        super(operatorId, planNodeId, "GpuSetBuilderOperator", inputTypes, poller, factory);
        this.supplier = supplier;
    }

    @Override
    public Operator createOperator(DriverContext driverContext)
    {
        if (closed) {
            throw new IllegalStateException("Factory is already closed");
        }
        OperatorContext operatorContext = driverContext.addOperatorContext(operatorId, planNodeId, operatorType);
        try {
            return new GpuSetBuilderOperator(operatorContext, GpuNative.createOperator(factory), inputTypes, poller, supplier);
        }
        catch (GpuNative.NativeError e) {
            throw GpuNative.toTrinoException(e);
        }
    }

    public static class GpuSetBuilderOperator
            extends GpuOperator
    {
        private final long supplier;
        private boolean recorded;

        GpuSetBuilderOperator(OperatorContext operatorContext, long handle, List<Type> inputTypes, ScheduledExecutorService poller, long supplier)
        {
            super(operatorContext, handle, inputTypes, poller);
            this.supplier = supplier;
        }

        @Override
        public void finish()
        {
            super.finish();
            if (recorded) {
                return;
            }
            long[] stats = new long[4];
            try {
                GpuNative.setSupplierStats(supplier, stats);
            }
            catch (GpuNative.NativeError e) {
                throw GpuNative.toTrinoException(e);
            }
            // operatorContext.recordOutput(channelSet.getEstimatedSizeInBytes(), channelSet.size()) (SetBuilderOperator.java:181)
            getOperatorContext().recordOutput(stats[2], stats[0]);
            recorded = true;
        }
    }
}

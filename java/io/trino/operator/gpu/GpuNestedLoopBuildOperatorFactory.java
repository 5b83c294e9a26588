package io.trino.operator.gpu;

import io.trino.operator.DriverContext;
import io.trino.operator.Operator;
import io.trino.operator.OperatorContext;
import io.trino.spi.Page;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.List;
import java.util.concurrent.ScheduledExecutorService;

/**
 * NestedLoopBuildOperatorFactory (core/trino-main/src/main/java/io/trino/operator/NestedLoopBuildOperator.java:33-94) over a tgpu_operator_factory
 * handle: its operators record every non-empty page they take as their output, as NestedLoopBuildOperator.addInput does (:124-140).  The pages
 * themselves stay in HBM behind the bridge (tgpu_nested_loop_bridge*) until the probes have closed.
 */
public class GpuNestedLoopBuildOperatorFactory
        extends GpuOperatorFactory
{
    GpuNestedLoopBuildOperatorFactory(int operatorId, PlanNodeId planNodeId, List<Type> inputTypes, ScheduledExecutorService poller, long factory)
    {
        super(operatorId, planNodeId, "GpuNestedLoopBuildOperator", inputTypes, poller, factory);
    }

    @Override
    public Operator createOperator(DriverContext driverContext)
    {
        if (closed) {
            throw new IllegalStateException("Factory is already closed");
        }
        OperatorContext operatorContext = driverContext.addOperatorContext(operatorId, planNodeId, operatorType);
        try {
            return new GpuNestedLoopBuildOperator(operatorContext, GpuNative.createOperator(factory), inputTypes, poller);
        }
        catch (GpuNative.NativeError e) {
            throw GpuNative.toTrinoException(e);
        }
    }

    public static class GpuNestedLoopBuildOperator
            extends GpuOperator
    {
        GpuNestedLoopBuildOperator(OperatorContext operatorContext, long handle, List<Type> inputTypes, ScheduledExecutorService poller)
        {
            super(operatorContext, handle, inputTypes, poller);
        }

        @Override
        public void addInput(Page page)
        {
            super.addInput(page);
            if (page.getPositionCount() > 0) {
                // operatorContext.recordOutput(page.getSizeInBytes(), page.getPositionCount()) (NestedLoopBuildOperator.java:139)
                getOperatorContext().recordOutput(page.getSizeInBytes(), page.getPositionCount());
            }
        }
    }
}

// window.h -- window functions over a sorted pages index in HBM: what WindowOperator computes at get_output.
// Reference: M/operator/WindowOperator.java:205-310,844-855 and the row loop of M/operator/window/WindowPartition.java:184-214 (peer groups
// :238-247, frames :281-345) over the functions of M/operator/window/.  Nothing is ported: partitions, peers and every running value come out of
// one segmented scan over the sorted order (window.hip).
#pragma once

#include "common.h"

namespace tgpu {

struct WindowFunctionSpec {
    int32_t function = 0, agg_function = 0, frame = 0;
    std::vector<int32_t> argument_channels;
    int32_t ignore_nulls = 0;
    // tgpu_window_factory_create_framed: `frame` is not read, the five fields below are the frame (tgpu_window_frame_spec).  The constructor turns
    // the three frames the old entry point knows back into their `frame` code (general = 0), so that they take the old path bit for bit.
    int32_t general = 0;
    int32_t frame_type = 0, start_type = 0, start_channel = -1, end_type = 0, end_channel = -1;
    // tgpu_window_factory_create_ranged: a RANGE frame may have PRECEDING / FOLLOWING bounds; start_channel / end_channel then hold the bound VALUE
    // and the two fields below the comparison key (tgpu_window_range_frame_spec).  Not read for any other frame.
    int32_t ranged = 0;
    int32_t start_sort_key_channel = -1, end_sort_key_channel = -1;
};

class WindowGpu {
public:
    static constexpr int kBlock = 256;             // threads of a scan workgroup = rows of one block scan
    static constexpr int64_t kTileRows = 2048;     // rows per workgroup of the scan's launches 1 and 3 (TGPU_WINDOW_TILE_ROWS replaces it)
    static constexpr int kAggsPerLaunch = 4;       // running aggregates one scan carries in registers; more functions: the scan runs again

    WindowGpu(Context *ctx, std::vector<int32_t> types, std::vector<WindowFunctionSpec> functions, std::vector<int32_t> partition_channels,
              std::vector<int32_t> sort_channels, std::vector<int32_t> sort_orders);
    // TGPU_ERR_INVALID_ARGUMENT / TGPU_ERR_NOT_SUPPORTED for whatever tgpu.h rules out (no device work)
    static void validate(const std::vector<int32_t> &types, const std::vector<WindowFunctionSpec> &functions, const std::vector<int32_t> &partition_channels,
                         const std::vector<int32_t> &sort_channels, const std::vector<int32_t> &sort_orders);
    void set_tile_rows(int64_t rows) { tile_rows_ = rows; }

    // `all` = every source channel of the whole input.  *positions = its rows in output order (null: arrival order, nothing was sorted);
    // the result = one column per function, in output order.  Raises the sum overflow / negative offset errors.
    std::vector<DeviceColumn> evaluate(const DevicePage &all, BufferPtr *positions);
    int64_t scratch_bytes() const { return scratch_bytes_; }   // positions + scan arrays + frame arrays + range-extreme index + RANGE search arrays of the last evaluate()

private:
    Context *ctx_;
    std::vector<int32_t> types_;
    std::vector<WindowFunctionSpec> functions_;
    std::vector<int32_t> partition_channels_, sort_channels_, sort_orders_;
    int64_t tile_rows_ = kTileRows, scratch_bytes_ = 0;
};

}  // namespace tgpu

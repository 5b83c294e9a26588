"""Host-side mirror of the reference's operator API over the C ABI (include/tgpu.h).

Same names and call protocol as io.trino.operator.Operator / OperatorFactory (M/operator/Operator.java:20-102,
OperatorFactory.java:18-50) so parity tests read like the reference's own operator tests
(T/operator/TestHashAggregationOperator.java, TestHashJoinOperator.java, TestFilterAndProjectOperator.java).
Everything here is a thin wrapper: the state machines live in csrc/operators.cpp, the work in the HIP kernels.
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from . import expressions as _expr
from .expressions import FlatProgram
from .spi import OutputPage, Page

COUNT_ALL, COUNT_COLUMN, SUM_BIGINT, SUM_DOUBLE, AVG_BIGINT, AVG_DOUBLE, MIN_BIGINT, MAX_BIGINT, MIN_DOUBLE, MAX_DOUBLE = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
MIN_INTEGER, MAX_INTEGER, MIN_DATE, MAX_DATE = 11, 12, 13, 14   # min / max over int32-stored types: output of the input's type, BIGINT intermediate
MIN_TIMESTAMP, MAX_TIMESTAMP = 17, 18                           # min / max over int64 microseconds: output TIMESTAMP, BIGINT intermediate
MIN_VARCHAR, MAX_VARCHAR = 15, 16                               # plain hash aggregation only; PARTIAL: count BIGINT, value VARCHAR
SINGLE, PARTIAL, FINAL = 0, 1, 2
# S/connector/SortOrder.java:18-21
ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST = 0, 1, 2, 3
INNER, PROBE_OUTER, LOOKUP_OUTER, FULL_OUTER = 0, 1, 2, 3   # LookupJoinOperators.JoinType ordinals
SUM_ORDER_EXACT, SUM_ORDER_JAVA = 0, 1                      # tgpu_double_sum_order


def _i32(seq):
    seq = list(seq)
    return (C.c_int32 * max(1, len(seq)))(*seq), len(seq)


class Context:
    """One HIP device + stream (tgpu_context).  stream: a hipStream_t address (e.g. torch.cuda.current_stream().cuda_stream)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_context_create(device, stream, C.byref(h)))
        self.handle = h

    def synchronize(self):
        _lib.check(_lib.lib().tgpu_context_synchronize(self.handle))

    def pinned_array(self, dtype, count):
        """a numpy array over page-locked host memory (tgpu_pinned_alloc): blocks built on it are transferred by asynchronous DMA;
        the array keeps the allocation alive and frees it with the context still open (call .base.free() or let it be collected)"""
        dt = np.dtype(dtype)
        p = C.c_void_p()
        _lib.check(_lib.lib().tgpu_pinned_alloc(self.handle, int(count) * dt.itemsize, C.byref(p)))
        ctx_handle = self.handle

        class _Pinned:
            def __init__(self):
                self.ptr = p.value
                self.__array_interface__ = {"shape": (int(count),), "typestr": dt.str, "data": (p.value, False), "version": 3}

            def free(self):
                if self.ptr:
                    _lib.lib().tgpu_pinned_free(ctx_handle, self.ptr)
                    self.ptr = None

        holder = _Pinned()
        return np.asarray(holder), holder

    def set_max_output_page(self, max_bytes=0, max_rows=0):
        """operators hand pages larger than this out as consecutive regions (PageBuilder.isFull granularity for Java consumers); 0 = no limit"""
        _lib.check(_lib.lib().tgpu_context_set_max_output_page(self.handle, int(max_bytes), int(max_rows)))

    def set_double_sum_order(self, order):
        """SUM_ORDER_EXACT (default) or SUM_ORDER_JAVA for the aggregation operators created from now on (tgpu.h)"""
        _lib.check(_lib.lib().tgpu_context_set_double_sum_order(self.handle, order))

    def set_device_input_stable(self, stable=True):
        """the promise of tgpu_context_set_device_input_stable: borrowed device blocks stay valid and unchanged until the operator they were given to has finished"""
        _lib.check(_lib.lib().tgpu_context_set_device_input_stable(self.handle, int(bool(stable))))

    def profile_enable(self, on=True):
        _lib.check(_lib.lib().tgpu_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        _lib.check(_lib.lib().tgpu_profile_reset(self.handle))

    def profile(self):
        L = _lib.lib()
        need = L.tgpu_profile_dump(self.handle, None, 0)
        buf = C.create_string_buffer(int(need))
        L.tgpu_profile_dump(self.handle, buf, need)
        return json.loads(buf.value.decode())

    def hash_page(self, page: Page, channels):
        ch, n = _i32(channels)
        out = np.zeros(max(page.position_count, 1), dtype=np.int64)
        cp, keep = page.to_c()
        _lib.check(_lib.lib().tgpu_hash_page(self.handle, C.byref(cp), n, ch, out.ctypes.data))
        return out[: page.position_count]

    def partition_page(self, page: Page, key_channels, partition_count, hash_channel=-1):
        ch, n = _i32(key_channels)
        counts = np.zeros(partition_count, dtype=np.int64)
        out = C.c_void_p()
        cp, keep = page.to_c()
        _lib.check(_lib.lib().tgpu_partition_page(self.handle, C.byref(cp), n, ch, hash_channel, partition_count, counts.ctypes.data, C.byref(out)))
        return counts, OutputPage(out)

    def serialize_page(self, page: Page, into=None):
        """PagesSerde.serialize + writeSerializedPage (M/execution/buffer/PagesSerde.java:64-115): the page as the reference's wire
        bytes.  `into` (a uint8 numpy buffer, e.g. a reused exchange buffer): written in place, returns the byte count."""
        cp, keep = page.to_c()
        need = C.c_int64()
        if into is not None:
            _lib.check(_lib.lib().tgpu_serialize_page(self.handle, C.byref(cp), into.ctypes.data, into.size, C.byref(need)))
            return int(need.value)
        _lib.check(_lib.lib().tgpu_serialize_page(self.handle, C.byref(cp), None, 0, C.byref(need)))
        buf = np.empty(max(int(need.value), 1), dtype=np.uint8)
        _lib.check(_lib.lib().tgpu_serialize_page(self.handle, C.byref(cp), buf.ctypes.data, buf.size, C.byref(need)))
        return buf[: need.value].tobytes()

    def deserialize_page(self, data: bytes, types):
        """PagesSerde.deserialize (PagesSerde.java:117-160) into a device-resident OutputPage; `types` = channel types"""
        t, n = _i32(types)
        raw = np.frombuffer(data, dtype=np.uint8)
        out = C.c_void_p()
        _lib.check(_lib.lib().tgpu_deserialize_page(self.handle, raw.ctypes.data, raw.size, n, t, C.byref(out)))
        return OutputPage(out)

    def close(self):
        if self.handle:
            _lib.lib().tgpu_context_destroy(self.handle)
            self.handle = None


class Operator:
    def __init__(self, handle):
        self.handle = handle

    def needsInput(self):
        return bool(_lib.check(_lib.lib().tgpu_operator_needs_input(self.handle)))

    def addInput(self, page):
        if isinstance(page, OutputPage):   # a page of this library: buffers shared, nothing copied (tgpu_operator_add_input_output_page)
            _lib.check(_lib.lib().tgpu_operator_add_input_output_page(self.handle, page.handle))
            return
        cp, keep = page.to_c()
        _lib.check(_lib.lib().tgpu_operator_add_input(self.handle, C.byref(cp)))

    def getOutput(self):
        out = C.c_void_p()
        self.last_get_output_status = _lib.check(_lib.lib().tgpu_operator_get_output(self.handle, C.byref(out)))   # 1 = TGPU_WOULD_BLOCK
        return OutputPage(out) if out.value else None

    def startMemoryRevoke(self):
        _lib.check(_lib.lib().tgpu_operator_start_memory_revoke(self.handle))

    def finishMemoryRevoke(self):
        _lib.check(_lib.lib().tgpu_operator_finish_memory_revoke(self.handle))

    def revocableMemoryBytes(self):
        """OperatorContext.getReservedRevocableBytes()"""
        return int(_lib.lib().tgpu_operator_revocable_memory_bytes(self.handle))

    def spillStats(self):
        """(spills so far, host bytes spilled)"""
        n, b = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tgpu_operator_spill_stats(self.handle, C.byref(n), C.byref(b)))
        return n.value, b.value

    def finish(self):
        _lib.check(_lib.lib().tgpu_operator_finish(self.handle))

    def isFinished(self):
        return bool(_lib.check(_lib.lib().tgpu_operator_is_finished(self.handle)))

    def isBlocked(self):
        return bool(_lib.check(_lib.lib().tgpu_operator_is_blocked(self.handle)))

    def memoryBytes(self):
        return _lib.lib().tgpu_operator_memory_bytes(self.handle)

    def close(self):
        if self.handle:
            _lib.lib().tgpu_operator_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # a constructor that failed before `handle` existed, or interpreter shutdown
            pass


class OperatorFactory:
    def __init__(self, handle, keep=None):
        self.handle = handle
        self._keep = keep

    def createOperator(self):
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_operator_factory_create_operator(self.handle, C.byref(h)))
        return Operator(h)

    def noMoreOperators(self):
        _lib.check(_lib.lib().tgpu_operator_factory_no_more_operators(self.handle))

    def setMaxPartialMemory(self, nbytes):
        """maxPartialMemory of HashAggregationOperatorFactory (M/operator/HashAggregationOperator.java:128-131), for operators created afterwards"""
        _lib.check(_lib.lib().tgpu_hash_aggregation_factory_set_max_partial_memory(self.handle, int(nbytes)))

    def setSpillEnabled(self, on=True):
        """spillEnabled of HashAggregationOperatorFactory (M/operator/HashAggregationOperator.java:133), for operators created afterwards;
        hash aggregation factories only (NOT_SUPPORTED otherwise)"""
        _lib.check(_lib.lib().tgpu_hash_aggregation_factory_set_spill_enabled(self.handle, int(on)))

    def duplicate(self):
        """OperatorFactory.duplicate() (M/operator/OperatorFactory.java:49)"""
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_operator_factory_duplicate(self.handle, C.byref(h)))
        dup = type(self).__new__(type(self))
        OperatorFactory.__init__(dup, h, self._keep)
        for k, v in self.__dict__.items():
            if k not in ("handle", "_keep"):
                setattr(dup, k, v)
        return dup

    def close(self):
        if self.handle:
            _lib.lib().tgpu_operator_factory_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # a constructor that failed before `handle` existed, or interpreter shutdown
            pass


class FilterAndProjectOperatorFactory(OperatorFactory):
    """FilterAndProjectOperator.createOperatorFactory (M/operator/FilterAndProjectOperator.java:73-88): the PageProcessor
    (filter + projections as RowExpressions) is compiled into one fused gfx950 kernel pair."""

    def __init__(self, ctx: Context, operator_id, input_types, filter_expr, projections):
        self.program = FlatProgram(filter_expr, projections)
        spec, keep = self.program.to_c()
        types, n = _i32(input_types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_filter_project_factory_create(ctx.handle, operator_id, n, types, C.byref(spec), C.byref(h)))
        super().__init__(h, keep)


class PageSource:
    """a ConnectorPageSource (S/connector/ConnectorPageSource.java) over Python pages, as the callbacks of tgpu_page_source"""

    def __init__(self, pages, blocked_polls=0):
        self.pages = list(pages)
        self.at = 0
        self.blocked_polls = blocked_polls      # isBlocked() reports "not done" this many times first
        self.current = None
        self.closed = False
        self._keep = None
        self._load_keep = []
        self.error = None
        self.struct = _lib.PageSource(None, _lib.SOURCE_NEXT_FN(self._next), _lib.SOURCE_FLAG_FN(self._finished), _lib.SOURCE_FLAG_FN(self._blocked),
                                      _lib.SOURCE_LOAD_FN(self._load), _lib.SOURCE_CLOSE_FN(self._close))

    def _next(self, user, out):
        try:
            if self.at >= len(self.pages):
                return 0
            self.current = self.pages[self.at]
            self.at += 1
            self._load_keep = []
            cp, self._keep = self.current.to_c()   # valid until the next call
            out[0].position_count, out[0].channel_count, out[0].blocks = cp.position_count, cp.channel_count, cp.blocks
            return 1
        except Exception as e:   # must not unwind through the C frames
            self.error = e
            return -1

    def _finished(self, user):
        return 1 if self.at >= len(self.pages) else 0

    def _blocked(self, user):
        if self.blocked_polls > 0:
            self.blocked_polls -= 1
            return 1
        return 0

    def _load(self, user, channel, out):
        try:
            blk = self.current.blocks[channel].load()
            blk._fill(out[0], self._load_keep)
            return 0
        except Exception as e:
            self.error = e
            return -1

    def _close(self, user):
        self.closed = True


class RecordCursor:
    """a RecordCursor (S/connector/RecordCursor.java) over Python rows (tuples; None = null), as the callbacks of tgpu_record_cursor"""

    def __init__(self, types, rows):
        self.types = list(types)
        self.rows = list(rows)
        self.at = -1
        self.closed = False
        self.error = None
        self._slice_keep = None
        self.struct = _lib.RecordCursor(None, _lib.SOURCE_FLAG_FN(self._advance), _lib.CURSOR_FIELD_FN(self._is_null), _lib.CURSOR_FIELD_FN(self._boolean),
                                        _lib.CURSOR_LONG_FN(self._long), _lib.CURSOR_DOUBLE_FN(self._double), _lib.CURSOR_SLICE_FN(self._slice),
                                        _lib.CURSOR_BYTES_FN(self._bytes), _lib.SOURCE_CLOSE_FN(self._close))

    def _advance(self, user):
        self.at += 1
        return 1 if self.at < len(self.rows) else 0

    def _is_null(self, user, field):
        return 1 if self.rows[self.at][field] is None else 0

    def _boolean(self, user, field):
        return 1 if self.rows[self.at][field] else 0

    def _long(self, user, field):
        return int(self.rows[self.at][field])

    def _double(self, user, field):
        return float(self.rows[self.at][field])

    def _slice(self, user, field, out_bytes, out_len):
        try:
            v = self.rows[self.at][field]
            b = v.encode("utf-8") if isinstance(v, str) else bytes(v)
            self._slice_keep = C.create_string_buffer(b, len(b)) if b else None   # valid until the next advance
            out_bytes[0] = C.cast(self._slice_keep, C.c_void_p).value if b else None
            out_len[0] = len(b)
            return 0
        except Exception as e:   # must not unwind through the C frames
            self.error = e
            return -1

    def _bytes(self, user):
        return 0

    def _close(self, user):
        self.closed = True


class ScanOperator(Operator):
    def addSplit(self, source):
        """SourceOperator.addSplit: the split's page source (PageSource) or record cursor (RecordCursor)"""
        self._sources = getattr(self, "_sources", []) + [source]
        if isinstance(source, RecordCursor):
            t, n = _i32(source.types)
            _lib.check(_lib.lib().tgpu_scan_operator_add_record_cursor(self.handle, C.byref(source.struct), n, t))
            return
        _lib.check(_lib.lib().tgpu_scan_operator_add_page_source(self.handle, C.byref(source.struct)))

    def noMoreSplits(self):
        _lib.check(_lib.lib().tgpu_scan_operator_no_more_splits(self.handle))

    def stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tgpu_scan_operator_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"processedPositions": a.value, "lazyBlocksLoaded": b.value, "lazyBlocksSkipped": c.value}


class ScanFilterAndProjectOperatorFactory(OperatorFactory):
    """ScanFilterAndProjectOperator.ScanFilterAndProjectOperatorFactory (M/operator/ScanFilterAndProjectOperator.java:449-560), page-source flavour"""

    def __init__(self, ctx: Context, operator_id, types, filter_expr, projections):
        self.program = FlatProgram(filter_expr, projections)
        spec, keep = self.program.to_c()
        t, n = _i32(types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_scan_filter_project_factory_create(ctx.handle, operator_id, n, t, C.byref(spec), C.byref(h)))
        super().__init__(h, keep)

    def createOperator(self):
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_operator_factory_create_operator(self.handle, C.byref(h)))
        return ScanOperator(h)


class MergeOperator(Operator):
    """MergeOperator (M/operator/MergeOperator.java:109-256): a source operator over sorted page streams"""

    def addSplit(self, source: PageSource):
        """SourceOperator.addSplit (:155-177): one sorted stream, as a PageSource (its load callback is never used)"""
        self._sources = getattr(self, "_sources", []) + [source]   # the callbacks must outlive the operator
        _lib.check(_lib.lib().tgpu_merge_operator_add_page_source(self.handle, C.byref(source.struct)))

    def noMoreSplits(self):
        _lib.check(_lib.lib().tgpu_merge_operator_no_more_splits(self.handle))


class MergeOperatorFactory(OperatorFactory):
    """MergeOperator.MergeOperatorFactory (M/operator/MergeOperator.java:47-107): the k-way merge of sorted streams (MergeSortedPages);
    rows that compare equal come out lower stream first, inside a stream in arrival order"""

    def __init__(self, ctx: Context, operator_id, types, output_channels, sort_channels, sort_orders):
        t, n = _i32(types)
        oc, no = _i32(output_channels)
        sc, ns = _i32(sort_channels)
        so, _ = _i32(sort_orders)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_merge_factory_create(ctx.handle, operator_id, n, t, no, oc, ns, sc, so, C.byref(h)))
        super().__init__(h)

    def createOperator(self):
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_operator_factory_create_operator(self.handle, C.byref(h)))
        return MergeOperator(h)


def precompile_page_processor(input_types, filter_expr, projections):
    """Compile the kernels of a page processor into the on-disk cache (no GPU needed)."""
    prog = FlatProgram(filter_expr, projections)
    spec, keep = prog.to_c()
    types, n = _i32(input_types)
    _lib.check(_lib.lib().tgpu_precompile_page_processor(n, types, C.byref(spec)))


def page_processor_source(input_types, filter_expr, projections):
    prog = FlatProgram(filter_expr, projections)
    spec, keep = prog.to_c()
    types, n = _i32(input_types)
    L = _lib.lib()
    need = _lib.check(L.tgpu_page_processor_source(n, types, C.byref(spec), None, 0))
    buf = C.create_string_buffer(int(need))
    L.tgpu_page_processor_source(n, types, C.byref(spec), buf, need)
    return buf.value.decode()


class HashAggregationOperatorFactory(OperatorFactory):
    """M/operator/HashAggregationOperator.java:54-262.  aggs: list of (function, input_channel, mask_channel)."""

    def __init__(self, ctx: Context, operator_id, group_by_types, group_by_channels, aggs, step=SINGLE, hash_channel=-1,
                 expected_groups=10_000, produce_default_output=False, spill_enabled=False):
        gt, ng = _i32(group_by_types)
        gc, _ = _i32(group_by_channels)
        arr = (_lib.AggSpec * max(1, len(aggs)))()
        for i, a in enumerate(aggs):
            f, ch = a[0], a[1]
            arr[i] = _lib.AggSpec(f, ch, a[2] if len(a) > 2 else -1)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_hash_aggregation_factory_create(ctx.handle, operator_id, ng, gt, gc, hash_channel, step, len(aggs), arr,
                                                                   expected_groups, int(produce_default_output), C.byref(h)))
        super().__init__(h)
        if spill_enabled:
            self.setSpillEnabled(True)


class StreamingAggregationOperatorFactory(OperatorFactory):
    """StreamingAggregationOperator.createOperatorFactory (M/operator/StreamingAggregationOperator.java:50-69): aggregation over input that
    arrives grouped on the keys.  types: the source types; aggs: list of (function, input_channel[, mask_channel]).  Output: the keys, then
    the aggregates in HashAggregationOperatorFactory's layouts, one row per run of not-distinct key rows, in stream order."""

    def __init__(self, ctx: Context, operator_id, types, group_by_channels, step, aggs):
        t, nt = _i32(types)
        gc, ng = _i32(group_by_channels)
        if ng == 0:   # (the library says the same; said here, it needs neither the library nor a device)
            raise _lib.TgpuError(-1, "streaming aggregation needs at least one group-by channel (a global aggregation stays with the hash operator)")
        arr = (_lib.AggSpec * max(1, len(aggs)))()
        for i, a in enumerate(aggs):
            arr[i] = _lib.AggSpec(a[0], a[1], a[2] if len(a) > 2 else -1)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_streaming_aggregation_factory_create(ctx.handle, operator_id, nt, t, ng, gc, step, len(aggs), arr, C.byref(h)))
        super().__init__(h)


class LookupSourceFactory:
    """The JoinBridge between the build and probe pipelines (M/operator/PartitionedLookupSourceFactory.java)."""

    def __init__(self, handle):
        self.handle = handle

    def setJoinFilter(self, probe_types, filter_expr):
        """JoinFilterFunction (M/operator/JoinHash.java:44-47,118-130): `filter_expr` over (build channels..., probe channels...)"""
        prog = FlatProgram(filter_expr, [])
        spec, keep = prog.to_c()
        t, nt = _i32(probe_types)
        _lib.check(_lib.lib().tgpu_lookup_source_factory_set_join_filter(self.handle, nt, t, C.byref(spec)))

    def stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tgpu_lookup_source_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return dict(positions=a.value, hash_size=b.value, link_count=c.value)

    def close(self):
        if self.handle:
            _lib.lib().tgpu_lookup_source_factory_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # a constructor that failed before `handle` existed, or interpreter shutdown
            pass


class HashBuilderOperatorFactory(OperatorFactory):
    """M/operator/HashBuilderOperator.java:54-152.  `lookup_source_factory` is the bridge to hand to the probe factory."""

    def __init__(self, ctx: Context, operator_id, types, output_channels, hash_channels, precomputed_hash_channel=-1, expected_positions=100, partition_count=1):
        """partition_count > 1: createOperator() hands out that many build operators, one per local-exchange partition
        (PartitionedLookupSourceFactory.java:110-124)"""
        t, nt = _i32(types)
        oc, no = _i32(output_channels)
        hc, nh = _i32(hash_channels)
        bridge, h = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().tgpu_partitioned_hash_builder_factory_create(ctx.handle, operator_id, nt, t, no, oc, nh, hc, precomputed_hash_channel,
                                                                           expected_positions, partition_count, C.byref(bridge), C.byref(h)))
        super().__init__(h)
        self.lookup_source_factory = LookupSourceFactory(bridge)


class LookupJoinOperatorFactory(OperatorFactory):
    """LookupJoinOperators.innerJoin / probeOuterJoin (M/operator/LookupJoinOperators.java:30-63)."""

    def __init__(self, ctx: Context, operator_id, lookup_source_factory: LookupSourceFactory, probe_types, probe_join_channels,
                 probe_hash_channel=-1, probe_output_channels=None, join_type=INNER):
        if probe_output_channels is None:
            probe_output_channels = list(range(len(probe_types)))
        t, nt = _i32(probe_types)
        jc, nj = _i32(probe_join_channels)
        oc, no = _i32(probe_output_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_lookup_join_factory_create(ctx.handle, operator_id, lookup_source_factory.handle, nt, t, nj, jc,
                                                              probe_hash_channel, no, oc, join_type, C.byref(h)))
        super().__init__(h)
        self._bridge = lookup_source_factory


class LookupOuterOperatorFactory(OperatorFactory):
    """LookupOuterOperator.LookupOuterOperatorFactory (M/operator/LookupOuterOperator.java:35-110): the unmatched build rows of a
    LOOKUP_OUTER / FULL_OUTER join, after every probe operator has finished"""

    def __init__(self, ctx: Context, operator_id, lookup_source_factory: LookupSourceFactory, probe_output_types):
        t, nt = _i32(probe_output_types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_lookup_outer_factory_create(ctx.handle, operator_id, lookup_source_factory.handle, nt, t, C.byref(h)))
        super().__init__(h)
        self._bridge = lookup_source_factory


class FilterProjectLookupJoinOperatorFactory(OperatorFactory):
    """FilterAndProjectOperator fused into the LookupJoin probe (one generated kernel); same results as the two reference
    operators back to back.  probe_join_channels / probe_output_channels index the page processor's projections."""

    def __init__(self, ctx: Context, operator_id, lookup_source_factory: LookupSourceFactory, input_types, filter_expr, projections,
                 probe_join_channels, probe_hash_channel=-1, probe_output_channels=None, join_type=INNER):
        if probe_output_channels is None:
            probe_output_channels = list(range(len(projections)))
        self.program = FlatProgram(filter_expr, projections)
        spec, keep = self.program.to_c()
        t, nt = _i32(input_types)
        jc, nj = _i32(probe_join_channels)
        oc, no = _i32(probe_output_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_filter_project_lookup_join_factory_create(ctx.handle, operator_id, lookup_source_factory.handle, nt, t, C.byref(spec),
                                                                             nj, jc, probe_hash_channel, no, oc, join_type, C.byref(h)))
        super().__init__(h, keep)
        self._bridge = lookup_source_factory


def _agg_array(aggs):
    arr = (_lib.AggSpec * max(1, len(aggs)))()
    for i, a in enumerate(aggs):
        arr[i] = _lib.AggSpec(a[0], a[1], a[2] if len(a) > 2 else -1)
    return arr


class TopNOperatorFactory(OperatorFactory):
    """TopNOperator.createOperatorFactory (M/operator/TopNOperator.java:47-62): the n first rows in the order of the sort channels."""

    def __init__(self, ctx: Context, operator_id, types, n, sort_channels, sort_orders):
        t, nt = _i32(types)
        sc, ns = _i32(sort_channels)
        so, no = _i32(sort_orders)
        assert ns == no, "sort channels and sort orders differ in length"
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_top_n_factory_create(ctx.handle, operator_id, nt, t, int(n), ns, sc, so, C.byref(h)))
        super().__init__(h)


class OrderByOperatorFactory(OperatorFactory):
    """OrderByOperator.OrderByOperatorFactory (M/operator/OrderByOperator.java:48-131): all rows in the order of the sort channels."""

    def __init__(self, ctx: Context, operator_id, types, output_channels, expected_positions, sort_channels, sort_orders):
        t, nt = _i32(types)
        oc, no = _i32(output_channels)
        sc, ns = _i32(sort_channels)
        so, nso = _i32(sort_orders)
        assert ns == nso, "sort channels and sort orders differ in length"
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_order_by_factory_create(ctx.handle, operator_id, nt, t, no, oc, expected_positions, ns, sc, so, C.byref(h)))
        super().__init__(h)


class FilterProjectHashAggregationOperatorFactory(OperatorFactory):
    """FilterAndProjectOperator fused into HashAggregationOperator (HandTpchQuery1's pipeline shape): group_by_channels and the
    aggregates' channels index the page processor's projections; same results as the two reference operators back to back."""

    def __init__(self, ctx: Context, operator_id, input_types, filter_expr, projections, group_by_types, group_by_channels, aggs, step=SINGLE,
                 hash_channel=-1, expected_groups=10_000):
        self.program = FlatProgram(filter_expr, projections)
        spec, keep = self.program.to_c()
        t, nt = _i32(input_types)
        gt, ng = _i32(group_by_types)
        gc, _ = _i32(group_by_channels)
        arr = _agg_array(aggs)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_filter_project_hash_aggregation_factory_create(ctx.handle, operator_id, nt, t, C.byref(spec), ng, gt, gc, hash_channel, step,
                                                                                  len(aggs), arr, expected_groups, C.byref(h)))
        super().__init__(h, keep)


def precompile_fused_aggregation(input_types, filter_expr, projections, aggs, group_by_channels=()):
    prog = FlatProgram(filter_expr, projections)
    spec, keep = prog.to_c()
    t, nt = _i32(input_types)
    arr = _agg_array(aggs)
    gc, ng = _i32(group_by_channels)
    _lib.check(_lib.lib().tgpu_precompile_fused_aggregation(nt, t, C.byref(spec), len(aggs), arr, ng, gc))


def precompile_fused_probe(input_types, filter_expr, projections, join_channel, probe_output_channels):
    prog = FlatProgram(filter_expr, projections)
    spec, keep = prog.to_c()
    t, nt = _i32(input_types)
    oc, no = _i32(probe_output_channels)
    _lib.check(_lib.lib().tgpu_precompile_fused_probe(nt, t, C.byref(spec), join_channel, no, oc))


def fused_probe_launch_counts():
    """(two-pass gather, full carry, partial carry): fused probe launches prepared so far in this process, by carry mode"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.lib().tgpu_fused_probe_launch_counts(out))
    return tuple(int(v) for v in out)


def fused_probe_depth_counts():
    """(depth 1, depth 2): fused probe launches prepared so far in this process, by the row sets pass 1 keeps in flight (jit.cpp FJ_DEPTH)"""
    out = (C.c_int64 * 2)()
    _lib.check(_lib.lib().tgpu_fused_probe_depth_counts(out))
    return tuple(int(v) for v in out)


class GroupByHash:
    """GroupByHash.createGroupByHash (M/operator/GroupByHash.java:45-59) over the GPU table."""

    def __init__(self, ctx: Context, types, hash_channels, input_hash_channel=None, expected_size=100):
        t, n = _i32(types)
        hc, _ = _i32(hash_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_group_by_hash_create(ctx.handle, n, t, hc, -1 if input_hash_channel is None else input_hash_channel,
                                                        expected_size, C.byref(h)))
        self.handle = h

    def addPage(self, page: Page):
        cp, keep = page.to_c()
        _lib.check(_lib.lib().tgpu_group_by_hash_add_page(self.handle, C.byref(cp)))

    def getGroupIds(self, page: Page):
        out = np.zeros(max(page.position_count, 1), dtype=np.int64)
        gc = C.c_int64()
        cp, keep = page.to_c()
        _lib.check(_lib.lib().tgpu_group_by_hash_get_group_ids(self.handle, C.byref(cp), out.ctypes.data, C.byref(gc)))
        return out[: page.position_count]

    def contains(self, position, page: Page):
        r = C.c_int32()
        cp, keep = page.to_c()
        _lib.check(_lib.lib().tgpu_group_by_hash_contains(self.handle, position, C.byref(cp), C.byref(r)))
        return bool(r.value)

    def getGroupCount(self):
        return _lib.lib().tgpu_group_by_hash_group_count(self.handle)

    def getCapacity(self):
        return _lib.lib().tgpu_group_by_hash_capacity(self.handle)

    def getRehashCount(self):
        return _lib.lib().tgpu_group_by_hash_rehash_count(self.handle)

    def getEstimatedSize(self):
        return _lib.lib().tgpu_group_by_hash_estimated_size(self.handle)

    def appendValues(self) -> Page:
        out = C.c_void_p()
        _lib.check(_lib.lib().tgpu_group_by_hash_append_values(self.handle, C.byref(out)))
        op = OutputPage(out)
        pg = op.to_host()
        op.release()
        return pg

    def appendValuesDevice(self) -> OutputPage:
        """appendValuesTo for every group, left on the device (the caller releases the page)"""
        out = C.c_void_p()
        _lib.check(_lib.lib().tgpu_group_by_hash_append_values(self.handle, C.byref(out)))
        return OutputPage(out)

    def close(self):
        if self.handle:
            _lib.lib().tgpu_group_by_hash_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # a constructor that failed before `handle` existed, or interpreter shutdown
            pass


def to_pages(operator: Operator, input_pages, to_host=True):
    """The reference's mini driver loop, T/operator/OperatorAssertion.java:82-137 (toPages)."""
    outputs = []
    it = iter(input_pages)
    pending = next(it, None)
    loops = 0
    while pending is not None and loops < 10_000_000:
        loops += 1
        if operator.isBlocked():
            raise RuntimeError("operator is blocked")
        if operator.needsInput():
            operator.addInput(pending)
            pending = next(it, None)
        out = operator.getOutput()
        if out is not None and out.position_count > 0:
            outputs.append(out)
    operator.finish()
    loops = 0
    while not operator.isFinished() and loops < 1_000_000:
        loops += 1
        out = operator.getOutput()
        if out is not None and out.position_count > 0:
            outputs.append(out)
    assert operator.isFinished() and not operator.needsInput() and not operator.isBlocked()
    if not to_host:
        return outputs
    host = [o.to_host() for o in outputs]
    for o in outputs:
        o.release()
    return host


DF_ALL, DF_VALUES, DF_RANGE, DF_NONE = 0, 1, 2, 3


class DynamicFilterSourceOperator(Operator):
    def domain(self, filter_channel):
        """after finish(): ("all",) | ("values", [..]) | ("range", lo, hi) | ("none",) -- DynamicFilterSourceOperator.finish() (:383-424)"""
        kind, out, lo, hi = C.c_int32(), C.c_void_p(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tgpu_dynamic_filter_source_result(self.handle, filter_channel, C.byref(kind), C.byref(out), C.byref(lo), C.byref(hi)))
        if kind.value == DF_VALUES:
            page = OutputPage(out)
            vals = page.to_host().blocks[0].to_list() if page.position_count else []
            page.release()
            return ("values", vals)
        if kind.value == DF_RANGE and out.value:      # a VARCHAR channel: two rows, min then max
            page = OutputPage(out)
            vals = page.to_host().blocks[0].to_list()
            page.release()
            return ("range", vals[0], vals[1])
        return {DF_ALL: ("all",), DF_RANGE: ("range", int(lo.value), int(hi.value)), DF_NONE: ("none",)}[kind.value]


class DynamicFilterSourceOperatorFactory(OperatorFactory):
    """DynamicFilterSourceOperator.DynamicFilterSourceOperatorFactory (M/operator/DynamicFilterSourceOperator.java:74-143)"""

    def __init__(self, ctx: Context, operator_id, types, channels, max_distinct_values, max_filter_size_in_bytes, min_max_collection_limit):
        t, nt = _i32(types)
        ch, nc = _i32(channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_dynamic_filter_source_factory_create(ctx.handle, operator_id, nt, t, nc, ch, int(max_distinct_values), int(max_filter_size_in_bytes),
                                                                        int(min_max_collection_limit), C.byref(h)))
        super().__init__(h)

    def createOperator(self):
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_operator_factory_create_operator(self.handle, C.byref(h)))
        return DynamicFilterSourceOperator(h)


SET_BITMAP, SET_HASH, SET_GENERIC = 0, 1, 2   # tgpu_set_supplier_stats layouts


class SetSupplier:
    """SetBuilderOperator.SetSupplier (M/operator/SetBuilderOperator.java:39-90): the bridge from the set builder to the semi join probes."""

    def __init__(self, handle):
        self.handle = handle

    def stats(self):
        """valid once the builder finished: size (distinct keys, a null counted: ChannelSet.size), contains_null, HBM bytes, layout"""
        size, cn, nbytes, layout = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int32()
        _lib.check(_lib.lib().tgpu_set_supplier_stats(self.handle, C.byref(size), C.byref(cn), C.byref(nbytes), C.byref(layout)))
        return dict(size=size.value, contains_null=bool(cn.value), bytes=nbytes.value, layout=layout.value)

    def close(self):
        if self.handle:
            _lib.lib().tgpu_set_supplier_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # a constructor that failed before `handle` existed, or interpreter shutdown
            pass


class SetBuilderOperatorFactory(OperatorFactory):
    """SetBuilderOperator.SetBuilderOperatorFactory (M/operator/SetBuilderOperator.java:92-135).  `set_supplier` is the bridge to hand
    to the HashSemiJoinOperatorFactory."""

    def __init__(self, ctx: Context, operator_id, types, set_channel, hash_channel=-1, expected_positions=10_000):
        t, nt = _i32(types)
        sup, h = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().tgpu_set_builder_factory_create(ctx.handle, operator_id, nt, t, int(set_channel), int(hash_channel), int(expected_positions),
                                                              C.byref(sup), C.byref(h)))
        super().__init__(h)
        self.set_supplier = SetSupplier(sup)


class HashSemiJoinOperatorFactory(OperatorFactory):
    """HashSemiJoinOperator.HashSemiJoinOperatorFactory (M/operator/HashSemiJoinOperator.java:44-118): the probe page plus one BOOLEAN
    channel, `probe_join_channel` IN the set."""

    def __init__(self, ctx: Context, operator_id, set_supplier: SetSupplier, probe_types, probe_join_channel, probe_hash_channel=-1):
        t, nt = _i32(probe_types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_hash_semi_join_factory_create(ctx.handle, operator_id, set_supplier.handle, nt, t, int(probe_join_channel),
                                                                 int(probe_hash_channel), C.byref(h)))
        super().__init__(h)
        self._supplier = set_supplier


class NestedLoopBridge:
    """NestedLoopJoinPagesSupplier (M/operator/NestedLoopJoinPagesSupplier.java): the bridge from the nested loop build operator to the probes."""

    def __init__(self, handle):
        self.handle = handle

    def stats(self):
        """valid once the build operator finished: kept pages (zero-channel pages re-cut to 8192 positions), their positions, their HBM bytes"""
        pages, positions, nbytes = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tgpu_nested_loop_bridge_stats(self.handle, C.byref(pages), C.byref(positions), C.byref(nbytes)))
        return dict(pages=pages.value, positions=positions.value, bytes=nbytes.value)

    def close(self):
        if self.handle:
            _lib.lib().tgpu_nested_loop_bridge_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # a constructor that failed before `handle` existed, or interpreter shutdown
            pass


class NestedLoopBuildOperatorFactory(OperatorFactory):
    """NestedLoopBuildOperator.NestedLoopBuildOperatorFactory (M/operator/NestedLoopBuildOperator.java:33-94).  `bridge` goes to the
    NestedLoopJoinOperatorFactory / FilterProjectNestedLoopJoinOperatorFactory."""

    def __init__(self, ctx: Context, operator_id, types):
        t, nt = _i32(types)
        b, h = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().tgpu_nested_loop_build_factory_create(ctx.handle, operator_id, nt, t, C.byref(b), C.byref(h)))
        super().__init__(h)
        self.bridge = NestedLoopBridge(b)


class NestedLoopJoinOperatorFactory(OperatorFactory):
    """NestedLoopJoinOperator.NestedLoopJoinOperatorFactory (M/operator/NestedLoopJoinOperator.java:44-108): the rows of the reference's
    output pages in their order, `probe_channels` then `build_channels`, at most `max_output_rows` rows per output page (0 = default)."""

    def __init__(self, ctx: Context, operator_id, bridge: NestedLoopBridge, probe_types, probe_channels, build_channels, max_output_rows=0):
        t, nt = _i32(probe_types)
        pc, npc = _i32(probe_channels)
        bc, nbc = _i32(build_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_nested_loop_join_factory_create(ctx.handle, operator_id, bridge.handle, nt, t, npc, pc, nbc, bc, int(max_output_rows), C.byref(h)))
        super().__init__(h)
        self._bridge = bridge


class FilterProjectNestedLoopJoinOperatorFactory(OperatorFactory):
    """NestedLoopJoin(all probe channels, all build channels) -> FilterAndProject as one operator.  Channel k < len(probe_types) of the
    expressions is probe channel k, the following ones are the build side's (probe first)."""

    def __init__(self, ctx: Context, operator_id, bridge: NestedLoopBridge, probe_types, filter_expr, projections, max_product_rows=0):
        self.program = FlatProgram(filter_expr, projections)
        spec, keep = self.program.to_c()
        t, nt = _i32(probe_types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_filter_project_nested_loop_join_factory_create(ctx.handle, operator_id, bridge.handle, nt, t, C.byref(spec), int(max_product_rows),
                                                                                  C.byref(h)))
        super().__init__(h, keep)
        self._bridge = bridge


def precompile_nested_loop_filter(probe_types, build_types, filter_expr):
    """Compile the pair filter's kernels into the on-disk cache (no GPU needed).  TgpuError NOT_SUPPORTED for a filter that is not fused."""
    spec, keep = FlatProgram(filter_expr, []).to_c()
    pt, npt = _i32(probe_types)
    bt, nbt = _i32(build_types)
    _lib.check(_lib.lib().tgpu_precompile_nested_loop_filter(npt, pt, nbt, bt, C.byref(spec)))


def nested_loop_filter_source(probe_types, build_types, filter_expr):
    """The generated source of the pair filter (tg_pair_filter, nlj_pair_count, nlj_pair_emit).  TgpuError NOT_SUPPORTED, with the reason
    as its message, for a filter that takes the unfused route."""
    spec, keep = FlatProgram(filter_expr, []).to_c()
    pt, npt = _i32(probe_types)
    bt, nbt = _i32(build_types)
    L = _lib.lib()
    need = _lib.check(L.tgpu_nested_loop_filter_source(npt, pt, nbt, bt, C.byref(spec), None, 0))
    buf = C.create_string_buffer(int(need))
    L.tgpu_nested_loop_filter_source(npt, pt, nbt, bt, C.byref(spec), buf, need)
    return buf.value.decode()


class MarkDistinctOperatorFactory(OperatorFactory):
    """MarkDistinctOperator.MarkDistinctOperatorFactory (M/operator/MarkDistinctOperator.java:39-92): the input page plus one BOOLEAN
    channel, true on the first row of every value of `mark_distinct_channels` the operator has not seen before."""

    def __init__(self, ctx: Context, operator_id, source_types, mark_distinct_channels, hash_channel=-1):
        t, nt = _i32(source_types)
        m, nm = _i32(mark_distinct_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_mark_distinct_factory_create(ctx.handle, operator_id, nt, t, nm, m, int(hash_channel), C.byref(h)))
        super().__init__(h)


class DistinctLimitOperatorFactory(OperatorFactory):
    """DistinctLimitOperator.DistinctLimitOperatorFactory (M/operator/DistinctLimitOperator.java:42-99): the first `limit` distinct rows
    of `distinct_channels`, in the order they arrive; output = the distinct channels, then the hash channel if there is one."""

    def __init__(self, ctx: Context, operator_id, source_types, distinct_channels, limit, hash_channel=-1):
        t, nt = _i32(source_types)
        d, nd = _i32(distinct_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_distinct_limit_factory_create(ctx.handle, operator_id, nt, t, nd, d, int(limit), int(hash_channel), C.byref(h)))
        super().__init__(h)


class RowNumberOperatorFactory(OperatorFactory):
    """RowNumberOperator.RowNumberOperatorFactory (M/operator/RowNumberOperator.java:43-119): `output_channels`, then the BIGINT number of
    the row inside its partition (the rows equal on `partition_channels`; none = one partition), counted from 1 in arrival order.  With
    `max_rows_per_partition` only the rows numbered up to it come out."""

    def __init__(self, ctx: Context, operator_id, source_types, output_channels, partition_channels, max_rows_per_partition=None, hash_channel=-1,
                 expected_positions=10):
        t, nt = _i32(source_types)
        o, no = _i32(output_channels)
        p, np_ = _i32(partition_channels)
        h = C.c_void_p()
        m = -1 if max_rows_per_partition is None else int(max_rows_per_partition)
        _lib.check(_lib.lib().tgpu_row_number_factory_create(ctx.handle, operator_id, nt, t, no, o, np_, p, m, int(hash_channel), int(expected_positions), C.byref(h)))
        super().__init__(h)


ROW_NUMBER, RANK, DENSE_RANK = 0, 1, 2   # tgpu_ranking_type = TopNRankingNode.RankingType's ordinal


class TopNRankingOperatorFactory(OperatorFactory):
    """TopNRankingOperator.TopNRankingOperatorFactory (M/operator/TopNRankingOperator.java:42-156): row_number() / rank() OVER (PARTITION BY
    `partition_channels` ORDER BY `sort_channels`) <= `max_rank_per_partition`.  One output page after finish(): `output_channels`, then
    -- unless `partial` -- the BIGINT ranking; partitions in the order of their keys' first arrival, rows that compare equal in arrival
    order.  RANK keeps every tie at the boundary; DENSE_RANK is an invalid argument, as in the reference."""

    def __init__(self, ctx: Context, operator_id, ranking_type, types, output_channels, partition_channels, sort_channels, sort_orders, max_rank_per_partition,
                 partial=False, hash_channel=-1, expected_positions=10):
        if len(sort_channels) != len(sort_orders):
            raise ValueError("sort channels and sort orders differ in length")
        t, nt = _i32(types)
        o, no = _i32(output_channels)
        p, np_ = _i32(partition_channels)
        sc, ns = _i32(sort_channels)
        so, _ = _i32(sort_orders)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_top_n_ranking_factory_create(ctx.handle, operator_id, int(ranking_type), nt, t, no, o, np_, p, ns, sc, so, int(max_rank_per_partition),
                                                                1 if partial else 0, int(hash_channel), int(expected_positions), C.byref(h)))
        super().__init__(h)


# tgpu_window_function / tgpu_window_frame
WINDOW_ROW_NUMBER, WINDOW_RANK, WINDOW_DENSE_RANK, WINDOW_PERCENT_RANK, WINDOW_CUME_DIST = 0, 1, 2, 3, 4
WINDOW_LAG, WINDOW_LEAD, WINDOW_FIRST_VALUE, WINDOW_LAST_VALUE, WINDOW_AGGREGATE = 5, 6, 7, 8, 9
FRAME_PARTITION, FRAME_RANGE_TO_CURRENT, FRAME_ROWS_TO_CURRENT = 0, 1, 2
# tgpu_window_factory_create_framed: two more functions, tgpu_frame_type / tgpu_frame_bound
WINDOW_NTH_VALUE, WINDOW_NTILE = 10, 11
FRAME_TYPE_RANGE, FRAME_TYPE_ROWS, FRAME_TYPE_GROUPS = 0, 1, 2
BOUND_UNBOUNDED_PRECEDING, BOUND_PRECEDING, BOUND_CURRENT_ROW, BOUND_FOLLOWING, BOUND_UNBOUNDED_FOLLOWING = 0, 1, 2, 3, 4


class WindowFrame:
    """A frame with bounds (tgpu_window_frame_spec; M/operator/window/FrameInfo.java): `type` = a FRAME_TYPE_* code, `start_type` / `end_type` =
    BOUND_* codes, `start_channel` / `end_channel` = the BIGINT or INTEGER source channel of a PRECEDING / FOLLOWING bound's offset, read per row."""

    def __init__(self, type, start_type, end_type, start_channel=-1, end_channel=-1):
        self.type, self.start_type, self.end_type = int(type), int(start_type), int(end_type)
        self.start_channel, self.end_channel = int(start_channel), int(end_channel)

    def spec(self):
        return _lib.WindowFrameSpec(self.type, self.start_type, self.start_channel, self.end_type, self.end_channel)


class WindowRangeFrame(WindowFrame):
    """A RANGE frame whose PRECEDING / FOLLOWING bounds are values (tgpu_window_range_frame_spec; tgpu_window_factory_create_ranged): `start_channel` /
    `end_channel` = the source channel of the bound's VALUE per row (sort key -/+ offset, see window_range_bound), `start_sort_key_channel` /
    `end_sort_key_channel` = the sort key coerced to that bound's type (FrameInfo.sortKeyChannelForStart/EndComparison)."""

    def __init__(self, start_type, end_type, start_channel=-1, end_channel=-1, start_sort_key_channel=-1, end_sort_key_channel=-1):
        super().__init__(FRAME_TYPE_RANGE, start_type, end_type, start_channel, end_channel)
        self.start_sort_key_channel, self.end_sort_key_channel = int(start_sort_key_channel), int(end_sort_key_channel)

    def range_spec(self):
        return _lib.WindowRangeFrameSpec(self.type, self.start_type, self.start_channel, self.end_type, self.end_channel, self.start_sort_key_channel,
                                         self.end_sort_key_channel)


def window_range_bound(key, offset, bound_type, sort_order, unit=None):
    """The RowExpression a planner projects in front of the window for a RANGE bound (QueryPlanner.planFrameBound): key - offset for ASC PRECEDING and
    DESC FOLLOWING, key + offset for the other two, checked arithmetic in the key's type.  `key` = the sort key (coerced to the offset's type),
    `offset` = an expression of that type or a Python number; on a DATE key, `unit` names the interval and `offset` is its BIGINT count:
    date_add(unit, -/+ offset, key)."""
    if bound_type not in (BOUND_PRECEDING, BOUND_FOLLOWING):
        raise ValueError("only PRECEDING and FOLLOWING bounds have a value")
    ascending = sort_order in (ASC_NULLS_FIRST, ASC_NULLS_LAST)
    subtract = (bound_type == BOUND_PRECEDING) == ascending
    if unit is not None:
        if isinstance(offset, _expr.RowExpression):
            return _expr.date_add(unit, -offset if subtract else offset, key)
        return _expr.date_add(unit, -int(offset) if subtract else int(offset), key)
    return key - offset if subtract else key + offset


# the three frames of tgpu_window_factory_create as the framed entry point takes them
_OLD_FRAMES = {FRAME_PARTITION: (FRAME_TYPE_RANGE, BOUND_UNBOUNDED_PRECEDING, BOUND_UNBOUNDED_FOLLOWING),
               FRAME_RANGE_TO_CURRENT: (FRAME_TYPE_RANGE, BOUND_UNBOUNDED_PRECEDING, BOUND_CURRENT_ROW),
               FRAME_ROWS_TO_CURRENT: (FRAME_TYPE_ROWS, BOUND_UNBOUNDED_PRECEDING, BOUND_CURRENT_ROW)}


class WindowFunction:
    """One window function of a WindowOperatorFactory (tgpu_window_function_spec): `function` = a WINDOW_* code, `argument_channels` = its 0 to 3
    source channels (lag / lead: value, offset, default; nth_value: value, offset; ntile: buckets), `frame` = a FRAME_* code or a WindowFrame (read
    by the aggregates and first / last / nth value), `agg_function` = the aggregate of WINDOW_AGGREGATE (COUNT_ALL, COUNT_COLUMN, SUM_BIGINT,
    MIN_* / MAX_*)."""

    def __init__(self, function, argument_channels=(), frame=FRAME_RANGE_TO_CURRENT, agg_function=0, ignore_nulls=False):
        self.function, self.argument_channels = int(function), tuple(int(c) for c in argument_channels)
        self.frame = frame if isinstance(frame, WindowFrame) else int(frame)
        self.agg_function, self.ignore_nulls = int(agg_function), bool(ignore_nulls)

    def framed(self):
        """needs tgpu_window_factory_create_framed"""
        return isinstance(self.frame, WindowFrame) or self.function > WINDOW_AGGREGATE

    def spec(self):
        if len(self.argument_channels) > 3:
            raise ValueError("a window function takes at most 3 argument channels")
        channels = self.argument_channels + (0,) * (3 - len(self.argument_channels))
        frame = 0 if isinstance(self.frame, WindowFrame) else self.frame
        return _lib.WindowFunctionSpec(self.function, self.agg_function, frame, len(self.argument_channels), (C.c_int32 * 3)(*channels),
                                       1 if self.ignore_nulls else 0)

    def frame_spec(self):
        if isinstance(self.frame, WindowFrame):
            return self.frame.spec()
        if self.frame not in _OLD_FRAMES:
            raise ValueError("unknown window frame")
        t, s, e = _OLD_FRAMES[self.frame]
        return _lib.WindowFrameSpec(t, s, -1, e, -1)

    def range_frame_spec(self):
        if isinstance(self.frame, WindowRangeFrame):
            return self.frame.range_spec()
        w = self.frame_spec()
        return _lib.WindowRangeFrameSpec(w.type, w.start_type, w.start_channel, w.end_type, w.end_channel, -1, -1)


class WindowOperatorFactory(OperatorFactory):
    """WindowOperator.WindowOperatorFactory (M/operator/WindowOperator.java:71-203): `functions` OVER (PARTITION BY `partition_channels` ORDER BY
    `sort_channels`).  One output page after finish(): `output_channels`, then one channel per function; rows in the order of the partition
    channels (ASC_NULLS_LAST) and the sort channels, rows that compare equal in arrival order; without either, arrival order and one partition
    of peers.  Partitions and peers are decided by IS NOT DISTINCT FROM."""

    def __init__(self, ctx: Context, operator_id, types, output_channels, functions, partition_channels, sort_channels, sort_orders, expected_positions=10):
        if len(sort_channels) != len(sort_orders):
            raise ValueError("sort channels and sort orders differ in length")
        functions = list(functions)
        t, nt = _i32(types)
        o, no = _i32(output_channels)
        p, np_ = _i32(partition_channels)
        sc, ns = _i32(sort_channels)
        so, _ = _i32(sort_orders)
        specs = (_lib.WindowFunctionSpec * max(1, len(functions)))(*[f.spec() for f in functions])
        h = C.c_void_p()
        if any(isinstance(f.frame, WindowRangeFrame) for f in functions):
            frames = (_lib.WindowRangeFrameSpec * max(1, len(functions)))(*[f.range_frame_spec() for f in functions])
            _lib.check(_lib.lib().tgpu_window_factory_create_ranged(ctx.handle, operator_id, nt, t, no, o, len(functions), specs, frames, np_, p, ns, sc, so,
                                                                    int(expected_positions), C.byref(h)))
        elif any(f.framed() for f in functions):
            frames = (_lib.WindowFrameSpec * max(1, len(functions)))(*[f.frame_spec() for f in functions])
            _lib.check(_lib.lib().tgpu_window_factory_create_framed(ctx.handle, operator_id, nt, t, no, o, len(functions), specs, frames, np_, p, ns, sc, so,
                                                                    int(expected_positions), C.byref(h)))
        else:
            _lib.check(_lib.lib().tgpu_window_factory_create(ctx.handle, operator_id, nt, t, no, o, len(functions), specs, np_, p, ns, sc, so, int(expected_positions),
                                                             C.byref(h)))
        super().__init__(h)


class LimitOperatorFactory(OperatorFactory):
    """LimitOperator.LimitOperatorFactory (M/operator/LimitOperator.java:27-60): the first `limit` rows of the stream; whole pages pass
    through, the crossing page is cut."""

    def __init__(self, ctx: Context, operator_id, source_types, limit):
        t, nt = _i32(source_types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_limit_factory_create(ctx.handle, operator_id, nt, t, int(limit), C.byref(h)))
        super().__init__(h)


class MergePagesOperatorFactory(OperatorFactory):
    """MergePages.mergePages (M/operator/project/MergePages.java:64-96) as an operator: small pages are coalesced in HBM, big ones pass through"""

    def __init__(self, ctx: Context, operator_id, types, min_page_size_in_bytes, min_row_count, max_page_size_in_bytes=1024 * 1024):
        t, nt = _i32(types)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_merge_pages_factory_create(ctx.handle, operator_id, nt, t, int(min_page_size_in_bytes), int(min_row_count), int(max_page_size_in_bytes),
                                                              C.byref(h)))
        super().__init__(h)


class PartitionedOutputOperator(Operator):
    """the sink side of PartitionedOutputOperator (M/operator/PartitionedOutputOperator.java:46-300): poll() hands out what the
    reference enqueues into its OutputBuffer"""

    def poll(self):
        """next pending (partition, OutputPage) pair, or None"""
        part, out = C.c_int32(-1), C.c_void_p()
        _lib.check(_lib.lib().tgpu_partitioned_output_poll(self.handle, C.byref(part), C.byref(out)))
        return (int(part.value), OutputPage(out)) if out.value else None

    def info(self):
        rows, pages = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tgpu_partitioned_output_info(self.handle, C.byref(rows), C.byref(pages)))
        return {"rowsAdded": int(rows.value), "pagesAdded": int(pages.value)}


class PartitionedOutputOperatorFactory(OperatorFactory):
    """PartitionedOutputOperator.PartitionedOutputFactory (M/operator/PartitionedOutputOperator.java:52-130): hash partitioning on
    `partition_channels` (or the precomputed `hash_channel`), `null_channel` / `replicates_any_row` replication (:411-418)."""

    def __init__(self, ctx: Context, operator_id, types, partition_channels, partition_count, hash_channel=-1, replicates_any_row=False, null_channel=-1, local=False):
        """local=True: the LocalExchange partition function (LocalPartitionGenerator.java:45-65; power-of-two partition count)"""
        t, nt = _i32(types)
        pc, npc = _i32(partition_channels)
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_partitioned_output_factory_create(ctx.handle, operator_id, nt, t, npc, pc, hash_channel, partition_count,
                                                                     1 if replicates_any_row else 0, null_channel, 1 if local else 0, C.byref(h)))
        super().__init__(h)

    def createOperator(self):
        h = C.c_void_p()
        _lib.check(_lib.lib().tgpu_operator_factory_create_operator(self.handle, C.byref(h)))
        return PartitionedOutputOperator(h)

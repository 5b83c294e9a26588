"""The factory protocol of every operator factory the package exports, through the C ABI: createOperator / duplicate / noMoreOperators
(M/operator/OperatorFactory.java:18-50) and the argument validation at factory creation.  Every page has 5 rows and every expected page
is written out: an operator of the original and one of its duplicate must both produce exactly these pages."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, STATE_ERROR, NOT_SUPPORTED = -1, -5, -8   # TGPU_ERR_INVALID_ARGUMENT, TGPU_ERR_INTERNAL (illegal state), TGPU_ERR_NOT_SUPPORTED
K = [3, 1, 3, 2, 1]
V = [10, 20, 30, 40, 50]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def bigints(pkg, *cols):
    return pkg.Page(*[pkg.Block(pkg.BIGINT, np.array(c, dtype=np.int64)) for c in cols])


def kv(pkg):
    return bigints(pkg, K, V)


def through(pkg, pages):
    """run(op): the pages OperatorAssertion.toPages gets out of `op` for `pages`, as lists of rows"""
    def run(op):
        out = [p.rows() for p in pkg.to_pages(op, pages)]
        op.close()
        return out
    return run


def built_join_bridge(pkg, ctx, keep, keys=(1, 2, 2)):
    """a finished hash build over `keys` (output: the key); the builder stays alive in `keep`"""
    bf = pkg.HashBuilderOperatorFactory(ctx, 90, [pkg.BIGINT], [0], [0])
    b = bf.createOperator()
    b.addInput(bigints(pkg, list(keys)))
    b.finish()
    keep += [bf, b]
    return bf.lookup_source_factory


def published_set(pkg, ctx, keep):
    """a finished set builder over the keys [1, 2]"""
    sf = pkg.SetBuilderOperatorFactory(ctx, 91, [pkg.BIGINT], 0)
    s = sf.createOperator()
    s.addInput(bigints(pkg, [1, 2, 1]))
    s.finish()
    keep += [sf, s]
    return sf.set_supplier


def case_filter_project(pkg, ctx, keep):
    f, B = pkg.field, pkg.BIGINT
    fac = pkg.FilterAndProjectOperatorFactory(ctx, 1, [B, B, B], f(0, B) > 899, [f(1, B) * f(2, B)])
    return fac, through(pkg, [bigints(pkg, [900, 1, 1000, 2, 899], [1, 2, 3, 4, 5], [10, 10, 10, 10, 10])]), [[(10,), (30,)]]


def case_scan_filter_project(pkg, ctx, keep):
    f, B = pkg.field, pkg.BIGINT
    fac = pkg.ScanFilterAndProjectOperatorFactory(ctx, 2, [B, B, B], f(0, B) > 899, [f(1, B) * f(2, B)])

    def run(op):
        op.addSplit(pkg.PageSource([bigints(pkg, [900, 1, 1000, 2, 899], [1, 2, 3, 4, 5], [10, 10, 10, 10, 10])]))
        op.noMoreSplits()
        out = []
        for _ in range(1000):
            if op.isFinished():
                break
            o = op.getOutput()
            if o is not None:
                out.append(o.to_host().rows())
                o.release()
        assert op.isFinished()
        op.close()
        return out
    return fac, run, [[(10,), (30,)]]


def case_hash_aggregation(pkg, ctx, keep):
    fac = pkg.HashAggregationOperatorFactory(ctx, 3, [pkg.BIGINT], [0], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)])
    return fac, through(pkg, [kv(pkg)]), [[(3, 2, 40), (1, 2, 70), (2, 1, 40)]]


def case_lookup_join(pkg, ctx, keep):
    B = pkg.BIGINT
    fac = pkg.LookupJoinOperatorFactory(ctx, 4, built_join_bridge(pkg, ctx, keep), [B, B], [0])
    return fac, through(pkg, [kv(pkg)]), [[(1, 20, 1), (2, 40, 2), (2, 40, 2), (1, 50, 1)]]


def case_filter_project_lookup_join(pkg, ctx, keep):
    f, B = pkg.field, pkg.BIGINT
    bridge = built_join_bridge(pkg, ctx, keep, keys=(1, 2, 7))   # unique build keys: the probe runs in the fused kernels
    fac = pkg.FilterProjectLookupJoinOperatorFactory(ctx, 5, bridge, [B, B], f(1, B) > 20, [f(0, B), f(1, B)], [0])
    return fac, through(pkg, [kv(pkg)]), [[(2, 40, 2), (1, 50, 1)]]


def case_filter_project_hash_aggregation(pkg, ctx, keep):
    f, B = pkg.field, pkg.BIGINT
    fac = pkg.FilterProjectHashAggregationOperatorFactory(ctx, 6, [B, B], f(1, B) > 10, [f(0, B), f(1, B)], [B], [0], [(pkg.COUNT_ALL, -1), (pkg.SUM_BIGINT, 1)])
    return fac, through(pkg, [kv(pkg)]), [[(1, 2, 70), (3, 1, 30), (2, 1, 40)]]


def case_top_n(pkg, ctx, keep):
    fac = pkg.TopNOperatorFactory(ctx, 7, [pkg.BIGINT, pkg.BIGINT], 3, [1], [pkg.DESC_NULLS_LAST])
    return fac, through(pkg, [kv(pkg)]), [[(1, 50), (2, 40), (3, 30)]]


def case_order_by(pkg, ctx, keep):
    fac = pkg.OrderByOperatorFactory(ctx, 8, [pkg.BIGINT, pkg.BIGINT], [1, 0], 10, [0, 1], [pkg.ASC_NULLS_LAST, pkg.DESC_NULLS_LAST])
    return fac, through(pkg, [kv(pkg)]), [[(50, 1), (20, 1), (40, 2), (30, 3), (10, 3)]]


def case_hash_semi_join(pkg, ctx, keep):
    fac = pkg.HashSemiJoinOperatorFactory(ctx, 9, published_set(pkg, ctx, keep), [pkg.BIGINT, pkg.BIGINT], 0)
    return fac, through(pkg, [kv(pkg)]), [[(3, 10, False), (1, 20, True), (3, 30, False), (2, 40, True), (1, 50, True)]]


def case_mark_distinct(pkg, ctx, keep):
    fac = pkg.MarkDistinctOperatorFactory(ctx, 10, [pkg.BIGINT, pkg.BIGINT], [0])
    return fac, through(pkg, [kv(pkg)]), [[(3, 10, True), (1, 20, True), (3, 30, False), (2, 40, True), (1, 50, False)]]


def case_distinct_limit(pkg, ctx, keep):
    fac = pkg.DistinctLimitOperatorFactory(ctx, 11, [pkg.BIGINT, pkg.BIGINT], [0], 2)
    return fac, through(pkg, [kv(pkg)]), [[(3,), (1,)]]


def case_row_number(pkg, ctx, keep):
    fac = pkg.RowNumberOperatorFactory(ctx, 12, [pkg.BIGINT, pkg.BIGINT], [0, 1], [0], 1)
    return fac, through(pkg, [kv(pkg)]), [[(3, 10, 1), (1, 20, 1), (2, 40, 1)]]


def case_limit(pkg, ctx, keep):
    fac = pkg.LimitOperatorFactory(ctx, 13, [pkg.BIGINT, pkg.BIGINT], 3)
    return fac, through(pkg, [kv(pkg)]), [[(3, 10), (1, 20), (3, 30)]]


def case_merge_pages(pkg, ctx, keep):
    fac = pkg.MergePagesOperatorFactory(ctx, 14, [pkg.BIGINT, pkg.BIGINT], 1 << 20, 100, 1 << 21)
    return fac, through(pkg, [kv(pkg), kv(pkg)]), [list(zip(K + K, V + V))]


def case_partitioned_output(pkg, ctx, keep):
    B = pkg.BIGINT
    fac = pkg.PartitionedOutputOperatorFactory(ctx, 15, [B, B, B], [], 2, hash_channel=2)   # partition = the precomputed hash modulo 2

    def run(op):
        op.addInput(bigints(pkg, K, V, [0, 1, 2, 3, 4]))
        out = []
        while True:
            pair = op.poll()
            if pair is None:
                break
            out.append((pair[0], pair[1].to_host().rows()))
            pair[1].release()
        op.finish()
        assert op.isFinished() and op.getOutput() is None
        op.close()
        return out
    return fac, run, [(0, [(3, 10, 0), (3, 30, 2), (1, 50, 4)]), (1, [(1, 20, 1), (2, 40, 3)])]


DUPLICATABLE = [case_filter_project, case_scan_filter_project, case_hash_aggregation, case_lookup_join, case_filter_project_lookup_join,
                case_filter_project_hash_aggregation, case_top_n, case_order_by, case_hash_semi_join, case_mark_distinct, case_distinct_limit,
                case_row_number, case_limit, case_merge_pages, case_partitioned_output]


def assert_closed(pkg, factory):
    with pytest.raises(pkg.TgpuError) as e:
        factory.createOperator()
    assert e.value.code == STATE_ERROR and "Factory is already closed" in e.value.message


@pytest.mark.parametrize("case", DUPLICATABLE, ids=lambda c: c.__name__[5:])
def test_duplicate_and_close(pkg, ctx, case):
    keep = []
    fac, run, expected = case(pkg, ctx, keep)
    dup = fac.duplicate()
    assert run(fac.createOperator()) == expected
    assert run(dup.createOperator()) == expected
    fac.noMoreOperators()
    assert_closed(pkg, fac)
    assert run(dup.createOperator()) == expected   # closing the original does not reach its duplicate
    dup.noMoreOperators()
    assert_closed(pkg, dup)
    fac.close()
    dup.close()


def case_hash_builder(pkg, ctx):
    return pkg.HashBuilderOperatorFactory(ctx, 20, [pkg.BIGINT], [0], [0])


def case_partitioned_hash_builder(pkg, ctx):
    return pkg.HashBuilderOperatorFactory(ctx, 21, [pkg.BIGINT], [0], [0], partition_count=2)


def case_lookup_outer(pkg, ctx):
    bf = case_hash_builder(pkg, ctx)
    fac = pkg.LookupOuterOperatorFactory(ctx, 22, bf.lookup_source_factory, [pkg.BIGINT])
    fac._builder = bf
    return fac


def case_set_builder(pkg, ctx):
    return pkg.SetBuilderOperatorFactory(ctx, 23, [pkg.BIGINT], 0)


def case_dynamic_filter_source(pkg, ctx):
    return pkg.DynamicFilterSourceOperatorFactory(ctx, 24, [pkg.BIGINT, pkg.BIGINT], [0], 100, 1 << 20, 100)


@pytest.mark.parametrize("case", [case_hash_builder, case_partitioned_hash_builder, case_lookup_outer, case_set_builder, case_dynamic_filter_source],
                         ids=lambda c: c.__name__[5:])
def test_duplicate_is_not_supported(pkg, ctx, case):
    fac = case(pkg, ctx)
    with pytest.raises(pkg.TgpuError) as e:
        fac.duplicate()
    assert e.value.code == NOT_SUPPORTED
    fac.createOperator().close()   # the refused duplicate left the factory usable
    fac.noMoreOperators()
    assert_closed(pkg, fac)
    fac.close()


def test_dynamic_filter_source_operator(pkg, ctx):
    """the one plain factory that cannot be duplicated: its operator passes the page through and collects the values"""
    fac = case_dynamic_filter_source(pkg, ctx)
    op = fac.createOperator()
    assert [p.rows() for p in pkg.to_pages(op, [kv(pkg)])] == [list(zip(K, V))]
    assert op.domain(0) == ("values", [3, 1, 2])
    op.close()
    fac.close()


def test_partitioned_hash_builder_hands_out_one_operator_per_partition(pkg, ctx):
    fac = case_partitioned_hash_builder(pkg, ctx)
    a, b = fac.createOperator(), fac.createOperator()
    with pytest.raises(pkg.TgpuError) as e:
        fac.createOperator()
    assert e.value.code == STATE_ERROR
    a.close(); b.close(); fac.close()


def test_lookup_outer_factory_creates_one_operator(pkg, ctx):
    fac = case_lookup_outer(pkg, ctx)
    op = fac.createOperator()
    with pytest.raises(pkg.TgpuError) as e:
        fac.createOperator()
    assert e.value.code == STATE_ERROR and "Only one outer operator can be created" in e.value.message
    op.close(); fac.close()


def test_semi_join_duplicate_shares_the_supplier(pkg, ctx):
    """HashSemiJoinOperator.java:115-118: probes of the original and of the duplicate, both created before the set exists, see the set the
    one builder publishes"""
    B = pkg.BIGINT
    sf = pkg.SetBuilderOperatorFactory(ctx, 30, [B], 0)
    fac = pkg.HashSemiJoinOperatorFactory(ctx, 31, sf.set_supplier, [B, B], 0)
    dup = fac.duplicate()
    probes = [fac.createOperator(), dup.createOperator()]
    assert all(p.isBlocked() and not p.needsInput() for p in probes)
    builder = sf.createOperator()
    builder.addInput(bigints(pkg, [2, 3]))
    builder.finish()
    assert all(not p.isBlocked() and p.needsInput() for p in probes)
    for p in probes:
        assert [pg.rows() for pg in pkg.to_pages(p, [kv(pkg)])] == [[(3, 10, True), (1, 20, False), (3, 30, True), (2, 40, True), (1, 50, False)]]
        p.close()
    builder.close(); fac.close(); dup.close(); sf.close()


def _bridge(pkg, ctx):
    return pkg.HashBuilderOperatorFactory(ctx, 40, [pkg.BIGINT], [0], [0])


BAD_ARGUMENTS = {
    "hash_aggregation_expected_groups_0": lambda p, c: p.HashAggregationOperatorFactory(c, 1, [p.BIGINT], [0], [(p.COUNT_ALL, -1)], expected_groups=0),
    "hash_aggregation_unknown_function": lambda p, c: p.HashAggregationOperatorFactory(c, 1, [p.BIGINT], [0], [(99, 1)]),
    "hash_builder_without_join_channel": lambda p, c: p.HashBuilderOperatorFactory(c, 1, [p.BIGINT], [0], []),
    "hash_builder_partition_count_3": lambda p, c: p.HashBuilderOperatorFactory(c, 1, [p.BIGINT], [0], [0], partition_count=3),
    "lookup_join_channel_out_of_range": lambda p, c: p.LookupJoinOperatorFactory(c, 1, _bridge(p, c).lookup_source_factory, [p.BIGINT], [1]),
    "lookup_outer_unknown_type": lambda p, c: p.LookupOuterOperatorFactory(c, 1, _bridge(p, c).lookup_source_factory, [99]),
    "filter_project_lookup_join_channel_out_of_range": lambda p, c: p.FilterProjectLookupJoinOperatorFactory(
        c, 1, _bridge(p, c).lookup_source_factory, [p.BIGINT], None, [p.field(0, p.BIGINT)], [1]),
    "filter_project_hash_aggregation_expected_groups_0": lambda p, c: p.FilterProjectHashAggregationOperatorFactory(
        c, 1, [p.BIGINT], None, [p.field(0, p.BIGINT)], [p.BIGINT], [0], [(p.COUNT_ALL, -1)], expected_groups=0),
    "top_n_unknown_sort_order": lambda p, c: p.TopNOperatorFactory(c, 1, [p.BIGINT], 3, [0], [99]),
    "top_n_negative_n": lambda p, c: p.TopNOperatorFactory(c, 1, [p.BIGINT], -1, [0], [p.ASC_NULLS_LAST]),
    "order_by_output_channel_out_of_range": lambda p, c: p.OrderByOperatorFactory(c, 1, [p.BIGINT], [1], 10, [0], [p.ASC_NULLS_LAST]),
    "order_by_sort_channel_out_of_range": lambda p, c: p.OrderByOperatorFactory(c, 1, [p.BIGINT], [0], 10, [1], [p.ASC_NULLS_LAST]),
    "dynamic_filter_source_duplicate_channel": lambda p, c: p.DynamicFilterSourceOperatorFactory(c, 1, [p.BIGINT], [0, 0], 100, 1 << 20, 100),
    "set_builder_set_channel_out_of_range": lambda p, c: p.SetBuilderOperatorFactory(c, 1, [p.BIGINT], 1),
    "set_builder_hash_channel_out_of_range": lambda p, c: p.SetBuilderOperatorFactory(c, 1, [p.BIGINT], 0, hash_channel=1),
    "hash_semi_join_key_type_differs": lambda p, c: p.HashSemiJoinOperatorFactory(c, 1, p.SetBuilderOperatorFactory(c, 2, [p.BIGINT], 0).set_supplier, [p.DOUBLE], 0),
    "hash_semi_join_hash_channel_out_of_range": lambda p, c: p.HashSemiJoinOperatorFactory(
        c, 1, p.SetBuilderOperatorFactory(c, 2, [p.BIGINT], 0).set_supplier, [p.BIGINT], 0, probe_hash_channel=1),
    "mark_distinct_hash_channel_not_bigint": lambda p, c: p.MarkDistinctOperatorFactory(c, 1, [p.BIGINT, p.DOUBLE], [0], hash_channel=1),
    "distinct_limit_without_channels": lambda p, c: p.DistinctLimitOperatorFactory(c, 1, [p.BIGINT], [], 2),
    "distinct_limit_negative_limit": lambda p, c: p.DistinctLimitOperatorFactory(c, 1, [p.BIGINT], [0], -1),
    "row_number_max_rows_minus_2": lambda p, c: p.RowNumberOperatorFactory(c, 1, [p.BIGINT], [0], [0], -2),
    "row_number_expected_positions_0": lambda p, c: p.RowNumberOperatorFactory(c, 1, [p.BIGINT], [0], [0], expected_positions=0),
    "limit_minus_1": lambda p, c: p.LimitOperatorFactory(c, 1, [p.BIGINT], -1),
    "merge_pages_max_below_min": lambda p, c: p.MergePagesOperatorFactory(c, 1, [p.BIGINT], 1 << 20, 10, 1 << 10),
    "partitioned_output_partition_count_0": lambda p, c: p.PartitionedOutputOperatorFactory(c, 1, [p.BIGINT], [0], 0),
    "partitioned_output_without_channels": lambda p, c: p.PartitionedOutputOperatorFactory(c, 1, [p.BIGINT], [], 2),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGUMENTS))
def test_factory_creation_validates_its_arguments(pkg, ctx, name):
    with pytest.raises(pkg.TgpuError) as e:
        BAD_ARGUMENTS[name](pkg, ctx)
    assert e.value.code == INVALID_ARGUMENT

"""What the nested loop join must give, restated in plain Python (imports neither the library nor a GPU).

NestedLoopJoinPagesBuilder (M/operator/NestedLoopJoinPagesBuilder.java:45-110): empty build pages are dropped; build pages WITHOUT channels
are only counted and re-cut into pages of PageProcessor.MAX_BATCH_SIZE = 8192 positions plus a remainder.

NestedLoopJoinOperator.getOutput / createNestedLoopOutputIterator (M/operator/NestedLoopJoinOperator.java:208-274, NestedLoopPageBuilder
:319-397): one probe page against each build page in turn.  For p probe rows and b build rows the LARGE side is the build page iff b > p (a
tie makes the probe page large); one output page per row of the small side, each the large page's rows with the small row repeated; channels
= probe_channels then build_channels.  With an empty channel list on the side that is not larger, the other side's page is repeated
(PageRepeatingIterator, :265-270) -- for an empty PROBE list that makes the build page the large one on a tie as well.  With both lists
empty only position counts come out (:249-264).

A page is a list of rows (tuples over all of its channels), or an int: a page without channels, by its position count."""
from collections import namedtuple

import expr_fuzz as F

MAX_BATCH_SIZE = 8192


def positions_of(page):
    return page if isinstance(page, int) else len(page)


class RefPage(namedtuple("RefPage", "positions probe build")):
    """One output page of the reference: `probe` / `build` are the side's rows over its output channels -- a list of `positions` rows (the
    large page), or a one-row list standing for that row repeated `positions` times (RunLengthEncodedBlock)."""

    def rows(self):
        side = lambda rows: rows if len(rows) == self.positions else rows * self.positions
        return [p + b for p, b in zip(side(self.probe), side(self.build))]


def build_side(build_pages):
    """the pages NestedLoopJoinPagesBuilder.build() publishes"""
    out, counter = [], 0
    for page in build_pages:
        if positions_of(page) == 0:
            continue
        if isinstance(page, int):
            counter += page
            while counter >= MAX_BATCH_SIZE:
                out.append(MAX_BATCH_SIZE)
                counter -= MAX_BATCH_SIZE
        else:
            out.append(page)
    if counter > 0:
        out.append(counter)
    return out


def _select(page, channels):
    if isinstance(page, int):
        assert not channels
        return [()] * page
    return [tuple(row[c] for c in channels) for row in page]


def pair_pages(probe_page, build_page, probe_channels, build_channels):
    """createNestedLoopOutputIterator for one (probe page, build page): its pages, lazily"""
    p, b = positions_of(probe_page), positions_of(build_page)
    if not probe_channels and not build_channels:
        if p * b <= MAX_BATCH_SIZE and p * b < 2**31:
            yield RefPage(p * b, [()], [()])
        else:
            for _ in range(min(p, b)):
                yield RefPage(max(p, b), [()], [()])
        return
    build_large = b > p or (b == p and not probe_channels)
    if build_large:
        large = _select(build_page, build_channels)
        for row in _select(probe_page, probe_channels):
            yield RefPage(b, [row], large)
    else:
        large = _select(probe_page, probe_channels)
        for row in _select(build_page, build_channels):
            yield RefPage(p, large, [row])


def reference_pages(probe_pages, build_pages, probe_channels, build_channels):
    """every output page of the reference, in order (a generator: a product may be far larger than its inputs)"""
    built = build_side(build_pages)
    for probe_page in probe_pages:
        if positions_of(probe_page) == 0:
            continue
        for build_page in built:
            yield from pair_pages(probe_page, build_page, list(probe_channels), list(build_channels))


def reference_rows(probe_pages, build_pages, probe_channels, build_channels):
    return [row for page in reference_pages(probe_pages, build_pages, probe_channels, build_channels) for row in page.rows()]


def filtered(program, probe_pages, build_pages):
    """NestedLoopJoin(all probe channels, all build channels) -> FilterAndProject(program): expr_fuzz.run_program over every reference page in
    order.  program.types = the probe types then the build types.  Returns Values(positions in the sequence, columns) or the first Failure
    (its position is the row within its reference page)."""
    n_probe = len(probe_pages[0][0]) if probe_pages and not isinstance(probe_pages[0], int) and probe_pages[0] else None
    positions, columns, at = [], [[] for _ in program.projections], 0
    for probe_page in probe_pages:
        if positions_of(probe_page) == 0:
            continue
        np_ = n_probe if n_probe is not None else len(probe_page[0])
        for ref in reference_pages([probe_page], build_pages, range(np_), range(len(program.types) - np_)):
            rows = ref.rows()
            page = [(t, [row[c] for row in rows]) for c, t in enumerate(program.types)]
            o = F.run_program(program, page)
            if isinstance(o, F.Failure):
                return o
            positions += [at + i for i in o.positions]
            for col, part in zip(columns, o.columns):
                col += part
            at += len(rows)
    return F.Values(positions, columns)

"""The lane-group launch rule (csrc/kad_groups.h) restated in plain Python and compared with the four calls that
use it, through their ``*_route_eval``: no GPU.

The rule: lanes per row = the mean items per row (rounded up), ``per_lane`` of them to a lane (rounded up),
rounded up to a power of two in [``min_width``, 64]; grid = min(ceil(rows / (256 / width)), 8 * n_cu); stride =
grid * (256 / width). Per call: auto-migration (8, 1) over all segments and, for the object kernel, over all
objects; cluster status (8, 8), status aggregation (1, 8) and rollout planning (1, 1) over the short rows, with a
grid over all rows that is 0 when every row is long. The grid crosses every boundary: means of 0, 1 and every power
of two from 8 to 512 with its neighbours (and 2 to 5, where a rule that starts at one lane switches), rows of 0, 1 and the values around 8 * n_cu * 256 / width for n_cu 1 and
256, and none, one or all of the rows long."""
from kubeadmiral_amd import runtime

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
N_CUS = (1, 256)
MEANS = sorted({0, 1, 2, 3, 4, 5} | {p + d for p in (8, 16, 32, 64, 128, 256, 512) for d in (-1, 0, 1)})
ROWS = {n_cu: sorted({0, 1} | {8 * n_cu * 256 // w + d for w in WIDTHS for d in (-1, 0, 1)}) for n_cu in N_CUS}


def ceil_div(a, b):
    return -(-a // b)


def width(items, rows, min_width, per_lane):
    mean = ceil_div(items, rows) if rows > 0 else 0
    want = ceil_div(mean, per_lane)
    w = min_width
    while w < 64 and w < want:
        w *= 2
    return w


def grid(rows, w, n_cu):
    return min(ceil_div(rows, 256 // w), 8 * n_cu)


def items_of(mean, rows):
    """The fewest items whose mean over ``rows`` rows rounds up to ``mean``."""
    return (mean - 1) * rows + 1 if mean > 0 and rows > 0 else 0


def cases():
    for n_cu in N_CUS:
        for rows in ROWS[n_cu]:
            for n_long in sorted({0, min(1, rows), rows}):
                for mean in MEANS:
                    yield n_cu, rows, n_long, mean


def test_restatement_crosses_every_width():
    """The grid of means reaches every width of both per_lane values, from both sides of each boundary."""
    for min_width, per_lane in ((8, 1), (8, 8), (1, 8), (1, 1)):
        got = {width(items_of(m, 7), 7, min_width, per_lane) for m in MEANS}
        assert got == {w for w in WIDTHS if w >= min_width}, (min_width, per_lane)
    for n_cu in N_CUS:
        for w in WIDTHS:  # below, at and above the grid cap
            cap = 8 * n_cu
            assert [grid(8 * n_cu * 256 // w + d, w, n_cu) for d in (-1, 0, 1)] == [cap, cap, cap]
            assert grid(8 * n_cu * 256 // w - 256 // w, w, n_cu) == cap - 1


def test_migrate_route_is_the_shared_rule():
    for n_cu, rows, n_long, mean in cases():
        # the segment kernel: every segment counts, long or not
        r = runtime.migrate_route_eval(rows, items_of(mean, rows), n_long, 1, n_cu)
        w = width(items_of(mean, rows), rows, 8, 1)
        g = grid(rows, w, n_cu)
        want = dict(width=w, long_min=1024, threads=256, grid=g, long_grid=n_long, stride=g * (256 // w),
                    obj_width=width(rows, 1, 8, 1), obj_grid=1)
        assert r == want, (n_cu, rows, n_long, mean)
        if n_long:
            continue
        # the object kernel: `rows` objects of `mean` segments
        S = items_of(mean, rows)
        r = runtime.migrate_route_eval(S, 0, 0, rows, n_cu)
        ow = width(S, rows, 8, 1)
        assert (r["obj_width"], r["obj_grid"]) == (ow, grid(rows, ow, n_cu)), (n_cu, rows, mean)
        assert (r["width"], r["grid"]) == (8, grid(S, 8, n_cu))


def test_cstat_route_is_the_shared_rule():
    for n_cu, rows, n_long, mean in cases():
        n_short = rows - n_long
        nodes, pods = items_of(mean, n_short), items_of(MEANS[-1] - mean, n_short)
        r = runtime.cstat_route_eval(rows, n_long, nodes, pods, 3 * n_long, n_cu)
        nw, pw = width(nodes, n_short, 8, 8), width(pods, n_short, 8, 8)
        want = dict(node_width=nw, pod_width=pw, long_min=4096, threads=256,
                    node_grid=grid(rows, nw, n_cu) if n_short else 0, pod_grid=grid(rows, pw, n_cu) if n_short else 0,
                    long_grid=n_long, chunk_grid=3 * n_long)
        assert r == want, (n_cu, rows, n_long, mean)


def test_sagg_route_is_the_shared_rule():
    for n_cu, rows, n_long, mean in cases():
        n_short = rows - n_long
        segs = items_of(mean, n_short)
        r = runtime.sagg_route_eval(rows, n_long, segs, n_cu)
        w = width(segs, n_short, 1, 8)
        g = grid(rows, w, n_cu) if n_short else 0
        want = dict(width=w, long_min=512, threads=256, grid=g, long_grid=n_long, stride=g * (256 // w))
        assert r == want, (n_cu, rows, n_long, mean)


def test_rollout_route_is_the_shared_rule():
    for n_cu, rows, n_long, mean in cases():
        n_short = rows - n_long
        tgts = items_of(mean, n_short)
        n_serial = min(rows, 2)
        r = runtime.rollout_route_eval(rows, n_long, tgts, n_serial, n_cu)
        w = width(tgts, n_short, 1, 1)
        g = grid(rows, w, n_cu) if n_short else 0
        want = dict(width=w, long_min=256, threads=256, grid=g, long_grid=ceil_div(n_long, 4), stride=g * (256 // w),
                    serial=n_serial)
        assert r == want, (n_cu, rows, n_long, mean)

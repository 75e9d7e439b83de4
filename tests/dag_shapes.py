"""The plan shapes of the task-DAG schedule that run under test (helper module; not collected by pytest).

A plan shape is what the planner (csrc/dag_plan.hip: dag_build_tasks) is called with: the chunk length, the band's height in
tiles, the taper's first length and js2, the strip-column at which the second phase begins.  The planner's CPU test
(test_dag_shapes_cpu.py) holds every list of this grid to the invariants the kernels rely on; the device test
(test_hip_dag_shapes.py) runs the same tuples at the orders of ORDERS and holds every factor and solve to the exact answer."""
import itertools

NTILES = (2, 3, 5, 10, 11, 12, 21)
CHUNKS = (1, 3, 64)
BAND_TILES = (4, 6, 8)        # option dag_band = 2 * band_tiles (64-row strips)
TAPER0S = (1, 2, 16)
JS2_KINDS = ("zero", "one", "half", "last", "nsc")

# (chunk, band_tiles, taper0) at which the device test also crosses dag_fill with the per-XCD queues and the gangs
CORNERS = ((1, 4, 1), (64, 4, 16), (1, 8, 16), (64, 8, 1))
FILLS = (0, 1)
QUEUES = ((0, 4), (1, 4), (1, -1))   # (dag_xcd_queues, dag_gang); -1: every task to queue 0 (the steal path)

# matrix order -> tiles of 128 rows of its padded order; the last three run with dag_min_rows lowered to 128
ORDERS = {1280: 10, 1300: 11, 1536: 12, 2688: 21, 200: 2, 384: 3, 640: 5}
SMALL_ORDERS = (200, 384, 640)


def nsc(ntile):
    """Strip-columns (256 columns) of a matrix of `ntile` tiles."""
    return (ntile + 1) // 2


def js2_values(ntile):
    """{kind: js2} of the grid, duplicates removed (the first kind keeps the value)."""
    n = nsc(ntile)
    out, seen = {}, set()
    for kind, v in zip(JS2_KINDS, (0, 1, n // 2, n - 1, n)):
        if v not in seen:
            seen.add(v)
            out[kind] = v
    return out


def shapes():
    """(chunk, band_tiles, taper0) of the grid, the shipped shape (64, 8, 2) first."""
    g = list(itertools.product(CHUNKS, BAND_TILES, TAPER0S))
    g.sort(key=lambda s: s != (64, 8, 2))
    return g


def grid(ntile):
    """Every (chunk, band_tiles, taper0, js2) of the grid for `ntile` tiles."""
    return [(c, b, t, j) for (c, b, t) in shapes() for j in js2_values(ntile).values()]

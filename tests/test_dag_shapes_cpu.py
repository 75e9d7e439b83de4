"""The planner of the task-DAG schedule over the whole grid of plan shapes the device test runs (tests/dag_shapes.py), without a
GPU: the invariants of test_dag_tasks_cpu.py for every tuple -- every lower tile covered exactly once, chunks contiguous, in order
and flagged FIRST / FINAL / BANDACC, waits only backwards, the Python mirror -- and what the two-phase driver rests on: n1 counts
exactly the tasks that are ready by tile column 2 js2, the second part closes no tile of the first phase's strip-columns and the
first part reads nothing the second phase's chain produces, and the parts that are empty are empty.  And the one host-only rule
for js2 (csrc/dag_plan.hip: dag_choose_js2) with its bound: the deep band never gets more strips than its partition has CUs."""
import pytest

from madnlp_jl_amd import _lib as L
from tests import dag_shapes as S
from tests.test_dag_tasks_cpu import BAND, FINAL, FIRST, _tasks
from tests.test_dag_tasks_cpu import test_task_list_covers_every_tile_once_and_waits_only_backwards as _list_invariants


@pytest.mark.parametrize("ntile", S.NTILES)
def test_every_plan_shape_of_the_grid_keeps_the_planner_invariants(ntile):
    for chunk, band_tiles, taper0, js2 in S.grid(ntile):
        try:
            _list_invariants(ntile, chunk, band_tiles, js2, taper0)
        except AssertionError as e:
            raise AssertionError(f"ntile={ntile} chunk={chunk} band_tiles={band_tiles} taper0={taper0} js2={js2}: {e}") from e


@pytest.mark.parametrize("ntile", S.NTILES)
def test_phase_closure(ntile):
    """What lets the second phase start on another stream pair, behind the END of the first: the list is sorted by the tile column
    that makes a task ready, n1 cuts it exactly behind the tasks ready by 2 js2, no task behind the cut closes a tile of a
    strip-column < js2 (the first phase's bulk kernel has closed them all when it ends), and no task in front of it reads a tile
    column >= 2 js2 or closes a tile of one (the first phase's chain never factors those)."""
    for chunk, band_tiles, taper0, js2 in S.grid(ntile):
        tag = f"ntile={ntile} chunk={chunk} band_tiles={band_tiles} taper0={taper0} js2={js2}"
        ts, n1 = _tasks(ntile, chunk, band_tiles, js2, taper0)
        ready = [ke for *_, ke in ts]
        assert ready == sorted(ready), tag
        assert n1 == sum(1 for r in ready if r <= 2 * js2), tag + f": n1 = {n1}"
        for idx, (flags, q, I, J, kb, ke) in enumerate(ts):
            closes = bool(flags & FINAL) and not (flags & BAND)
            if idx < n1:
                assert ke <= 2 * js2, tag + f": task {idx} of the first part reads tile column {ke - 1}"
                assert not closes or J < 2 * js2, tag + f": task {idx} of the first part closes a tile of column {J}"
            else:
                assert ke > 2 * js2, tag + f": task {idx} of the second part was ready in the first"
                assert not (closes and J // 2 < js2), tag + f": task {idx} of the second part closes tile ({I}, {J})"
                # all rows are in the band from js2 on: the second part only accumulates band tiles, of strip-columns > js2
                assert (flags & BAND) and J // 2 > js2, tag + f": task {idx} of the second part is not a band accumulation"


@pytest.mark.parametrize("ntile", S.NTILES)
def test_empty_parts(ntile):
    """A matrix of two or three tiles has no bulk task under any shape (the band covers it, and no band tile has a column to
    accumulate: 2 Js - 2 <= 0); js2 = 0 has no first part and only band accumulation; js2 = nsc has no second part; and the first
    tile column whose band tiles accumulate is 4, so with five tiles and more the list is not empty."""
    nsc = S.nsc(ntile)
    for chunk, band_tiles, taper0, js2 in S.grid(ntile):
        tag = f"ntile={ntile} chunk={chunk} band_tiles={band_tiles} taper0={taper0} js2={js2}"
        ts, n1 = _tasks(ntile, chunk, band_tiles, js2, taper0)
        if ntile <= 3:
            assert ts == [] and n1 == 0, tag
            continue
        assert len(ts) > 0, tag
        if js2 == 0:
            assert n1 == 0 and all(f & BAND for f, *_ in ts), tag
        if js2 == nsc:
            assert n1 == len(ts), tag
        if 0 < js2 < nsc:
            # strip-column js2's own band tiles (columns < 2 js2 - 2) and every closing task sit in the first part
            assert all(idx < n1 for idx, (f, q, I, J, kb, ke) in enumerate(ts) if J // 2 == js2 or not (f & BAND)), tag
            # (strip-column Js accumulates the tile columns < 2 Js - 2: ready in the first phase up to Js = js2 + 1, so the second
            # part is empty -- its bulk launch is skipped -- exactly when no strip-column follows js2 + 1)
            assert (n1 == len(ts)) == (js2 >= nsc - 2), tag
    assert FIRST == 4


# ------------------------------------------------------------------------------------------------------------- js2
def _js2(Np, cus2, deep_rows=5376, override=-1):
    return L.lib().mnk_debug_dag_js2(Np, cus2, deep_rows, override)


@pytest.mark.parametrize("Np", [1280, 5376, 5504, 11264])
def test_js2_by_size(Np):
    """Up to dag_deep_rows (and 64 rows per CU of the deep band's partition) every row is in the band; above, and without a deep
    band at all, none."""
    nsc = (Np + 255) // 256
    assert _js2(Np, 0) == nsc
    assert _js2(Np, 96) == (0 if Np <= 5376 else nsc)
    assert _js2(Np, 96, deep_rows=1 << 40) == (0 if Np <= 96 * 64 else nsc)     # (the partition bounds dag_deep_rows)
    assert _js2(Np, 16) == (0 if Np <= 1024 else nsc)
    assert _js2(Np, 96, deep_rows=0) == nsc


def test_js2_override_is_raised_to_the_smallest_admissible_strip_column():
    # 11264 rows are 176 strips; 96 CUs hold the strips of 6144 rows: js2 >= (11264 - 6144) / 256 = 20
    assert _js2(11264, 96, override=0) == 20
    assert _js2(11264, 96, override=19) == 20
    assert _js2(11264, 96, override=20) == 20
    assert _js2(11264, 96, override=21) == 21
    assert _js2(11264, 96, override=44) == 44 == _js2(11264, 96, override=1000)
    # 6400 rows: one strip-column (256 rows) has to go before 96 strips remain
    assert _js2(6400, 96, override=0) == 1
    assert _js2(6400, 96, override=1) == 1
    assert _js2(6144, 96, override=0) == 0
    assert _js2(6272, 96, override=0) == 1       # (6272 - 6144 = 128 rows over: a whole strip-column)
    # no deep band: band + bulk kernel throughout, whatever is asked for
    assert _js2(6400, 0, override=0) == 25 == _js2(6400, 0, override=3)
    # a partition so small that nothing fits: capped at nsc
    assert _js2(1280, 1, override=0) == 5
    assert _js2(1280, 4, override=0) == 4
    # every shape of the device test's orders is admissible on the default partition as it is asked for
    for n, ntile in S.ORDERS.items():
        for js2 in S.js2_values(ntile).values():
            assert _js2(128 * ntile, 96, override=js2) == js2, (n, js2)


def test_js2_never_leaves_the_deep_band_more_strips_than_cus():
    for Np in range(128, 12289, 128):
        nsc = (Np + 255) // 256
        for cus2 in (0, 16, 42, 96):
            for override in range(-1, nsc + 2):
                js2 = _js2(Np, cus2, 5376, override)
                assert 0 <= js2 <= nsc and Np - 256 * js2 <= 64 * cus2, (Np, cus2, override, js2)
                if cus2 and override >= 0 and Np - 256 * min(override, nsc) <= 64 * cus2:
                    assert js2 == min(override, nsc), (Np, cus2, override, js2)


def test_js2_entry_rejects_bad_arguments():
    assert _js2(0, 96) == -1 and _js2(100, 96) == -1 and _js2(1280, -1) == -1 and _js2(1280, 96, deep_rows=-1) == -1

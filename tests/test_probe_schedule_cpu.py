"""The schedule of the leading-block probe (csrc/ls.h: LeadingBlockProbe), host only through mnk_debug_probe_schedule: a fresh
history is run over a sequence of verdicts and reports, in front of each, the order of the block the next matrix would be probed
through.  The rule: a rejection in the first half of the columns re-arms the hint, every other verdict ages it; a probe is due when
the last verdict was an acceptance and the hint is at most three verdicts old, through m = (hint + 256) / 256 * 256 if m >= 512 and
2 m <= N.  The expected orders are worked out by hand from that rule."""
import numpy as np
import pytest

from madnlp_jl_amd import _lib as L


def _orders(N, first_bad_pivots):
    """first_bad_pivots[i]: the first pivot of matrix i that is not positive (-1: none, the matrix is accepted); the leaf stops at
    the end of that pivot's 64-column block."""
    cols = np.array([k // 64 * 64 + 63 if k >= 0 else -1 for k in first_bad_pivots], dtype=np.int64)
    orders = np.full(len(cols), -7, dtype=np.int64)
    assert L.lib().mnk_debug_probe_schedule(N, len(cols), cols.ctypes.data, orders.ctypes.data) == 0
    return orders.tolist()


@pytest.mark.parametrize("N, bad, expected", [
    # the sequence of tests/test_hip_pivot_ladder.py::test_leading_block_probe_gives_the_verdict_of_the_full_factorization_exactly
    (2600, [700, -1, 300, -1, 1000, -1, 1030, -1, -1, 64, -1, 1100, -1, 5, -1],
     [0, 0, 768, 0, 512, 0, 1024, 0, 1280, 1280, 0, 0, 0, 1280, 0]),
    # ageing: the hint serves three acceptances, the fourth verdict behind it is too old
    (2600, [700, -1, -1, -1, -1, -1], [0, 0, 768, 768, 768, 0]),
    # a rejection in the second half ages the hint, it does not re-arm it
    (2600, [700, -1, 2000, -1, -1], [0, 0, 768, 0, 768]),
    # 2 m <= N fails for the smallest block, m = 512
    (1000, [300, -1, -1, 100, -1, -1], [0, 0, 0, 0, 0, 0]),
], ids=["ladder_sequence", "ageing", "second_half_ages", "too_small"])
def test_probe_schedule(N, bad, expected):
    assert _orders(N, bad) == expected


def test_probe_schedule_refuses_bad_arguments():
    assert L.lib().mnk_debug_probe_schedule(0, 0, None, None) == -1
    assert L.lib().mnk_debug_probe_schedule(2600, 2, None, None) == -1
    assert L.lib().mnk_debug_probe_schedule(2600, 0, None, None) == 0

"""The CU-mask rules of the hot path (csrc/stream_plan.hip), without a GPU: which mask bits the two streams of every CU-masked
pair get (`mnk_debug_stream_split`) and the chain partitions of a round of small factorizations (`mnk_debug_small_rounds`).
The expectations below restate the rules as they stood inline in the executor before the planner existed -- two masked streams
per pair, made by the first context of a device (task-DAG pair), the first deep-band factorization, the first large batch, the
first round of small systems of a size, the first look-ahead factorization -- they are not taken from the planner."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madnlp_jl_amd import _lib as L  # noqa: E402

DAG, DEEP, BATCH, SMALL, PANEL = range(5)
NUM_CU = (16, 32, 63, 64, 96, 128, 255, 256, 304)
SENTINEL = 0xDEADBEEF


def _split(kind, num_cu, dag_cus, dag_cus2, arg):
    words = (num_cu + 31) // 32
    split = np.full(5, -77, dtype=np.int32)
    mc = np.full(words + 1, SENTINEL, dtype=np.uint32)
    mr = np.full(words + 1, SENTINEL, dtype=np.uint32)
    rc = L.lib().mnk_debug_stream_split(kind, num_cu, dag_cus, dag_cus2, arg, split.ctypes.data, mc.ctypes.data, mr.ctypes.data)
    assert rc in (0, 1)
    assert split[4] == -77 and mc[words] == SENTINEL and mr[words] == SENTINEL   # nothing written behind the arrays
    return rc == 1, tuple(int(x) for x in split[:4]), mc[:words], mr[:words]


def _mask(num_cu, first, count):
    """The words the executor handed to the runtime: bit b of word b / 32 for every listed bit inside the device."""
    m = np.zeros((num_cu + 31) // 32, dtype=np.uint32)
    for b in range(first, first + count):
        if 0 <= b < num_cu:
            m[b // 32] |= np.uint32(1 << (b % 32))
    return m


def _bits(m):
    return {32 * w + b for w in range(len(m)) for b in range(32) if (int(m[w]) >> b) & 1}


def _expected(kind, num_cu, dag_cus, dag_cus2, arg):
    """(chain_first, chain_count, rest_first, rest_count) or None where no pair was made."""
    dag = num_cu >= 64 and 0 < dag_cus < num_cu           # the first context of a device: from 64 CUs on, MNK_DAG_CUS inside the device
    if kind == DAG:
        return (0, dag_cus, dag_cus, num_cu - dag_cus) if dag else None
    if kind == DEEP:                                       # dag_cus2 = 0 without the first pair, and outside (0, num_cu)
        return (0, dag_cus2, dag_cus2, num_cu - dag_cus2) if dag and 0 < dag_cus2 < num_cu else None
    if kind == BATCH:                                      # the next dag_cus bits | the CUs outside both: at least 32 of them
        return (dag_cus, dag_cus, 2 * dag_cus, num_cu - 2 * dag_cus) if dag and not (2 * dag_cus + 32 > num_cu) else None
    if kind == SMALL:                                      # the first chain_cus bits | all the others, none when it is the whole device
        return (0, arg, arg, num_cu - arg) if 0 < arg <= num_cu else None
    if kind == PANEL:
        return (0, arg, arg, num_cu - arg) if 0 < arg < num_cu else None
    raise AssertionError(kind)


def _args(kind, num_cu):
    if kind == SMALL:
        return sorted(set(range(64, num_cu + 1, 64)) | {0, num_cu, num_cu + 64})
    if kind == PANEL:
        return [0, 4, num_cu // 4, num_cu]
    return [0]


@pytest.mark.parametrize("kind", [DAG, DEEP, BATCH, SMALL, PANEL])
def test_split_and_mask_words_of_every_pair_kind(kind):
    made = 0
    for num_cu in NUM_CU:
        for dag_cus in (0, 8, 16, 32):
            for dag_cus2 in (0, 96, num_cu):
                for arg in _args(kind, num_cu):
                    exists, split, mc, mr = _split(kind, num_cu, dag_cus, dag_cus2, arg)
                    want = _expected(kind, num_cu, dag_cus, dag_cus2, arg)
                    what = (kind, num_cu, dag_cus, dag_cus2, arg)
                    assert exists == (want is not None), what        # "no such pair" exactly where none was made
                    if want is None:
                        assert split == (0, 0, 0, 0) and not mc.any() and not mr.any(), what
                        continue
                    made += 1
                    assert split == want, what
                    assert np.array_equal(mc, _mask(num_cu, want[0], want[1])) and np.array_equal(mr, _mask(num_cu, want[2], want[3])), what
                    bc, br = _bits(mc), _bits(mr)
                    assert not (bc & br), what                                              # disjoint
                    assert all(0 <= b < num_cu for b in bc | br), what                      # inside the device: no bit at or above num_cu
                    assert len(bc) == split[1] and len(br) == split[3], what                # popcounts = the split
                    assert bc == set(range(split[0], split[0] + split[1])) and br == set(range(split[2], split[2] + split[3])), what
                    assert split[1] > 0 and (split[3] > 0 or (kind == SMALL and arg == num_cu)), what
    assert made > 0


def test_default_panel_split_is_a_quarter_of_the_device():
    """Without MNK_PANEL_CUS the panel stream got max(4, num_cu / 4) CUs, on devices of at least 16 CUs."""
    for num_cu in (1, 8, 15) + NUM_CU:
        exists, split, _, _ = _split(PANEL, num_cu, 16, 96, -1)
        q4 = max(4, num_cu // 4)
        assert exists == (num_cu >= 16), num_cu
        assert split == ((0, q4, q4, num_cu - q4) if exists else (0, 0, 0, 0)), num_cu


def test_stream_split_rejects_bad_arguments():
    buf = np.zeros(16, dtype=np.uint32)
    f = L.lib().mnk_debug_stream_split
    assert f(5, 256, 16, 96, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == -1
    assert f(-1, 256, 16, 96, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == -1
    assert f(0, 0, 16, 96, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == -1
    assert f(0, 256, 16, 96, 0, None, buf.ctypes.data, buf.ctypes.data) == -1
    assert L.lib().mnk_debug_small_rounds(0, 256, 1, 1, buf.ctypes.data) == -1


def _rounds(strips, num_cu, has_bulk, k):
    out = np.full(4, -77, dtype=np.int32)
    assert L.lib().mnk_debug_small_rounds(strips, num_cu, int(has_bulk), k, out.ctypes.data) == 0
    assert out[3] == -77
    return int(out[0]), int(out[1]), int(out[2])


@pytest.mark.parametrize("has_bulk", [False, True])
def test_chain_partitions_of_small_system_rounds(has_bulk):
    """Rounds of k small systems of `strips` 64-row strips: the chains need a CU per strip, ALL resident, which the dispatcher only
    grants on masks that give every shader engine of every XCD the same number of CUs (multiples of 32; of 64 to keep the number
    of stream pairs down) -- five 34-strip systems on 176 CUs stalled into the schedule's time-out."""
    num_cu = 256
    for strips in (4, 8, 11, 20, 34, 40, 84):
        # the loop as it stood in the batch driver
        bulk_min = max(32, num_cu // 4) if has_bulk else 0
        chain = lambda k: min(num_cu, (k * strips + 63) // 64 * 64)   # noqa: E731
        kmax = min(32, (num_cu - bulk_min) // strips)
        while kmax > 1 and chain(kmax) > num_cu - bulk_min:
            kmax -= 1
        got_min, got_kmax, _ = _rounds(strips, num_cu, has_bulk, 1)
        assert (got_min, got_kmax) == (bulk_min, kmax), strips
        assert kmax >= 2, strips                                       # (every one of these sizes runs in rounds on 256 CUs)
        for k in range(1, kmax + 1):
            c = _rounds(strips, num_cu, has_bulk, k)[2]
            assert c == chain(k), (strips, k)
            assert c % 64 == 0 or c == num_cu, (strips, k)
            assert k * strips <= c, (strips, k)
            if has_bulk:
                assert num_cu - c >= bulk_min, (strips, k)
    # the documented stall: five systems of 34 strips get 192 CUs (or the round takes fewer systems), never 176
    _, kmax34, c5 = _rounds(34, num_cu, True, 5)
    assert c5 != 176 and (c5 == 192 or kmax34 < 5)
    assert _rounds(34, num_cu, True, min(5, kmax34))[2] <= 192

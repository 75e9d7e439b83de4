"""Host logic of the per-XCD task queues of the task-DAG schedule (csrc/dag.hip: dag_deal_tasks), without a GPU.  The finished task
list is PARTITIONED into eight queues; the bulk kernel's workgroups pop the head of their own XCD's queue and steal from the head of
the fullest other queue once their own is exhausted.  Checked here: the partition (every queue a subsequence of the list), the load
balance at every position of the list, how much of the K-loop work lands behind a gang-mate (same B rows, same k-range), and -- by a
replay of the pop rule over random service times -- that every list is finished whatever the timing."""
import ctypes as C
import heapq
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madnlp_jl_amd import _lib as L  # noqa: E402

BAND, FINAL, FIRST, FILL = 1, 2, 4, 8
NQ = 8
CHUNK, BAND_TILES, TAPER0 = 64, 8, 2          # the shipped settings: dag_chunk 64, dag_band 16 strips = 8 tile rows, dag_taper0 2
NTILES = (10, 12, 44, 88, 154, 240)
DEEP_TILES = 42                                # orders up to 5376 rows put every row into the chain's band (dag_deep_rows): js2 = 0


def _js2(ntile):
    return 0 if ntile <= DEEP_TILES else (ntile + 1) // 2


def _deal(ntile, gang, fill, nq=NQ, ninst=1, period=0):
    cap = 1200000
    tasks = np.zeros(4 * cap, dtype=np.int32)
    order = np.zeros(cap, dtype=np.int32)
    off = np.zeros(2 * (nq + 1), dtype=np.int32)
    n1 = C.c_int(0)
    n = L.lib().mnk_debug_dag_deal(ntile, CHUNK, BAND_TILES, _js2(ntile), TAPER0, int(fill), ninst, period, nq, gang,
                                   tasks.ctypes.data, order.ctypes.data, cap, off.ctypes.data, C.byref(n1))
    assert 0 <= n <= cap
    t = tasks[: 4 * n].reshape(n, 4).astype(np.int64)
    T = dict(flags=t[:, 0] & 255, q=t[:, 0] >> 8, I=t[:, 1] & 0xffff, inst=t[:, 1] >> 16, J=t[:, 2], kb=t[:, 3] & 0xffff, ke=t[:, 3] >> 16)
    T["ksteps"] = np.where(T["flags"] & FILL, 0, T["ke"] - T["kb"])
    return T, order[:n].astype(np.int64), off.reshape(2, nq + 1).astype(np.int64), n1.value, n


def _queues(order, off):
    """[(phase, [positions of queue 0], ...)]"""
    return [[order[off[ph][x]: off[ph][x + 1]] for x in range(off.shape[1] - 1)] for ph in range(2)]


CASES = [(nt, g, fill) for nt in NTILES for g in (1, 2, 4, 8) for fill in (0, 1)]


@pytest.mark.parametrize("ntile,gang,fill", CASES)
def test_partition_and_balance(ntile, gang, fill):
    T, order, off, n1, n = _deal(ntile, gang, fill)
    _check_partition_and_balance(T, order, off, n1, n, gang)


def _check_partition_and_balance(T, order, off, n1, n, gang):
    assert sorted(order.tolist()) == list(range(n))            # every task in exactly one queue
    assert off[0][0] == 0 and off[0][-1] == n1 == off[1][0] and off[1][-1] == n
    kmax = int(T["ksteps"].max()) if n else 0
    for ph, (t0, t1) in enumerate(((0, n1), (n1, n))):
        qs = _queues(order, off)[ph]
        dealt = np.zeros((len(qs), t1 - t0), dtype=np.int64)   # k-steps per list position, by queue
        for x, qx in enumerate(qs):
            assert np.all(np.diff(qx) > 0)                      # a subsequence of the list in list order
            assert np.all((qx >= t0) & (qx < t1))               # ... of its own phase
            dealt[x, qx - t0] = T["ksteps"][qx]
        if t1 > t0:
            load = np.cumsum(dealt, axis=1)                     # at every prefix of the list
            spread = load.max(axis=0) - load.min(axis=0)
            assert spread.max() <= (gang + 1) * kmax, (ph, spread.max(), gang, kmax)
            # (the sharper statement of "one gang's k-steps plus one task's": no gang of this list is heavier than that)
            assert spread.max() <= _heaviest_gang(T, t0, t1, gang) + kmax


def _heaviest_gang(T, t0, t1, gang):
    best, run, runk = 0, 0, 0
    key = None
    for t in range(t0, t1):
        f = int(T["flags"][t])
        chunk = not (f & FILL) and ((f & BAND) or not (f & FINAL))
        k = (int(T["inst"][t]), f & (BAND | FINAL), int(T["J"][t]), int(T["kb"][t]), int(T["ke"][t])) if chunk else None
        if k is not None and k == key and run < gang:
            run, runk = run + 1, runk + int(T["ksteps"][t])
        else:
            key, run, runk = k, 1, int(T["ksteps"][t])
        best = max(best, runk)
    return best


def _sharing(T, order, off):
    """share of the K-loop k-steps (body chunks and band accumulation) whose task follows a gang-mate in its queue"""
    kloop = (~(T["flags"] & FILL).astype(bool)) & (((T["flags"] & BAND) != 0) | ((T["flags"] & FINAL) == 0))
    shared = 0
    for ph in range(2):
        for qx in _queues(order, off)[ph]:
            if len(qx) < 2:
                continue
            a, b = qx[:-1], qx[1:]
            mate = kloop[a] & kloop[b] & (T["J"][a] == T["J"][b]) & (T["kb"][a] == T["kb"][b]) & (T["ke"][a] == T["ke"][b]) & (T["inst"][a] == T["inst"][b])
            shared += int(T["ksteps"][b][mate].sum())
    return shared / int(T["ksteps"][kloop].sum())


def test_sharing_on_the_bench_list():
    """ntile 88 (N = 11 192), no zero-fill tasks: the 18 299 tasks of DESIGN.md section 5c.  Below these shares the queues cannot do
    what they are for."""
    shares, loads = {}, {}
    for gang in (1, 2, 4, 8):
        T, order, off, n1, n = _deal(88, gang, 0)
        assert n == 18299
        shares[gang] = _sharing(T, order, off)
        loads[gang] = [int(T["ksteps"][qx].sum()) for qx in _queues(order, off)[0]]
    print("share of K-loop k-steps behind a gang-mate:", {g: round(s, 3) for g, s in shares.items()})
    print("k-steps per queue:", loads)
    assert shares[2] >= 0.45 and shares[4] >= 0.70
    assert shares[1] <= shares[2] <= shares[4] <= shares[8]
    for g, ld in loads.items():   # (what the balance at every prefix implies for the totals: within one gang plus one task)
        assert max(ld) - min(ld) <= (g + 1) * CHUNK, (g, ld)
    T, order, off, n1, n = _deal(88, 4, 1)   # (with the zero-fill tasks between them)
    assert _sharing(T, order, off) >= 0.60


@pytest.mark.parametrize("ntile", NTILES)
def test_one_queue_is_the_list(ntile):
    for fill in (0, 1):
        T, order, off, n1, n = _deal(ntile, 4, fill, nq=1)
        assert order.tolist() == list(range(n))
        assert off.tolist() == [[0, n1], [n1, n]]


def test_negative_gang_deals_everything_to_queue_0():
    T, order, off, n1, n = _deal(88, -1, 1)
    assert order.tolist() == list(range(n))
    assert off[0].tolist() == [0] + [n1] * NQ


def test_merged_list_of_three_instances():
    for ntile, period in ((44, 22), (88, 44), (154, 80)):
        for gang in (1, 4):
            T, order, off, n1, n = _deal(ntile, gang, 1, ninst=3, period=period)
            assert n1 == n and set(T["inst"].tolist()) == {0, 1, 2}
            _check_partition_and_balance(T, order, off, n1, n, gang)
            _replay(T, order, off, n1, n, workers=2, seed=ntile + gang)


# ---------------------------------------------------------------------------------------------------------------------
# Replay of the pop rule.  Dependences from the task fields: the chunks of a tile are applied in order (a chunk waits for the one in
# front of it), and a task that reads tile columns [.., kend) of rows I and J waits for the closing tasks (row, kend - 1) of both rows
# where the bulk kernel closes them (the closing tasks of a row wait for each other in column order; rows inside the band are the
# pivot chain's, which waits only for tasks whose operands it has produced itself).  A worker holds its task while it waits.
def _deps(T, n):
    close, chunk, lastclose = {}, {}, {}
    for t in range(n):
        f = int(T["flags"][t])
        if f & FILL:
            continue
        inst, I, J = int(T["inst"][t]), int(T["I"][t]), int(T["J"][t])
        chunk[(inst, I, J, int(T["q"][t]))] = t
        if (f & FINAL) and not (f & BAND):
            close[(inst, I, J)] = t
            lastclose[(inst, I)] = max(lastclose.get((inst, I), -1), J)
    deps = [[] for _ in range(n)]
    for t in range(n):
        f = int(T["flags"][t])
        if f & FILL:
            continue
        inst, I, J, q, ke = int(T["inst"][t]), int(T["I"][t]), int(T["J"][t]), int(T["q"][t]), int(T["ke"][t])
        if q > 0:
            deps[t].append(chunk[(inst, I, J, q - 1)])
        for row in (I, J):
            k = min(ke - 1, lastclose.get((inst, row), -1))
            if (f & FINAL) and not (f & BAND) and row == I:
                k = min(k, J - 1)
            if k >= 0 and close[(inst, row, k)] != t:
                deps[t].append(close[(inst, row, k)])
    return deps


def _replay(T, order, off, n1, n, workers, seed):
    rng = np.random.default_rng(seed)
    service = rng.exponential(1.0, n) * (1 + T["ksteps"])
    deps = _deps(T, n)
    for t in range(n):
        assert all(d < t for d in deps[t])        # (the list's own property: every dependence points backwards)
    waiters = [[] for _ in range(n)]
    for t in range(n):
        for d in deps[t]:
            waiters[d].append(t)
    missing = [len(d) for d in deps]
    done = np.zeros(n, dtype=bool)
    popped = np.zeros(n, dtype=bool)
    stolen = 0
    now = 0.0
    for ph, (t0, t1) in enumerate(((0, n1), (n1, n))):   # (a phase is a launch of its own)
        if t1 == t0:
            continue
        qs = _queues(order, off)[ph]
        nq = len(qs)
        head = [0] * nq
        heap = []    # (time, kind, task | worker): kind 0 = a task finishes, 1 = a worker is free
        holder = {}
        finished = 0

        def pop(x):
            nonlocal stolen
            if head[x] < len(qs[x]):                  # the head of the own queue ...
                head[x] += 1
                return int(qs[x][head[x] - 1])
            left = [len(qs[y]) - head[y] for y in range(nq)]   # ... and only when that is exhausted the head of the fullest one
            y = int(np.argmax(left))
            if left[y] <= 0:
                return -1
            head[y] += 1
            stolen += 1
            return int(qs[y][head[y] - 1])

        for w in range(nq * workers):
            heapq.heappush(heap, (now + 1e-3 * rng.random(), 1, w))
        while heap:
            now, kind, who = heapq.heappop(heap)
            if kind == 1:
                t = pop(who % nq)
                if t < 0:
                    continue
                popped[t] = True
                holder[t] = who
                if missing[t] == 0:
                    heapq.heappush(heap, (now + service[t], 0, t))
            else:
                t = who
                assert missing[t] == 0 and popped[t] and not done[t]
                done[t] = True
                finished += 1
                for u in waiters[t]:
                    missing[u] -= 1
                    if missing[u] == 0 and popped[u]:
                        heapq.heappush(heap, (now + service[u], 0, u))
                heapq.heappush(heap, (now, 1, holder.pop(t)))
        assert finished == t1 - t0, f"phase {ph}: the replay stopped with {t1 - t0 - finished} tasks unfinished ({len(holder)} held by waiting workers)"
    assert done.all()
    return stolen


@pytest.mark.parametrize("ntile,gang,fill", CASES + [(88, -1, 1), (44, -1, 0)])
def test_replay_finishes_every_list(ntile, gang, fill):
    T, order, off, n1, n = _deal(ntile, gang, fill)
    # (few workers per queue: the argument holds for any grid with a workgroup on every XCD -- one per XCD is the hardest case)
    for workers, seed in ((1, 1), (3, 2)) if ntile <= 88 else ((1, 1),):
        stolen = _replay(T, order, off, n1, n, workers, seed + ntile)
        if gang < 0 and n:
            assert stolen >= (n * 3) // 4

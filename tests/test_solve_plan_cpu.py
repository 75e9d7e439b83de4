"""The planner of solve! (csrc/solve_plan.hip), host only through mnk_debug_solve_plan and mnk_debug_solve_batch_groups: which way a
single solve runs and on how many workgroups, which solves a batch may queue, and how a batch's queue becomes launches.

The reference of the comparisons is a restatement of the rules as they stood inline in csrc/solve.hip before the planner existed
(mnk_ls_run_solve, solve_eligible, the loop of solve_batch_flush and the G of solve_batch_launch), written out below -- not the
planner.  The invariants are what the kernels need: every workgroup of a launch resident (one per CU), at most 12 blocks per
workgroup, one right-hand side per solver and launch, a solver's right-hand sides in queue order."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

from madnlp_jl_amd import _lib as L

STEPWISE, ONE_256, ONE_512, MERGED = 1, 2, 3, 4
MAXOWN = 12
NPS = list(range(64, 8192 + 1, 64)) + [11200, 16384, 16448, 85568, 196608, 196672]
CUS = (1, 2, 3, 4, 16, 64, 240, 256)
FLAGS = ("pivoted", "persistent_opt", "solve512_opt", "have_linv512", "partitioned", "abort_raised", "debug_missing", "tracing", "ldl")


def ceil_div(a, b):
    return -(-a // b)


def plan(Np, num_cu, linv_mfma=1, **flags):
    out = (C.c_int * 5)(-1, -1, -1, -1, -1)
    assert L.lib().mnk_debug_solve_plan(Np, num_cu, *(int(flags.get(f, 0)) for f in FLAGS), linv_mfma, out) == 0
    return {"path": out[0], "G": out[1], "batchable": bool(out[2]), "want512": bool(out[3]), "inv_batchable": bool(out[4])}


# ---- the rules as they stood in solve.hip ----
def parent_single(Np, num_cu, pivoted, persistent_opt, solve512_opt, have_linv512):
    nb64 = Np // 64
    G = min(nb64, num_cu)
    persistent = (not pivoted) and persistent_opt and G >= 1 and ceil_div(nb64, G) <= MAXOWN and (G >= 4 or nb64 <= G)
    nb32 = Np // 32
    G5 = min(nb32, num_cu)
    use512 = persistent and solve512_opt and have_linv512 and ceil_div(nb32, G5) <= MAXOWN and (G5 >= 16 or nb32 <= G5)
    return (ONE_512, G5) if use512 else (ONE_256, G) if persistent else (STEPWISE, 0)


def parent_eligible(Np, num_cu, pivoted, persistent_opt, solve512_opt, have_linv512, partitioned, abort_raised, debug_missing, tracing):
    nb64 = Np // 64
    G = min(nb64, num_cu)
    return bool((not pivoted) and persistent_opt and not (solve512_opt and have_linv512) and (not partitioned) and
                ceil_div(nb64, G) <= MAXOWN and (G >= 4 or nb64 <= G) and (not abort_raised) and (not debug_missing) and not tracing)


def parent_groups(reqs):
    """reqs: (solver, device, Np, ldl, num_cu) in queue order -> [(indices, G)]; G = 0 for a launch of one (an ordinary solve)."""
    pend, out = list(range(len(reqs))), []
    while pend:
        _, dev0, Np0, ldl0, cu0 = reqs[pend[0]]
        nb64 = Np0 // 64
        g4 = max(1, min(nb64, cu0 // 4))
        maxq = max(1, min(32, cu0 // g4))
        g, rest = [], []
        for i in pend:
            sid, dev, Np, ldl, _ = reqs[i]
            take = len(g) < maxq and dev == dev0 and Np == Np0 and ldl == ldl0
            take = take and all(reqs[t][0] != sid for t in g) and all(reqs[t][0] != sid for t in rest)
            if take:
                Gq = min(nb64, cu0 // (len(g) + 1))
                take = (Gq >= 4 or nb64 <= Gq) and ceil_div(nb64, Gq) <= MAXOWN
                take = take or not g
            (g if take else rest).append(i)
        pend = rest
        out.append((g, min(nb64, cu0 // len(g)) if len(g) >= 2 else 0))   # (the G solve_batch_launch computed for itself)
    return out


def groups(reqs):
    n = len(reqs)
    cols = [np.array([r[k] for r in reqs], dtype=dt) for k, dt in enumerate((np.int64, np.int32, np.int64, np.int32, np.int32))]
    begin, idx, G = np.full(n + 1, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    nl = L.lib().mnk_debug_solve_batch_groups(n, *(c.ctypes.data for c in cols), begin.ctypes.data, idx.ctypes.data, G.ctypes.data)
    assert 0 <= nl <= n and begin[0] == 0 and begin[nl] == n
    return [(idx[begin[l]:begin[l + 1]].tolist(), int(G[l])) for l in range(nl)]


# ---- single plans ----
def test_single_plans_over_the_grid_match_the_inline_rules_and_what_the_kernels_need():
    rest = list(itertools.product((0, 1), repeat=len(FLAGS) - 4))
    entry, out = L.lib().mnk_debug_solve_plan, (C.c_int * 5)()
    seen = set()
    for Np, cu in itertools.product(NPS, CUS):
        want512 = int(Np >= 4096 and Np % 512 != 384)
        for head in itertools.product((0, 1), repeat=4):   # pivoted, persistent_opt, solve512_opt, have_linv512: all the path depends on
            pivoted, _, solve512_opt, have_linv512 = head
            ref = parent_single(Np, cu, *head)
            path, G = ref   # (every plan below is asserted equal to it, so what holds for it holds for them)
            seen.add(path)
            if path != STEPWISE:
                blocks = Np // (64 if path == ONE_256 else 32)
                assert 1 <= G <= cu and ceil_div(blocks, G) <= MAXOWN, (Np, cu, head, ref)
            assert not pivoted or path == STEPWISE
            if path == ONE_512:
                assert solve512_opt and have_linv512 and (G >= 16 or G == Np // 32), (Np, cu, head, ref)
            for tail in rest:
                assert entry(Np, cu, *head, *tail, 1, out) == 0
                assert (out[0], out[1]) == ref and out[3] == want512, (Np, cu, head, tail, out[:], ref)
                assert out[2] == parent_eligible(Np, cu, *head, *tail[:4]), (Np, cu, head, tail, out[:])
                assert not out[2] or out[0] == ONE_256
    assert seen == {STEPWISE, ONE_256, ONE_512}


def test_inverses_of_a_batch_round_and_bad_arguments():
    for mfma, s512 in itertools.product((0, 1), repeat=2):
        assert plan(2048, 256, linv_mfma=mfma, solve512_opt=s512)["inv_batchable"] == bool(mfma and not s512)
    out = (C.c_int * 5)()
    f = L.lib().mnk_debug_solve_plan
    assert f(100, 256, *([0] * 9), 1, out) == -1 and f(0, 256, *([0] * 9), 1, out) == -1
    assert f(512, 0, *([0] * 9), 1, out) == -1 and f(512, 256, *([0] * 9), 1, None) == -1
    g = L.lib().mnk_debug_solve_batch_groups
    one = np.zeros(1, np.int32)
    assert g(-1, *([None] * 8)) == -1 and g(0, *([None] * 5), one.ctypes.data, None, None) == 0
    assert g(1, *([None] * 5), one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1


# ---- groups ----
def check_groups(reqs, got):
    n = len(reqs)
    flat = [i for g, _ in got for i in g]
    assert sorted(flat) == list(range(n)), "every request is in exactly one launch"
    last = {}
    for l, (g, G) in enumerate(got):
        assert g == sorted(g) and len(g) >= 1
        _, dev0, Np0, ldl0, cu0 = reqs[g[0]]
        assert all(reqs[i][1:4] == (dev0, Np0, ldl0) for i in g), "a launch's requests share device, order and algorithm"
        sids = [reqs[i][0] for i in g]
        assert len(set(sids)) == len(sids), "... and name distinct solvers"
        nb64 = Np0 // 64
        g4 = max(1, min(nb64, cu0 // 4))
        assert len(g) <= max(1, min(32, cu0 // g4))
        if len(g) >= 2:
            q = len(g)
            assert G == min(nb64, cu0 // q) and G >= 1 and q * G <= cu0 and ceil_div(nb64, G) <= MAXOWN, (g, G)
        else:
            assert G == 0
        for i in g:   # for every solver, its requests appear in launches in queue order
            sid = reqs[i][0]
            assert sid not in last or (last[sid][0] < l and last[sid][1] < i), (sid, last.get(sid), l, i)
            last[sid] = (l, i)


def random_list(rng):
    nsolvers = rng.randint(1, 8)
    solvers = [(1000 + 8 * k, rng.randrange(2), rng.choice((512, 2048, 6400, 11200, 131072)), rng.randrange(2), rng.choice((16, 64, 256)))
               for k in range(nsolvers)]
    kind = rng.randrange(3)
    if kind == 0:   # the common case: solvers of one shape
        shape = solvers[0][2:]
        solvers = [(s[0], s[1]) + shape for s in solvers]
    reqs = [rng.choice(solvers) for _ in range(rng.randint(0, 40))]
    if kind == 2:   # every field of every request on its own: no real queue (a solver has one device, order and algorithm), but the
        # planner's input allows it, and only here does "a solver's right-hand sides keep their order" need a rule of its own
        reqs = [(r[0], rng.randrange(2), rng.choice((512, 2048, 6400, 11200, 131072)), rng.randrange(2), rng.choice((16, 64, 256)))
                for r in reqs]
    return reqs


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_queues_group_as_the_inline_loop_did(seed):
    rng = random.Random(seed)
    sizes = set()
    for _ in range(1000):
        reqs = random_list(rng)
        got = groups(reqs)
        check_groups(reqs, got)
        assert got == parent_groups(reqs), reqs
        sizes.update(len(g) for g, _ in got)
    assert {1, 2, 3, 4} <= sizes and max(sizes) >= 5   # (merged launches of large and of small systems both occur)


def distinct(n, Np, cu, dev=0, ldl=1):
    return [(100 + i, dev, Np, ldl, cu) for i in range(n)]


def test_hand_worked_queues():
    # (a) 175 blocks on 256 CUs: g4 = 64, four systems per launch at most; G = min(175, 256 / 4) and min(175, 256 / 2)
    assert groups(distinct(6, 11200, 256)) == [([0, 1, 2, 3], 64), ([4, 5], 128)]
    # (b) A B A C: A's second right-hand side waits for the next launch, C does not wait with it
    A, B, Cc = (1, 0, 11200, 1, 256), (2, 0, 11200, 1, 256), (3, 0, 11200, 1, 256)
    assert groups([A, B, A, Cc]) == [([0, 1, 3], 85), ([2], 0)]
    # (c) 100 blocks on 16 CUs: two systems would leave 8 workgroups each, 13 blocks per workgroup
    assert groups(distinct(3, 6400, 16)) == [([0], 0), ([1], 0), ([2], 0)]
    # (d) 8 blocks on 256 CUs: 32 systems of 8 workgroups fill the chip
    assert groups(distinct(40, 512, 256)) == [(list(range(32)), 8), (list(range(32, 40)), 8)]
    # (e) two devices, alternating
    reqs = [(100 + i, i % 2, 2048, 0, 256) for i in range(6)]
    assert groups(reqs) == [([0, 2, 4], 32), ([1, 3, 5], 32)]
    # ... and two algorithms or two orders on one device do not mix either
    reqs = [(1, 0, 2048, 0, 256), (2, 0, 2048, 1, 256), (3, 0, 4096, 0, 256), (4, 0, 2048, 0, 256)]
    assert groups(reqs) == [([0, 3], 32), ([1], 0), ([2], 0)]

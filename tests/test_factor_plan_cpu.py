"""The step lists of the launch-per-panel factorization schedules (panel_algo 1 and 4; csrc/factor_plan.hip), host only through
mnk_debug_factor_plan: a small simulator replays a list and checks what every list must satisfy (csrc/factor_plan.h):

  (a) every 64-column block is factored exactly once and in order;
  (b) when a block is factored (leaf / solve, or inside a persistent panel, whose fused prologue applies its K columns to the
      launch's own columns), every earlier block's contribution has been applied to it exactly once -- the two launches of one
      shared tile queue count as one update;
  (c) every block an update reads as source is factored, and that happens-before the update;
  (d) two steps that touch the same block or the same W buffer, at least one of them writing, are ordered (the two launches of one
      shared queue excepted);
  (e) all streams are joined into the caller's stream at the end.

Order is stream order plus record -> wait edges, tracked with vector clocks over the three streams.  A wait takes the event as it
was recorded last before the wait was enqueued, as the runtime does."""
import ctypes as C
import itertools

import numpy as np
import pytest

from madnlp_jl_amd import _lib as L

LEAF, TRSM, PPANEL, UPDATE, RECORD, WAIT = 1, 2, 3, 4, 5, 6
CALLER, PANEL, UPD = 0, 1, 2
SMALL, PLAIN, QUEUE = 0, 1, 2
EV_A, EV_B, EV_PANEL, EV_NEXT, EV_NEXT2, EV_BDONE = range(6)
FIELDS = ("kind", "stream", "col", "n", "rows", "src", "K", "variant", "slot", "cus", "whalf", "wko", "rhalf", "rko", "event", "index")
F = {name: i for i, name in enumerate(FIELDS)}
NUM_CU = 256


def plan(Np, ldl, algo, lookahead, width, fuse_rows=4096, share=1, small_tiles=400, panel_cus=64):
    cap = 8 * (Np // 64) + 64
    out = np.full((cap, len(FIELDS)), -77, dtype=np.int32)
    shape = (C.c_int * 2)(-1, -1)
    n = L.lib().mnk_debug_factor_plan(Np, int(ldl), algo, int(lookahead), width, fuse_rows, share, small_tiles, NUM_CU, panel_cus,
                                      out.ctypes.data, cap, shape)
    assert 0 < n <= cap
    return out[:n], (shape[0], bool(shape[1]))


class Violation(AssertionError):
    pass


def simulate(steps, Np, ldl):
    """Replays `steps` (rows of FIELDS); raises Violation at the first broken invariant."""
    nb = Np // 64
    clock = np.zeros((3, 3), dtype=np.int64)        # clock[s]: the vector clock of stream s
    wrote = np.zeros((nb + 2, 3), dtype=np.int64)   # per resource (blocks, then the two W buffers) and stream: time of its last write
    read = np.zeros((nb + 2, 3), dtype=np.int64)    # ... of its last read
    applied = np.zeros((nb, nb), dtype=np.int64)    # applied[dst, src]: updates of block dst by block src
    factored = np.zeros(nb, dtype=bool)
    events, queues = {}, {}
    wcols = [None, None]   # the matrix columns [lo, hi) a W buffer holds, all of one outer panel
    state = {"next": 0, "solve_due": None}

    def need(cond, what, i):
        if not cond:
            raise Violation(f"step {i} {dict(zip(FIELDS, steps[i].tolist()))}: {what}")

    def access(i, s, reads, writes, partner=None):
        clock[s, s] += 1
        now = clock[s]
        for r in reads:
            need((wrote[r] <= now).all(), f"(d) reads resources {r} that an unordered step writes", i)
        for r in writes:
            late = wrote[r] > now
            if partner is not None:   # the other launch of the same shared queue
                late[:, partner[0]] &= wrote[r][:, partner[0]] != partner[1]
            need(not late.any() and (read[r] <= now).all(), f"(d) writes resources {r} that an unordered step touches", i)
        for r in reads:
            read[r, s] = now[s]
        for r in writes:
            wrote[r, s] = now[s]
        return int(now[s])

    def blocks(col, ncols):
        return slice(col // 64, (col + ncols) // 64)

    def factor_block(i, b):
        need(b == state["next"], "(a) blocks are factored once and in order", i)
        need((applied[b, :b] == 1).all() and (applied[b, b:] == 0).all(), "(b) every earlier block applied exactly once", i)
        factored[b] = True
        state["next"] = b + 1

    def w_written(i, t, col, ncols):
        h = t[F["whalf"]]
        need((h in (0, 1)) == ldl, "a W buffer is written iff LDL^T", i)
        if not ldl:
            return []
        if wcols[h] is None or wcols[h][0] != t[F["wko"]]:
            wcols[h] = [t[F["wko"]], t[F["wko"]]]
        need(wcols[h][1] == col, "W columns are written in order", i)
        wcols[h][1] = col + ncols
        return [slice(nb + h, nb + h + 1)]

    def w_read(i, t):
        h = t[F["rhalf"]]
        need((h in (0, 1)) == ldl, "a W buffer is read iff LDL^T", i)
        if not ldl:
            return []
        need(wcols[h] is not None and wcols[h][0] == t[F["rko"]] and wcols[h][0] <= t[F["src"]]
             and t[F["src"]] + t[F["K"]] <= wcols[h][1], "the W buffer holds the source columns", i)
        return [slice(nb + h, nb + h + 1)]

    for i, t in enumerate(steps.tolist()):
        kind, s, col, n = t[F["kind"]], t[F["stream"]], t[F["col"]], t[F["n"]]
        need(s in (CALLER, PANEL, UPD), "stream", i)
        if kind in (LEAF, PPANEL):
            need(state["solve_due"] is None, "a leaf with rows below it is followed by its solve", i)
        if kind == LEAF:
            access(i, s, [], [blocks(col, 64)])
            factor_block(i, col // 64)
            state["solve_due"] = col if col + 64 < Np else None
        elif kind == TRSM:
            need(state["solve_due"] == col and n in (1, 2), "the solve of the block just factored", i)
            state["solve_due"] = None
            access(i, s, [], [blocks(col, 64)] + w_written(i, t, col, 64))
        elif kind == PPANEL:
            need(1 <= n <= 4 and col + 64 * n <= Np, "a persistent launch of 1 .. 4 blocks", i)
            reads, own = [], blocks(col, 64 * n)
            if t[F["K"]] > 0:
                src = blocks(t[F["src"]], t[F["K"]])
                need(t[F["src"]] + t[F["K"]] <= col and factored[src].all(), "(c) the prologue's source is factored", i)
                reads = [src] + w_read(i, t)
                applied[own, src] += 1
            access(i, s, reads, [own] + w_written(i, t, col, 64 * n))
            for b in range(own.start, own.stop):
                factor_block(i, b)
                applied[b + 1:own.stop, b] += 1
        elif kind == UPDATE:
            src, dst = blocks(t[F["src"]], t[F["K"]]), blocks(col, n)
            need(t[F["K"]] > 0 and n > 0 and t[F["src"]] + t[F["K"]] <= col and col + n <= Np and t[F["rows"]] == Np - col, "geometry", i)
            need(factored[src].all(), "(c) the source is factored", i)
            need(t[F["variant"]] in (SMALL, PLAIN, QUEUE), "variant", i)
            partner = None
            if t[F["variant"]] == QUEUE:
                geometry = tuple(t[F[k]] for k in ("col", "n", "rows", "src", "K", "rhalf", "rko"))
                need(t[F["cus"]] > 0, "a queue launch names its CUs", i)
                first = queues.get(t[F["slot"]])
                if first is None:
                    applied[dst, src] += 1
                else:
                    need(first[0] == geometry and first[1] != s and first[3] == 1, "the second launch of a queue repeats the first on another stream", i)
                    partner = (first[1], first[2])
            else:
                applied[dst, src] += 1
            ts = access(i, s, [src] + w_read(i, t), [dst], partner)
            if t[F["variant"]] == QUEUE:
                queues[t[F["slot"]]] = (geometry, s, ts, 1 if partner is None else 2)
        elif kind == RECORD:
            events[(t[F["event"]], t[F["index"]])] = clock[s].copy()
        elif kind == WAIT:
            need((t[F["event"]], t[F["index"]]) in events, "waits for an event that this factorization has recorded", i)
            clock[s] = np.maximum(clock[s], events[(t[F["event"]], t[F["index"]])])
        else:
            need(False, "kind", i)
    last = len(steps) - 1
    need(state["next"] == nb and state["solve_due"] is None, "(a) every block is factored", last)
    need(all(q[3] == 2 for q in queues.values()), "a shared queue is launched on both streams", last)
    need(clock[CALLER, PANEL] == clock[PANEL, PANEL] and clock[CALLER, UPD] == clock[UPD, UPD], "(e) the streams are joined into the caller's", last)


def _grid():
    for Np in (64, 128, 320, 640, 1152, 2560, 4672, 8192):
        for ldl, algo, la in itertools.product((False, True), (1, 4), (False, True)):
            for width in sorted({128, 192, 256, 512, 1024, Np}):
                # what only one schedule reads is varied only there: pp_fuse_rows under 4, the rest under the look-ahead
                for fuse in ((0, 4096, 10**6) if algo == 4 else (4096,)):
                    for share, st, pcus in (itertools.product((0, 1, 2), (0, 400, 10**5), (0, 64)) if la else ((1, 400, 64),)):
                        yield Np, ldl, algo, la, width, fuse, share, st, pcus


def test_every_plan_of_the_grid_keeps_the_invariants():
    seen, nplans = set(), 0
    for Np, ldl, algo, la, width, fuse, share, st, pcus in _grid():
        steps, (npanel, lookahead) = plan(Np, ldl, algo, la, width, fuse, share, st, pcus)
        nplans += 1
        assert lookahead == (la and npanel > 1)
        assert lookahead or (steps[:, F["stream"]] == CALLER).all()
        assert (steps[:, F["kind"]] == PPANEL).any() == (algo == 4) and (steps[:, F["kind"]] == LEAF).any() == (algo == 1)
        if share == 0 or pcus == 0 or not lookahead:
            assert not ((steps[:, F["kind"]] == UPDATE) & (steps[:, F["variant"]] == QUEUE)).any()
        key = (Np, ldl, steps.tobytes())   # (options that do not change the list are not replayed again)
        if key in seen:
            continue
        seen.add(key)
        try:
            simulate(steps, Np, ldl)
        except Violation as e:
            raise AssertionError(f"Np={Np} ldl={ldl} algo={algo} lookahead={la} width={width} pp_fuse_rows={fuse} share={share} "
                                 f"small_tiles={st} panel_cus={pcus}: {e}") from None
    # both look-ahead deliveries of (a), the fused one and shared queues all occur in the grid
    assert nplans > 3000 and len(seen) > 300


def _rows(steps, names):
    return [tuple(r[F[k]] for k in names) for r in steps.tolist()]


def test_schedule_1_one_outer_panel_by_hand():
    """Np = 512, schedule 1, no look-ahead, one outer panel of 512 columns: eight blocks, after block jj the last 64 (jj & -jj) columns
    are applied to as many columns behind them; the last block has no rows below it and nothing behind it."""
    steps, shape = plan(512, False, 1, False, 512)
    assert shape == (1, False)
    expected = []
    for j, (n, src, K) in enumerate([(64, 0, 64), (128, 0, 128), (64, 128, 64), (256, 0, 256), (64, 256, 64), (128, 256, 128), (64, 384, 64)]):
        col = 64 * j
        expected += [(LEAF, CALLER, col, 0, 0, 0, 0), (TRSM, CALLER, col, 1, 0, 0, 0),
                     (UPDATE, CALLER, col + 64, n, 448 - col, src, K)]
    expected += [(LEAF, CALLER, 448, 0, 0, 0, 0)]
    assert _rows(steps, ("kind", "stream", "col", "n", "rows", "src", "K")) == expected
    assert all(v == SMALL for k, v in _rows(steps, ("kind", "variant")) if k == UPDATE)
    assert all(r == (-1, -1) for r in _rows(steps, ("whalf", "rhalf")))
    simulate(steps, 512, False)


def test_schedule_4_look_ahead_ldl_by_hand():
    """Np = 1152, schedule 4, look-ahead, outer width 256, LDL^T: five outer panels (256 is the tail's width already), every one a
    single persistent launch; from the second on the launch applies the panel in front of it itself (fused prologue, so there is no
    (a) update), the update stream applies panel k to the columns behind panel k + 1 ((b), plain: too short to share), and the
    panel stream waits for (b) of the panel before because that wrote its columns and read the W buffer it now overwrites."""
    steps, shape = plan(1152, True, 4, True, 256)
    assert shape == (5, True)
    names = ("kind", "stream", "col", "n", "src", "K", "whalf", "wko", "rhalf", "rko", "event", "index")
    none = (0, 0, 0, 0, -1, 0, -1, 0)

    def rec(stream, event, index=0):
        return (RECORD, stream) + none + (event, index)

    def wait(stream, event, index=0):
        return (WAIT, stream) + none + (event, index)

    expected = [
        (PPANEL, CALLER, 0, 4, 0, 0, 0, 0, -1, 0, 0, 0),
        rec(CALLER, EV_A), wait(PANEL, EV_A), wait(UPD, EV_A), rec(PANEL, EV_PANEL, 0),
        # k = 0
        wait(UPD, EV_PANEL, 0),
        (UPDATE, UPD, 512, 640, 0, 256, -1, 0, 0, 0, 0, 0), rec(UPD, EV_BDONE, 0),
        (PPANEL, PANEL, 256, 4, 0, 256, 1, 256, 0, 0, 0, 0), rec(PANEL, EV_PANEL, 1),
        # k = 1
        wait(UPD, EV_PANEL, 1), wait(PANEL, EV_BDONE, 0),
        (UPDATE, UPD, 768, 384, 256, 256, -1, 0, 1, 256, 0, 0), rec(UPD, EV_BDONE, 1),
        (PPANEL, PANEL, 512, 4, 256, 256, 0, 512, 1, 256, 0, 0), rec(PANEL, EV_PANEL, 2),
        # k = 2
        wait(UPD, EV_PANEL, 2), wait(PANEL, EV_BDONE, 1),
        (UPDATE, UPD, 1024, 128, 512, 256, -1, 0, 0, 512, 0, 0), rec(UPD, EV_BDONE, 2),
        (PPANEL, PANEL, 768, 4, 512, 256, 1, 768, 0, 512, 0, 0), rec(PANEL, EV_PANEL, 3),
        # k = 3: nothing behind the last panel
        wait(UPD, EV_PANEL, 3), wait(PANEL, EV_BDONE, 2), rec(UPD, EV_BDONE, 3),
        (PPANEL, PANEL, 1024, 2, 768, 256, 0, 1024, 1, 768, 0, 0), rec(PANEL, EV_PANEL, 4),
        rec(PANEL, EV_A), rec(UPD, EV_B), wait(CALLER, EV_A), wait(CALLER, EV_B),
    ]
    assert _rows(steps, names) == expected
    assert all(v == PLAIN for k, v in _rows(steps, ("kind", "variant")) if k == UPDATE)
    simulate(steps, 1152, True)


def test_factor_plan_refuses_bad_arguments():
    f = L.lib().mnk_debug_factor_plan
    assert f(0, 0, 1, 0, 512, 0, 0, 400, 256, 0, None, 0, None) == -1
    assert f(100, 0, 1, 0, 512, 0, 0, 400, 256, 0, None, 0, None) == -1      # not a multiple of 64
    assert f(512, 0, 5, 0, 512, 0, 0, 400, 256, 0, None, 0, None) == -1      # schedule 5 has no step list
    assert f(512, 0, 1, 0, 0, 0, 0, 400, 256, 0, None, 0, None) == -1
    assert f(512, 0, 1, 0, 512, 0, 3, 400, 256, 0, None, 0, None) == -1
    assert f(512, 0, 1, 0, 512, 0, 0, 400, 256, 256, None, 0, None) == -1    # no CU left for the update stream
    assert f(512, 0, 1, 0, 512, 0, 0, 400, 256, 0, None, 4, None) == -1      # room for steps but no buffer
    assert f(512, 0, 1, 0, 512, 0, 0, 400, 256, 0, None, 0, None) == 22      # (the count alone)

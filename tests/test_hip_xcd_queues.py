"""Per-XCD task queues of the task-DAG bulk kernel (-m gpu).  The task list of a single factorization is
PARTITIONED into eight subsequences, one per XCD, so that chunks that walk the same B rows run behind one L2; a workgroup pops the
head of its own XCD's queue and steals from the head of another once that is empty.  No task changes and every tile still sees its
chunks in the same order, so the factor must keep its bits: everything here compares option dag_xcd_queues = 1 with 0 byte by byte.
(The merged launch of a batch keeps its single queue; it is compared with lone factorizations that use the queues.)"""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd.problems import OPF_CASES, opf_shaped  # noqa: E402

# (nbus, ngen, nbranch) -> order n = 2 nbus + 2 ngen + 4 nbranch
SHAPES = {
    "n1504": (160, 32, 280),       # deep band: the bulk kernel accumulates band tiles only (too few tasks for eight queues)
    "n2600": (300, 50, 475),
    "n5376": (560, 100, 1014),     # the largest deep-band order
    "n5808": (600, 104, 1100),     # band + bulk
    "case1354pegase": OPF_CASES["case1354pegase"],   # 11 192: the bench system (C3)
    "n19680": (2400, 440, 3500),
}
STATS = ("panel_algo", "pp_fallbacks", "stall_ms_process", "early_reject_col", "dag_nq", "dag_steals", "dag_ntasks")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def _kkt(P, ctx, alg):
    return mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                       opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=alg))


def _load(k, P, hess=None):
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess if hess is None else hess
    k.compress_jacobian()
    k.compress_hessian()
    k.set_aug_diagonal()
    k.build_kkt()


def _factor(ls, n, **options):
    for key, val in options.items():
        ls.set_option(key, val)
    stall0 = ls.get_stat("stall_ms_process")   # (a counter of the whole process: other tests of a session time out on purpose)
    ls.factorize()
    inertia = ls.inertia()
    stats = {s: ls.get_stat(s) for s in STATS}
    stats["stall_ms_process"] -= stall0
    Lf, D = ls.get_factor_device()
    rng = np.random.default_rng(7)
    xs = [ls.solve_linear_system(rng.standard_normal(n)) for _ in range(2)]
    return dict(L=torch.tril(Lf).clone(), D=D.clone(), inertia=inertia, info=ls.info, xs=xs, stats=stats)


def _assert_bytes(a, b, what):
    assert a["inertia"] == b["inertia"] and a["info"] == b["info"], what
    assert a["stats"]["early_reject_col"] == b["stats"]["early_reject_col"], what
    assert torch.equal(a["L"].view(torch.int64), b["L"].view(torch.int64)), what
    assert torch.equal(a["D"].view(torch.int64), b["D"].view(torch.int64)), what
    for xa, xb in zip(a["xs"], b["xs"]):
        assert np.array_equal(np.asarray(xa).view(np.int64), np.asarray(xb).view(np.int64)), what


def _assert_clean(r, what):
    assert r["stats"]["panel_algo"] == 5.0 and r["stats"]["pp_fallbacks"] == 0.0 and r["stats"]["stall_ms_process"] == 0.0, (what, r["stats"])


@pytest.mark.parametrize("alg", [mj.BUNCHKAUFMAN, mj.CHOLESKY])
@pytest.mark.parametrize("shape,seed", [("n1504", 1), ("n2600", 4), ("n5376", 5), ("n5808", 2), ("case1354pegase", None), ("n19680", 3)])
def test_queues_keep_the_bits_kkt_handle(ctx, shape, seed, alg):
    P = opf_shaped(SHAPES[shape], seed=seed, du=1e-8)
    k = _kkt(P, ctx, alg)
    try:
        _load(k, P)
        ls = k.linear_solver
        for env in (1, 0):
            on = _factor(ls, P.n, envelope=env, dag_xcd_queues=1)
            off = _factor(ls, P.n, envelope=env, dag_xcd_queues=0)
            on2 = _factor(ls, P.n, envelope=env, dag_xcd_queues=1)
            for r in (on, off, on2):
                _assert_clean(r, (shape, alg, env))
            assert on["inertia"] == (P.n, 0, 0)
            assert off["stats"]["dag_nq"] == 0.0 and off["stats"]["dag_steals"] == 0.0
            if P.n > 5376:   # band + bulk: thousands of tasks on the full grid
                assert on["stats"]["dag_nq"] == 8.0
            _assert_bytes(on, off, (shape, alg, env))
            _assert_bytes(on2, off, (shape, alg, env))
            print(f"{shape} {alg} envelope {env}: queues {on['stats']['dag_nq']:.0f}, tasks {on['stats']['dag_ntasks']:.0f}, stolen {on['stats']['dag_steals']:.0f}")
    finally:
        k.close()


@pytest.mark.parametrize("alg", [mj.BUNCHKAUFMAN, mj.CHOLESKY])
@pytest.mark.parametrize("source", ["csc", "dense"])
def test_queues_keep_the_bits_csc_and_dense_sources(ctx, source, alg):
    P = opf_shaped("case1354pegase", seed=11, du=1e-8)
    k = _kkt(P, ctx, alg)
    try:
        _load(k, P)
        colptr, rowval, nzval = np.asarray(k.aug_com.colptr), np.asarray(k.aug_com.rowval), np.array(k.aug_com.nzval)
        A = (colptr, rowval, nzval) if source == "csc" else k.aug_com.to_dense()
    finally:
        k.close()
    ls = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg, panel_algo=5))
    try:
        on = _factor(ls, P.n, dag_xcd_queues=1)
        off = _factor(ls, P.n, dag_xcd_queues=0)
        for r in (on, off):
            _assert_clean(r, (source, alg))
        assert on["stats"]["dag_nq"] == 8.0 and on["inertia"] == (P.n, 0, 0)
        _assert_bytes(on, off, (source, alg))
    finally:
        ls.close()


def test_queues_with_early_rejection_and_nan(ctx):
    """The abort path: an indefinite matrix under early rejection stops at the same column, and a NaN input gives the same info,
    inertia and pivots."""
    P = opf_shaped("case1354pegase", indefinite=True, du=1e-8)
    k = _kkt(P, ctx, mj.BUNCHKAUFMAN)
    try:
        _load(k, P)
        ls = k.linear_solver
        ls.set_option("accept_only_pd", 1)
        ls.set_option("early_reject", 1)
        res = []
        stall0 = ls.get_stat("stall_ms_process")
        for xq in (1, 0):
            ls.set_option("dag_xcd_queues", xq)
            ls.factorize()
            res.append((ls.inertia(), ls.info, ls.get_stat("early_reject_col"), ls.get_stat("pp_fallbacks"), ls.get_stat("stall_ms_process") - stall0))
        assert res[0] == res[1] and res[0][0] != (P.n, 0, 0) and res[0][3] == 0.0 and res[0][4] == 0.0, res
    finally:
        k.close()
    P = opf_shaped("case1354pegase", du=1e-8)
    hess = P.hess.copy()
    hess[len(hess) // 3] = np.nan
    k = _kkt(P, ctx, mj.BUNCHKAUFMAN)
    try:
        _load(k, P, hess)
        ls = k.linear_solver
        res = []
        for xq in (1, 0):
            ls.set_option("dag_xcd_queues", xq)
            ls.factorize()
            _, D = ls.get_factor_device()
            res.append((ls.inertia(), ls.info, ls.get_stat("pp_fallbacks"), D.cpu().numpy().view(np.int64)))
        assert res[0][:3] == res[1][:3] and res[0][2] == 0.0, (res[0][:3], res[1][:3])
        assert np.array_equal(res[0][3], res[1][3])
    finally:
        k.close()


def test_steal_path_every_task_in_queue_0(ctx):
    """A load-balance extreme, not a fault: dag_gang < 0 deals EVERY task to queue 0, so seven of the eight XCDs find their own
    queue empty at once and live on stolen tasks -- the same bytes, and about 7/8 of the tasks stolen."""
    P = opf_shaped("case1354pegase", seed=21, du=1e-8)
    k = _kkt(P, ctx, mj.BUNCHKAUFMAN)
    try:
        _load(k, P)
        ls = k.linear_solver
        ref = _factor(ls, P.n, dag_xcd_queues=0)
        for gang in (-1, 1, 2, 8, 4):
            r = _factor(ls, P.n, dag_xcd_queues=1, dag_gang=gang)
            _assert_clean(r, gang)
            assert r["stats"]["dag_nq"] == 8.0
            _assert_bytes(r, ref, gang)
            share = r["stats"]["dag_steals"] / r["stats"]["dag_ntasks"]
            print(f"dag_gang {gang}: {r['stats']['dag_steals']:.0f} of {r['stats']['dag_ntasks']:.0f} tasks stolen ({share:.3f})")
            if gang < 0:
                assert 0.80 <= share <= 0.95, share   # (7/8 = 0.875 if the XCDs work at the same rate)
            else:
                assert share <= 0.25, share           # (balanced queues: only the ends of the queues are stolen)
    finally:
        k.close()


def test_every_workgroup_takes_its_first_task_at_once(ctx):
    """The residency criterion of the bulk grid on the trace of the queues: every workgroup takes its first task within 2 ms of
    the first one, every one works, every queue is owned by workgroups (1 + queue in word 5 of the per-workgroup record)."""
    P = opf_shaped("case1354pegase", seed=31, du=1e-8)
    k = _kkt(P, ctx, mj.BUNCHKAUFMAN)
    try:
        _load(k, P)
        ls = k.linear_solver
        ls.set_option("dag_fill", 0)
        ls.factorize()
        nwg = int(ls.get_stat("dag_bulk_wgs"))
        ls.set_option("dag_trace", 1)
        ls.factorize()
        assert ls.inertia() == (P.n, 0, 0) and ls.get_stat("panel_algo") == 5.0 and ls.get_stat("pp_fallbacks") == 0.0
        assert ls.get_stat("dag_nq") == 8.0
        ntasks = int(ls.get_stat("dag_ntasks"))
        tr = np.zeros(ntasks * 8 + 4096 * 8 + 1024 * 8, dtype=np.uint64)
        L.check(L.lib().mnk_ls_debug_solve_trace(ls._h, tr.ctypes.data, tr.size), "trace")
        assert np.all(tr[: ntasks * 8].reshape(ntasks, 8)[:, 0] > 0), "a task without a trace record"
        w = tr[ntasks * 8 + 4096 * 8:].reshape(1024, 8).astype(np.int64)
        assert np.all(w[:nwg, 3] > 0) and not w[nwg:].any()
        assert w[:nwg, 3].sum() == ntasks
        late_ms = (w[:nwg, 0] - w[:nwg, 0].min()) / 1e5
        assert late_ms.max() <= 2.0, late_ms.max()
        owners = np.bincount(w[:nwg, 5], minlength=9)
        assert owners[0] == 0 and np.all(owners[1:9] > 0), owners
        assert w[:nwg, 6].sum() == ls.get_stat("dag_steals")
        print(f"workgroups per queue {owners[1:9].tolist()}, stolen {w[:nwg, 6].sum()} of {ntasks}")
        ls.set_option("dag_trace", 0)
    finally:
        k.close()


def test_batch_of_16_matches_lone_factorizations_with_queues(ctx):
    base = OPF_CASES["case1354pegase"][0]
    Ps = [opf_shaped("case1354pegase", seed=base + 500 + i, du=1e-8) for i in range(16)]
    ks = [_kkt(P, ctx, mj.BUNCHKAUFMAN) for P in Ps]
    try:
        ref = []
        for P, k in zip(Ps, ks):
            _load(k, P)
            k.linear_solver.factorize()
            assert k.linear_solver.inertia() == (P.n, 0, 0) and k.linear_solver.get_stat("dag_nq") == 8.0
            Lf, D = k.linear_solver.get_factor_device()
            ref.append((torch.tril(Lf).clone(), D.clone()))
        with mj.factorize_batch():
            for k in ks:
                k.linear_solver.factorize_async()
        for i, (P, k) in enumerate(zip(Ps, ks)):
            ls = k.linear_solver
            assert ls.inertia() == (P.n, 0, 0)
            assert ls.get_stat("panel_algo") == 5.0 and ls.get_stat("pp_fallbacks") == 0.0
            Lf, D = ls.get_factor_device()
            assert torch.equal(torch.tril(Lf).view(torch.int64), ref[i][0].view(torch.int64)) and torch.equal(D.view(torch.int64), ref[i][1].view(torch.int64)), i
    finally:
        for k in ks:
            k.close()


def test_soak_2000_factorizations_without_a_fallback(ctx):
    """About 2000 factorizations of the bench system with the queues on; stops at the first fall-back or stall and reports it."""
    P = opf_shaped("case1354pegase", du=1e-8)
    k = _kkt(P, ctx, mj.BUNCHKAUFMAN)
    try:
        _load(k, P)
        ls = k.linear_solver
        stall0 = ls.get_stat("stall_ms_process")
        for i in range(2000):
            k.build_kkt()
            ls.factorize()
            if i % 50 == 49 or i == 0:
                assert ls.inertia() == (P.n, 0, 0), i
                st = {s: ls.get_stat(s) for s in ("panel_algo", "pp_fallbacks", "stall_ms_process", "timeout_site", "dag_nq")}
                assert st["panel_algo"] == 5.0 and st["pp_fallbacks"] == 0.0 and st["stall_ms_process"] == stall0 and st["dag_nq"] == 8.0, (i, st)
    finally:
        k.close()

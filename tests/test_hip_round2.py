"""GPU parity tests added in round 2 (all through the C ABI, against the CPU oracle):

  * the bench's own algorithm (BUNCHKAUFMAN -> device LDL^T) at the bench's own size (C3, N = 11 192)
    against LAPACK on the same matrix;
  * BASELINE config C5's per-GPU share: 16 independent case1354pegase-shaped scenarios (seeds 1354 + i)
    time-sharing one GPU on 4 contexts, every instance checked against the oracle;
  * the persistent solve's give-up path (a peer workgroup that never becomes resident): the host path
    degrades to the stepwise solve and returns the right answer, the device path reports it.

Tolerances (fp64): assembly bit-exact; solves backward error <= 1e-13 relative to |K||x| + |b|;
solution agreement with LAPACK scaled by the residual-based bound (stated per test).
"""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd.problems import OPF_CASES, dense_dummy_qp, opf_shaped  # noqa: E402
from oracle import kernels as okern  # noqa: E402
from oracle import sparse_condensed as osc  # noqa: E402
from oracle.lapack_cpu import BUNCHKAUFMAN, CHOLESKY, LapackCPUSolver  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def _oracle_sc(P, alg=CHOLESKY):
    k = osc.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb,
                                     P.ind_ub, lambda A: LapackCPUSolver(A, alg))
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess
    k.compress_jacobian()
    k.compress_hessian()
    okern.set_aug_diagonal(k)
    k.build_kkt()
    return k


def _hip_sc(P, ctx, alg, **opt):
    k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub,
                                    ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=alg, **opt))
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess
    return k


def _full(ko):
    Kl = sp.csc_matrix((ko.aug_com.nzval, ko.aug_com.rowval, ko.aug_com.colptr), shape=(ko.n, ko.n))
    return (Kl + sp.tril(Kl, -1).T).tocsr()


def _bwd(K, x, b):
    return np.abs(K @ x - b).max() / (abs(K).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


# --------------------------------------------------------------------------- bench algorithm at bench size
@pytest.mark.parametrize("alg", [mj.BUNCHKAUFMAN, mj.CHOLESKY])
def test_c3_size_factorization_vs_lapack(ctx, alg):
    """The bench line's own path -- `BUNCHKAUFMAN` (device: LDL^T) on the case1354pegase-shaped condensed KKT,
    N = 11 192 -- against LAPACK on the same (bit-identical) matrix.  K is SPD here, so the CPU side is dpotrf
    (seconds, not the minute a pivoted dsytrf takes on few cores); the reference's Bunch-Kaufman inertia of an
    SPD matrix is (N, 0, 0) by Sylvester's law.  Checks: inertia; backward error of the device solve <= 1e-13
    and no worse than 50x LAPACK's; the difference of the two solutions is the difference of their residuals
    pushed through LAPACK's factor (1e-6 |x|) and stays below 1e-4 |x| (conditioning-limited); and
    L D L^T reproduces K on random probe vectors to 1e-12 |K| (no O(N^3) host product)."""
    P = opf_shaped("case1354pegase", du=1e-8)
    assert P.n == 11192
    ko = _oracle_sc(P, CHOLESKY)
    kh = _hip_sc(P, ctx, alg)
    kh.compress_jacobian(); kh.compress_hessian(); kh.set_aug_diagonal(); kh.build_kkt()
    np.testing.assert_array_equal(kh.aug_com.nzval, ko.aug_com.nzval)  # same bits go into both factorizations
    kh.linear_solver.factorize()
    ko.linear_solver.factorize()
    assert kh.linear_solver.inertia() == ko.linear_solver.inertia() == (P.n, 0, 0)
    K = _full(ko)
    rng = np.random.default_rng(1354)
    b = rng.standard_normal(P.n)
    xh = kh.linear_solver.solve_linear_system(b.copy())
    xo = ko.linear_solver.solve_linear_system(b.copy())
    rh, ro = _bwd(K, xh, b), _bwd(K, xo, b)
    assert rh <= 1e-13 and rh <= 50 * ro + 1e-16, (rh, ro)
    # forward agreement is conditioning-limited (Sigma_s spans 16 decades): x_h - x_o = K^-1 (r_o - r_h), so the
    # difference must be explained by the two residuals pushed through LAPACK's factor, up to 1e-6 of |x|
    dr = (b - K @ xo) - (b - K @ xh)
    dx = ko.linear_solver.solve_linear_system(dr.copy())
    err = np.abs((xh - xo) - dx).max() / np.abs(xo).max()
    fwd = np.abs(xh - xo).max() / np.abs(xo).max()
    assert err <= 1e-6 and fwd <= 1e-4, (err, fwd, rh, ro)
    # factor probes: (L D L^T) v == K v
    Lg, D = kh.linear_solver.get_factor()
    Lg = np.tril(Lg, -1)
    V = rng.standard_normal((P.n, 3))
    if alg == mj.CHOLESKY:
        Ld = np.tril(kh.linear_solver.get_factor()[0])
        LV = Ld @ (Ld.T @ V)
    else:
        T = Lg.T @ V + V
        T *= D[:, None]
        LV = Lg @ T + T
    KV = K @ V
    assert np.abs(LV - KV).max() <= 1e-12 * abs(K).sum(axis=1).max() * np.abs(V).max()
    kh.close()


# --------------------------------------------------------------------------- persistent solve: give-up path
def _solve_path(M):
    """Statistic "solve_path" (csrc/solve_plan.h: 1 stepwise, 2 one launch over 256-column steps, 3 over 512-column steps, 4 a system
    of a merged launch), or None from a build of the library that does not report it (A/B runs through MNK_LIBPATH)."""
    try:
        return M.get_stat("solve_path")
    except mj.HipError:
        return None


def _spd(rng, N):
    R = rng.standard_normal((N, 64))
    return np.asfortranarray(R @ R.T + N * np.eye(N))


@pytest.mark.parametrize("alg", [mj.CHOLESKY, mj.LDL])
def test_persistent_solve_abort_falls_back_to_stepwise_on_host_path(ctx, alg):
    """A workgroup of the one-launch solve that never shows up (simulated: option debug_ps_missing makes it leave
    at once) must not hang the GPU: the others give up after `ps_spin_limit` polls, and a host-resident caller
    gets the right answer from the stepwise redo -- silently, as part of the same call."""
    rng = np.random.default_rng(77)
    N = 3000
    A = _spd(rng, N)
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg))
    M.factorize()
    b = rng.standard_normal(N)
    x_ok = M.solve_linear_system(b.copy())
    M.set_option("ps_spin_limit", 2048)
    M.set_option("debug_ps_missing", 5)
    assert _solve_path(M) in (2, None)
    x = M.solve_linear_system(b.copy())      # aborts inside, redone stepwise
    assert _solve_path(M) in (1, None)
    assert np.abs(A @ x - b).max() <= 1e-10 * N
    np.testing.assert_allclose(x, x_ok, rtol=0, atol=1e-12 * np.abs(x_ok).max() * 10)
    x2 = M.solve_linear_system(b.copy())     # persistent_solve is off now: no further abort
    assert _solve_path(M) in (1, None)
    np.testing.assert_array_equal(x2, x)
    M.close()


def test_persistent_solve_abort_is_reported_to_device_resident_callers(ctx):
    rng = np.random.default_rng(78)
    N = 2000
    A = _spd(rng, N)
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
    M.factorize()
    b = rng.standard_normal(N)
    xd = torch.from_numpy(b).cuda()
    M.solve_linear_system(xd)
    M.check_solve()                           # healthy
    M.set_option("ps_spin_limit", 2048)
    M.set_option("debug_ps_missing", 0)
    xd = torch.from_numpy(b).cuda()
    M.solve_linear_system(xd)                 # result invalid, nobody has looked yet
    with pytest.raises(mj.SolveException):
        M.check_solve()
    xd = torch.from_numpy(b).cuda()
    M.solve_linear_system(xd)                 # stepwise from here on
    M.check_solve()
    assert _solve_path(M) in (1, None)
    assert np.abs(A @ xd.cpu().numpy() - b).max() <= 1e-10 * N
    M.close()


def test_solve_kkt_redoes_an_aborted_persistent_solve(ctx):
    """mnk_sc_solve_kkt with host vectors must not return rc = 0 with an invalid w after a persistent
    solve gave up; it detects the abort after its stream synchronization, before the copy-back, and redoes the
    whole solve_kkt! with the stepwise solve.  N = 1088 (case118 shape): 17 workgroups in the one-launch solve."""
    P = opf_shaped("case118", du=1e-8)
    ko = _oracle_sc(P)
    ko.linear_solver.factorize()
    kh = _hip_sc(P, ctx, mj.BUNCHKAUFMAN)
    kh.compress_jacobian(); kh.compress_hessian(); kh.set_aug_diagonal(); kh.build_kkt()
    kh.linear_solver.factorize()
    kh.upload_barrier_terms()
    rng = np.random.default_rng(5)
    bo, bh = okern.UnreducedKKTVector.from_kkt(ko), mj.UnreducedKKTVector.from_kkt(kh)
    bv = rng.standard_normal(len(bo.values))
    bo.values[:] = bv
    ko.solve_kkt(bo)
    bh.values[:] = bv
    kh.solve_kkt_device(bh)
    good = bh.values.copy()
    assert np.abs(good - bo.values).max() <= 1e-6 * np.abs(bo.values).max()
    kh.linear_solver.set_option("ps_spin_limit", 2048)
    kh.linear_solver.set_option("debug_ps_missing", 1)
    bh.values[:] = bv
    kh.solve_kkt_device(bh)                  # the persistent solve inside gives up; redone stepwise in the same call
    assert np.abs(bh.values - good).max() <= 1e-10 * np.abs(good).max()
    kh.linear_solver.check_solve()           # nothing left pending
    assert _solve_path(kh.linear_solver) in (1, None)
    kh.close()


# --------------------------------------------------------------------------- BUNCHKAUFMAN: the pivoted tier
def _bk_reconstruct(M, A):
    """P A P' = L D L' from the device factor: returns the max entry of the residual."""
    active, count, perm, doff = M.bk_info()
    assert active
    Lg, D = M.get_factor()
    N = A.shape[0]
    Lu = np.tril(Lg, -1) + np.eye(N)
    Dm = np.diag(D)
    for k in np.nonzero(doff)[0]:
        Dm[k + 1, k] = Dm[k, k + 1] = doff[k]
    Af = np.tril(A) + np.tril(A, -1).T
    PAP = Af[np.ix_(perm, perm)]
    return np.abs(Lu @ Dm @ Lu.T - PAP).max(), perm, doff


def _not_quasi_definite(rng, n1, n2, kind):
    """Symmetric indefinite matrices that an unpivoted LDL' cannot factor in the given order."""
    if kind == "saddle_zero_dual" and n2 > n1:
        n1, n2 = n2, n1                   # J must have full row rank, or the saddle matrix is singular
    N = n1 + n2
    A = np.zeros((N, N))
    B = rng.standard_normal((n2, n1))
    if kind == "zero_leading_block":      # [[0, B'], [B, C]]: every leading pivot is exactly zero
        A[n1:, :n1] = B
        C = rng.standard_normal((n2, n2))
        A[n1:, n1:] = (C + C.T) / 2
    elif kind == "saddle_zero_dual":      # [[H, J'], [J, 0]] with an INDEFINITE H whose (0,0) entry is zero
        H = rng.standard_normal((n1, n1)); H = (H + H.T) / 2
        H[0, 0] = 0.0
        A[:n1, :n1] = H
        A[n1:, :n1] = B
    else:                                 # dense random symmetric with a zero diagonal
        S = rng.standard_normal((N, N)); A = (S + S.T) / 2
        np.fill_diagonal(A, 0.0)
        return np.asfortranarray(A)
    A = np.tril(A) + np.tril(A, -1).T
    return np.asfortranarray(A)


@pytest.mark.parametrize("kind", ["zero_leading_block", "saddle_zero_dual", "zero_diagonal"])
@pytest.mark.parametrize("n1,n2", [(3, 4), (40, 60), (150, 250)])
def test_bunchkaufman_pivoted_tier_matches_dsytrf(ctx, kind, n1, n2):
    """SURVEY 8(f).2 / ADVICE r1: on matrices that are NOT quasi-definite in the given order the static-pivot
    LDL' breaks down (exact zero pivots); BUNCHKAUFMAN then refactors with 1x1 / 2x2 Bunch-Kaufman pivoting
    (dsytf2's strategy) and must report LAPACK dsytrf's inertia through the reference's own rule
    (src/LinearSolvers/lapack.jl:240-268), reconstruct P A P' = L D L' to 1e-11 |A|, and solve with a backward
    error <= 1e-11 (the bar VERDICT r1 set) -- compared with dsytrf/dsytrs on the same matrix."""
    rng = np.random.default_rng(100 * n1 + n2 + len(kind))
    A = _not_quasi_definite(rng, n1, n2, kind)
    N = A.shape[0]
    A_l = A.copy(order="F")
    A_l[np.triu_indices(N, 1)] = np.nan     # 'L' storage
    M = mj.HipLinearSolver(A_l, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    ref = LapackCPUSolver(A, BUNCHKAUFMAN).factorize()
    assert ref.info == 0
    active, count, perm, doff = M.bk_info()
    assert active and count == 1, "the static factorization should have broken down on this matrix"
    assert M.inertia() == ref.inertia()
    ev = np.linalg.eigvalsh(A)
    assert M.inertia() == (int((ev > 0).sum()), 0, int((ev < 0).sum()))
    err, perm, doff = _bk_reconstruct(M, A)
    assert err <= 1e-11 * np.abs(A).max() * max(1, N / 16)
    assert sorted(perm.tolist()) == list(range(N))
    assert np.count_nonzero(doff) >= 1     # at least one 2x2 pivot was needed
    b = rng.standard_normal(N)
    x = M.solve_linear_system(b.copy())
    xr = ref.solve_linear_system(b.copy())
    nrm = np.abs(A).sum(axis=1).max()
    res = np.abs(A @ x - b).max() / (nrm * np.abs(x).max() + np.abs(b).max())
    res_ref = np.abs(A @ xr - b).max() / (nrm * np.abs(xr).max() + np.abs(b).max())
    assert res <= 1e-11 and res <= 1e3 * res_ref + 1e-15, (res, res_ref)
    # matrix right-hand sides and device-resident vectors take the same path
    xd = torch.from_numpy(b.copy()).cuda()
    M.solve_linear_system(xd)
    M.check_solve()
    np.testing.assert_array_equal(xd.cpu().numpy(), x)
    # the next factorization of a quasi-definite matrix goes back to the fast tier
    M.close()


def test_bunchkaufman_tiers_and_the_ldl_option(ctx):
    """LDL keeps static pivoting only (breakdown -> num_zero, the IPM regularizes); BUNCHKAUFMAN with
    bk_fallback = 0 behaves the same; a quasi-definite matrix never takes the pivoted tier; an exactly singular
    matrix reports num_zero = 1 through info as the reference does."""
    rng = np.random.default_rng(9)
    A = _not_quasi_definite(rng, 20, 30, "zero_leading_block")
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
    M.factorize()
    assert M.inertia()[1] > 0 and M.bk_info()[:2] == (False, 0)
    M.close()
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.set_option("bk_fallback", 0)
    M.factorize()
    assert M.inertia()[1] > 0 and M.bk_info()[:2] == (False, 0)
    M.set_option("bk_fallback", 1)
    M.factorize()
    assert M.inertia() == LapackCPUSolver(A, BUNCHKAUFMAN).factorize().inertia() and M.bk_info()[:2] == (True, 1)
    M.close()
    # quasi-definite: fast tier
    H = rng.standard_normal((30, 30)); H = H @ H.T + 30 * np.eye(30)
    J = rng.standard_normal((10, 30))
    K = np.zeros((40, 40)); K[:30, :30] = H; K[30:, :30] = J; K[:30, 30:] = J.T; K[30:, 30:] = -1e-8 * np.eye(10)
    K = np.asfortranarray(K)
    M = mj.HipLinearSolver(K, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    assert M.inertia() == (30, 0, 10) and M.bk_info()[:2] == (False, 0)
    M.close()
    # exactly singular: dsytrf reports info > 0 -> num_zero = 1
    S = np.zeros((6, 6)); S[1, 0] = S[0, 1] = 1.0; S[3, 2] = S[2, 3] = 2.0   # rows/cols 4, 5 are zero
    S = np.asfortranarray(S)
    M = mj.HipLinearSolver(S, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    ref = LapackCPUSolver(S, BUNCHKAUFMAN).factorize()
    assert ref.info > 0
    assert M.inertia() == ref.inertia()
    M.close()


def test_dense_kkt_system_with_zero_dual_block_uses_pivoting(ctx):
    """DenseKKTSystem (augmented form, reference src/KKT/Dense/augmented.jl:116-145) at a point where the primal
    block is singular in the given order (zero Hessian, pr_diag = 0 on the first variables, du_diag = 0): LAPACK
    needs 2x2 pivots; the HIP path must agree with the oracle's inertia and solve_kkt! result."""
    from oracle import dense as odense
    rng = np.random.default_rng(4)
    n, m = 12, 5
    A = np.zeros((n + m, n + m))
    d = np.ones(n); d[:4] = 0.0
    A[:n, :n] = np.diag(d)
    J = rng.standard_normal((m, n))
    A[n:, :n] = J
    A = np.asfortranarray(np.tril(A) + np.tril(A, -1).T)
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    ref = LapackCPUSolver(A, BUNCHKAUFMAN).factorize()
    assert M.inertia() == ref.inertia() == (n, 0, m)
    b = rng.standard_normal(n + m)
    x = M.solve_linear_system(b.copy())
    assert np.abs(A @ x - b).max() <= 1e-11 * (np.abs(A).sum(axis=1).max() * np.abs(x).max() + 1)
    M.close()


# --------------------------------------------------------------------------- lootsma: the reference's hard-coded answers
@pytest.mark.parametrize("kind", ["dense", "dense_condensed", "sparse_condensed"])
def test_ipm_lootsma_hip_reproduces_reference_answers(ctx, kind):
    """The HIP back-end driven by the IPM mirror reaches the primal solution and multipliers the reference's own
    test suite hard-codes for `lootsma` (lib/MadNLPTests/src/MadNLPTests.jl:175-194, atol = rtol = sqrt(tol)), with
    the same iteration history as the CPU oracle (the reference's CPU == GPU acceptance)."""
    from madnlp_jl_amd.problems import LootsmaModel
    from tests.test_hip_parity import _assert_ipm_parity, _ipm_pair
    nlp = LootsmaModel()
    so, sh = _ipm_pair(kind, nlp, ctx, 1e-8 if kind != "sparse_condensed" else 1e-6)
    _assert_ipm_parity(so, sh, 3)
    tol = np.sqrt(sh.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731
    assert cmp(sh.x[:3], nlp.LOOTSMA_X) and cmp(sh.y, nlp.LOOTSMA_Y), (sh.x[:3], sh.y)
    sh.kkt.close()


# --------------------------------------------------------------------------- persistent panel kernel: safety net
@pytest.mark.parametrize("N,expect", [(1000, 4.0), (2300, 5.0)])
def test_persistent_schedules_stay_in_use_next_to_other_contexts(ctx, N, expect):
    """panel_algo = 4 / 5 keep waiting workgroups resident, which is only safe while no other persistent kernel runs on
    the same CUs.  Round 3 gave the persistent schedules up as soon as a second context was alive (one launch per piece,
    12.4 instead of 9.3 ms at C3); since round 4 the persistent operations of a process take turns on the device
    (mnk_persist_begin), so a second live context changes nothing: same schedule (small systems: the persistent panel
    kernel; from dag_min_rows on: the task-DAG schedule), same bits."""
    rng = np.random.default_rng(4)
    A = _spd(rng, N)
    b = rng.standard_normal(N)
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
    M.factorize()
    alone = M.get_stat("panel_algo")
    assert alone == expect
    x4 = M.solve_linear_system(b.copy())
    L4, D4 = M.get_factor()
    other = mj.HipContext(0)
    try:
        M2 = mj.HipLinearSolver(A, ctx=other, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
        M2.factorize()
        M.factorize()
        assert M.get_stat("panel_algo") == alone and M2.get_stat("panel_algo") == alone
        assert M.get_stat("pp_fallbacks") == 0.0 and M2.get_stat("pp_fallbacks") == 0.0
        x1 = M.solve_linear_system(b.copy())
        x2 = M2.solve_linear_system(b.copy())
        L1, D1 = M.get_factor()
        M2.close()
    finally:
        other.close()
    assert np.abs(A @ x4 - b).max() <= 1e-10 * N
    assert np.array_equal(x1, x4) and np.array_equal(x2, x4)
    assert np.array_equal(np.tril(L1), np.tril(L4)) and np.array_equal(D1, D4)
    M.close()


@pytest.mark.parametrize("alg", [mj.CHOLESKY, mj.LDL])
@pytest.mark.parametrize("N,expect", [(1000, 4.0), (2100, 5.0)])
def test_persistent_panel_that_gives_up_is_redone_without_it(ctx, alg, N, expect):
    """A diagonal strip that never publishes (simulated: option debug_pp_missing; in the field: another process'
    persistent kernels starving it) must not hang: the waiters give up after a bounded number of polls (info = -7),
    the factorization is redone with one launch per panel piece when `info` is read, and the solver stays there.
    Both persistent schedules: the panel kernel (N = 1000) and the task-DAG schedule's chain + bulk kernels (N = 2100)."""
    rng = np.random.default_rng(5)
    A = _spd(rng, N)
    b = rng.standard_normal(N)
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg))
    M.set_option("dag_spin_limit", 1 << 17)   # (the default bound is sized for factorizations that take seconds)
    M.factorize()
    assert M.get_stat("panel_algo") == expect, "the module's context should be the only live one here"
    x_ok = M.solve_linear_system(b.copy())
    M.set_option("debug_pp_missing", 1)
    M.factorize()
    assert M.inertia() == (N, 0, 0)
    assert M.get_stat("pp_fallbacks") == 1.0 and M.get_stat("panel_algo") == 1.0
    x = M.solve_linear_system(b.copy())
    assert np.abs(A @ x - b).max() <= 1e-10 * N
    np.testing.assert_allclose(x, x_ok, rtol=0, atol=1e-11 * np.abs(x_ok).max())
    M.factorize()                      # stays on the safe path: no second time-out
    assert M.get_stat("pp_fallbacks") == 1.0 and M.get_stat("panel_algo") == 1.0
    # ... for 16 factorizations; then the persistent schedule gets another chance (the time-out may have been transient)
    M.set_option("debug_pp_missing", -1)
    for _ in range(16):
        M.factorize()
    assert M.get_stat("pp_fallbacks") == 1.0 and M.get_stat("panel_algo") == expect
    x = M.solve_linear_system(b.copy())
    np.testing.assert_allclose(x, x_ok, rtol=0, atol=1e-11 * np.abs(x_ok).max())
    M.close()


# --------------------------------------------------------------------------- device-side feeders (SURVEY 8(a)11 on the device)
def _iterate(rng, ntot, ind_lb, ind_ub):
    """A strictly interior iterate: full-length x, xl, xu, zl, zu (zl/zu zero off their bound sets)."""
    xl = np.full(ntot, -np.inf); xu = np.full(ntot, np.inf)
    xl[ind_lb] = -rng.uniform(0.5, 2.0, len(ind_lb)); xu[ind_ub] = rng.uniform(0.5, 2.0, len(ind_ub))
    x = rng.uniform(-0.4, 0.4, ntot) * 10.0 ** rng.uniform(-6, 0, ntot)
    zl = np.zeros(ntot); zu = np.zeros(ntot)
    zl[ind_lb] = 10.0 ** rng.uniform(-8, 2, len(ind_lb)); zu[ind_ub] = 10.0 ** rng.uniform(-8, 2, len(ind_ub))
    # the library never reads bound values outside ind_lb / ind_ub; keep them finite for the host->device copy
    return x, np.where(np.isfinite(xl), xl, -1e300), np.where(np.isfinite(xu), xu, 1e300), zl, zu


def _oracle_feed(k, x, xl, xu, zl, zu, primal_reg, dual_reg, dw, dc):
    """reference set_aug_diagonal! (src/IPM/kernels.jl:4-27) + regularize_diagonal! (src/KKT/KKTsystem.jl:222-226)
    on an oracle KKT object's host fields."""
    k.reg[:] = primal_reg
    k.du_diag[:] = -dual_reg
    k.l_diag[:] = xl[k.ind_lb] - x[k.ind_lb]
    k.u_diag[:] = x[k.ind_ub] - xu[k.ind_ub]
    k.l_lower[:] = zl[k.ind_lb]
    k.u_lower[:] = zu[k.ind_ub]
    okern.set_aug_diagonal(k)
    okern.regularize_diagonal(k, dw, dc)


@pytest.mark.parametrize("where", ["host", "device"])
def test_device_feeders_sparse_condensed_bit_exact(ctx, where):
    """`mnk_sc_set_aug_diagonal` + `mnk_sc_regularize_diagonal` + `mnk_sc_build(NULL, NULL)`: the diagonals the handle
    computes from the iterate are bit-identical to the oracle's (same IEEE operations, no contraction possible), and
    the condensed KKT built from them is bit-identical to the one built from host diagonals."""
    P = opf_shaped("case118", du=0.0)
    rng = np.random.default_rng(11)
    ko = _oracle_sc(P)
    kh = _hip_sc(P, ctx, mj.BUNCHKAUFMAN)
    ntot = P.n + P.m
    x, xl, xu, zl, zu = _iterate(rng, ntot, ko.ind_lb, ko.ind_ub)
    _oracle_feed(ko, x, xl, xu, zl, zu, 1e-3, 2e-9, 1e-4, 1e-8)
    vec = [x, xl, xu, zl, zu]
    if where == "device":
        vec = [torch.from_numpy(v).cuda() for v in vec]
    kh.compress_jacobian(); kh.compress_hessian()
    kh.set_aug_diagonal_device(*vec, primal_reg=1e-3, dual_reg=2e-9)
    kh.regularize_diagonal_device(1e-4, 1e-8)
    got = kh.get_diagonals_device()
    for name in ("pr_diag", "du_diag", "reg", "l_diag", "u_diag", "l_lower", "u_lower"):
        np.testing.assert_array_equal(got[name], getattr(ko, name), err_msg=name)
    kh.build_kkt_device()
    ko.build_kkt()
    np.testing.assert_array_equal(kh.aug_com.nzval, ko.aug_com.nzval)
    # and the device-side solve_kkt! works off the same handle state (barrier terms came with the feeder)
    kh.linear_solver.factorize()
    ko.linear_solver.factorize()
    w = okern.UnreducedKKTVector.from_kkt(ko)
    w.values[:] = rng.standard_normal(len(w.values))
    wo = w.copy()
    ko.solve_kkt(wo)
    wd = w.values.copy()
    kh.solve_kkt_device(wd)
    assert np.abs(wd - wo.values).max() <= 1e-9 * max(1.0, np.abs(wo.values).max())
    kh.close()


@pytest.mark.parametrize("kind", ["dense_condensed", "dense"])
def test_device_feeders_dense_systems_bit_exact(ctx, kind):
    from oracle import dense as odense
    P = dense_dummy_qp(96, 40, 8 if kind == "dense_condensed" else 0, seed=3)
    rng = np.random.default_rng(12)
    if kind == "dense_condensed":
        ko = odense.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, lambda A: LapackCPUSolver(A, BUNCHKAUFMAN))
        kh = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx)
    else:
        ko = odense.DenseKKTSystem(P.n, P.m, P.ind_ineq, P.ind_lb, P.ind_ub, lambda A: LapackCPUSolver(A, BUNCHKAUFMAN))
        kh = mj.DenseKKTSystem(P.n, P.m, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx)
    for k in (ko, kh):
        k.hess[...] = P.hess
        k.jac[...] = P.jac
    ntot = len(ko.pr_diag)
    x, xl, xu, zl, zu = _iterate(rng, ntot, ko.ind_lb, ko.ind_ub)
    _oracle_feed(ko, x, xl, xu, zl, zu, 0.0, 0.0, 1e-4, 1e-8)
    kh.set_aug_diagonal_device(x, xl, xu, zl, zu)
    kh.regularize_diagonal_device(1e-4, 1e-8)
    got = kh.get_diagonals_device()
    for name in ("pr_diag", "du_diag", "reg", "l_diag", "u_diag", "l_lower", "u_lower"):
        np.testing.assert_array_equal(got[name], getattr(ko, name), err_msg=name)
    for k in (ko, kh):
        k.compress_jacobian()
        k.compress_hessian()
    kh._upload()
    kh.build_kkt_device()
    ko.build_kkt()
    kh.linear_solver.factorize()
    ko.linear_solver.factorize()
    assert kh.linear_solver.inertia() == ko.linear_solver.inertia()
    w = okern.UnreducedKKTVector.from_kkt(ko)
    w.values[:] = rng.standard_normal(len(w.values))
    wo = w.copy()
    ko.solve_kkt(wo)
    wd = w.values.copy()
    kh.solve_kkt_device(wd)
    assert np.abs(wd - wo.values).max() <= 1e-8 * max(1.0, np.abs(wo.values).max())
    kh.close()


# --------------------------------------------------------------------------- growth guard of the static-pivot tier (round 3)
def _bwd_full(A, x, b):
    nrm = np.abs(A).sum(axis=1).max()
    return np.abs(A @ x - b).max() / (nrm * np.abs(x).max() + np.abs(b).max())


@pytest.mark.parametrize("N,seed", [(300, 1), (640, 2), (1000, 3)])
def test_growth_guard_random_indefinite_without_exact_zeros(ctx, N, seed):
    """VERDICT r2 / ADVICE r1: `BUNCHKAUFMAN` = dsytrf in the reference (src/LinearSolvers/lapack.jl:164-172), stable on
    ANY symmetric matrix.  A random symmetric indefinite matrix that is not quasi-definite and has no exact zero anywhere
    never breaks the static-pivot LDL' down -- its small pivots are merely small -- but the Schur complements leave the
    scale of the matrix.  The growth guard (max|d_k| / max|a_ij| > bk_growth_tol) must hand such a factorization to the
    pivoted tier: inertia == dsytrf's, backward error within 1e3 x dsytrs's."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((N, N))
    A = np.asfortranarray((S + S.T) / 2)          # indefinite, dense, diagonal entries O(1): no zero pivots
    b = rng.standard_normal(N)
    ref = LapackCPUSolver(A, BUNCHKAUFMAN).factorize()
    xr = ref.solve_linear_system(b.copy())
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    x = M.solve_linear_system(b.copy())
    assert M.inertia() == ref.inertia()
    res, res_ref = _bwd_full(A, x, b), _bwd_full(A, xr, b)
    assert res <= 1e3 * res_ref + 1e-15, (res, res_ref, M.get_stat("growth"), M.bk_info()[:2])
    # what the static tier alone would have delivered (LDL = static pivoting only): the guard's reason to exist
    Ms = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
    Ms.factorize()
    xs = Ms.solve_linear_system(b.copy())
    print(f"N={N}: growth {M.get_stat('growth'):.2e}, pivoted tier {M.bk_info()[0]}, backward error {res:.1e} "
          f"(dsytrs {res_ref:.1e}, static pivoting alone {_bwd_full(A, xs, b):.1e})")
    Ms.close()
    M.close()


@pytest.mark.parametrize("tiny", [1e-14, 1e-300])
def test_growth_guard_tiny_nonzero_pivot(ctx, tiny):
    """A pivot of 1e-14 or 1e-300 is not an exact zero: the static tier accepts it, the next Schur complement is
    1/tiny times the matrix.  The guard must send the matrix to the pivoted tier, whose answer matches dsytrf's."""
    rng = np.random.default_rng(7)
    N = 200
    S = rng.standard_normal((N, N))
    A = (S + S.T) / 2
    A[0, 0] = tiny                                  # first pivot: tiny, not zero
    A = np.asfortranarray(A)
    b = rng.standard_normal(N)
    ref = LapackCPUSolver(A, BUNCHKAUFMAN).factorize()
    xr = ref.solve_linear_system(b.copy())
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    x = M.solve_linear_system(b.copy())
    assert M.bk_info()[0], "the growth guard should have handed this factorization to the pivoted tier"
    assert M.get_stat("growth") > 1e4   # (1 / tiny times the matrix)
    assert M.inertia() == ref.inertia()
    assert _bwd_full(A, x, b) <= 1e3 * _bwd_full(A, xr, b) + 1e-15
    M.close()


def test_growth_guard_leaves_definite_and_quasi_definite_systems_alone(ctx):
    """SPD matrices have d_k <= a_kk (growth <= 1) whatever their conditioning, and the KKT systems of the path are
    quasi-definite: the guard must never cost them the fast tier."""
    rng = np.random.default_rng(11)
    N = 900
    G = rng.standard_normal((N, 40))
    sc = 10.0 ** rng.uniform(-6, 6, N)              # IPM-like spread of the diagonal
    A = np.asfortranarray(G @ G.T + np.diag(sc))
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    assert M.inertia() == (N, 0, 0) and M.bk_info()[:2] == (False, 0) and M.get_stat("growth") <= 1.0 + 1e-12
    M.close()
    n1, n2 = 600, 200                                # [[H, J'], [J, -C]], H and C positive definite
    H = rng.standard_normal((n1, n1)); H = H @ H.T / n1 + np.eye(n1)
    J = rng.standard_normal((n2, n1))
    K = np.zeros((n1 + n2, n1 + n2))
    K[:n1, :n1] = H; K[n1:, :n1] = J; K[:n1, n1:] = J.T; K[n1:, n1:] = -1e-8 * np.eye(n2)
    K = np.asfortranarray(K)
    M = mj.HipLinearSolver(K, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    assert M.inertia() == (n1, 0, n2) and M.bk_info()[:2] == (False, 0)
    b = rng.standard_normal(n1 + n2)
    x = M.solve_linear_system(b.copy())
    assert _bwd_full(K, x, b) <= 1e-13
    M.close()


@pytest.mark.parametrize("kind,N", [("random", 4000), ("saddle", 3000)])
def test_blocked_bunchkaufman_at_scale(ctx, kind, N):
    """the pivoted tier is blocked (dlasyf-style 64-column panels, MFMA trailing update): a C3-order
    indefinite matrix costs tens of milliseconds, not seconds.  Inertia == dsytrf's, P A P' = L D L' to 1e-11 |A|,
    backward error within 1e3 x dsytrs's -- at N = 3000 / 4000 (the unblocked tier of round 2 was tested to N = 400)."""
    import time
    rng = np.random.default_rng(N)
    if kind == "random":
        S = rng.standard_normal((N, N)); A = (S + S.T) / 2
    else:                                   # [[H, J'], [J, 0]] with an indefinite H: needs 2x2 pivots
        n1 = 2 * N // 3
        H = rng.standard_normal((n1, n1)); H = (H + H.T) / 2
        J = rng.standard_normal((N - n1, n1))
        A = np.zeros((N, N)); A[:n1, :n1] = H; A[n1:, :n1] = J; A[:n1, n1:] = J.T
    A = np.asfortranarray(A)
    b = rng.standard_normal(N)
    ref = LapackCPUSolver(A, BUNCHKAUFMAN).factorize()
    xr = ref.solve_linear_system(b.copy())
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.factorize()
    assert M.inertia() == ref.inertia()      # (reads the info: the tiers are decided here)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M.factorize()
    inertia = M.inertia()
    ms = 1e3 * (time.perf_counter() - t0)
    assert inertia == ref.inertia() and M.bk_info()[0]
    x = M.solve_linear_system(b.copy())
    res, res_ref = _bwd_full(A, x, b), _bwd_full(A, xr, b)
    assert res <= 1e3 * res_ref + 1e-15, (res, res_ref)
    err, perm, doff = _bk_reconstruct(M, A)
    assert err <= 1e-11 * np.abs(A).max() * max(1, N / 16)
    print(f"{kind} N={N}: static tier + pivoted tier + inertia {ms:.1f} ms, 2x2 pivots {np.count_nonzero(doff)}, "
          f"backward error {res:.1e} (dsytrs {res_ref:.1e})")
    assert ms < 2000.0, "the blocked tier should take tens of milliseconds at this order"
    M.close()


def test_fallback_tier_refuses_a_destroyed_kkt_handle(ctx):
    """An asynchronous factorize! keeps a way back to the KKT handle's matrix for the pivoted tier.  If the handle is
    destroyed before the inertia is fetched, the fall-back must fail with a message -- not read freed memory."""
    from madnlp_jl_amd import _lib as L
    from madnlp_jl_amd.linear_solver import InertiaException
    rng = np.random.default_rng(4)
    n, m = 12, 5
    k = mj.DenseKKTSystem(n, m, [], [], [], ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    k.jac[:] = rng.standard_normal((m, n))
    k.pr_diag[:] = 1.0
    k.pr_diag[:4] = 0.0            # zero pivots in the given order: the static-pivot tier breaks down
    k.build_kkt()
    k.linear_solver.factorize_async()
    import ctypes
    L.check(L.lib().mnk_dc_destroy(k._h), "mnk_dc_destroy")
    k._h = ctypes.c_void_p()
    with pytest.raises(InertiaException, match="destroyed"):
        k.linear_solver.inertia()
    k.linear_solver.close()


def test_condensed_systems_do_not_pay_for_the_pivoted_tier(ctx):
    """`SparseCondensedKKTSystem` accepts positive definite matrices only (`is_inertia_correct`, reference
    src/KKT/Sparse/condensed.jl:138-140): a zero pivot of the static-pivot tier proves "not positive definite", so the solver
    the system creates reports the static tier's counts instead of re-factoring with Bunch-Kaufman pivoting (option
    accept_only_pd); a stand-alone BUNCHKAUFMAN solver on the same matrix still takes the pivoted tier."""
    from madnlp_jl_amd.problems import opf_shaped
    P = opf_shaped("case30", indefinite=True)
    # (early_reject off: this test is about the COUNTS the static tier reports; with it the factorization stops at the first
    # non-positive pivot and the counts are a lower bound -- tests/test_hip_round5.py)
    k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                    opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), early_reject=False)
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess
    k.pr_diag[:] = P.pr_diag
    k.compress_jacobian(); k.compress_hessian(); k.build_kkt()
    k.linear_solver.factorize()
    npos, nzero, nneg = k.linear_solver.inertia()
    assert nneg + nzero > 0 and not k.is_inertia_correct(npos, nzero, nneg)
    assert k.linear_solver.get_stat("bk_count") == 0          # no pivoted factorization was paid for
    assert k.linear_solver.get_stat("early_rejects") == 0
    # the same matrix through a solver of its own: BUNCHKAUFMAN semantics, the pivoted tier may run (zero pivots do occur
    # only by accident here, so only the inertia is compared)
    A = k.aug_com.to_dense() if hasattr(k.aug_com, "to_dense") else None
    if A is not None:
        M = mj.HipLinearSolver(np.asfortranarray(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
        M.factorize()
        assert M.inertia() == (npos, nzero, nneg) or M.bk_info()[1] > 0
        M.close()
    k.close()


@pytest.mark.parametrize("N,alg", [(3968, "LDL"), (4096, "CHOLESKY"), (5000, "LDL"), (6100, "LDL"), (11192, "LDL")])
def test_solve_with_512_column_steps_matches_the_256_column_solve(ctx, N, alg):
    """Option solve512: the one-launch solve with 32-row blocks, 512-column steps and 512 x 512 explicit inverses assembled from
    the 256 x 256 ones on the MFMA tile kernel (half the steps per sweep).  Same solution as the default solve to rounding,
    same backward error; orders whose padded size leaves a 384-row last triangle keep the 256-column steps."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(N)
    R = torch.randn(N, 64, dtype=torch.float64, device="cuda", generator=g)
    A = R @ R.T + torch.diag(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) * 10 + 1.0)
    if alg == "LDL":
        h = N // 3
        A[N - h:, N - h:] = -(A[N - h:, N - h:] + 2.0 * torch.eye(h, dtype=torch.float64, device="cuda") * N ** 0.5)
    b = torch.randn(N, dtype=torch.float64, device="cuda", generator=g)
    xs = []
    for s512 in (0, 1):
        x = b.clone()
        torch.cuda.synchronize()   # A, b, x were produced on torch's stream, the solver works on the context's
        ls = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg))
        ls.set_option("solve512", s512)
        ls.factorize()
        ls.solve_linear_system(x)
        ctx.synchronize()
        # (N = 3968: fewer than 4096 rows, and a 384-row last triangle: the option changes nothing there)
        assert _solve_path(ls) in (3 if s512 and N != 3968 else 2, None), (s512, _solve_path(ls))
        xs.append(x.cpu().numpy())
        ls.close()
    An = torch.linalg.matrix_norm(A, ord=float("inf")).item()
    res = (torch.abs(A @ torch.from_numpy(xs[1]).cuda() - b).max() / (An * np.abs(xs[1]).max() + torch.abs(b).max())).item()
    assert res <= 1e-14, res
    assert np.abs(xs[0] - xs[1]).max() <= 1e-10 * np.abs(xs[0]).max()


@pytest.mark.parametrize("N,alg", [(700, "LDL"), (2048, "CHOLESKY"), (2100, "LDL"), (5000, "CHOLESKY"), (11192, "LDL")])
def test_inverses_from_the_matrix_cores_match_the_scalar_ones(ctx, N, alg):
    """The 256 x 256 explicit inverses the solves apply come from an MFMA kernel that pushes identity rows through the panel
    factorization's row operations (option linv_mfma, default) instead of the scalar block substitution: same solutions
    (orders with a 128-row last triangle included), backward error at rounding level."""
    rng = np.random.default_rng(N)
    R = rng.standard_normal((N, 48))
    A = R @ R.T + np.diag(rng.random(N) * 10 + 1.0)
    if alg == "LDL":
        h = N // 3
        A[N - h:, N - h:] = -(A[N - h:, N - h:] + 2.0 * np.eye(h) * N ** 0.5)
    b = rng.standard_normal(N)
    xs = []
    for mfma in (0, 1):
        ls = mj.HipLinearSolver(np.asfortranarray(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg))
        ls.set_option("linv_mfma", mfma)
        ls.factorize()
        x = b.copy()
        ls.solve_linear_system(x)
        xs.append(x)
        ls.close()
    res = np.abs(A @ xs[1] - b).max() / (np.abs(A).sum(axis=1).max() * np.abs(xs[1]).max() + np.abs(b).max())
    assert res <= 1e-14, res
    assert np.abs(xs[0] - xs[1]).max() <= 1e-10 * np.abs(xs[0]).max()


def test_environment_overrides_win_over_set_option(ctx, monkeypatch, capfd):
    """MNK_OPTIONS="key=value,..." fixes options for unmodified callers: read at mnk_ls_create, kept against later
    mnk_ls_set_option calls (the mirror sets its HipSolverOptions right after the constructor), unknown keys reported and
    ignored."""
    rng = np.random.default_rng(3)
    N = 1700
    R = rng.standard_normal((N, 32))
    A = R @ R.T + np.eye(N) * 5.0
    monkeypatch.setenv("MNK_OPTIONS", "panel_algo=1,no_such_option=3,dag_chunk=8")
    ls = mj.HipLinearSolver(np.asfortranarray(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm="CHOLESKY", panel_algo=5))
    ls.factorize()
    assert ls.inertia() == (N, 0, 0)
    assert ls.get_stat("panel_algo") == 1.0
    ls.close()
    assert "no_such_option" in capfd.readouterr().err
    monkeypatch.delenv("MNK_OPTIONS")
    ls = mj.HipLinearSolver(np.asfortranarray(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm="CHOLESKY", panel_algo=5))
    ls.factorize()
    assert ls.get_stat("panel_algo") == 5.0
    ls.close()


def test_deployment_shorthands_pin_the_non_persistent_schedules(ctx, monkeypatch):
    """MNK_PANEL_ALGO / MNK_PERSISTENT_SOLVE, the two shorthands INTEGRATION.md gives a deployment that shares a GPU between
    processes: read at mnk_ls_create like MNK_OPTIONS, pinned against later set_option calls; the factorization then runs one
    launch per piece and the stepwise solve still solves."""
    rng = np.random.default_rng(4)
    N = 1700
    R = rng.standard_normal((N, 32))
    A = R @ R.T + np.eye(N) * 5.0
    monkeypatch.setenv("MNK_PANEL_ALGO", "1")
    monkeypatch.setenv("MNK_PERSISTENT_SOLVE", "0")
    ls = mj.HipLinearSolver(np.asfortranarray(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm="CHOLESKY", panel_algo=5))
    ls.set_option("persistent_solve", 1)   # ignored: pinned
    ls.factorize()
    assert ls.inertia() == (N, 0, 0)
    assert ls.get_stat("panel_algo") == 1.0
    assert ls.get_stat("pinned:panel_algo") == 1.0 and ls.get_stat("pinned:persistent_solve") == 1.0
    b = rng.standard_normal(N)
    x = b.copy()
    ls.solve_linear_system(x)
    res = np.abs(A @ x - b).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
    assert res <= 1e-14, res
    ls.close()
    monkeypatch.delenv("MNK_PANEL_ALGO")
    monkeypatch.delenv("MNK_PERSISTENT_SOLVE")
    ls = mj.HipLinearSolver(np.asfortranarray(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm="CHOLESKY", panel_algo=5))
    assert ls.get_stat("pinned:panel_algo") == 0.0 and ls.get_stat("pinned:persistent_solve") == 0.0
    ls.close()

"""(-m gpu) The device eigendecomposition solver (lapack_algorithm = EVD; csrc/evd.hip) against dsyevd: exact answers on a
family of diagonal matrices, LAPACK's scaled test ratios within 20 x max(1, dsyevd's own) on five kinds of matrices, the
oracle's inertia, backward-stable solves from every matrix source, non-finite input, bit-identical repeats (batches and
concurrent host threads included), the contract of an inertia-revealing solver, and the IPM mirror's inertia-based runs with
it against the oracle's EVD.  The measured ratios go to profiles/evd_accuracy.json when MNK_EVD_ACCURACY_OUT names a file."""
import json
import os
import threading
import time

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp
import torch

import madnlp_jl_amd as mj
from madnlp_jl_amd.problems import dense_dummy_qp, opf_shaped
from oracle.lapack_cpu import EVD, LapackCPUSolver
from tests.evd_cases import (DIAG_SIZES, EPS, KINDS, SIZES, backward_error, diag_family, dsyevd, eigenvalue_ratio,
                             is_permutation, lower_with_garbage, ratios, sym_matrix)

pytestmark = pytest.mark.gpu

FACTOR = 20.0        # device ratio <= FACTOR * max(1, dsyevd's ratio on the same matrix)
SWEEP_CAP = 60        # evd_sweep_cap of csrc/evd.hip
OPT = mj.HipSolverOptions(lapack_algorithm=mj.EVD)
_measured = {}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()
    out = os.environ.get("MNK_EVD_ACCURACY_OUT")
    if out and _measured:
        with open(out, "w") as f:
            json.dump({"bound": "device <= 20 * max(1, dsyevd)", "cases": _measured}, f, indent=1, sort_keys=True)


def evd_of(src, ctx):
    s = mj.HipLinearSolver(src, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.EVD))
    s.factorize()
    Q, lam = s.get_factor()
    return s, Q, lam


def check_against_dsyevd(name, A, Q, lam):
    """The three ratios of the device's decomposition, each within FACTOR x max(1, dsyevd's own ratio)."""
    lam_ref, Q_ref = dsyevd(A)
    res, orth = ratios(A, lam, Q)
    res_ref, orth_ref = ratios(A, lam_ref, Q_ref)
    eig = eigenvalue_ratio(lam, lam_ref)
    _measured[name] = {"residual": res, "orthogonality": orth, "eigenvalues": eig, "residual_dsyevd": res_ref,
                       "orthogonality_dsyevd": orth_ref}
    print(f"{name}: residual {res:.3g} (dsyevd {res_ref:.3g}), orthogonality {orth:.3g} (dsyevd {orth_ref:.3g}), "
          f"eigenvalues {eig:.3g}")
    assert np.all(np.diff(lam) >= 0)
    assert res <= FACTOR * max(1.0, res_ref), (res, res_ref)
    assert orth <= FACTOR * max(1.0, orth_ref), (orth, orth_ref)
    assert eig <= FACTOR, eig
    return lam_ref


# --------------------------------------------------------------------------- exact answers
def check_exact(s, Q, lam, A, d):
    assert s.info == 0
    assert np.array_equal(lam, np.sort(d))
    assert is_permutation(Q)
    assert np.array_equal(A @ Q, Q * lam)
    ref = LapackCPUSolver(A, EVD).factorize()
    assert s.inertia() == ref.inertia() == (int((d > 0).sum()), 1, int((d < 0).sum()))


@pytest.mark.parametrize("N", DIAG_SIZES)
def test_diagonal_family_is_exact(ctx, N):
    A, d = diag_family(N)
    s, Q, lam = evd_of(lower_with_garbage(A), ctx)
    check_exact(s, Q, lam, A, d)
    s.close()


@pytest.mark.parametrize("N", [65, 1000, 2100])
def test_diagonal_family_lower_csc_and_device_input(ctx, N):
    A, d = diag_family(N, seed=N + 1)
    Lc = sp.csc_matrix(np.tril(A))
    s, Q, lam = evd_of((Lc.indptr, Lc.indices, Lc.data), ctx)
    check_exact(s, Q, lam, A, d)
    s.close()
    s, Q, lam = evd_of(torch.from_numpy(lower_with_garbage(A, 3)).cuda(), ctx)
    check_exact(s, Q, lam, A, d)
    s.close()


def test_zero_matrix(ctx):
    N = 200
    s, Q, lam = evd_of(np.zeros((N, N), order="F"), ctx)
    assert s.info == 0
    assert np.array_equal(lam, np.zeros(N))
    assert is_permutation(Q)
    assert s.inertia() == (0, N, 0)
    x = s.solve_linear_system(np.ones(N))      # an IEEE division by the zero eigenvalues, no exception
    assert not np.isfinite(x).any()
    s.close()


# --------------------------------------------------------------------------- random kinds against dsyevd
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_random_matrices_against_dsyevd(ctx, kind, N):
    A = sym_matrix(N, kind)
    s, Q, lam = evd_of(lower_with_garbage(A), ctx)
    assert s.info == 0
    assert 1 <= s.get_stat("evd_sweeps") <= SWEEP_CAP
    check_against_dsyevd(f"{kind}-{N}", A, Q, lam)
    assert s.inertia() == LapackCPUSolver(A, EVD).factorize().inertia()
    b = np.random.default_rng(N + 1).standard_normal(N)
    x = s.solve_linear_system(b.copy())
    err = backward_error(A, x, b)
    _measured[f"{kind}-{N}"]["solve_backward_error"] = err
    _measured[f"{kind}-{N}"]["sweeps"] = s.get_stat("evd_sweeps")
    assert err <= 1e-13, err
    s.close()


# --------------------------------------------------------------------------- sources
def _sc_system(ctx, P):
    k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                    opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.EVD))
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess
    k.compress_jacobian()
    k.compress_hessian()
    k.set_aug_diagonal()
    k.build_kkt()
    return k


def test_sparse_condensed_source_indefinite(ctx):
    P = opf_shaped("case118", du=1e-8, indefinite=True)
    k = _sc_system(ctx, P)
    k.linear_solver.factorize()
    assert k.linear_solver.info == 0
    Kd = k.aug_com.to_dense()
    K = Kd + np.tril(Kd, -1).T
    Q, lam = k.linear_solver.get_factor()
    lam_ref = check_against_dsyevd("sparse_condensed-case118", K, Q, lam)
    assert lam_ref.min() < 0
    b = np.random.default_rng(5).standard_normal(P.n)
    x = k.linear_solver.solve_linear_system(b.copy())
    assert backward_error(K, x, b) <= 1e-13
    k.close()


def test_dense_condensed_source(ctx):
    P = dense_dummy_qp(300, 100, 7)
    kh = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx,
                                    opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.EVD))
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(kh, f)[:] = getattr(P, f)
    kh.hess[...] = P.hess
    kh.jac[...] = P.jac
    kh.set_aug_diagonal()
    kh.compress_hessian()
    kh.compress_jacobian()
    kh.build_kkt()
    kh.linear_solver.factorize()
    K = kh.aug_com.to_host()
    K = np.tril(K) + np.tril(K, -1).T
    Q, lam = kh.linear_solver.get_factor()
    check_against_dsyevd("dense_condensed-300", K, Q, lam)
    b = np.random.default_rng(6).standard_normal(K.shape[0])
    x = kh.linear_solver.solve_linear_system(b.copy())
    assert backward_error(K, x, b) <= 1e-13
    kh.close()


def test_three_right_hand_sides_in_a_strided_device_view(ctx):
    N, ld = 500, 520
    A = sym_matrix(N, "indefinite", 8)
    s = mj.HipLinearSolver(torch.from_numpy(A).cuda(), ctx=ctx, opt=OPT)
    s.factorize()
    B = np.random.default_rng(9).standard_normal((N, 3))
    buf = torch.zeros((3, ld), dtype=torch.float64, device="cuda")
    buf[:, :N] = torch.from_numpy(B.T.copy())
    X = buf[:, :N].T          # (N, 3) view, stride(1) = ld
    assert X.stride(1) == ld
    s.solve_linear_system(X)
    s.check_solve()
    Xh = X.cpu().numpy()
    for j in range(3):
        assert backward_error(A, Xh[:, j], B[:, j]) <= 1e-13
    assert torch.all(buf[:, N:] == 0)     # nothing written between the columns
    # a host matrix of right-hand sides gives the same bits
    Bh = np.asfortranarray(B.copy())
    s.solve_linear_system(Bh)
    assert np.array_equal(Bh, Xh)
    s.close()


C3_TIME_LIMIT_S = 150.0   # see the docstring below


def test_full_size_c3_matrix(ctx):
    """The order of the bench's C3 system (N = 11 192), once: an SPD matrix (the host's dpotrf succeeds), so the inertia is
    (N, 0, 0); trace and Frobenius norm are invariants of the similarity.  No host eigendecomposition at this size.
    Time limit: ten times the first measured run (14.7 s for 23 sweeps on one MI355X), rounded up."""
    P = opf_shaped("case1354pegase", du=1e-8)
    assert P.n == 11192
    N = P.n
    k = _sc_system(ctx, P)
    Kd = k.aug_com.to_dense()
    K = Kd + np.tril(Kd, -1).T
    del Kd
    _, info = sl.lapack.dpotrf(K, lower=1)
    assert info == 0
    t0 = time.perf_counter()
    k.linear_solver.factorize()
    elapsed = time.perf_counter() - t0
    print(f"C3 EVD factorize!: {elapsed:.2f} s, {k.linear_solver.get_stat('evd_sweeps'):.0f} sweeps")
    _measured["c3-11192"] = {"factorize_s": elapsed, "sweeps": k.linear_solver.get_stat("evd_sweeps")}
    assert k.linear_solver.info == 0
    assert k.linear_solver.inertia() == (N, 0, 0)
    _, lam = k.linear_solver.get_factor_device()
    lam = lam.cpu().numpy()
    assert np.all(np.diff(lam) >= 0)
    fro = np.linalg.norm(K)
    tol = FACTOR * N * EPS * fro
    _measured["c3-11192"]["trace_ratio"] = abs(lam.sum() - np.trace(K)) / (N * EPS * fro)
    _measured["c3-11192"]["norm_ratio"] = abs(np.linalg.norm(lam) - fro) / (N * EPS * fro)
    assert abs(lam.sum() - np.trace(K)) <= tol
    assert abs(np.linalg.norm(lam) - fro) <= tol
    b = np.random.default_rng(18).standard_normal(N)
    x = k.linear_solver.solve_linear_system(b.copy())
    err = backward_error(K, x, b)
    _measured["c3-11192"]["solve_backward_error"] = err
    assert err <= 1e-13, err
    assert elapsed <= C3_TIME_LIMIT_S, elapsed
    k.close()


# --------------------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_returns_with_positive_info(ctx, bad):
    N = 300
    A = sym_matrix(N, "indefinite", 19)
    A[200, 100] = A[100, 200] = bad
    s = mj.HipLinearSolver(A, ctx=ctx, opt=OPT)
    s.factorize()                      # returns: a norm that is not finite, or the sweep cap, ends it
    assert s.info > 0
    assert s.get_stat("evd_sweeps") <= SWEEP_CAP
    p, z, n = s.inertia()              # the counts never include the padding
    assert p + z + n == N and min(p, z, n) >= 0
    # the next factorization of a clean matrix on the same solver is correct: nothing of the padding was poisoned
    B = sym_matrix(N, "indefinite", 20)
    A[...] = B                         # (the solver keeps a reference to A)
    s.factorize()
    assert s.info == 0
    Q, lam = s.get_factor()
    check_against_dsyevd(f"after-{bad}", B, Q, lam)
    assert s.inertia() == LapackCPUSolver(B, EVD).factorize().inertia()
    b = np.ones(N)
    assert backward_error(B, s.solve_linear_system(b.copy()), b) <= 1e-13
    s.close()


# --------------------------------------------------------------------------- determinism
def test_repeats_are_bit_identical(ctx):
    N = 1500
    A = sym_matrix(N, "zero_block", 11)
    b = np.random.default_rng(12).standard_normal(N)
    s = mj.HipLinearSolver(A, ctx=ctx, opt=OPT)
    out = []
    for _ in range(2):
        s.factorize()
        Q, lam = s.get_factor()
        out.append((Q, lam, s.solve_linear_system(b.copy())))
    for a, b_ in zip(*out):
        assert np.array_equal(a, b_)
    s.close()


def test_batches_give_the_bits_of_lone_calls(ctx):
    """Inside a factorization batch an EVD factorize! runs when called; an EVD solve inside a solve batch runs at once."""
    N = 1100
    A = sym_matrix(N, "spd", 13)
    dA = torch.from_numpy(A).cuda()
    b = np.random.default_rng(14).standard_normal(N)
    s = mj.HipLinearSolver(dA, ctx=ctx, opt=OPT)
    s.factorize()
    Q0, lam0 = s.get_factor()
    xd = torch.from_numpy(b.copy()).cuda()
    s.solve_linear_system(xd)
    s.check_solve()
    x0 = xd.cpu().numpy()
    other = mj.HipLinearSolver(dA, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY))
    with mj.factorize_batch():
        s.factorize()
        other.factorize()
    Q1, lam1 = s.get_factor()
    assert np.array_equal(Q0, Q1) and np.array_equal(lam0, lam1)
    assert other.inertia() == (N, 0, 0)
    xd = torch.from_numpy(b.copy()).cuda()
    with mj.solve_batch():
        s.solve_linear_system(xd)
    s.check_solve()
    assert np.array_equal(xd.cpu().numpy(), x0)
    other.close()
    s.close()


def test_two_contexts_on_two_threads_get_the_same_bits():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    N = 900
    A = sym_matrix(N, "zero_block", 15)
    b = np.random.default_rng(16).standard_normal(N)
    res, errs = [None, None], []

    def work(i):
        try:
            c = mj.HipContext(0)
            s = mj.HipLinearSolver(A, ctx=c, opt=mj.HipSolverOptions(lapack_algorithm=mj.EVD))
            for _ in range(2):
                s.factorize()
            Q, lam = s.get_factor()
            res[i] = (Q, lam, s.solve_linear_system(b.copy()))
            s.close()
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for a, b_ in zip(res[0], res[1]):
        assert np.array_equal(a, b_)
    assert backward_error(A, res[0][2], b) <= 1e-13


# --------------------------------------------------------------------------- contract
def test_contract_of_an_inertia_revealing_solver(ctx):
    N = 200
    A = sym_matrix(N, "indefinite", 21)
    s = mj.HipLinearSolver(A, ctx=ctx, opt=OPT)
    assert s.is_inertia()
    assert "EVD" in s.introduce()
    with pytest.raises(mj.SolveException):
        s.solve_linear_system(np.ones(N))      # a solve before a factorization
    for key, val in (("accept_only_pd", 1), ("early_reject", 1), ("envelope", 0), ("probe", 0), ("panel_algo", 1)):
        s.set_option(key, val)                 # what the KKT systems set on any solver: accepted, ignored
    s.factorize()
    assert s.info == 0
    assert 1 <= s.get_stat("evd_sweeps") <= SWEEP_CAP
    lam_ref, _ = dsyevd(A)
    assert s.inertia() == (int((lam_ref > 0).sum()), 0, int((lam_ref < 0).sum()))
    with pytest.raises(mj.HipError):
        s.get_pivots()
    assert s.bk_info()[0] is False
    s.close()


def test_schur_stage_refuses_evd(ctx):
    blk, nd = 8, 3
    rng = np.random.default_rng(17)
    A = [np.asfortranarray(np.eye(blk))]
    Cs = [np.asfortranarray(rng.standard_normal((nd, blk)))]
    with pytest.raises(mj.HipError):
        mj.SchurDenseStage(A, Cs, np.eye(nd), nd, blk, ctx=ctx, algorithm=mj.EVD)


# --------------------------------------------------------------------------- end to end: the IPM mirror, inertia-based
def _evd_factory(kind, nlp, ctx):
    opt = mj.HipSolverOptions(lapack_algorithm=mj.EVD)

    def make(info):
        if kind == "sparse_condensed":
            return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J,
                                               info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx, opt_linear_solver=opt)
        if kind == "dense_condensed":
            return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                              info["ind_ub"], ctx=ctx, opt_linear_solver=opt)
        return mj.DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx,
                                 opt_linear_solver=opt)
    return make


def _evd_vs_oracle_evd(kind, nlp, ctx, tol, n):
    from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
    from tests.test_inertia_free_cpu import factory
    sparse = kind == "sparse_condensed"
    runs = []
    for fac in (factory(kind, nlp, EVD), _evd_factory(kind, nlp, ctx)):
        opt = IPMOptions(tol=tol)
        if sparse:
            opt.relax_equality, opt.dual_initialization = True, "zero"
        s = MadNLPSolver(nlp, fac, opt, sparse=sparse)
        s.solve()
        runs.append(s)
    so, sh = runs
    assert "EVD" in sh.kkt.linear_solver.introduce()
    assert so.inertia_correction_method == sh.inertia_correction_method == "inertia_based"
    assert so.status == sh.status == "SOLVE_SUCCEEDED", (so.status, sh.status)
    assert abs(sh.cnt.k - so.cnt.k) <= 2, (sh.cnt.k, so.cnt.k)
    np.testing.assert_allclose(sh.x[:n], so.x[:n], atol=1e-6)
    if hasattr(sh.kkt, "close"):
        sh.kkt.close()


@pytest.mark.parametrize("kind", ["dense_condensed", "sparse_condensed"])
def test_ipm_hs15_evd_inertia_based(ctx, kind):
    from madnlp_jl_amd.problems import HS15Model
    _evd_vs_oracle_evd(kind, HS15Model(), ctx, 1e-8 if kind != "sparse_condensed" else 1e-6, 2)


@pytest.mark.parametrize("n,m,n_eq", [(10, 5, 0), (50, 10, 0), (20, 15, 2)])
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_ipm_dense_qp_evd_inertia_based(ctx, kind, n, m, n_eq):
    from madnlp_jl_amd.problems import DenseQPModel
    _evd_vs_oracle_evd(kind, DenseQPModel(n, m, n_eq), ctx, 1e-8, n)


def test_ipm_sparse_qp_evd_inertia_based(ctx):
    from madnlp_jl_amd.problems import SparseQPModel
    nlp = SparseQPModel("case30")
    _evd_vs_oracle_evd("sparse_condensed", nlp, ctx, 1e-6, nlp.n)

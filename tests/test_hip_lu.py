"""(-m gpu) The device LU solver (lapack_algorithm = LU; csrc/lu.hip): dgetrf's factors, pivots and info bit for bit on matrices
whose elimination is exact (tests/lu_exact.py), to rounding on general ones, backward-stable solves from every matrix source,
singular and non-finite input, bit-identical repeats (batches and concurrent host threads included), the contract of a solver
without inertia, and the IPM mirror's inertia-free runs with it against the oracle's LU."""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp
import torch

import madnlp_jl_amd as mj
from madnlp_jl_amd.problems import dense_dummy_qp, opf_shaped
from tests.lu_exact import exact_kkt

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def sym_matrix(N, kind, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, N))
    if kind == "spd":
        A = G @ G.T / N + np.eye(N)
    else:
        A = (G + G.T) / 2
        if kind == "zero_block":   # a zero leading diagonal block (KKT-like)
            k = N // 3
            A[:k, :k] = 0.0
    return np.asfortranarray(A)


def backward_error(A, x, b):
    return np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())


def lower_with_garbage(A, seed=7):
    """'L' storage: the strict upper triangle may hold anything."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.tril(A) + np.triu(rng.standard_normal(A.shape), 1))


def row_perm(ipiv):
    """perm with (P A)[i] = A[perm[i]] for dgetrf's 1-based ipiv."""
    perm = np.arange(len(ipiv))
    for k, p in enumerate(ipiv - 1):
        perm[[k, p]] = perm[[p, k]]
    return perm


def factor_residual(A, F, ipiv):
    Lf = np.tril(F, -1) + np.eye(F.shape[0])
    return np.linalg.norm(A[row_perm(ipiv)] - Lf @ np.triu(F)) / np.linalg.norm(A)


def lu_of(src, ctx):
    s = mj.HipLUSolver(src, ctx=ctx)
    s.factorize()
    F, D = s.get_factor()
    return s, F, D, s.get_pivots()


@pytest.mark.parametrize("N", [5, 63, 64, 65, 300, 1000, 2100, 4672])
def test_exact_matrices_equal_dgetrf(ctx, N):
    """Dense input with garbage in the upper triangle: ipiv, L\\U, diag(U) and info equal dgetrf's, bit for bit."""
    A, _ = exact_kkt(N, N)
    lu, piv, info = sl.lapack.dgetrf(A)
    assert info == 0
    s, F, D, ipiv = lu_of(lower_with_garbage(A), ctx)
    assert s.info == info
    assert np.array_equal(ipiv, piv + 1)
    assert np.array_equal(F, lu)
    assert np.array_equal(D, np.diag(lu))
    s.close()


@pytest.mark.parametrize("N", [65, 1000, 2100])
def test_exact_matrices_lower_csc_and_device_input(ctx, N):
    A, _ = exact_kkt(N, N + 1)
    lu, piv, info = sl.lapack.dgetrf(A)
    Lc = sp.csc_matrix(np.tril(A))
    s, F, _, ipiv = lu_of((Lc.indptr, Lc.indices, Lc.data), ctx)
    assert s.info == info == 0
    assert np.array_equal(ipiv, piv + 1) and np.array_equal(F, lu)
    s.close()
    s, F, _, ipiv = lu_of(torch.from_numpy(lower_with_garbage(A, 3)).cuda(), ctx)
    assert np.array_equal(ipiv, piv + 1) and np.array_equal(F, lu)
    b = np.random.default_rng(N).standard_normal(N)
    assert backward_error(A, s.solve_linear_system(b.copy()), b) <= 1e-13
    s.close()


@pytest.mark.parametrize("N,kind", [(64, "indefinite"), (100, "zero_block"), (257, "spd"), (1000, "zero_block"),
                                    (2048, "indefinite"), (4672, "zero_block")])
def test_random_matrices_match_dgetrf(ctx, N, kind):
    A = sym_matrix(N, kind, N)
    s, F, D, ipiv = lu_of(lower_with_garbage(A), ctx)
    lu, piv, info = sl.lapack.dgetrf(A)
    assert s.info == info == 0
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)  # noqa: E731
    assert rel(F, lu) <= 1e-12
    assert factor_residual(A, F, ipiv) <= 1e-13
    b = np.random.default_rng(N + 1).standard_normal(N)
    x = s.solve_linear_system(b.copy())
    assert backward_error(A, x, b) <= 1e-13
    s.close()


def _sc_system(ctx, P):
    k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                    linear_solver=mj.HipLUSolver)
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
    assert np.linalg.eigvalsh(K).min() < 0
    F, _ = k.linear_solver.get_factor()
    assert factor_residual(K, F, k.linear_solver.get_pivots()) <= 1e-13
    b = np.random.default_rng(5).standard_normal(P.n)
    x = k.linear_solver.solve_linear_system(b.copy())
    assert backward_error(K, x, b) <= 1e-13
    k.close()


def test_dense_condensed_source(ctx):
    P = dense_dummy_qp(300, 100, 7)
    kh = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx, linear_solver=mj.HipLUSolver)
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
    b = np.random.default_rng(6).standard_normal(K.shape[0])
    x = kh.linear_solver.solve_linear_system(b.copy())
    assert backward_error(K, x, b) <= 1e-13
    kh.close()


def test_three_right_hand_sides_in_a_strided_device_view(ctx):
    N, ld = 500, 520
    A = sym_matrix(N, "indefinite", 8)
    s = mj.HipLUSolver(torch.from_numpy(A).cuda(), ctx=ctx)
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
    s.close()


def test_full_size_c3_matrix(ctx):
    """The order of the bench's C3 system (N = 11 192): one factorize! + solve!."""
    P = opf_shaped("case1354pegase", du=1e-8)
    assert P.n == 11192
    k = _sc_system(ctx, P)
    k.linear_solver.factorize()
    assert k.linear_solver.info == 0
    Kd = k.aug_com.to_dense()
    K = Kd + np.tril(Kd, -1).T
    del Kd
    b = np.random.default_rng(18).standard_normal(P.n)
    x = k.linear_solver.solve_linear_system(b.copy())
    assert backward_error(K, x, b) <= 1e-12
    k.close()


# --------------------------------------------------------------------------- singular and non-finite input
def test_zero_matrix_gives_info_1(ctx):
    A = np.zeros((200, 200), order="F")
    s = mj.HipLUSolver(A, ctx=ctx)
    s.factorize()                      # never raises on a numerical breakdown
    assert s.info == 1
    assert np.array_equal(s.get_pivots(), np.arange(1, 201))
    s.close()


@pytest.mark.parametrize("N,row", [(300, 7), (1000, 250), (2100, 600)])
def test_exact_zero_pivot_gives_dgetrf_info(ctx, N, row):
    """A zero J entry: a zero row and column.  info, pivots and factors are dgetrf's (the elimination goes on past the zero
    pivot), and the solve returns what getrs returns."""
    A, _ = exact_kkt(N, N, zero_j_row=row)
    lu, piv, info = sl.lapack.dgetrf(A)
    assert info > 0
    s, F, _, ipiv = lu_of(A, ctx)
    assert s.info == info
    assert np.array_equal(ipiv, piv + 1) and np.array_equal(F, lu)
    b = np.ones(N)
    x = s.solve_linear_system(b.copy())
    assert not np.isfinite(x).all()
    s.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_completes(ctx, bad):
    N = 700
    A = sym_matrix(N, "indefinite", 19)
    A[400, 200] = A[200, 400] = bad
    s = mj.HipLUSolver(A, ctx=ctx)
    s.factorize()
    F, _ = s.get_factor()
    assert not np.isfinite(F).all()
    x = s.solve_linear_system(np.ones(N))
    lu, piv, _ = sl.lapack.dgetrf(A)
    x_ref, _ = sl.lapack.dgetrs(lu, piv, np.ones(N))
    # what getrs gives: NaN spreads into the solution; an Inf pivot leaves zero multipliers and a finite solution
    assert np.isfinite(x).all() == np.isfinite(x_ref).all() == (bad == np.inf)
    s.close()
    # the solver is still usable afterwards
    B = sym_matrix(N, "indefinite", 20)
    t = mj.HipLUSolver(B, ctx=ctx)
    t.factorize()
    b = np.ones(N)
    assert backward_error(B, t.solve_linear_system(b.copy()), b) <= 1e-13
    t.close()


# --------------------------------------------------------------------------- determinism
def test_repeats_are_bit_identical(ctx):
    N = 1500
    A = sym_matrix(N, "zero_block", 11)
    b = np.random.default_rng(12).standard_normal(N)
    s = mj.HipLUSolver(A, ctx=ctx)
    out = []
    for _ in range(2):
        s.factorize()
        F, D = s.get_factor()
        out.append((F, D, s.get_pivots(), s.solve_linear_system(b.copy())))
    for a, b_ in zip(*out):
        assert np.array_equal(a, b_)
    s.close()


def test_batches_give_the_bits_of_lone_calls(ctx):
    """Inside a factorization batch an LU factorize! runs when called; an LU solve inside a solve batch runs at once."""
    N = 1100
    A = sym_matrix(N, "indefinite", 13)
    dA = torch.from_numpy(A).cuda()
    b = np.random.default_rng(14).standard_normal(N)
    s = mj.HipLUSolver(dA, ctx=ctx)
    s.factorize()
    F0, p0 = s.get_factor()[0], s.get_pivots()
    xd = torch.from_numpy(b.copy()).cuda()
    s.solve_linear_system(xd)
    s.check_solve()
    x0 = xd.cpu().numpy()
    other = mj.HipLinearSolver(dA, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY))
    with mj.factorize_batch():
        s.factorize()
        other.factorize()
    assert np.array_equal(F0, s.get_factor()[0]) and np.array_equal(p0, s.get_pivots())
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
    N = 1300
    A = sym_matrix(N, "zero_block", 15)
    b = np.random.default_rng(16).standard_normal(N)
    res, errs = [None, None], []

    def work(i):
        try:
            c = mj.HipContext(0)
            s = mj.HipLUSolver(A, ctx=c)
            for _ in range(3):
                s.factorize()
            F, D = s.get_factor()
            res[i] = (F, D, s.get_pivots(), s.solve_linear_system(b.copy()))
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
    assert backward_error(A, res[0][3], b) <= 1e-13


# --------------------------------------------------------------------------- contract
def test_contract_of_a_solver_without_inertia(ctx):
    s = mj.HipLUSolver(sym_matrix(200, "indefinite", 21), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LU))
    assert not s.is_inertia()
    assert "LU" in s.introduce()
    s.factorize()
    with pytest.raises(mj.InertiaException):
        s.inertia()
    p, z, n = C.c_int64(), C.c_int64(), C.c_int64()
    assert mj.lib().mnk_ls_inertia(s._h, C.byref(p), C.byref(z), C.byref(n)) != 0
    msg = mj.lib().mnk_last_error_string()
    assert b"inertia" in msg and b"LU" in msg
    s.close()
    for algo in (mj.QR, mj.LDL):
        t = mj.HipLinearSolver(np.eye(4, order="F"), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=algo))
        t.factorize()
        with pytest.raises(mj.HipError):
            t.get_pivots()
        t.close()


def test_schur_stage_refuses_lu(ctx):
    blk, nd = 8, 3
    rng = np.random.default_rng(17)
    A = [np.asfortranarray(np.eye(blk))]
    Cs = [np.asfortranarray(rng.standard_normal((nd, blk)))]
    with pytest.raises(mj.HipError):
        mj.SchurDenseStage(A, Cs, np.eye(nd), nd, blk, ctx=ctx, algorithm=mj.LU)


# --------------------------------------------------------------------------- end to end: the IPM mirror, inertia-free
def _lu_factory(kind, nlp, ctx):
    def make(info):
        if kind == "sparse_condensed":
            return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J,
                                               info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx, linear_solver=mj.HipLUSolver)
        if kind == "dense_condensed":
            return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                              info["ind_ub"], ctx=ctx, linear_solver=mj.HipLUSolver)
        return mj.DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx,
                                 linear_solver=mj.HipLUSolver)
    return make


def _lu_vs_oracle_lu(kind, nlp, ctx, tol, n):
    from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
    from oracle.lapack_cpu import LU
    from tests.test_inertia_free_cpu import factory
    sparse = kind == "sparse_condensed"
    runs = []
    for fac in (factory(kind, nlp, LU), _lu_factory(kind, nlp, ctx)):
        opt = IPMOptions(tol=tol)
        if sparse:
            opt.relax_equality, opt.dual_initialization = True, "zero"
        s = MadNLPSolver(nlp, fac, opt, sparse=sparse)
        s.solve()
        runs.append(s)
    so, sh = runs
    assert so.inertia_correction_method == sh.inertia_correction_method == "inertia_free"
    assert so.status == sh.status == "SOLVE_SUCCEEDED", (so.status, sh.status)
    assert abs(sh.cnt.k - so.cnt.k) <= 2, (sh.cnt.k, so.cnt.k)
    np.testing.assert_allclose(sh.x[:n], so.x[:n], atol=1e-6)
    if hasattr(sh.kkt, "close"):
        sh.kkt.close()


@pytest.mark.parametrize("kind", ["dense", "dense_condensed", "sparse_condensed"])
def test_ipm_hs15_lu_inertia_free(ctx, kind):
    from madnlp_jl_amd.problems import HS15Model
    _lu_vs_oracle_lu(kind, HS15Model(), ctx, 1e-8 if kind != "sparse_condensed" else 1e-6, 2)


@pytest.mark.parametrize("n,m,n_eq", [(10, 5, 0), (50, 10, 0), (20, 15, 2)])
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_ipm_dense_qp_lu_inertia_free(ctx, kind, n, m, n_eq):
    from madnlp_jl_amd.problems import DenseQPModel
    _lu_vs_oracle_lu(kind, DenseQPModel(n, m, n_eq), ctx, 1e-8, n)


def test_ipm_sparse_qp_lu_inertia_free(ctx):
    from madnlp_jl_amd.problems import SparseQPModel
    nlp = SparseQPModel("case30")
    _lu_vs_oracle_lu("sparse_condensed", nlp, ctx, 1e-6, nlp.n)

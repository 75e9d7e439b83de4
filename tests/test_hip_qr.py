"""(-m gpu) The device QR solver (lapack_algorithm = QR; csrc/qr.hip): dgeqrf's factor layout to rounding, backward-stable solves
from every matrix source, bit-identical repeats (batches and concurrent host threads included), the contract of a solver without
inertia, and the IPM mirror's inertia-free runs with it against the oracle's LU inertia-free runs."""
import threading

import numpy as np
import pytest
import scipy.linalg as sl
import torch

import madnlp_jl_amd as mj
from madnlp_jl_amd.problems import dense_dummy_qp, opf_shaped

pytestmark = pytest.mark.gpu

QR_OPT = mj.HipSolverOptions(lapack_algorithm=mj.QR)


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
        if kind == "zero_block":   # a zero leading diagonal block (KKT-like: not positive definite, no usable pivots there)
            k = N // 3
            A[:k, :k] = 0.0
    return np.asfortranarray(A)


def backward_error(A, x, b):
    return np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())


def lower_with_garbage(A, seed=7):
    """'L' storage: the strict upper triangle may hold anything."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.tril(A) + np.triu(rng.standard_normal(A.shape), 1))


@pytest.mark.parametrize("N,kind", [(64, "indefinite"), (100, "zero_block"), (257, "spd"), (1000, "zero_block"),
                                    (2048, "indefinite"), (4672, "zero_block")])
def test_factor_matches_lapack_dgeqrf(ctx, N, kind):
    """R, V and tau as dgeqrf puts them, to rounding, on tril_to_full(A) (dlarfg's sign rule: no column sign flips)."""
    A = sym_matrix(N, kind, N)
    s = mj.HipLinearSolver(lower_with_garbage(A), ctx=ctx, opt=QR_OPT)
    s.factorize()
    assert s.info == 0
    F, tau = s.get_factor()
    qr, tau_ref, _, info = sl.lapack.dgeqrf(A)
    assert info == 0
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)  # noqa: E731
    assert rel(np.triu(F), np.triu(qr)) <= 1e-12
    assert rel(np.tril(F, -1), np.tril(qr, -1)) <= 1e-12
    assert rel(tau, tau_ref) <= 1e-12
    s.close()


def test_solve_dense_sources_host_and_device(ctx):
    """The dense source from the host and from the device, both with a leading dimension larger than the order."""
    import ctypes as C
    N, lda = 777, 800
    A = sym_matrix(N, "zero_block", 1)
    M = lower_with_garbage(A)
    b = np.random.default_rng(2).standard_normal(N)
    Ah = np.zeros((lda, N), order="F")
    Ah[:N] = M
    s = mj.HipLinearSolver(M, ctx=ctx, opt=QR_OPT)
    info = C.c_int(-1)
    mj._lib.check(mj.lib().mnk_ls_factorize_dense(s._h, C.c_void_p(Ah.ctypes.data), lda, mj._lib.MNK_HOST, C.byref(info)))
    assert info.value == 0
    x = s.solve_linear_system(b.copy())
    assert backward_error(A, x, b) <= 1e-13
    s.close()
    buf = torch.zeros((N, lda), dtype=torch.float64, device="cuda")   # row c = column c of the column-major matrix
    buf[:, :N] = torch.from_numpy(np.ascontiguousarray(M.T)).cuda()
    dA = buf[:, :N].T
    assert max(dA.stride()) == lda
    sd = mj.HipLinearSolver(dA, ctx=ctx, opt=QR_OPT)
    sd.factorize()
    xd = torch.from_numpy(b.copy()).cuda()
    sd.solve_linear_system(xd)
    sd.check_solve()
    assert backward_error(A, xd.cpu().numpy(), b) <= 1e-13
    sd.close()


def test_solve_csc_source(ctx):
    import scipy.sparse as sp
    N = 600
    rng = np.random.default_rng(3)
    S = sp.random(N, N, density=0.02, random_state=4, format="csc")
    A = (S + S.T).toarray() + np.diag(rng.standard_normal(N))
    Lc = sp.csc_matrix(np.tril(A))
    s = mj.HipLinearSolver((Lc.indptr, Lc.indices, Lc.data), ctx=ctx, opt=QR_OPT)
    s.factorize()
    b = rng.standard_normal(N)
    x = s.solve_linear_system(b.copy())
    assert backward_error(A, x, b) <= 1e-13
    s.close()


def _sc_system(ctx, P):
    k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                    opt_linear_solver=QR_OPT)
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess
    k.compress_jacobian()
    k.compress_hessian()
    k.set_aug_diagonal()
    k.build_kkt()
    return k


def test_solve_sparse_condensed_source_indefinite(ctx):
    """An indefinite opf-shaped KKT matrix (the options the system sets for its solver, accept_only_pd / early_reject, are ignored)."""
    P = opf_shaped("case118", du=1e-8, indefinite=True)
    k = _sc_system(ctx, P)
    k.linear_solver.factorize()
    Kd = k.aug_com.to_dense()
    K = Kd + np.tril(Kd, -1).T
    assert np.linalg.eigvalsh(K).min() < 0
    b = np.random.default_rng(5).standard_normal(P.n)
    x = k.linear_solver.solve_linear_system(b.copy())
    assert backward_error(K, x, b) <= 1e-13
    k.close()


def test_solve_dense_condensed_source(ctx):
    P = dense_dummy_qp(300, 100, 7)
    kh = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx, opt_linear_solver=QR_OPT)
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
    s = mj.HipLinearSolver(torch.from_numpy(A).cuda(), ctx=ctx, opt=QR_OPT)
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


def test_a_matrix_the_static_pivot_ldl_cannot_factor(ctx):
    """[[0, 1], [1, 0]] blocks on the diagonal: every static pivot is zero; QR solves it."""
    N = 300
    rng = np.random.default_rng(10)
    A = np.zeros((N, N))
    for i in range(0, N, 2):
        A[i, i + 1] = A[i + 1, i] = 1.0
    A = np.asfortranarray(A)
    ldl = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
    ldl.factorize()
    assert ldl.info != 0             # the static-pivot LDL^T breaks down at its first pivot
    ldl.close()
    s = mj.HipLinearSolver(A, ctx=ctx, opt=QR_OPT)
    s.factorize()
    b = rng.standard_normal(N)
    x = s.solve_linear_system(b.copy())
    assert backward_error(A, x, b) <= 1e-13
    s.close()


def test_repeats_are_bit_identical(ctx):
    N = 1500
    A = sym_matrix(N, "zero_block", 11)
    b = np.random.default_rng(12).standard_normal(N)
    s = mj.HipLinearSolver(A, ctx=ctx, opt=QR_OPT)
    out = []
    for _ in range(2):
        s.factorize()
        F, tau = s.get_factor()
        out.append((F, tau, s.solve_linear_system(b.copy())))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])
    s.close()


def test_batches_give_the_bits_of_lone_calls(ctx):
    """Inside a factorization batch a QR factorize! runs when called; a QR solve inside a solve batch runs at once."""
    N = 1100
    A = sym_matrix(N, "indefinite", 13)
    dA = torch.from_numpy(A).cuda()
    b = np.random.default_rng(14).standard_normal(N)
    s = mj.HipLinearSolver(dA, ctx=ctx, opt=QR_OPT)
    s.factorize()
    F0, t0 = s.get_factor()
    xd = torch.from_numpy(b.copy()).cuda()
    s.solve_linear_system(xd)
    s.check_solve()
    x0 = xd.cpu().numpy()
    other = mj.HipLinearSolver(dA, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY))
    with mj.factorize_batch():
        s.factorize()
        other.factorize()
    F1, t1 = s.get_factor()
    assert np.array_equal(F0, F1) and np.array_equal(t0, t1)
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
            s = mj.HipLinearSolver(A, ctx=c, opt=QR_OPT)
            for _ in range(3):
                s.factorize()
            F, tau = s.get_factor()
            res[i] = (F, tau, s.solve_linear_system(b.copy()))
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


def test_contract_of_a_solver_without_inertia(ctx):
    A = np.zeros((200, 200), order="F")     # singular: factorize! does not raise, geqrf's info is 0
    s = mj.HipLinearSolver(A, ctx=ctx, opt=QR_OPT)
    assert not s.is_inertia()
    assert "QR" in s.introduce()
    s.factorize()
    assert s.info == 0
    with pytest.raises(mj.InertiaException):
        s.inertia()
    import ctypes as C
    p, z, n = C.c_int64(), C.c_int64(), C.c_int64()
    assert mj.lib().mnk_ls_inertia(s._h, C.byref(p), C.byref(z), C.byref(n)) != 0
    assert b"inertia" in mj.lib().mnk_last_error_string()
    s.close()
    t = mj.HipLinearSolver(np.eye(4, order="F"), ctx=ctx)
    assert t.is_inertia()
    t.close()


def test_schur_stage_still_refuses_qr(ctx):
    blk, nd = 8, 3
    rng = np.random.default_rng(17)
    A = [np.asfortranarray(np.eye(blk))]
    Cs = [np.asfortranarray(rng.standard_normal((nd, blk)))]
    with pytest.raises(mj.HipError):
        mj.SchurDenseStage(A, Cs, np.eye(nd), nd, blk, ctx=ctx, algorithm=mj.QR)


# --------------------------------------------------------------------------- end to end: the IPM mirror, inertia-free
def _qr_factory(kind, nlp, ctx):
    def make(info):
        if kind == "sparse_condensed":
            return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J,
                                               info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx, opt_linear_solver=QR_OPT)
        if kind == "dense_condensed":
            return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                              info["ind_ub"], ctx=ctx, opt_linear_solver=QR_OPT)
        return mj.DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx,
                                 opt_linear_solver=QR_OPT)
    return make


def _qr_vs_oracle_lu(kind, nlp, ctx, tol, n):
    from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
    from oracle.lapack_cpu import LU
    from tests.test_inertia_free_cpu import factory
    sparse = kind == "sparse_condensed"
    runs = []
    for fac in (factory(kind, nlp, LU), _qr_factory(kind, nlp, ctx)):
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
def test_ipm_hs15_qr_inertia_free(ctx, kind):
    from madnlp_jl_amd.problems import HS15Model
    _qr_vs_oracle_lu(kind, HS15Model(), ctx, 1e-8 if kind != "sparse_condensed" else 1e-6, 2)


@pytest.mark.parametrize("n,m,n_eq", [(10, 5, 0), (50, 10, 0), (20, 15, 2)])
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_ipm_dense_qp_qr_inertia_free(ctx, kind, n, m, n_eq):
    from madnlp_jl_amd.problems import DenseQPModel
    _qr_vs_oracle_lu(kind, DenseQPModel(n, m, n_eq), ctx, 1e-8, n)


def test_ipm_sparse_qp_qr_inertia_free(ctx):
    from madnlp_jl_amd.problems import SparseQPModel
    nlp = SparseQPModel("case30")
    _qr_vs_oracle_lu("sparse_condensed", nlp, ctx, 1e-6, nlp.n)


def test_full_size_c3_matrix(ctx):
    """The order of the bench's C3 system (case1354pegase-shaped sparse condensed KKT, N = 11 192): one factorize! + solve!."""
    P = opf_shaped("case1354pegase", du=1e-8)
    assert P.n == 11192
    k = _sc_system(ctx, P)
    k.linear_solver.factorize()
    Kd = k.aug_com.to_dense()
    K = Kd + np.tril(Kd, -1).T
    del Kd
    b = np.random.default_rng(18).standard_normal(P.n)
    x = k.linear_solver.solve_linear_system(b.copy())
    r = K @ x - b
    assert np.linalg.norm(r) / (np.linalg.norm(K, "fro") * np.linalg.norm(x) + np.linalg.norm(b)) <= 1e-12
    assert backward_error(K, x, b) <= 1e-12
    k.close()

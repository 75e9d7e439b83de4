"""(-m gpu) The device QR solver (csrc/qr.hip) at its edges, against answers that are exact or against columnwise measures
(tests/qr_cases.py): the pairing family's factor, tau and solution bit for bit from every matrix source (tau = 0 inside a
panel, reflectors across panels and 256-row blocks, orders around the padding, K-splits with a ragged last split); exact
covariance under scaling by powers of two; the columnwise backward error, the reflectors' orthogonality and the columnwise
residual on badly scaled matrices, to 8 x LAPACK's own maxima; exactly zero columns; the zero matrix and non-finite input,
and the solver's state after them."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import madnlp_jl_amd as mj
from tests import qr_cases as qc

pytestmark = pytest.mark.gpu

QR_OPT = mj.HipSolverOptions(lapack_algorithm=mj.QR)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def lower_with_garbage(A, seed=7):
    """'L' storage: the strict upper triangle may hold anything."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.tril(A) + np.triu(rng.standard_normal(A.shape), 1))


def padded_device(M, ld):
    """M (column-major image) as a device tensor view with leading dimension ld > n."""
    n = M.shape[0]
    buf = torch.zeros((n, ld), dtype=torch.float64, device="cuda")   # row c = column c of the column-major matrix
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(M.T)).cuda()
    dA = buf[:, :n].T
    assert max(dA.stride()) == ld
    return dA


def qr_of(src, ctx, b=None):
    """(info, F, tau, x) of one fresh solver on src; x solves for b (host vector or column-major matrix)."""
    s = mj.HipLinearSolver(src, ctx=ctx, opt=QR_OPT)
    s.factorize()
    F, tau = s.get_factor()
    x = None if b is None else s.solve_linear_system(b.copy(order="F"))
    info = s.info
    s.close()
    return info, F, tau, x


def assert_same_factor(F, tau, F_ref, tau_ref):
    assert np.array_equal(np.triu(F), np.triu(F_ref))
    assert np.array_equal(np.tril(F, -1), np.tril(F_ref, -1))
    assert np.array_equal(tau, tau_ref)


# --------------------------------------------------------------------------------------------------------------- pairing
@pytest.mark.parametrize("n,fixed_frac", qc.PAIRING_CASES)
def test_pairing_family_bit_for_bit(ctx, n, fixed_frac):
    """R, V, tau and the solution of an integer right-hand side equal the exact answer (which is dgeqrf's, bit for bit:
    tests/test_qr_cases_cpu.py)."""
    A, F_ref, tau_ref = qc.pairing(n, n, fixed_frac)
    b = qc.integer_rhs(n, n)
    x_ref = qc.pairing_solution(A, b)
    sources = [lower_with_garbage(A)]
    if n in qc.PAIRING_SOURCES_SIZES:
        Lc = sp.csc_matrix(np.tril(A))
        sources += [(Lc.indptr, Lc.indices, Lc.data), padded_device(lower_with_garbage(A, 3), n + 23)]
    for src in sources:
        info, F, tau, x = qr_of(src, ctx, b)
        assert info == 0
        assert_same_factor(F, tau, F_ref, tau_ref)
        assert np.array_equal(x, x_ref)


# ------------------------------------------------------------------------------------------------- power-of-two scaling
@pytest.mark.parametrize("n", qc.SCALING_SIZES)
def test_scaling_by_powers_of_two_is_exact(ctx, n):
    """2^k A has the V and tau of A and 2^k times its R, and the solution scales by 2^-k, bit for bit, while every square
    that the one-pass dlarfg forms stays representable."""
    A = qc.graded(n, qc.case_seed(n, "indefinite"), "indefinite", emax=qc.SCALING_EMAX)
    b = np.random.default_rng(n).standard_normal(n)
    info, F0, tau0, x0 = qr_of(A, ctx, b)
    assert info == 0 and np.isfinite(F0).all() and np.isfinite(x0).all()
    amax, amin = np.abs(A).max(), np.abs(A[A != 0]).min()
    for k in qc.SCALING_SHIFTS:
        # inside the range where the property is exact: no square overflows, none is subnormal
        assert np.isfinite((amax * 2.0 ** abs(k)) ** 2 * n) and (amin * 2.0 ** -abs(k)) ** 2 >= np.finfo(np.float64).tiny
        info, F, tau, x = qr_of(np.asfortranarray(A * 2.0 ** k), ctx, b)
        assert info == 0
        assert_same_factor(F, tau, np.triu(F0) * 2.0 ** k + np.tril(F0, -1), tau0)
        assert np.array_equal(x, x0 * 2.0 ** -k), k


# ------------------------------------------------------------------------------------------------- columnwise accuracy
def measures(A, F, tau, seed, X=None, B=None):
    cb = qc.col_backward(A, F, tau, qc.check_columns(A, seed))
    rd = qc.reflector_defect(F, tau)
    om = None if X is None else max(qc.omega(A, X[:, k], B[:, k]) for k in range(B.shape[1]))
    return cb, rd, om


def assert_measures(cb, rd, om):
    msg = f"col_backward {cb:.2f} u (tol {qc.COL_BACKWARD_TOL:.1f}), reflector_defect {rd:.2f} u (tol {qc.REFLECTOR_TOL:.1f}), " \
          f"omega {om if om is None else round(om, 2)} u (tol {qc.OMEGA_TOL:.1f})"
    print(msg)
    assert cb <= qc.COL_BACKWARD_TOL, msg
    assert rd <= qc.REFLECTOR_TOL, msg
    assert om is None or om <= qc.OMEGA_TOL, msg


@pytest.mark.parametrize("n,kind", qc.ACCURACY_CASES)
def test_columnwise_accuracy_on_graded_matrices(ctx, n, kind):
    """Column scales over 2^+-60: every column's backward error relative to its own norm, every reflector's orthogonality and
    the columnwise residual of b = A x_true stay within 8 x LAPACK's maxima.  (576, indefinite) solves three right-hand sides
    whose norms differ by 2^40 in one call."""
    seed = qc.case_seed(n, kind)
    A = qc.graded_case(n, kind)
    scales = qc.MULTI_RHS_SCALES if (n, kind) == qc.MULTI_RHS_CASE else (1.0,)
    _, B = qc.graded_rhs(A, seed, scales)
    info, F, tau, X = qr_of(lower_with_garbage(A), ctx, B)
    assert info == 0
    assert_measures(*measures(A, F, tau, seed, X, B))


@pytest.mark.parametrize("n", qc.ZERO_COLUMN_SIZES)
def test_exactly_zero_columns(ctx, n):
    """A zero row and column in the middle of panel 0 and of a later panel: the column of the factor stays exactly zero
    (R and V), its tau is 0, and the other columns keep their accuracy.  (The matrix is singular: no solve.)"""
    seed = qc.case_seed(n, "zero_column")
    A = qc.graded_case(n, "zero_column")
    info, F, tau, _ = qr_of(lower_with_garbage(A), ctx)
    assert info == 0
    for k in qc.zero_columns(n):
        assert not A[:, k].any()
        assert np.array_equal(F[:k + 1, k], np.zeros(k + 1))
        assert np.array_equal(F[k + 1:, k], np.zeros(n - k - 1))
        assert tau[k] == 0.0
    assert_measures(*measures(A, F, tau, seed))


# ---------------------------------------------------------------------------------------------------- degenerate input
def _refactor_matches_fresh(s, n, ctx):
    """The solver s (order n), after a bad matrix, factors a clean graded matrix to the bits of a fresh solver."""
    A = qc.graded(n, 4242, "indefinite")
    b = np.random.default_rng(n).standard_normal(n)
    info0, F0, tau0, x0 = qr_of(A, ctx, b)
    assert info0 == 0 and np.isfinite(F0).all() and np.isfinite(x0).all()
    s.A[...] = A
    s.factorize()
    F, tau = s.get_factor()
    assert s.info == 0
    assert_same_factor(F, tau, F0, tau0)
    assert np.array_equal(s.solve_linear_system(b.copy()), x0)


def test_zero_matrix(ctx):
    """dgeqrf's answer: F = 0, tau = 0, info = 0; the solve divides by R's zero diagonal like dtrtrs' substitution and returns."""
    n = 100
    s = mj.HipLinearSolver(np.zeros((n, n), order="F"), ctx=ctx, opt=QR_OPT)
    s.factorize()
    F, tau = s.get_factor()
    assert s.info == 0
    assert np.array_equal(F, np.zeros((n, n))) and np.array_equal(tau, np.zeros(n))
    x = s.solve_linear_system(np.ones(n))
    assert x.shape == (n,)                       # non-finite values are accepted
    _refactor_matches_fresh(s, n, ctx)
    s.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_completes_and_leaves_no_state(ctx, bad):
    n = 130
    A = qc.graded(n, 77, "indefinite")
    A[100, 40] = A[40, 100] = bad
    s = mj.HipLinearSolver(A, ctx=ctx, opt=QR_OPT)
    s.factorize()
    F, _ = s.get_factor()
    assert not np.isfinite(F).all()
    x = s.solve_linear_system(np.ones(n))
    assert x.shape == (n,)
    _refactor_matches_fresh(s, n, ctx)
    s.close()

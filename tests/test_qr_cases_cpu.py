"""The QR tests' cases and measures (tests/qr_cases.py) checked on the CPU: the pairing family's expected factor is dgeqrf's
bit for bit; the longdouble measures agree with 40-digit mpmath; LAPACK itself sits at or below one eighth of each tolerance on
every case the GPU tests use; and four planted defects that the normwise criteria of tests/test_hip_qr.py cannot see are all
caught by the columnwise measures."""
import mpmath as mp
import numpy as np
import pytest
import scipy.linalg as sl

from tests import qr_cases as qc


# --------------------------------------------------------------------------------------------------------------- pairing
@pytest.mark.parametrize("fixed_frac", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("n", sorted({n for n, _ in qc.PAIRING_CASES}))
def test_pairing_expected_factor_is_dgeqrf_bit_for_bit(n, fixed_frac):
    A, F, tau = qc.pairing(n, n, fixed_frac)
    assert np.array_equal(A, A.T) and np.count_nonzero(A) == n
    qr, tau_ref, _, info = sl.lapack.dgeqrf(A)
    assert info == 0
    assert np.array_equal(qr, F) and np.array_equal(tau_ref, tau)
    b = qc.integer_rhs(n, n)
    x = qc.pairing_solution(A, b)
    assert np.array_equal(A @ x, b)
    assert np.array_equal(qc.lapack_qr_solve(qr, tau_ref, b), x)


@pytest.mark.parametrize("n,fixed_frac", qc.PAIRING_CASES)
def test_pairing_places_the_pairs_the_kernels_need(n, fixed_frac):
    A, _, tau = qc.pairing(n, n, fixed_frac)
    i, j = np.nonzero(np.triu(A, 1))
    if fixed_frac == 1.0:
        assert len(i) == 0 and not tau.any()
        return
    if fixed_frac == 0.0:
        assert not np.diag(A).any()
    if n >= 2:
        assert (i // 64 == j // 64).any()                 # a pair inside one panel
    if n > 128:
        assert ((i < 64) & (j >= n - 64)).any()           # a reflector from panel 0 into the last 64 rows
    if n > 256:
        assert ((i < 256) & (j >= 256)).any()             # a pair across the first 256-row block boundary


# -------------------------------------------------------------------------------------------- the measures against mpmath
def _mp_measures(A, F, tau, x, b):
    n = A.shape[0]
    with mp.workdps(40):
        u = mp.mpf(2) ** -53
        C = [[mp.mpf(float(A[i, j])) for j in range(n)] for i in range(n)]      # C[i][j]
        V = [[mp.mpf(float(F[i, j])) for j in range(n)] for i in range(n)]
        t = [mp.mpf(float(v)) for v in tau]
        refl = mp.mpf(0)
        for j in range(n):
            if t[j] == 0:
                continue
            v = [mp.mpf(1)] + [V[i][j] for i in range(j + 1, n)]
            refl = max(refl, abs(t[j] * mp.fsum(e * e for e in v) / 2 - 1))
            for c in range(n):
                w = t[j] * mp.fsum(v[i - j] * C[i][c] for i in range(j, n))
                for i in range(j, n):
                    C[i][c] -= v[i - j] * w
        cb = mp.mpf(0)
        for c in range(n):
            num = mp.sqrt(mp.fsum((C[i][c] - (V[i][c] if i <= c else 0)) ** 2 for i in range(n)))
            cb = max(cb, num / mp.sqrt(mp.fsum(mp.mpf(float(A[i, c])) ** 2 for i in range(n))))
        xs = [mp.mpf(float(v)) for v in x]
        r = [mp.mpf(float(b[i])) - mp.fsum(mp.mpf(float(A[i, j])) * xs[j] for j in range(n)) for i in range(n)]
        den = mp.fsum(mp.sqrt(mp.fsum(mp.mpf(float(A[i, j])) ** 2 for i in range(n))) * abs(xs[j]) for j in range(n))
        den += mp.sqrt(mp.fsum(mp.mpf(float(v)) ** 2 for v in b))
        om = mp.sqrt(mp.fsum(e * e for e in r)) / den
        return float(cb / u), float(refl / u), float(om / u)


def test_longdouble_measures_agree_with_mpmath():
    """At n = 65 (two panels on the device).  The longdouble evaluation's own error: each of the n reflector applications and
    each length-n sum adds at most a few 2^-64 relative to the column's scale, 4 n 2^-64 = 0.13 u in all."""
    n, kind = 65, "zero_block"
    A = qc.graded_case(n, kind)
    F, tau = qc.lapack_qr(A)
    _, B = qc.graded_rhs(A, qc.case_seed(n, kind))
    b = B[:, 0]
    x = qc.lapack_qr_solve(F, tau, b)
    bound = 4 * n * 2.0 ** -64 / qc.U
    cb, rd, om = _mp_measures(A, F, tau, x, b)
    assert cb > 1 and rd > 0.5 and om > 0.05          # the measures see LAPACK's rounding: they are not trivially zero
    assert abs(qc.col_backward(A, F, tau, np.arange(n)) - cb) <= bound
    assert abs(qc.reflector_defect(F, tau) - rd) <= bound
    assert abs(qc.omega(A, x, b) - om) <= bound


# ---------------------------------------------------------------------------------- LAPACK on the cases of the GPU tests
@pytest.fixture(scope="module")
def lapack_values():
    cases = qc.ACCURACY_CASES + [(n, "zero_column") for n in qc.ZERO_COLUMN_SIZES]
    return {c: qc.lapack_measures(*c) for c in cases}


def test_lapack_stays_within_an_eighth_of_every_tolerance(lapack_values):
    assert qc.MULTI_RHS_CASE in lapack_values
    for case, (cb, rd, om) in lapack_values.items():
        assert cb <= qc.COL_BACKWARD_TOL / 8, (case, cb)
        assert rd <= qc.REFLECTOR_TOL / 8, (case, rd)
        assert om is None or om <= qc.OMEGA_TOL / 8, (case, om)


def test_tolerances_are_eight_times_the_recorded_maxima(lapack_values):
    """The constants are 8 x the maxima written beside them, and those are not inflated: LAPACK reaches four fifths of
    each here (the maxima move by up to a tenth with the BLAS thread count; the recorded ones are the largest seen)."""
    assert qc.COL_BACKWARD_TOL == 8 * qc.LAPACK_MAX_COL_BACKWARD
    assert qc.REFLECTOR_TOL == 8 * qc.LAPACK_MAX_REFLECTOR
    assert qc.OMEGA_TOL == 8 * qc.LAPACK_MAX_OMEGA
    vals = list(lapack_values.values())
    assert max(v[0] for v in vals) >= 0.8 * qc.LAPACK_MAX_COL_BACKWARD
    assert max(v[1] for v in vals) >= 0.8 * qc.LAPACK_MAX_REFLECTOR
    assert max(v[2] for v in vals if v[2] is not None) >= 0.8 * qc.LAPACK_MAX_OMEGA


def test_zero_columns_stay_exactly_zero_in_dgeqrf():
    for n in qc.ZERO_COLUMN_SIZES:
        A = qc.graded_case(n, "zero_column")
        F, tau = qc.lapack_qr(A)
        ks = qc.zero_columns(n)
        assert ks[0] < 64 <= ks[1] < n and ks[1] % 64 not in (0, 63)
        for k in ks:
            assert not A[:, k].any() and not A[k, :].any() and not F[:, k].any() and tau[k] == 0.0


def test_scaling_cases_stay_inside_the_exact_range():
    """The one-pass dlarfg is exact under 2^k scaling only while no square overflows and none is subnormal."""
    for n in qc.SCALING_SIZES:
        A = qc.graded(n, qc.case_seed(n, "indefinite"), "indefinite", emax=qc.SCALING_EMAX)
        amax, amin = np.abs(A).max(), np.abs(A[A != 0]).min()
        for k in qc.SCALING_SHIFTS:
            assert np.isfinite((amax * 2.0 ** abs(k)) ** 2 * n)
            assert (amin * 2.0 ** -abs(k)) ** 2 >= np.finfo(np.float64).tiny


# --------------------------------------------------------------------------------------------------------- planted defects
def _old_factor_criterion(F, tau, F_ref, tau_ref):
    """tests/test_hip_qr.py::test_factor_matches_lapack_dgeqrf"""
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)  # noqa: E731
    return max(rel(np.triu(F), np.triu(F_ref)), rel(np.tril(F, -1), np.tril(F_ref, -1)), rel(tau, tau_ref)) <= 1e-12


def _old_solve_criterion(A, F, tau, b):
    """tests/test_hip_qr.py::backward_error <= 1e-13 of the solve with this factor (Q^T b from the reflectors, then R)."""
    y = b.copy()
    for j in range(len(b)):
        v = F[j:, j].copy()
        v[0] = 1.0
        y[j:] -= tau[j] * v * (v @ y[j:])
    x = sl.solve_triangular(np.triu(F), y)
    return np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()) <= 1e-13


@pytest.fixture(scope="module")
def planted():
    n, kind = 257, "indefinite"
    A = qc.graded_case(n, kind)
    F, tau = qc.lapack_qr(A)
    _, B = qc.graded_rhs(A, qc.case_seed(n, kind))
    nrm = np.linalg.norm(A, axis=0)
    return A, F, tau, B[:, 0], nrm


def _caught_and_missed(planted, F, tau, measure):
    A, F_ref, tau_ref, b, _ = planted
    cols = np.arange(A.shape[0])
    assert qc.col_backward(A, F_ref, tau_ref, cols) <= qc.COL_BACKWARD_TOL / 8      # the unspoiled factor passes
    assert qc.reflector_defect(F_ref, tau_ref) <= qc.REFLECTOR_TOL / 8
    if measure == "col_backward":
        assert qc.col_backward(A, F, tau, cols) > qc.COL_BACKWARD_TOL
    else:
        assert qc.reflector_defect(F, tau) > qc.REFLECTOR_TOL
    assert _old_factor_criterion(F, tau, F_ref, tau_ref)           # ... and the normwise criteria do not see it
    assert _old_solve_criterion(A, F, tau, b)


def test_planted_wrong_tau_is_caught(planted):
    _, F, tau, _, _ = planted
    tau = tau.copy()
    tau[100] *= 1 + 1e-11
    _caught_and_missed(planted, F, tau, "reflector_defect")


def test_planted_wrong_v_entry_in_the_smallest_column_is_caught(planted):
    """One V entry of the smallest-norm column off by 1e-9 relative: the largest entry of that column whose change the
    Frobenius criterion over the whole of V cannot see (|dv| <= 0.5e-12 ||V||_F)."""
    _, F, tau, _, nrm = planted
    n = F.shape[0]
    j = int(np.argmin(nrm[:n - 64]))            # (a column with a long reflector)
    v = np.abs(F[j + 1:, j])
    hidden = np.where(1e-9 * v <= 0.5e-12 * np.linalg.norm(np.tril(F, -1)), v, 0.0)
    k = j + 1 + int(np.argmax(hidden))
    assert hidden.max() > 0
    F = F.copy()
    F[k, j] *= 1 + 1e-9
    _caught_and_missed(planted, F, tau, "col_backward")


def test_planted_wrong_r_entry_in_the_smallest_column_is_caught(planted):
    A, F, tau, _, nrm = planted
    j = int(np.argmin(nrm))
    F = F.copy()
    F[j // 2, j] += 1e-8 * nrm[j]
    _caught_and_missed(planted, F, tau, "col_backward")


def test_planted_lost_reflector_contribution_is_caught(planted):
    """Column c (the smallest-norm one of the last panel's) misses what reflector p of an earlier panel adds to it: a lost
    term of the trailing update.  R(:, c) is what the later reflectors make of the column without it."""
    A, F, tau, _, nrm = planted
    n = A.shape[0]
    c = 192 + int(np.argmin(nrm[192:256]))
    p = 70
    a = A[:, c].copy()
    for j in range(c):
        if j == p:
            continue
        v = F[j:, j].copy()
        v[0] = 1.0
        a[j:] -= tau[j] * v * (v @ a[j:])
    F = F.copy()
    assert not np.array_equal(F[:c, c], a[:c])
    F[:c, c] = a[:c]
    _caught_and_missed(planted, F, tau, "col_backward")

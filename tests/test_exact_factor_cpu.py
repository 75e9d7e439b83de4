"""The construction of tests/exact_factor.py, pinned on the CPU: its LDL^T factors are exact whatever the blocking and the
summation order, dpotrf's info is k + 1 at a breakdown in column k, LAPACK's Bunch-Kaufman inertia is the Sylvester count,
and the scalar reference of the static-pivot LDL^T returns the exact factors when no pivot breaks down."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack

from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver
from tests.exact_factor import TINY, blocked_ldl, make_exact, scalar_ldl, with_pivot


@pytest.mark.parametrize("n", [5, 63, 65, 130, 300])
@pytest.mark.parametrize("positive", [True, False])
def test_blocked_eliminations_are_bit_exact(n, positive):
    c = make_exact(n, 11 + n, positive=positive)
    Lx = c.L
    rng = np.random.default_rng(n)
    for nb, chunk in ((1, 0), (4, 1), (16, 4), (37, 5), (64, 16), (64, 0)):
        L, d = blocked_ldl(c.A, nb, rng, chunk)
        assert np.array_equal(d, c.d), (n, nb, chunk)
        assert np.array_equal(L, Lx), (n, nb, chunk)


@pytest.mark.parametrize("n", [63, 200])
def test_cholesky_factor_is_exact(n):
    c = make_exact(n, 5 + n)
    F, info = lapack.dpotrf(c.A, lower=1, clean=1)
    assert info == 0
    assert np.array_equal(F, c.L * np.sqrt(c.d)), n


@pytest.mark.parametrize("n", [5, 70, 300])
def test_dpotrf_info_is_the_first_bad_column_plus_one(n):
    base = make_exact(n, 7 * n)
    for k in sorted({0, 1, 3, 4, 15, 16, 63, 64, n // 2, n - 2, n - 1}):
        if k >= n:
            continue
        for v in (-1.0, 0.0, -TINY):
            c = with_pivot(base, k, v)
            _, info = lapack.dpotrf(c.A, lower=1)
            assert info == c.dpotrf_info() == k + 1, (n, k, v, info)
    # two breakdowns in one 4-group: the first one counts
    c = with_pivot(with_pivot(base, 2, -4.0), 0, 0.0)
    assert lapack.dpotrf(c.A, lower=1)[1] == c.dpotrf_info() == 1


def test_with_pivot_equals_a_fresh_construction():
    n = 150
    base = make_exact(n, 3, positive=False)
    for k, v in ((0, -1.0), (17, 0.0), (149, TINY)):
        a = with_pivot(base, k, v)
        b = make_exact(n, 3, {k: v}, positive=False)
        assert np.array_equal(a.A, b.A) and np.array_equal(a.d, b.d), k


@pytest.mark.parametrize("n", [5, 63, 300])
def test_lapack_bunch_kaufman_inertia_is_the_sylvester_count(n):
    for seed in range(3):
        c = make_exact(n, 100 * n + seed, positive=False)
        ref = LapackCPUSolver(np.asfortranarray(np.tril(c.A)), BUNCHKAUFMAN).factorize()
        assert tuple(int(v) for v in ref.inertia()) == c.inertia(), (n, seed)


@pytest.mark.parametrize("n", [5, 63, 65, 300])
def test_scalar_reference_returns_the_exact_factors(n):
    for positive in (True, False):
        c = make_exact(n, 17 * n, positive=positive)
        L, d = scalar_ldl(c.A)
        assert np.array_equal(d, c.d) and np.array_equal(L, c.L), (n, positive)
    # a zero pivot (pivot_tol = 0): recorded 0, its column of L zero, everything else exact
    c = with_pivot(make_exact(n, 19 * n), n // 2, 0.0)
    L, d = scalar_ldl(c.A)
    assert np.array_equal(d, c.d) and np.array_equal(L, c.L)


def test_scalar_reference_tolerance_and_non_finite_rules():
    n = 40
    c = with_pivot(make_exact(n, 23), 9, TINY)
    L, d = scalar_ldl(c.A, pivot_tol=1e-10)
    assert d[9] == 0.0 and np.array_equal(d[:9], c.d[:9])
    assert np.array_equal(L[:, :9], c.L[:, :9])
    # column 9 keeps the Schur complement's column as it is (harmless pivot 1): TINY times the exact multipliers
    assert np.array_equal(L[10:, 9], TINY * c.L[10:, 9])
    assert np.all(d[10:] != 0.0)
    # a NaN below the diagonal: exact before the first affected pivot, zero at every non-finite one, never NaN
    c = make_exact(n, 29)
    A = c.A.copy(order="F")
    A[30, 12] = A[12, 30] = np.nan
    L, d = scalar_ldl(A)
    assert np.all(np.isfinite(d))
    assert np.array_equal(d[:30], c.d[:30]) and np.all(d[30:] == 0.0)
    # a NaN on the diagonal: that pivot recorded 0, its column used as it is, nothing else touched
    A = c.A.copy(order="F")
    A[5, 5] = np.nan
    L, d = scalar_ldl(A)
    assert d[5] == 0.0 and np.all(np.isfinite(d)) and np.array_equal(d[:5], c.d[:5])


def test_lower_csc_holds_every_entry_of_every_edit():
    n = 200
    base = make_exact(n, 31, positive=False)
    pat = base.lower_pattern()
    for k, v in ((0, 0.0), (57, -1.0), (199, TINY)):
        c = with_pivot(base, k, v)
        colptr, rowval, nzval = c.lower_csc(pat)
        D = np.zeros((n, n))
        D[rowval, np.repeat(np.arange(n), np.diff(colptr))] = nzval
        assert np.array_equal(D, np.tril(c.A)), k

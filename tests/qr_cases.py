"""Matrices and measures for the QR solver's exact-answer and columnwise accuracy tests (helper of tests/test_qr_cases_cpu.py
and tests/test_hip_qr_exact.py, not a test module).

pairing: symmetric signed generalised permutation matrices with entries +-2^e.  Their Householder QR is exact in fp64
whatever the blocking and the order of the sums: every sum that dgeqrf or the device forms has at most one nonzero term, every
norm is the square root of one square of a power of two, and every reflector is either the identity (a fixed point i:
x = 0, tau = 0, R(i, i) = A(i, i)) or the exchange of two rows (a pair i < j with value b: alpha = 0, beta = -|b|, tau_i = 1,
v = e_i + sign(b) e_j, which leaves R(i, i) = R(j, j) = -|b|, nothing else in row i, and x = 0, tau_j = 0 in column j).

graded: d S d with S a symmetric Gaussian matrix and d = 2^U{-emax..emax} -- the column scaling of a KKT matrix whose
Sigma = z / s diagonals span many decades.  Householder QR promises a columnwise bound on such a matrix: the backward error
of column j is small relative to ||A_j||, not to ||A||.  col_backward, reflector_defect and omega measure exactly that, in
np.longdouble and in units of u = 2^-53.

The three tolerances are 8 x the largest value LAPACK itself (dgeqrf, dormqr('L','T'), dtrtrs) attains over the cases that
the GPU tests use (`python -m tests.qr_cases` prints the maxima; tests/test_qr_cases_cpu.py asserts LAPACK <= TOL / 8 case by
case).  The factor 8 covers the device's different but fixed orders of summation (up to 16 K-splits, 4-deep MFMA chains, norms
from per-block partial sums); it does not cover a lost term.  No device result enters them."""
import numpy as np
import scipy.linalg as sl

LD = np.longdouble
U = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------- the cases
PAIRING_CASES = ([(n, 0.2) for n in (1, 2, 63, 64, 65, 255, 257, 320, 576, 832)]
                 + [(n, 1.0) for n in (5, 130)] + [(130, 0.0)])
PAIRING_SOURCES_SIZES = (65, 576)          # these also run through the lower-CSC source and a padded device tensor
GRADED_KINDS = ("indefinite", "zero_block", "zero_column")
ACCURACY_CASES = [(n, kind) for kind in ("indefinite", "zero_block") for n in (65, 257, 320, 576, 832)]
ZERO_COLUMN_SIZES = (130, 320)
MULTI_RHS_CASE = (576, "indefinite")
MULTI_RHS_SCALES = (2.0 ** -40, 1.0, 2.0 ** 40)
SCALING_SIZES = (257, 576)
SCALING_EMAX = 20
SCALING_SHIFTS = (-200, -60, 60, 200)

# LAPACK's maxima over ACCURACY_CASES, the zero_column cases (the two factor measures) and the MULTI_RHS_CASE (omega), in
# units of u.  The blocked dgeqrf's sums depend on the BLAS thread count, so each figure is the largest over 1, 2, 4, 8, 16, 32
# and 64 threads, rounded up to two digits: col_backward 8.859 u at (576, indefinite) with any count; reflector_defect 3.963 u
# with 4 threads (3.704 ... 3.787 u otherwise); omega 1.552 u with 1 thread (1.384 u otherwise), both at (65, indefinite).
LAPACK_MAX_COL_BACKWARD = 8.9
LAPACK_MAX_REFLECTOR = 4.0
LAPACK_MAX_OMEGA = 1.6
COL_BACKWARD_TOL = 8 * LAPACK_MAX_COL_BACKWARD
REFLECTOR_TOL = 8 * LAPACK_MAX_REFLECTOR
OMEGA_TOL = 8 * LAPACK_MAX_OMEGA


def case_seed(n, kind):
    return 1000 * GRADED_KINDS.index(kind) + n


# ---------------------------------------------------------------------------------------------------------------- pairing
def pairing(n, seed, fixed_frac):
    """(A, F, tau): the matrix (Fortran order) and dgeqrf's exact output for it.  fixed_frac of the indices (about) are fixed
    points of the involution, the others are paired at random; fixed_frac = 1 is the diagonal family (every tau is 0).  Unless
    fixed_frac = 1, one pair lies inside one 64-column panel; for n > 128 one pair has i < 64 and j >= n - 64, and for n > 256
    one pair has i < 256 <= j."""
    rng = np.random.default_rng(seed)
    free = np.ones(n, dtype=bool)
    pairs = []

    def take(lo, hi):
        k = int(rng.choice(np.flatnonzero(free[lo:hi]))) + lo
        free[k] = False
        return k
    if fixed_frac < 1 and n >= 2:
        if n > 256:
            pairs.append((take(64, 256), take(256, n)))
        if n > 128:
            pairs.append((take(0, 64), take(n - 64, n)))
        p0 = int(rng.choice([p for p in range(0, n, 64) if free[p:p + 64].sum() >= 2]))
        i, j = sorted((take(p0, min(p0 + 64, n)), take(p0, min(p0 + 64, n))))
        pairs.append((i, j))
    rest = rng.permutation(np.flatnonzero(free))
    nfix = int(round(fixed_frac * len(rest)))
    nfix += (len(rest) - nfix) % 2
    for a, b in rest[nfix:].reshape(-1, 2):
        pairs.append((int(min(a, b)), int(max(a, b))))
    fixed = set(int(k) for k in rest[:nfix])
    val = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-20, 21, n)
    A = np.zeros((n, n), order="F")
    F = np.zeros((n, n), order="F")
    tau = np.zeros(n)
    for i in fixed:
        A[i, i] = F[i, i] = val[i]
    for i, j in pairs:
        assert i < j
        A[i, j] = A[j, i] = val[i]
        F[i, i] = F[j, j] = -abs(val[i])
        F[j, i] = np.sign(val[i])
        tau[i] = 1.0
    assert len(fixed) + 2 * len(pairs) == n and np.count_nonzero(A) == n
    return A, F, tau


def pairing_solution(A, b):
    """The exact x of A x = b for a pairing matrix: x[j] = b[i] / A[i, j] (a division by a power of two)."""
    i, j = np.nonzero(A)
    x = np.zeros(A.shape[0])
    x[j] = b[i] / A[i, j]
    return x


def integer_rhs(n, seed):
    return np.random.default_rng(seed).integers(-9, 10, n).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------- graded
def zero_columns(n):
    """The exactly zero rows / columns of graded(n, ., 'zero_column'): the middle of panel 0 and the middle of a later panel."""
    return (31, 64 * ((n - 1) // 64 - 1) + 33)


def graded(n, seed, kind, emax=30):
    """d S d (Fortran order; an exact scaling of S): S symmetric Gaussian, d = 2^U{-emax..emax}.  'zero_block': the leading
    n/3 x n/3 block is zero (KKT-like); 'zero_column': rows and columns zero_columns(n) are exactly zero."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    S = (G + G.T) / 2
    d = 2.0 ** rng.integers(-emax, emax + 1, n)
    if kind == "zero_block":
        S[:n // 3, :n // 3] = 0.0
    elif kind == "zero_column":
        for k in zero_columns(n):
            S[k, :] = 0.0
            S[:, k] = 0.0
    else:
        assert kind == "indefinite"
    return np.asfortranarray(d[:, None] * S * d[None, :])


def graded_case(n, kind):
    return graded(n, case_seed(n, kind), kind)


def graded_rhs(A, seed, scales=(1.0,)):
    """(X_true, B): B[:, k] = scales[k] * (A @ X_true[:, k]), Fortran order.  (B is rounded; it is the right-hand side given
    to the solver and to omega alike.)"""
    rng = np.random.default_rng(seed + 7919)
    X = rng.standard_normal((A.shape[0], len(scales)))
    return X, np.asfortranarray((A @ X) * np.asarray(scales)[None, :])


def check_columns(A, seed):
    """The columns col_backward looks at: all of nonzero norm up to n = 320 (the longdouble product is too slow beyond), else
    the 16 of smallest and the 16 of largest nonzero norm and 32 more drawn with the seed."""
    nrm = np.linalg.norm(A, axis=0)
    nz = np.flatnonzero(nrm > 0)
    if A.shape[0] <= 320:
        return nz
    order = nz[np.argsort(nrm[nz], kind="stable")]
    mid = np.random.default_rng(seed).choice(order[16:-16], 32, replace=False)
    return np.sort(np.concatenate([order[:16], order[-16:], mid]))


# --------------------------------------------------------------------------------------------------------------- measures
def _assert_longdouble():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not wider than fp64 here"


def col_backward(A, F, tau, cols):
    """max over cols of ||(Q^T A - R)_j||_2 / ||A_j||_2 in units of u, with Q^T = H_n ... H_1 built from the V and tau of F."""
    _assert_longdouble()
    n = A.shape[0]
    cols = np.asarray(cols)
    C = A[:, cols].astype(LD)
    Fl, tl = F.astype(LD), tau.astype(LD)
    for j in range(n):
        if tl[j] == 0:
            continue
        v = Fl[j:, j].copy()
        v[0] = 1
        C[j:] -= np.outer(tl[j] * v, v @ C[j:])
    E = C - np.triu(Fl)[:, cols]
    num = np.sqrt((E * E).sum(0))
    Al = A[:, cols].astype(LD)
    den = np.sqrt((Al * Al).sum(0))
    return float((num / den).max() / U)


def reflector_defect(F, tau):
    """max over tau_j != 0 of |tau_j ||v_j||^2 / 2 - 1| in units of u (H_j is orthogonal iff tau_j ||v_j||^2 = 2)."""
    _assert_longdouble()
    Fl, tl = F.astype(LD), tau.astype(LD)
    worst = LD(0)
    for j in np.flatnonzero(tau != 0):
        x = Fl[j + 1:, j]
        worst = max(worst, abs(tl[j] * (1 + x @ x) / 2 - 1))
    return float(worst / U)


def omega(A, x, b):
    """||b - A x||_2 / (sum_j ||A_j||_2 |x_j| + ||b||_2) in units of u: the residual against the columnwise scale of A x."""
    _assert_longdouble()
    Al, xl, bl = A.astype(LD), x.astype(LD), b.astype(LD)
    r = bl - Al @ xl
    den = np.sqrt((Al * Al).sum(0)) @ np.abs(xl) + np.sqrt(bl @ bl)
    return float(np.sqrt(r @ r) / den / U)


# ----------------------------------------------------------------------------------------------------------------- LAPACK
def lapack_qr(A):
    F, tau, _, info = sl.lapack.dgeqrf(A)
    assert info == 0
    return F, tau


def lapack_qr_solve(F, tau, b):
    """dormqr('L','T') then dtrtrs('U','N','N'), as the reference's solve_qr! does."""
    c = np.asfortranarray(b.reshape(len(b), -1).copy())
    lwork = max(1, int(sl.lapack.dormqr("L", "T", F, tau, c, -1)[1][0]))
    y, _, info = sl.lapack.dormqr("L", "T", F, tau, c, lwork)
    assert info == 0
    x, info = sl.lapack.dtrtrs(F, y, lower=0, trans=0, unitdiag=0)
    assert info == 0
    return x.reshape(b.shape)


def lapack_measures(n, kind):
    """LAPACK's (col_backward, reflector_defect, omega) on one graded case; omega is None for the singular zero_column kind and
    the largest of the three columns for the MULTI_RHS_CASE."""
    seed = case_seed(n, kind)
    A = graded_case(n, kind)
    F, tau = lapack_qr(A)
    cb = col_backward(A, F, tau, check_columns(A, seed))
    rd = reflector_defect(F, tau)
    if kind == "zero_column":
        return cb, rd, None
    scales = MULTI_RHS_SCALES if (n, kind) == MULTI_RHS_CASE else (1.0,)
    _, B = graded_rhs(A, seed, scales)
    X = lapack_qr_solve(F, tau, B)
    return cb, rd, max(omega(A, X[:, k], B[:, k]) for k in range(len(scales)))


if __name__ == "__main__":
    rows = [(n, kind) + lapack_measures(n, kind) for n, kind in ACCURACY_CASES + [(n, "zero_column") for n in ZERO_COLUMN_SIZES]]
    for r in rows:
        print(r)
    print("maxima (u): col_backward %.3f  reflector_defect %.3f  omega %.3f"
          % (max(r[2] for r in rows), max(r[3] for r in rows), max(r[4] for r in rows if r[4] is not None)))

"""Matrices and measures of the EVD tests (tests/test_evd_cpu.py, tests/test_hip_evd.py): symmetric matrices of five kinds, a
family of diagonal matrices whose eigendecomposition is exact, LAPACK's own scaled test ratios of an eigendecomposition, and a
numpy model of the two-sided cyclic block Jacobi that csrc/evd.hip implements (documentation of the algorithm; no test depends
on it)."""
import numpy as np
import scipy.linalg as sl

EPS = np.finfo(float).eps
KINDS = ["spd", "indefinite", "zero_block", "kkt4", "kkt8"]
SIZES = [64, 100, 257, 1000, 2100]
DIAG_SIZES = [5, 63, 64, 65, 300, 1000, 2100]
# An inertia comparison means something only if no eigenvalue sits at rounding level: every case must have dsyevd's
# min |lambda| >= SEPARATION * |A|_2 (tests/test_evd_cpu.py asserts it for each of them; 1e-9 >> N eps).
SEPARATION = 1e-9
# (Hessian diagonal spread, dual block spread) of the two KKT kinds.  |A|_2 is about 10^spread; the smallest |lambda| is the
# smaller of ~0.09 (the Wishart part of H on the directions whose diagonal term is small) and the smallest entry of D (a row
# of the sparse J may be empty).  The spreads 10^+-8 / 10^[-8, 0] of the first model runs gave min |lambda| / |A|_2 between
# 2.6e-11 and 3e-9, below SEPARATION; these are narrowed until every case clears it with a margin (condition up to ~1e9).
KKT_SPREAD = {"kkt4": (4, 4), "kkt8": (7, 1.5)}


def kkt(N, seed, spread=8, dual_spread=8):
    """[[H, J'], [J, -D]]: H = R R' / n + diag(10^U(-spread, spread)), J sparse (5 %), D = diag(10^U(-dual_spread, 0))."""
    rng = np.random.default_rng(seed)
    n = int(N * 0.7)
    m = N - n
    R = rng.standard_normal((n, n))
    H = R @ R.T / n + np.diag(10.0 ** rng.uniform(-spread, spread, n))
    J = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.05)
    K = np.zeros((N, N))
    K[:n, :n] = H
    K[n:, :n] = J
    K[:n, n:] = J.T
    K[n:, n:] = -np.diag(10.0 ** rng.uniform(-dual_spread, 0, m))
    return K


def sym_matrix(N, kind, seed=None):
    """The case (kind, N); the seed defaults to N."""
    seed = N if seed is None else seed
    if kind in KKT_SPREAD:
        return np.asfortranarray(kkt(N, seed, *KKT_SPREAD[kind]))
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, N))
    if kind == "spd":
        A = G @ G.T / N + np.eye(N)
    else:
        A = (G + G.T) / 2
        if kind == "zero_block":   # a zero leading diagonal block (KKT-like)
            A[: N // 3, : N // 3] = 0.0
    return np.asfortranarray(A)


def diag_family(N, seed=None):
    """A diagonal matrix in random order: powers of two with random signs and one exact zero.  Its eigenvalues are its sorted
    diagonal and its eigenvectors columns of the identity, without any rounding."""
    rng = np.random.default_rng(1000 + N if seed is None else seed)
    d = rng.choice([-1.0, 1.0], N) * 2.0 ** rng.integers(-20, 21, N)
    d[rng.integers(0, N)] = 0.0
    return np.asfortranarray(np.diag(d)), d


def lower_with_garbage(A, seed=7):
    """'L' storage: the strict upper triangle may hold anything."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.tril(A) + np.triu(rng.standard_normal(A.shape), 1))


def dsyevd(A):
    lam, Q, info = sl.lapack.dsyevd(np.array(A, order="F"), compute_v=1, lower=1)
    assert info == 0
    return lam, Q


def ratios(A, lam, Q):
    """LAPACK's test ratios of an eigendecomposition (ddrvst): |A Q - Q L|_1 / (N eps |A|_1) and |Q' Q - I|_1 / (N eps)."""
    N = A.shape[0]
    n1 = lambda M: np.abs(M).sum(0).max()  # noqa: E731
    res = n1(A @ Q - Q * lam) / (N * EPS * max(n1(A), np.finfo(float).tiny))
    orth = n1(Q.T @ Q - np.eye(N)) / (N * EPS)
    return res, orth


def eigenvalue_ratio(lam, lam_ref):
    N = len(lam)
    return np.abs(lam - lam_ref).max() / (N * EPS * max(np.abs(lam_ref).max(), np.finfo(float).tiny))


def backward_error(A, x, b):
    return np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())


def is_permutation(Q):
    return bool(np.isin(Q, (0.0, 1.0)).all() and (Q.sum(0) == 1).all() and (Q.sum(1) == 1).all())


def block_jacobi(A, b=32, cap=30):
    """The algorithm of csrc/evd.hip on the host, for N a multiple of 2 b (the device pads): round-robin rounds of disjoint
    block pairs, each pivot block diagonalized completely, its eigenvector matrix ordered to stay near the identity; stop at
    off(A) <= N eps |A|_F.  Returns (lambda ascending, Q, sweeps)."""
    N = A.shape[0]
    nb = N // b
    A = A.copy()
    V = np.eye(N)
    nrm = np.linalg.norm(A)
    for sweep in range(cap):
        if np.linalg.norm(A - np.diag(np.diag(A))) <= N * EPS * nrm:
            break
        order = list(range(nb))
        for _ in range(nb - 1):
            for i in range(nb // 2):
                p, q = sorted((order[i], order[nb - 1 - i]))
                ii = np.r_[p * b:(p + 1) * b, q * b:(q + 1) * b]
                S = A[np.ix_(ii, ii)]
                _, R = np.linalg.eigh((S + S.T) / 2)
                R = R[:, np.argsort(np.argmax(np.abs(R), axis=0), kind="stable")]
                A[:, ii] = A[:, ii] @ R
                A[ii, :] = R.T @ A[ii, :]
                V[:, ii] = V[:, ii] @ R
            order = [order[0], order[-1]] + order[1:-1]
    lam = np.diag(A).copy()
    o = np.argsort(lam, kind="stable")
    return lam[o], V[:, o], sweep

"""Shared pieces of the compact L-BFGS tests (tests/test_compact_lbfgs_cpu.py, tests/test_hip_compact_lbfgs.py): secant pairs
with positive curvature, the dense BFGS recursion in `np.longdouble`, and the longdouble compact representation."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def random_pairs(n, k, seed):
    """k pairs (s_i, y_i = A s_i) with a fixed symmetric positive definite A: s'y > 0, and the pairs are those of one function."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, n))
    A = Q @ Q.T / n + np.eye(n)
    S = rng.standard_normal((n, k))
    return S, A @ S


def ld_bfgs(sigma, S, Y):
    """The dense BFGS recursion started from sigma I over the columns of S, Y (oldest first), in longdouble:
    B <- B - (B s)(B s)' / s'B s + y y' / y's."""
    n = S.shape[0]
    B = LD(sigma) * np.eye(n, dtype=LD)
    for i in range(S.shape[1]):
        s, y = S[:, i].astype(LD), Y[:, i].astype(LD)
        bs = B @ s
        B = B - np.outer(bs, bs) / (s @ bs) + np.outer(y, y) / (y @ s)
    return B


def ld_uv(sigma, S, Y):
    """U, V of the compact representation (quasi_newton.jl:388-420) in longdouble, from float64 S, Y and sigma."""
    S, Y = S.astype(LD), Y.astype(LD)
    k = S.shape[1]
    SY = S.T @ Y
    D = np.diag(SY).copy()
    Lk = np.tril(SY, -1)
    M = LD(sigma) * (S.T @ S) + (Lk / D[None, :]) @ Lk.T
    J = np.zeros((k, k), dtype=LD)            # Cholesky in longdouble (numpy's runs in float64)
    for j in range(k):
        J[j, j] = np.sqrt(M[j, j] - J[j, :j] @ J[j, :j])
        for i in range(j + 1, k):
            J[i, j] = (M[i, j] - J[i, :j] @ J[j, :j]) / J[j, j]
    V = Y / np.sqrt(D)[None, :]
    W = LD(sigma) * S + (Y / D[None, :]) @ Lk.T
    Ut = np.zeros((k, S.shape[0]), dtype=LD)  # U' = J^-1 W'
    for i in range(k):
        Ut[i] = (W[:, i] - Ut[:i].T @ J[i, :i]) / J[i, i]
    return Ut.T, V


def compact_dense(sigma, U, V):
    """sigma I - U U' + V V' in longdouble from whatever precision U, V have."""
    U, V = np.asarray(U).astype(LD), np.asarray(V).astype(LD)
    return LD(sigma) * np.eye(U.shape[0], dtype=LD) - U @ U.T + V @ V.T


def scripted_sequence(n, seed=3):
    """10 pairs for history 3: four performed (growth, then the shift), one isolated skip (the history stays), two performed,
    two skips in a row (`skipped_iter` is cleared by a reset only, as in the reference: the first of the two is the second skip
    since the start and empties the memory, the second one starts the next count), regrowth.  Returns [(s, y, performed)]."""
    S, Y = random_pairs(n, 10, seed)
    plan = [True, True, True, True, False, True, True, False, False, True]
    out = []
    for i, ok in enumerate(plan):
        out.append((S[:, i].copy(), (Y[:, i] if ok else -Y[:, i]).copy(), ok))
    return out

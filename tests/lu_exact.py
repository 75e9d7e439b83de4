"""Symmetric KKT matrices whose LU factorization with partial pivoting is exact in fp64 (helper of tests/test_lu_cpu.py and
tests/test_hip_lu.py, not a test module).

K = [[H, J^T], [J, 0]], symmetrically permuted at random: H is diagonal with entries +-2^-e, e in [4, 8]; J has one entry +-1
or +-2 per row, in distinct columns.  Every pivot of the elimination is then a unique maximum of its column (a J entry beats
every H entry), every multiplier is dyadic and every Schur complement entry a short dyadic sum, so any order of the
arithmetic -- LAPACK's, a Fraction elimination's, the device's blocked one -- gives the same bits, row interchanges included."""
from fractions import Fraction

import numpy as np


def exact_kkt(N, seed, zero_j_row=None):
    """The N x N matrix (Fortran order) and its size split (n, m); m = N // 3 constraints.  zero_j_row: that constraint's J
    entry is zero, which makes K singular (a zero row and column)."""
    rng = np.random.default_rng(seed)
    m = N // 3
    n = N - m
    H = rng.choice([-1.0, 1.0], n) * 2.0 ** -rng.integers(4, 9, n)
    cols = rng.permutation(n)[:m]
    vals = rng.choice([-2.0, -1.0, 1.0, 2.0], m)
    if zero_j_row is not None:
        vals[zero_j_row] = 0.0
    K = np.zeros((N, N))
    K[np.arange(n), np.arange(n)] = H
    K[n + np.arange(m), cols] = vals
    K[cols, n + np.arange(m)] = vals
    p = rng.permutation(N)
    return np.asfortranarray(K[np.ix_(p, p)]), (n, m)


def fraction_getrf(A):
    """dgetf2 in exact rational arithmetic: (LU as Fractions, ipiv 1-based, info).  idamax's pivot: the first largest |a|."""
    N = A.shape[0]
    M = [[Fraction(float(A[i, j])) for j in range(N)] for i in range(N)]
    ipiv = np.zeros(N, dtype=np.int64)
    info = 0
    for j in range(N):
        p = max(range(j, N), key=lambda i: (abs(M[i][j]), -i))
        ipiv[j] = p + 1
        if M[p][j] != 0:
            M[j], M[p] = M[p], M[j]
            for i in range(j + 1, N):
                M[i][j] /= M[j][j]
        elif info == 0:
            info = j + 1
        for i in range(j + 1, N):
            if M[i][j] != 0:
                for k in range(j + 1, N):
                    M[i][k] -= M[i][j] * M[j][k]
    return M, ipiv, info


def fractions_to_float(M):
    """Fraction matrix -> float64 array; raises if an entry is not representable exactly."""
    N = len(M)
    out = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            f = float(M[i][j])
            if Fraction(f) != M[i][j]:
                raise ValueError(f"entry ({i}, {j}) = {M[i][j]} is not exact in fp64")
            out[i, j] = f
    return np.asfortranarray(out)

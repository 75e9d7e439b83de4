"""Matrices whose LDL^T factors are exact in fp64 whatever the blocking and summation order, and a plain scalar
reference of the static-pivot LDL^T (helper module of the pivot-breakdown tests; not collected by pytest).

A = (I + N) D (I + N)^T with the columns split at random into sources S and targets T, N nonzero only at (i, j) with
i in T, j in S, j < i (so N^2 = 0 and inv(I + N) = I - N, on every diagonal block as well), entries of N in
{+-1, +-1/2, +-1/4} (about six per target row, plus one in the first source column, which makes the T x T block dense) and
d_k = +-4^e, e in [-2, 3].  Every partial Schur complement and every multiplier is a short sum of dyadic numbers, so the
static-pivot LDL^T returns exactly L = I + N and D = diag(d) whatever its blocking, and Cholesky L sqrt(D).

A breakdown at column k is an edit of d_k: negative (rejection / failed Cholesky: dpotrf info = k + 1), 0 (singular;
column k of L is then zero), 4^-20 (a pivot below pivot_tol).  The inertia is the count of the signs of d (Sylvester)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

TINY = 4.0 ** -20      # a pivot below pivot_tol = 1e-10 (and above 0)
_NVALS = np.array([1.0, -1.0, 0.5, -0.5, 0.25, -0.25])


@dataclass
class ExactCase:
    n: int
    Nmat: sp.csc_matrix   # strictly lower, nonzero at (target row, source column) only
    d: np.ndarray         # the pivots, breakdowns applied
    A: np.ndarray         # dense symmetric, column-major

    @property
    def L(self):
        """The exact unit lower factor (column k zero below the diagonal where d_k = 0)."""
        Lm = self.Nmat.toarray()
        Lm[:, self.d == 0.0] = 0.0
        return np.asfortranarray(Lm + np.eye(self.n))

    def lower_pattern(self):
        """(colptr, rowval) of the structural lower triangle of A (that of |I + N| |I + N|^T: no cancellation, the same for
        every edit of d), 0-based, sorted rows."""
        M = abs(sp.identity(self.n, format="csc") + self.Nmat)
        P = sp.csc_matrix(sp.tril(M @ M.T))
        P.sort_indices()
        return P.indptr.astype(np.int32), P.indices.astype(np.int32)

    def lower_csc(self, pattern=None):
        """(colptr, rowval, nzval) of tril(A) on the structural pattern (explicit zeros kept), 0-based."""
        colptr, rowval = pattern if pattern is not None else self.lower_pattern()
        cols = np.repeat(np.arange(self.n), np.diff(colptr))
        return colptr, rowval, np.ascontiguousarray(self.A[rowval, cols])

    def inertia(self):
        """Sylvester: the signs of d (a non-finite entry of A voids this)."""
        return (int(np.sum(self.d > 0)), int(np.sum(self.d == 0)), int(np.sum(self.d < 0)))

    def dpotrf_info(self):
        """1-based column of the first pivot that is not positive, 0 if none (the info of LAPACK's dpotrf)."""
        bad = np.flatnonzero(~(self.d > 0))
        return int(bad[0]) + 1 if len(bad) else 0


def draw_factors(n: int, seed: int, breakdowns: dict | None = None, positive: bool = True, per_row: int = 6,
                 exponents: tuple = (-2, 3)):
    """(N sparse, d) of make_exact, without the dense A (orders at which forming it on the host is too slow)."""
    rng = np.random.default_rng(seed)
    src = rng.random(n) < 0.5
    src[0] = True
    srcs = np.flatnonzero(src)
    s0 = int(srcs[0])
    rows, cols, vals = [], [], []
    for i in np.flatnonzero(~src):
        below = srcs[srcs < i]
        if len(below) == 0:
            continue
        pick = rng.choice(below, size=min(per_row, len(below)), replace=False)
        pick = np.unique(np.concatenate((pick, [s0])))
        rows.append(np.full(len(pick), i))
        cols.append(pick)
        vals.append(rng.choice(_NVALS, size=len(pick)))
    if rows:
        Nmat = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    else:
        Nmat = sp.csc_matrix((n, n))
    d = 4.0 ** rng.integers(exponents[0], exponents[1] + 1, size=n)
    if not positive:
        d *= rng.choice([-1.0, 1.0], size=n)
    for k, v in (breakdowns or {}).items():
        d[k] = v
    return Nmat, d


def make_exact(n: int, seed: int, breakdowns: dict | None = None, positive: bool = True, per_row: int = 6,
               exponents: tuple = (-2, 3)) -> ExactCase:
    """`breakdowns`: {column: new d_k}.  `positive`: every other pivot > 0 (else random signs).  `exponents`: the range
    (inclusive) of e in |d_k| = 4^e."""
    Nmat, d = draw_factors(n, seed, breakdowns, positive, per_row, exponents)
    M = sp.identity(n, format="csc") + Nmat
    A = (M @ sp.diags(d) @ M.T).toarray()
    return ExactCase(n, Nmat, d, np.asfortranarray(A))


def with_pivot(case: ExactCase, k: int, value: float) -> ExactCase:
    """The same case with d_k replaced: A + (value - d_k) m_k m_k^T (m_k = column k of I + N), exact entry by entry."""
    m = case.Nmat[:, [k]].toarray().ravel()
    m[k] = 1.0
    nz = np.flatnonzero(m)
    A = case.A.copy(order="F")
    A[np.ix_(nz, nz)] += (value - case.d[k]) * np.outer(m[nz], m[nz])
    d = case.d.copy()
    d[k] = value
    return ExactCase(case.n, case.Nmat, d, A)


def blocked_ldl(A: np.ndarray, nb: int, rng: np.random.Generator | None = None, chunk: int = 0):
    """Right-looking blocked LDL^T without pivoting (unblocked inside a block of `nb` columns; the trailing update of every
    block is summed over column chunks of `chunk` in random order when `rng` is given).  Returns (L, d)."""
    n = A.shape[0]
    S = np.array(A, dtype=np.float64)
    L = np.eye(n)
    d = np.zeros(n)
    for j0 in range(0, n, nb):
        j1 = min(n, j0 + nb)
        for k in range(j0, j1):   # the block column: unblocked
            d[k] = S[k, k]
            c = S[k + 1:, k].copy()
            L[k + 1:, k] = c / d[k]
            S[k + 1:j1, k + 1:j1] -= np.outer(L[k + 1:j1, k], c[:j1 - k - 1])
            S[j1:, k + 1:j1] -= np.outer(L[j1:, k], c[:j1 - k - 1])
        if j1 < n:
            W = L[j1:, j0:j1] * d[j0:j1]              # V = L D of the block column
            ks = list(range(j0, j1, chunk or (j1 - j0)))
            if rng is not None:
                rng.shuffle(ks)
            for c0 in ks:
                c1 = min(j1, c0 + (chunk or (j1 - j0)))
                S[j1:, j1:] -= L[j1:, c0:c1] @ W[:, c0 - j0:c1 - j0].T
    return L, d


def scalar_ldl(A: np.ndarray, pivot_tol: float = 0.0):
    """Plain scalar reference of the static-pivot LDL^T of the HIP leaf (factor_piv4_vals, LDL^T branch): unblocked,
    right-looking, on the lower triangle of A.  A pivot with |d| <= pivot_tol or a non-finite pivot is recorded as 0 and the
    harmless pivot 1 is used in its place: its column of L is the column of the Schur complement as it is (V = L D = that
    column), and the elimination goes on.  Returns (L unit lower, d recorded)."""
    n = A.shape[0]
    assert n <= 700, "the scalar reference is meant for small orders"
    S = np.tril(np.array(A, dtype=np.float64))
    L = np.eye(n)
    d = np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(n):
            p = S[k, k]
            zero = not (abs(p) > pivot_tol) or not (abs(p) <= np.finfo(np.float64).max)
            s = 1.0 if zero else 1.0 / p
            d[k] = 0.0 if zero else p
            c = S[k + 1:, k].copy()            # V = L D on column k
            x = c * s                          # L
            L[k + 1:, k] = x
            # lower triangle of the trailing block: S[r, q] -= x_r c_q (r >= q > k)
            S[k + 1:, k + 1:] -= np.tril(np.outer(x, c))
    return L, d

"""Linear systems whose solve! has one right answer in fp64 whatever the blocking, the summation order and the fusing of products
(helper module of the exact-answer tests of the static-pivot tier's solves; not collected by pytest).

A = (I + N) D (I + N)^T is a matrix of tests/exact_factor.py (N^2 = 0, entries of N in {+-1, +-1/2, +-1/4}, d_k = +-4^e): its
LDL^T is L = I + N, D = diag(d) exactly, its Cholesky factor (I + N) sqrt(D), inv(L_kk) = I - N_kk on every diagonal block of
every size, every product N_ab N_bc an inverse kernel forms is zero term by term (N_ik != 0 makes k a source column, N_kj != 0 a
target row), and the 512-row off-diagonal block -inv(L_22) L_21 inv(L_11) is -N_21.  The solution x* has integer entries in
[-8, 8] times {1, 1/2, 1/4}.  Then b = A x*, the forward sweep, the D^-1 scaling and the backward sweep add and multiply dyadic
numbers of a common granule (2^-10 or coarser) whose partial sums stay far below 2^53 granules (`bit_budget`): no operation
rounds, so every grouping of the sums returns x* bit for bit.

Scaling A -> S A S, b -> S b with S = diag(2^k_i) multiplies row i of every one of these sums by the one power of two 2^k_i
(L becomes S L S^-1, D becomes S D S; for Cholesky L = S (I + N) sqrt(D) with sqrt(4^e) = 2^e exact): still exact, and the
answer is S^-1 x*, whose entries span `scale_bits` binary orders of magnitude -- no norm-wise check sees the small ones."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from tests.exact_factor import draw_factors

GRANULE = 2.0 ** -10     # of every product the sweeps form: N (2^-2) d (4^-2) N (2^-2) x* (2^-2); the other sums are coarser
ULP1 = 1.0 + 2.0 ** -52  # the factor of a one-ulp error in a product


@dataclass
class SolveCase:
    n: int
    positive: bool        # d > 0 (CHOLESKY) or mixed signs (LDL)
    Nmat: sp.csc_matrix   # strictly lower, N^2 = 0
    d: np.ndarray         # the pivots of the unscaled matrix
    k: np.ndarray         # the scaling's exponents: S = diag(2^k)
    xstar: np.ndarray     # the solution of the unscaled system
    A: np.ndarray | None  # S A S dense, column-major (None: the order is too large to form it on the host -- device_system)

    @property
    def s(self):
        return np.ldexp(1.0, self.k)

    @property
    def x(self):
        """The solution of the scaled system: S^-1 x*."""
        return np.ldexp(self.xstar, -self.k)

    @property
    def b(self):
        """S A x*, from the sparse factors (every partial sum is exact: test_solve_exact_cpu.py checks it against longdouble)."""
        M = sp.identity(self.n, format="csr") + self.Nmat.tocsr()
        return np.ldexp(M @ (self.d * (M.T @ self.xstar)), self.k)

    def inertia(self):
        return (int(np.sum(self.d > 0)), 0, int(np.sum(self.d < 0)))

    def factor(self):
        """(L dense, dinv): the exact factor of S A S -- LDL^T: L = S (I + N) S^-1 (unit diagonal), dinv = 1 / (S D S);
        Cholesky (`positive`): L = S (I + N) sqrt(D), dinv None."""
        M = sp.identity(self.n, format="csc") + self.Nmat
        if self.positive:
            L = sp.diags(self.s) @ M @ sp.diags(np.sqrt(self.d))
            return np.asfortranarray(L.toarray()), None
        L = sp.diags(self.s) @ M @ sp.diags(1.0 / self.s)
        return np.asfortranarray(L.toarray()), 1.0 / (self.d * self.s * self.s)


def solve_case(n: int, seed: int, positive: bool, scale_bits: int = 0, dense: bool = True, per_row: int = 6) -> SolveCase:
    """The case of order n: A (scaled), b, x (properties), the inertia and the scaling S = diag(2^k), k_i uniform in
    [0, scale_bits].  `dense=False` leaves A out (the sparse factors are all `device_system` and `bit_budget` need)."""
    Nmat, d = draw_factors(n, seed, positive=positive, per_row=per_row)
    rng = np.random.default_rng([seed, 77])
    xstar = rng.integers(-8, 9, size=n) * rng.choice([1.0, 0.5, 0.25], size=n)
    k = rng.integers(0, scale_bits + 1, size=n) if scale_bits else np.zeros(n, dtype=np.int64)
    A = None
    if dense:
        M = sp.diags(np.ldexp(1.0, k)) @ (sp.identity(n, format="csc") + Nmat)
        A = np.asfortranarray((M @ sp.diags(d) @ M.T).toarray())
    return SolveCase(n, positive, Nmat, d, k, xstar, A)


def device_system(case: SolveCase, dev):
    """(A, b) of the scaled system as torch tensors on `dev`, formed there from the sparse factors: M = S (I + N) dense,
    A = (M d) M^T, b = A (S^-1 x*).  Dyadic data: exact in any summation order (entry (i, j) of every partial sum of A is scaled
    by the one power of two s_i s_j, row i of b by s_i), so nothing of order n^2 crosses the bus."""
    import torch
    n = case.n
    C = case.Nmat.tocoo()
    s = torch.from_numpy(case.s).to(dev)
    rows, cols = torch.from_numpy(C.row.astype(np.int64)).to(dev), torch.from_numpy(C.col.astype(np.int64)).to(dev)
    M = torch.zeros((n, n), dtype=torch.float64, device=dev)
    M[rows, cols] = s[rows] * torch.from_numpy(C.data).to(dev)
    M.diagonal().copy_(s)
    A = (M * torch.from_numpy(case.d).to(dev)) @ M.T
    b = A @ torch.from_numpy(case.x).to(dev)
    return A, b


def bit_budget(case: SolveCase) -> int:
    """An a-priori bound on the significant bits of any partial sum of forming A, of b = A x*, of the two sweeps (explicit block
    inverses included) and of the D^-1 scaling, from the sparse factors alone: the sum of the magnitudes of the terms of a row
    over the granule (the scaling multiplies both by the same power of two, so it does not enter).  With |M| = |I + N|:
      entries of A           |M| |d| |M|^T <= max_i (|M| |d|)_i            (|M_jk| <= 1)
      b and its partial sums |A| |x*|      <= u = |M| (|d| (|M|^T |x*|))
      forward right-hand side b - L y      <= w = u + |N| |y|,  |y| <= |d| (|M|^T |x*|)   (Cholesky: the same terms, row-scaled)
      inverse applied to it  (I - N_kk) w  <= |M| w
      backward               z - N^T x, (I - N_kk)^T of it  <= |M|^T (|M|^T |x*| + |N|^T |x*|)."""
    M = abs(sp.identity(case.n, format="csr") + case.Nmat.tocsr())
    Nabs = abs(case.Nmat.tocsr())
    ax, ad = np.abs(case.xstar), np.abs(case.d)
    z = M.T @ ax
    y = ad * z
    w = M @ y + Nabs @ y
    bound = max((M @ ad).max(), (M @ w).max(), (M.T @ (z + Nabs.T @ ax)).max())
    return int(np.ceil(np.log2(bound / GRANULE))) + 1


MI355X_CUS = 256


def ownership_orders(cus: int):
    """The smallest orders at which a workgroup of a one-launch solve owns more than one block on a device of `cus` CUs
    (csrc/solve_plan.h: blocks are owned round-robin by min(blocks, CUs) workgroups): (n of the 256-column solve with its
    64-row blocks, n of the 512-column solve with its 32-row blocks; the latter moved on by 64 where its padded order would
    leave a 384-row last triangle, which keeps the 256-column steps)."""
    n2, n3 = 64 * (cus + 3) + 5, 32 * (cus + 5) + 3
    if (n3 + 63) // 64 * 64 % 512 == 384:
        n3 += 64
    return n2, n3


# ------------------------------------------------------------------------------------------------ the emulation
def _shuffled(Amat, B, rng, bump=None):
    """Amat @ B summed over column chunks of random sizes of a random permutation of the inner index.  `bump` = (i, k) (B a
    vector): the one product Amat[i, k] B[k] is multiplied by 1 + 2^-52 (its excess joins the chunks as a term of its own)."""
    m = Amat.shape[1]
    acc = np.zeros((Amat.shape[0],) + B.shape[1:])
    if m == 0:
        return acc
    perm = rng.permutation(m)
    cuts = np.sort(rng.choice(np.arange(1, m), size=min(m - 1, max(1, m // 16)), replace=False)) if m > 1 else []
    for p in np.split(perm, cuts):
        acc += Amat[:, p] @ B[p]
    if bump is not None:
        i, k = bump
        p = Amat[i, k] * B[k]
        acc[i] += p * ULP1 - p
    return acc


def _inverse256(L, j0, j1, rng):
    """inv(L[j0:j1, j0:j1]) as linv_tri_kernel forms it from the 64 x 64 inverses: X_qq = inv(L_qq),
    X_bq = -inv(L_bb) sum_{q <= b' < b} L_bb' X_b'q."""
    m = j1 - j0
    X = np.zeros((m, m))
    e = list(range(0, m, 64)) + [m]
    i64 = [sla.solve_triangular(L[j0 + a:j0 + z, j0 + a:j0 + z], np.eye(z - a), lower=True) for a, z in zip(e[:-1], e[1:])]
    for q in range(len(i64)):
        X[e[q]:e[q + 1], e[q]:e[q + 1]] = i64[q]
        for b in range(q + 1, len(i64)):
            S = _shuffled(L[j0 + e[b]:j0 + e[b + 1], j0 + e[q]:j0 + e[b]], X[e[q]:e[b], e[q]:e[q + 1]], rng)
            X[e[b]:e[b + 1], e[q]:e[q + 1]] = -_shuffled(i64[b], S, rng)
    return X


def _block_inverse(L, j0, j1, step, rng):
    """The explicit inverse of the diagonal block of a step: of 256 columns as above; of 512 columns assembled from the two
    256-column ones as inv512_gemm_kernel does, [A^-1 0; -D^-1 (C A^-1)  D^-1]."""
    if step == 256 or j1 - j0 <= 256:
        return _inverse256(L, j0, j1, rng)
    h = j0 + 256
    Ai, Di = _inverse256(L, j0, h, rng), _inverse256(L, h, j1, rng)
    X = np.zeros((j1 - j0, j1 - j0))
    X[:256, :256], X[256:, 256:] = Ai, Di
    X[256:, :256] = -_shuffled(Di, _shuffled(L[h:j1, j0:h], Ai, rng), rng)
    return X


def emulated_solve(case: SolveCase, step: int, rng: np.random.Generator, bump: tuple | None = None):
    """The blocked solve of the library in numpy, on the exact factor: both sweeps right-looking over steps of `step` (256 or
    512) columns, the diagonal blocks applied as products with their explicit inverses, every sum in a shuffled order.
    `bump` = (kind, row): one product of the solve is multiplied by 1 + 2^-52 -- "fwd" / "bwd": the diagonal term of `row` in
    the forward / backward product with the inverse; "dinv": the D^-1 scaling of `row`."""
    assert step in (256, 512)
    n = case.n
    L, dinv = case.factor()
    x = case.b.copy()
    steps = [(j0, min(n, j0 + step)) for j0 in range(0, n, step)]
    inv = [_block_inverse(L, j0, j1, step, rng) for j0, j1 in steps]

    def at(kind, j0, j1):
        return (bump[1] - j0, bump[1] - j0) if bump is not None and bump[0] == kind and j0 <= bump[1] < j1 else None

    for (j0, j1), X in zip(steps, inv):
        y = _shuffled(X, x[j0:j1], rng, at("fwd", j0, j1))
        x[j0:j1] = y
        x[j1:] -= _shuffled(L[j1:, j0:j1], y, rng)
    if dinv is not None:
        x *= dinv
    if bump is not None and bump[0] == "dinv":
        x[bump[1]] *= ULP1
    for (j0, j1), X in zip(steps[::-1], inv[::-1]):
        xk = _shuffled(X.T, x[j0:j1], rng, at("bwd", j0, j1))
        x[j0:j1] = xk
        x[:j0] -= _shuffled(L[j0:j1, :j0].T, xk, rng)
    return x

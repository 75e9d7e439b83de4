"""KKT systems on which the handles' `mul!`, `build_kkt!` and `solve_kkt!` have one right answer in fp64 (helper module of the
exact-answer tests of `mnk_dc_*` / `mnk_sc_*`; not collected by pytest), and their rounded twins.

`exact_kkt_case(kind, n, m, n_eq, seed)` draws a system of general structure -- equality and inequality rows interleaved, primal
entries with both bounds, one bound or none, dense inequality rows -- whose every datum is dyadic:

  * l_diag, u_diag = -2^-k, l_lower, u_lower = 2^j, reg = 2^-k on x and 0 on the slacks;
  * Sigma_s = pr_diag[n + k] = 4^e (a slack with both bounds: two equal halves 2^(2e-1)), du_diag[ineq] = 0 or -3 / Sigma_s, so
    D = Sigma_s / (1 - du Sigma_s) is Sigma_s or Sigma_s / 4 and sqrt(D) (scale_transpose_kernel) is exact;
  * inequality rows of J from {0, 0, 0, +-1, +-1/2, +-2};
  * the condensed matrix is a matrix of tests/exact_factor.py, A = (I + N) diag(d) (I + N)' of order n + n_eq (N^2 = 0, entries
    of N in {+-1, +-1/2, +-1/4}, d = +-4^e, d > 0 on the first n pivots and d < 0 on the last n_eq), drawn by `draw_kkt_factors`:
    the last n_eq rows are targets whose source sets are pairwise disjoint and leave the shared first source column out, so
    A[n:, n:] is diagonal.  Then J[ind_eq] = A[n:, :n], du_diag[ind_eq] = diag(A[n:, n:]) and
    H = A[:n, :n] - diag(pr_diag[:n]) - J_i' D J_i, computed in scaled integers (every term is a multiple of 2^-8);
  * the solution x* over the unreduced vector (x, s, y, z_l, z_u) has integer entries in [-8, 8] times {1, 1/2, 1/4} and
    b = K_u x* with K_u = `unreduced_matrix(case)`, the matrix of `mul!` (reference src/IPM/factorization.jl:289-330,
    src/IPM/kernels.jl:161-204) written out entry by entry.

No operation of `mul!`, of `build_kkt!` or of the condensed `solve_kkt!` chain (reduce_rhs, condensed right-hand side, J' buffer,
the LDL' sweeps with L = I + N, J x, expansion, finish_aug) rounds on these data: every partial sum is a multiple of a common
granule and stays below 2^53 granules (`bit_budget`), so any summation order, tiling or fusing gives the same bits and a single
wrong index shows as a wrong bit.  The augmented system of the `dense` kind has no such factorization (with a dense J the Schur
complement of its y block is no short dyadic sum): its `mul!` and `build_kkt!` are exact, its `solve_kkt!` is checked on rounded
data only.

`scaled_case(case, a, b, c)` is the same system in the units x -> 2^a x, s -> 2^b s, y -> 2^c y (b + c even): H, J, Sigma_s, du
and the bound terms are multiplied by the powers of two that keep the structure (the -I blocks stay -I, Sigma_s stays a power of
four), every row of every sum of the chains is multiplied by one power of two, so exactness holds, and the solution is x* scaled
block by block: x by 2^a, s by 2^b, y by 2^c, the bound multipliers of x entries by 2^(b+c-a), those of slacks by 2^c.

`random_kkt_case` has the same structure with continuous values: H = R R'/n + I and J standard normal (sparse_condensed: half
of J kept and H = R R' + I with about three entries per column of R, so that there is a sparsity pattern), bound slacks (-l_diag,
-u_diag) log-uniform in [1e-2, 1], multipliers in [1e-3, 1], du_diag[ineq] in -[1e-8, 1e-2], du_diag[eq] = 0, reg = 1e-4 on x.
The ranges first planned were bound slacks in [1e-3, 1] and multipliers in [1e-3, 10], narrowed because the acceptance of
`solve_kkt!` (100 x the oracle's residual, floor 1e-10) means something only where the oracle's own residual stays below 1e-12
(tests/test_kkt_exact_cpu.py asserts it): with the wider ranges Sigma reaches 2e4 and the LAPACK oracle's residual at
(130, 97, 14) is between 4e-13 and 4e-12 over a dozen seeds, above 1e-12 for half of them; with the narrower ones (Sigma <= 200)
it is at most 9e-14.  Nothing else was narrowed.

`mul_bound` / `build_bound` are the per-entry error bounds of a correctly rounded fp64 evaluation:
  mul!        |got_i - ref_i| <= (t_i + 6) 2^-53 S_i,  S_i = |alpha| sum_j |K_ij| |x_j| + |beta| |w_i|,  t_i the structural nonzeros
              of row i: t_i + 1 for the summation of t_i rounded products, 5 for the alpha scaling, the beta term and the three
              later kernels that update the entry;
  build_kkt!  |K_ij - ref_ij| <= (ns + 8) 2^-53 (|H_ij| + delta_ij |pr_i| + sum_k |J_ki| D_k |J_kj|): 8 for the two rounded
              factors J sqrt(D) of a term and the additions of H and the diagonal."""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np
import scipy.sparse as sp

from tests.exact_factor import _NVALS
from tests.solve_exact import SolveCase
from tests.solve_exact import bit_budget as _sweep_bits

KINDS = ("dense_condensed", "dense", "sparse_condensed")
SHAPES = {
    "dense_condensed": [(5, 3, 1), (64, 64, 0), (65, 70, 8), (130, 97, 14), (257, 130, 1)],
    "dense": [(5, 3, 1), (65, 70, 8), (130, 97, 14)],
    "sparse_condensed": [(5, 3, 0), (65, 70, 0), (130, 97, 0)],
}
ROUNDED_SHAPES = [(65, 70, 8), (130, 97, 14)]
ALPHA_BETA = ((1.0, 0.0), (-1.0, 1.0), (0.75, -0.5), (0.5, 2.0))
BLOCKS = ("x", "s", "y", "z_l", "z_u")
GBITS = 8          # every datum of an exact case is a multiple of 2^-8
U = 2.0 ** -53
_JVALS = np.array([0.0, 0.0, 0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0])
_XMULT = np.array([1.0, 0.5, 0.25])


@dataclass
class KKTCase:
    kind: str
    n: int
    m: int
    n_eq: int
    ind_eq: np.ndarray
    ind_ineq: np.ndarray
    ind_lb: np.ndarray
    ind_ub: np.ndarray
    reg: np.ndarray
    du_diag: np.ndarray
    l_diag: np.ndarray
    u_diag: np.ndarray
    l_lower: np.ndarray
    u_lower: np.ndarray
    H: np.ndarray                      # symmetric, n x n
    jac: np.ndarray                    # m x n, column-major
    garbage: np.ndarray                # what the strict upper triangle of the dense `hess` holds
    xstar: np.ndarray | None = None
    Nmat: sp.csc_matrix | None = None  # the factors of the condensed matrix (exact cases)
    d: np.ndarray | None = None
    coo: dict = field(default_factory=dict)   # sparse_condensed: jac_I, jac_J, jac, hess_I, hess_J, hess (COO, 0-based)
    base: "KKTCase | None" = None      # scaled_case: the unscaled case
    units: tuple = (0, 0, 0)

    @property
    def ns(self):
        return len(self.ind_ineq)

    @property
    def npr(self):
        return self.n + self.ns

    @property
    def order(self):
        """Of the matrix the handle factors."""
        return self.n + self.ns + self.m if self.kind == "dense" else self.n + self.n_eq

    @property
    def lw(self):
        return self.npr + self.m + len(self.ind_lb) + len(self.ind_ub)

    @property
    def pr_diag(self):
        """`_set_aug_diagonal!` (reference src/IPM/kernels.jl:22-27); exact on the dyadic cases."""
        pr = self.reg.copy()
        np.subtract.at(pr, self.ind_lb, self.l_lower / self.l_diag)
        np.subtract.at(pr, self.ind_ub, self.u_lower / self.u_diag)
        return pr

    @property
    def D(self):
        Ss = self.pr_diag[self.n:]
        return Ss / (1.0 - self.du_diag[self.ind_ineq] * Ss)

    @property
    def hess(self):
        """The dense `hess` field: 'L' storage, the strict upper triangle holds finite garbage."""
        return np.asfortranarray(np.tril(self.H) + np.triu(self.garbage, 1))

    @property
    def A(self):
        """The exact condensed matrix (I + N) diag(d) (I + N)', dense column-major."""
        M = sp.identity(self.n + self.n_eq, format="csc") + self.Nmat
        return np.asfortranarray((M @ sp.diags(self.d) @ M.T).toarray())

    @property
    def b(self):
        return unreduced_matrix(self) @ self.xstar

    def blocks(self):
        """{name: slice} of the unreduced vector."""
        e = np.cumsum([0, self.n, self.ns, self.m, len(self.ind_lb), len(self.ind_ub)])
        return {k: slice(int(e[i]), int(e[i + 1])) for i, k in enumerate(BLOCKS)}

    def inertia(self):
        return (int(np.sum(self.d > 0)), int(np.sum(self.d == 0)), int(np.sum(self.d < 0)))


# ------------------------------------------------------------------------------------------------ structure
def _structure(kind, n, m, n_eq, rng):
    """Index sets: equality / inequality rows from a random permutation (sorted: the two sets interleave); bounds on random
    subsets of the primal block -- x entries with both bounds, one or none (each kind at least once from n = 4 on), every slack
    with at least one."""
    perm = rng.permutation(m)
    ind_eq, ind_ineq = np.sort(perm[:n_eq]), np.sort(perm[n_eq:])
    ns = m - n_eq
    cx = rng.permutation(np.concatenate((np.arange(min(n, 4)), rng.integers(0, 4, max(n - 4, 0)))))   # 0 both 1 lb 2 ub 3 none
    cs = rng.permutation(np.concatenate((np.arange(min(ns, 3)), rng.integers(0, 3, max(ns - 3, 0)))))
    cat = np.concatenate((cx, cs)).astype(np.int64)
    ind_lb = np.flatnonzero((cat == 0) | (cat == 1))
    ind_ub = np.flatnonzero((cat == 0) | (cat == 2))
    return ind_eq, ind_ineq, ind_lb, ind_ub, cat


def draw_kkt_factors(n, n_eq, rng, per_row=6, exponents=(-2, 3)):
    """(N, d) of order n + n_eq, the variant of `exact_factor.draw_factors` for a condensed KKT matrix: the first n columns as
    there (random sources and targets, a target row draws about `per_row` sources below it plus the first source column); each
    of the last n_eq rows is a target that draws from a source set of its own, disjoint from the others' and without the first
    source column (A[n:, n:] is then diagonal).  d = 4^e > 0 on the first n pivots, -4^e on the last n_eq."""
    src = rng.random(n) < 0.5
    src[0] = True
    srcs = np.flatnonzero(src)
    s0 = int(srcs[0])
    rows, cols, vals = [], [], []
    for i in np.flatnonzero(~src):
        below = srcs[srcs < i]
        pick = rng.choice(below, size=min(per_row, len(below)), replace=False)
        pick = np.unique(np.concatenate((pick, [s0])))
        rows.append(np.full(len(pick), i))
        cols.append(pick)
        vals.append(rng.choice(_NVALS, size=len(pick)))
    if n_eq:
        pool = srcs[1:] if len(srcs) - 1 >= n_eq else srcs
        assert len(pool) >= n_eq, "too few source columns for disjoint equality rows"
        pool = rng.permutation(pool)
        per = max(1, min(per_row, len(pool) // n_eq))
        for k in range(n_eq):
            pick = np.sort(pool[k * per:(k + 1) * per])
            rows.append(np.full(len(pick), n + k))
            cols.append(pick)
            vals.append(rng.choice(_NVALS, size=len(pick)))
    N = n + n_eq
    if rows:
        Nmat = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    else:
        Nmat = sp.csc_matrix((N, N))
    d = 4.0 ** rng.integers(exponents[0], exponents[1] + 1, size=N)
    d[n:] *= -1.0
    return Nmat, d


def to_int(a, bits=GBITS):
    """a 2^bits as int64, asserting that it is integral (a is a multiple of 2^-bits)."""
    v = np.ldexp(np.asarray(a, dtype=np.float64), bits)
    assert np.all(v == np.rint(v)) and np.all(np.abs(v) < 2.0 ** 52), "not a multiple of the granule"
    return v.astype(np.int64)


def _sparse_patterns(H, jac, rng):
    """COO data of the sparse condensed handle: the nonzeros of J with some (i, j) reported twice (values 2v and -v) and the
    nonzeros of tril(H) with every fifth entry reported in the upper triangle and some reported twice."""
    jI, jJ = np.nonzero(jac)
    jv = jac[jI, jJ]
    dup = rng.random(len(jI)) < 0.15
    jI, jJ = np.concatenate((jI, jI[dup])), np.concatenate((jJ, jJ[dup]))
    jv = np.concatenate((np.where(dup, 2.0 * jv, jv), -jv[dup]))
    p = rng.permutation(len(jI))
    hI, hJ = np.nonzero(np.tril(H))
    hv = H[hI, hJ]
    dup = rng.random(len(hI)) < 0.1
    hI, hJ = np.concatenate((hI, hI[dup])), np.concatenate((hJ, hJ[dup]))
    hv = np.concatenate((np.where(dup, 2.0 * hv, hv), -hv[dup]))
    q = rng.permutation(len(hI))
    hI, hJ, hv = hI[q], hJ[q], hv[q]
    up = np.arange(len(hI)) % 5 == 0
    hI, hJ = np.where(up, hJ, hI), np.where(up, hI, hJ)
    return dict(jac_I=jI[p], jac_J=jJ[p], jac=jv[p], hess_I=hI, hess_J=hJ, hess=hv)


def exact_kkt_case(kind, n, m, n_eq, seed=0) -> KKTCase:
    assert kind in KINDS and (kind != "sparse_condensed" or n_eq == 0)
    rng = np.random.default_rng([seed, n, m, n_eq, KINDS.index(kind)])
    ind_eq, ind_ineq, ind_lb, ind_ub, cat = _structure(kind, n, m, n_eq, rng)
    ns, npr = m - n_eq, n + m - n_eq
    # bound and barrier terms
    reg = np.concatenate((2.0 ** rng.integers(-3, 1, n), np.zeros(ns)))
    kl, ku = rng.integers(0, 4, len(ind_lb)), rng.integers(0, 4, len(ind_ub))
    l_diag, u_diag = -(2.0 ** -kl), -(2.0 ** -ku)
    l_lower, u_lower = 2.0 ** rng.integers(-2, 3, len(ind_lb)), 2.0 ** rng.integers(-2, 3, len(ind_ub))
    e = rng.integers(-1, 3, ns)                                    # Sigma_s = 4^e
    share = 2 * e - (cat[n:] == 0)                                 # log2 of a bound's share: all of it, or one of two halves
    sl, su = ind_lb >= n, ind_ub >= n
    l_lower[sl] = 2.0 ** (share[ind_lb[sl] - n] - kl[sl])
    u_lower[su] = 2.0 ** (share[ind_ub[su] - n] - ku[su])
    du_diag = np.zeros(m)
    du_diag[ind_ineq] = np.where(rng.random(ns) < 0.5, 0.0, -3.0 / 4.0 ** e)
    # Jacobian, condensed matrix, Hessian
    jac = np.zeros((m, n), order="F")
    jac[ind_ineq] = rng.choice(_JVALS, size=(ns, n))
    Nmat, d = draw_kkt_factors(n, n_eq, rng)
    case = KKTCase(kind, n, m, n_eq, ind_eq, ind_ineq, ind_lb, ind_ub, reg, du_diag, l_diag, u_diag, l_lower, u_lower,
                   np.zeros((n, n)), jac, rng.standard_normal((n, n)), Nmat=Nmat, d=d)
    A = case.A
    jac[ind_eq] = A[n:, :n]
    du_diag[ind_eq] = np.diagonal(A)[n:]
    assert np.array_equal(case.pr_diag[n:], 4.0 ** e)
    Ji = to_int(jac[ind_ineq], 1)                                   # 2 J_i
    JDJ = Ji.T @ (to_int(case.D, 6)[:, None] * Ji)                   # 2^8 J_i' D J_i
    Hi = to_int(A[:n, :n]) - np.diag(to_int(case.pr_diag[:n])) - JDJ
    assert np.abs(Hi).max() < 2 ** 52
    case.H = np.ldexp(Hi.astype(np.float64), -GBITS)
    case.xstar = rng.integers(-8, 9, size=case.lw) * rng.choice(_XMULT, size=case.lw)
    if kind == "sparse_condensed":
        case.coo = _sparse_patterns(case.H, jac, rng)
    return case


def draw_vector(case, seed):
    """A vector drawn like x*."""
    rng = np.random.default_rng([seed, case.lw])
    return rng.integers(-8, 9, size=case.lw) * rng.choice(_XMULT, size=case.lw)


def scaled_case(c: KKTCase, a: int, b: int, cc: int) -> KKTCase:
    """`c` in the units x -> 2^a x, s -> 2^b s, y -> 2^cc y (see the module's docstring)."""
    assert (b + cc) % 2 == 0 and c.base is None
    n = c.n
    sl, su = c.ind_lb >= n, c.ind_ub >= n
    f = lambda v, k: np.ldexp(v, k)  # noqa: E731
    out = replace(
        c, H=f(c.H, b + cc - 2 * a), jac=np.asfortranarray(f(c.jac, b - a)), du_diag=f(c.du_diag, b - cc),
        reg=np.concatenate((f(c.reg[:n], b + cc - 2 * a), c.reg[n:])),
        l_diag=f(c.l_diag, np.where(sl, b - cc, 2 * a - b - cc)), u_diag=f(c.u_diag, np.where(su, b - cc, 2 * a - b - cc)),
        base=c, units=(a, b, cc))
    sx, se = (b + cc - 2 * a) // 2, (b - cc) // 2                        # A' = S A S, S = diag(2^sx on x, 2^se on the equality rows)
    s = np.concatenate((np.full(n, sx), np.full(c.n_eq, se))).astype(np.int64)
    out.Nmat = sp.csc_matrix(sp.diags(np.ldexp(1.0, s)) @ c.Nmat @ sp.diags(np.ldexp(1.0, -s)))
    out.d = np.ldexp(c.d, 2 * s)
    out.xstar = np.ldexp(c.xstar, solution_units(out))
    return out


def solution_units(c: KKTCase):
    """log2 of the factor on every entry of the solution of a scaled case."""
    a, b, cc = c.units
    k = np.zeros(c.lw, dtype=np.int64)
    bl = c.blocks()
    k[bl["x"]], k[bl["s"]], k[bl["y"]] = a, b, cc
    k[bl["z_l"]] = np.where(c.ind_lb >= c.n, cc, b + cc - a)
    k[bl["z_u"]] = np.where(c.ind_ub >= c.n, cc, b + cc - a)
    return k


def rhs_units(c: KKTCase):
    """log2 of the factor on every entry of the right-hand side of a scaled case."""
    a, b, cc = c.units
    k = np.zeros(c.lw, dtype=np.int64)
    bl = c.blocks()
    k[bl["x"]], k[bl["s"]], k[bl["y"]] = b + cc - a, cc, b
    k[bl["z_l"]] = np.where(c.ind_lb >= c.n, b, a)
    k[bl["z_u"]] = np.where(c.ind_ub >= c.n, b, a)
    return k


# ------------------------------------------------------------------------------------------------ the matrices
def unreduced_matrix(c: KKTCase, dtype=np.float64):
    """K_u of `mul!` over (x, s, y, z_l, z_u), entry by entry (reference src/IPM/factorization.jl:303-324 and `_kktmul!`,
    src/IPM/kernels.jl:161-180):
        x rows    (H + reg) x + J' y - z_l[x part] + z_u[x part]
        s rows    reg s - y[ineq] - z_l[s part] + z_u[s part]
        y rows    J x - s (inequality rows) + du_diag y
        z_l rows  l_lower xp[ind_lb] - l_diag z_l
        z_u rows  u_lower xp[ind_ub] + u_diag z_u"""
    n, ns, m, npr = c.n, c.ns, c.m, c.npr
    nlb, nub = len(c.ind_lb), len(c.ind_ub)
    K = np.zeros((c.lw, c.lw), dtype=dtype)
    K[:n, :n] = c.H
    ip = np.arange(npr)
    K[ip, ip] += c.reg
    K[npr:npr + m, :n] = c.jac
    K[:n, npr:npr + m] = c.jac.T
    si, yi = n + np.arange(ns), npr + c.ind_ineq
    K[si, yi] = -1.0
    K[yi, si] = -1.0
    ym = npr + np.arange(m)
    K[ym, ym] = c.du_diag
    il, iu = npr + m + np.arange(nlb), npr + m + nlb + np.arange(nub)
    K[c.ind_lb, il] = -1.0
    K[il, c.ind_lb] = c.l_lower
    K[il, il] = -c.l_diag.astype(dtype)
    K[c.ind_ub, iu] = 1.0
    K[iu, c.ind_ub] = c.u_lower
    K[iu, iu] = c.u_diag
    return K


def row_nonzeros(c: KKTCase):
    """t_i: the structural nonzeros of row i of K_u (a Hessian / Jacobian entry counts where the handle stores one: everywhere
    for the dense kinds, on the COO pattern for the sparse one; the diagonal of the primal and dual blocks always)."""
    S = unreduced_matrix(replace(c, H=np.ones_like(c.H), jac=np.ones_like(c.jac), reg=np.ones_like(c.reg),
                                 du_diag=np.ones_like(c.du_diag))) != 0
    if c.kind == "sparse_condensed":
        n, npr, m = c.n, c.npr, c.m
        P = np.zeros((n, n), dtype=bool)
        P[c.coo["hess_I"], c.coo["hess_J"]] = True
        P |= P.T | np.eye(n, dtype=bool)
        Jp = np.zeros((m, n), dtype=bool)
        Jp[c.coo["jac_I"], c.coo["jac_J"]] = True
        S[:n, :n] = P
        S[npr:npr + m, :n] = Jp
        S[:n, npr:npr + m] = Jp.T
    return S.sum(axis=1)


def reduced_matrix(c: KKTCase, dtype=np.float64):
    """The matrix `build_kkt!` forms: the condensed one [H + pr_x + J_i' D J_i, J_e'; J_e, du_e] (dense_condensed,
    sparse_condensed) or the augmented one [H + pr_x, 0, J'; 0, Sigma_s, -I; J, -I, du] (dense), in `dtype` from the fp64 data."""
    n, ns, m, npr = c.n, c.ns, c.m, c.npr
    pr, du = c.pr_diag.astype(dtype), c.du_diag.astype(dtype)
    H, J = c.H.astype(dtype), c.jac.astype(dtype)
    if c.kind == "dense":
        K = np.zeros((c.order, c.order), dtype=dtype)
        K[:n, :n] = H
        ip = np.arange(npr)
        K[ip, ip] += pr
        K[npr:, :n] = J
        K[:n, npr:] = J.T
        si, yi = n + np.arange(ns), npr + c.ind_ineq
        K[si, yi] = -1.0
        K[yi, si] = -1.0
        ym = npr + np.arange(m)
        K[ym, ym] = du
        return K
    Ss = pr[n:]
    D = Ss / (1 - du[c.ind_ineq] * Ss)
    Ji = J[c.ind_ineq]
    K = np.zeros((c.order, c.order), dtype=dtype)
    K[:n, :n] = H + np.diag(pr[:n]) + Ji.T @ (D[:, None] * Ji)
    K[n:, :n] = J[c.ind_eq]
    K[:n, n:] = J[c.ind_eq].T
    ie = n + np.arange(c.n_eq)
    K[ie, ie] = du[c.ind_eq]
    return K


def exact_mul(c: KKTCase, x, w, alpha, beta):
    """alpha K_u x + beta w in scaled integers (K_u 2^8, x and w 2^2, alpha 2^2, beta 2^1): the one right answer."""
    Ki, xi, wi = to_int(unreduced_matrix(c)), to_int(x, 2), to_int(w, 2)
    ai, bi = int(to_int(alpha, 2)), int(to_int(beta, 1))
    r = ai * (Ki @ xi) + bi * (wi << (GBITS + 1))          # 2^12 (alpha K_u x + beta w)
    assert np.abs(r).max() < 2 ** 53
    return np.ldexp(r.astype(np.float64), -(GBITS + 4))


# ------------------------------------------------------------------------------------------------ the fp64 chain
def _dot(M, v, order, rng):
    """M v accumulated column by column: "forward", "backward" or in a random order."""
    k = M.shape[1]
    idx = {"forward": np.arange(k), "backward": np.arange(k)[::-1]}.get(order)
    if idx is None:
        idx = rng.permutation(k)
    acc = np.zeros(M.shape[0])
    for j in idx:
        acc += M[:, j] * v[j]
    return acc


def solve_chain(c: KKTCase, rhs, order="forward", seed=0):
    """The condensed `solve_kkt!` in plain fp64 (reference src/IPM/factorization.jl:143-167,190-229) with every sum taken in
    `order`: reduce_rhs, condensed right-hand side, J' buffer, the LDL' sweeps on the exact factor (inv(I + N) = I - N), J x,
    expansion, finish_aug."""
    assert c.kind != "dense"
    rng = np.random.default_rng(seed)
    n, ns, m, npr = c.n, c.ns, c.m, c.npr
    bl = c.blocks()
    w = np.array(rhs, dtype=np.float64)
    wl, wu = w[bl["z_l"]], w[bl["z_u"]]
    np.subtract.at(w, c.ind_lb, wl / c.l_diag)
    np.subtract.at(w, c.ind_ub, wu / c.u_diag)
    wx, ws, dual = w[bl["x"]], w[bl["s"]], w[bl["y"]]
    Ss, D = c.pr_diag[n:], c.D
    buffer = np.zeros(m)
    buffer[c.ind_ineq] = D * (dual[c.ind_ineq] + ws / Ss)
    pd = np.concatenate((_dot(np.ascontiguousarray(c.jac.T), buffer, order, rng) + wx, dual[c.ind_eq]))
    Nd = c.Nmat.toarray()
    y = (pd - _dot(Nd, pd, order, rng)) / c.d
    sol = y - _dot(np.ascontiguousarray(Nd.T), y, order, rng)
    wx[:] = sol[:n]
    dual[:] = _dot(c.jac, wx, order, rng)
    z = dual[c.ind_ineq] * D - buffer[c.ind_ineq]
    dual[c.ind_ineq] = z
    dual[c.ind_eq] = sol[n:]
    ws[:] = (ws + z) / Ss
    wl[:] = (-wl + c.l_lower * w[c.ind_lb]) / c.l_diag
    wu[:] = (wu - c.u_lower * w[c.ind_ub]) / c.u_diag
    return w


def _lsb(a):
    """The exponent of the lowest set bit over the nonzero entries of a (a large number for an all-zero array: no term)."""
    a = np.abs(np.asarray(a, dtype=np.float64)).ravel()
    a = a[a != 0]
    if len(a) == 0:
        return 4096
    mant, ex = np.frexp(a)
    mi = np.ldexp(mant, 53).astype(np.int64)
    return int((ex - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)).min())


def bit_budget(c: KKTCase) -> int:
    """An a-priori bound, in bits, on the significand any partial sum of `mul!`, `build_kkt!` or the condensed `solve_kkt!` chain
    needs: log2 of (the sum of the magnitudes of the terms of a row) / (the granule of the terms: the lowest set bit of any of
    them, for a product the sum of those of its factors).  A scaled case multiplies both by the same power of two, row by row:
    its budget is its base's.
      mul!         |alpha| |K_u| |x| + |beta| |w| with |x|, |w| <= 8 of granule 2^-2, alpha of granule 2^-2, beta 2^-1
      build_kkt!   |H| + |pr| + |J_i|' D |J_i|
      solve_kkt!   the stages of `solve_chain` on b = K_u x*, the sums |M| |v| with the values v of the exact run, and the sweeps
                   by `solve_exact.bit_budget` on the condensed solution (x*_x, y*_eq)."""
    c = c.base or c
    n, npr = c.n, c.npr
    bits = []

    def stage(bound, g):
        top = float(np.max(bound)) if np.size(bound) else 0.0
        if top > 0.0:
            assert g < 4096
            bits.append(int(np.ceil(np.log2(top))) - g + 1)

    Ka = np.abs(unreduced_matrix(c))
    stage(Ka @ np.full(c.lw, 8.0) + 2.0 * 8.0, min(_lsb(Ka) - 4, -3))
    Ji, D, pr = np.abs(c.jac[c.ind_ineq]), c.D, c.pr_diag
    stage(np.abs(c.H) + np.diag(pr[:n]) + Ji.T @ (D[:, None] * Ji), min(_lsb(c.H), _lsb(pr[:n]), 2 * _lsb(Ji) + _lsb(D)))
    if c.kind == "dense":
        return max(bits)
    bl = c.blocks()
    xs, b = c.xstar, c.b
    stage(Ka @ np.abs(xs), _lsb(Ka) + _lsb(xs))                                     # b itself
    w = solve_chain(c, b)                                                            # (exact when the budget holds: x*)
    dl, du = np.zeros(npr), np.zeros(npr)
    dl[c.ind_lb], du[c.ind_ub] = b[bl["z_l"]] / c.l_diag, b[bl["z_u"]] / c.u_diag
    red = np.array(b)
    red[:npr] -= dl + du
    stage(np.abs(b[:npr]) + np.abs(dl) + np.abs(du), min(_lsb(b[:npr]), _lsb(dl), _lsb(du)))   # reduce_rhs
    Ss = pr[n:]
    rz, rs = red[bl["y"]][c.ind_ineq], red[bl["s"]] / Ss
    buffer = np.zeros(c.m)
    buffer[c.ind_ineq] = D * (rz + rs)
    stage(np.abs(rz) + np.abs(rs), min(_lsb(rz), _lsb(rs)))
    stage(np.abs(c.jac.T) @ np.abs(buffer) + np.abs(red[bl["x"]]), min(_lsb(c.jac) + _lsb(buffer), _lsb(red[bl["x"]])))
    xc = np.concatenate((xs[bl["x"]], xs[bl["y"]][c.ind_eq]))
    bits.append(_sweep_bits(SolveCase(c.order, c.n_eq == 0, c.Nmat, c.d, np.zeros(c.order, dtype=np.int64), xc, None)))
    stage(np.abs(c.jac) @ np.abs(xc[:n]), _lsb(c.jac) + _lsb(xc[:n]))              # J x
    jxd = (c.jac[c.ind_ineq] @ xc[:n]) * D
    stage(np.abs(jxd) + np.abs(buffer[c.ind_ineq]), min(_lsb(jxd), _lsb(buffer)))   # expansion
    z = w[bl["y"]][c.ind_ineq]
    stage(np.abs(red[bl["s"]]) + np.abs(z), min(_lsb(red[bl["s"]]), _lsb(z)))
    for lower, ind, blk in ((c.l_lower, c.ind_lb, "z_l"), (c.u_lower, c.ind_ub, "z_u")):   # finish_aug
        stage(np.abs(red[bl[blk]]) + np.abs(lower * w[ind]), min(_lsb(red[bl[blk]]), _lsb(lower * w[ind])))
    return max(bits)


# ------------------------------------------------------------------------------------------------ rounded data
def random_kkt_case(kind, n, m, n_eq, seed=0) -> KKTCase:
    """The structure of `exact_kkt_case` with continuous values (see the module's docstring)."""
    assert kind in KINDS
    if kind == "sparse_condensed":
        n_eq = 0
    rng = np.random.default_rng([seed, n, m, n_eq, 17 + KINDS.index(kind)])
    ind_eq, ind_ineq, ind_lb, ind_ub, _ = _structure(kind, n, m, n_eq, rng)
    ns = m - n_eq
    logu = lambda lo, hi, k: 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), k)  # noqa: E731
    reg = np.concatenate((np.full(n, 1e-4), np.zeros(ns)))
    l_diag, u_diag = -logu(1e-2, 1.0, len(ind_lb)), -logu(1e-2, 1.0, len(ind_ub))
    l_lower, u_lower = logu(1e-3, 1.0, len(ind_lb)), logu(1e-3, 1.0, len(ind_ub))
    du_diag = np.zeros(m)
    du_diag[ind_ineq] = -logu(1e-8, 1e-2, ns)
    R = rng.standard_normal((n, n))
    jac = np.asfortranarray(rng.standard_normal((m, n)))
    if kind == "sparse_condensed":                             # a sparse pattern: half of J, about three entries per column of R
        jac *= rng.random((m, n)) < 0.5
        R *= rng.random((n, n)) < 3.0 / n
        H = R @ R.T + np.eye(n)
    else:
        H = R @ R.T / n + np.eye(n)
    H = (H + H.T) / 2
    case = KKTCase(kind, n, m, n_eq, ind_eq, ind_ineq, ind_lb, ind_ub, reg, du_diag, l_diag, u_diag, l_lower, u_lower, H, jac,
                   rng.standard_normal((n, n)))
    if kind == "sparse_condensed":
        coo = _sparse_patterns(H, jac, rng)
        # what the handle holds is the sum of the duplicates in COO order, rounded: make H and J exactly that
        Hs, Js = np.zeros((n, n)), np.zeros((m, n))
        I, J = np.maximum(coo["hess_I"], coo["hess_J"]), np.minimum(coo["hess_I"], coo["hess_J"])
        np.add.at(Hs, (I, J), coo["hess"])
        np.add.at(Js, (coo["jac_I"], coo["jac_J"]), coo["jac"])
        case.H = np.tril(Hs) + np.tril(Hs, -1).T
        case.jac = np.asfortranarray(Js)
        case.coo = coo
    return case


def mul_bound(c: KKTCase, x, w, alpha, beta):
    """(reference in longdouble, per-entry bound) of alpha K_u x + beta w."""
    K = unreduced_matrix(c, np.longdouble)
    xl, wl = x.astype(np.longdouble), w.astype(np.longdouble)
    ref = np.longdouble(alpha) * (K @ xl) + np.longdouble(beta) * wl
    S = abs(alpha) * (np.abs(K) @ np.abs(xl)) + abs(beta) * np.abs(wl)
    return ref, (row_nonzeros(c) + 6) * U * S


def build_bound(c: KKTCase):
    """(reference in longdouble, per-entry bound) of the dense condensed matrix."""
    n = c.n
    ref = reduced_matrix(c, np.longdouble)
    Ji = np.abs(c.jac[c.ind_ineq]).astype(np.longdouble)
    pr, du = c.pr_diag.astype(np.longdouble), c.du_diag.astype(np.longdouble)
    D = pr[n:] / (1 - du[c.ind_ineq] * pr[n:])
    S = np.zeros_like(ref)
    S[:n, :n] = np.abs(c.H) + np.diag(np.abs(pr[:n])) + Ji.T @ (D[:, None] * Ji)
    return ref, (c.ns + 8) * U * S


def residual(c: KKTCase, x, b):
    """max |K_u x - b| / (max |b| + max |x|) in longdouble."""
    K = unreduced_matrix(c, np.longdouble)
    r = K @ x.astype(np.longdouble) - b.astype(np.longdouble)
    return float(np.abs(r).max() / (np.abs(b).max() + np.abs(x).max()))


# ------------------------------------------------------------------------------------------------ the oracle on a case
def oracle_system(c: KKTCase, build=True):
    """The `oracle/` class of the case's kind (LAPACK: Bunch-Kaufman, Cholesky for the sparse condensed system) fed with its data;
    `build`: after `build_kkt`."""
    from oracle import dense as odense
    from oracle import sparse_condensed as osc
    from oracle.lapack_cpu import BUNCHKAUFMAN, CHOLESKY, LapackCPUSolver
    if c.kind == "sparse_condensed":
        q = c.coo
        ko = osc.SparseCondensedKKTSystem(c.n, c.m, q["jac_I"], q["jac_J"], q["hess_I"], q["hess_J"], c.ind_ineq, c.ind_lb,
                                          c.ind_ub, lambda A: LapackCPUSolver(A, CHOLESKY))
        ko.jac[:] = q["jac"]
        ko.hess[:] = q["hess"]
    else:
        fac = lambda A: LapackCPUSolver(A, BUNCHKAUFMAN)  # noqa: E731
        if c.kind == "dense_condensed":
            ko = odense.DenseCondensedKKTSystem(c.n, c.m, c.ind_ineq, c.ind_eq, c.ind_lb, c.ind_ub, fac)
        else:
            ko = odense.DenseKKTSystem(c.n, c.m, c.ind_ineq, c.ind_lb, c.ind_ub, fac)
        ko.hess[...] = c.hess
        ko.jac[...] = c.jac
    for name in ("reg", "pr_diag", "du_diag", "l_diag", "u_diag", "l_lower", "u_lower"):
        getattr(ko, name)[:] = getattr(c, name)
    ko.compress_jacobian()
    ko.compress_hessian()
    if build:
        ko.build_kkt()
    return ko


def oracle_vector(ko, values):
    from oracle import kernels as okern
    v = okern.UnreducedKKTVector.from_kkt(ko)
    v.values[:] = values
    return v


def oracle_residual(c: KKTCase, b):
    """(solution, residual) of the oracle's `solve_kkt` on the case."""
    ko = oracle_system(c)
    ko.linear_solver.factorize()
    x = ko.solve_kkt(oracle_vector(ko, b)).values
    return x, residual(c, x, b)

"""Quasi-Newton Hessians: `hessian_approximation = BFGS / DampedBFGS` of the dense KKT systems and `CompactLBFGS` of the
sparse condensed one (reference `src/quasi_newton.jl:72-437`), restated in numpy.

This is the host specification of the updates and the comparator of the device paths (`csrc/qn.hip`,
`kkt._DenseBase.qn_update_device`; `csrc/lbfgs.hip`, `kkt.SparseCondensedKKTSystem.attach_quasi_newton`).  The dense
approximation `B` is the n x n Hessian buffer of a dense KKT system.  Like the reference (dsymv / dsyr with `'L'`) the dense
routines read and write the LOWER triangle only: the strict upper triangle keeps whatever it held.

    init        src/quasi_newton.jl:194-206     B's diagonal = 2 rho0 (Gilbert & Lemarechal), the rest zero
    BFGS        src/quasi_newton.jl:112-130     B -= bs bs' / s'bs ; B += y y' / s'y ; skipped when s'y < 1e-8
    DampedBFGS  src/quasi_newton.jl:163-192     Powell's damping (Nocedal & Wright, procedure 18.2), never skipped

    CompactLBFGS  src/quasi_newton.jl:210-437   B = sigma I - U U' + V V' (Byrd, Nocedal & Schnabel); `B` is the n-vector of a
                                                DIAGONAL Hessian pattern and holds sigma, U and V stay in the object.  The
                                                reference applies the low-rank part by Sherman-Morrison-Woodbury around its
                                                SparseKKTSystem (src/IPM/factorization.jl:76-140); here the same identity is
                                                applied around the sparse CONDENSED system (`kkt.LowRankHessianKKT`, DESIGN.md
                                                section 18), a combination the reference refuses (factorization.jl:176-181).

Every sum over the n variables of `CompactLBFGS` and of the low-rank products below is an `ipm.ordered_sum`, the order of the
device reductions (`csrc/lbfgs.hip`): both back-ends produce the same bits from the same vectors.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

HESSIAN_APPROXIMATIONS = ("exact", "bfgs", "damped_bfgs", "compact_lbfgs")
QN_BFGS, QN_DAMPED_BFGS = 1, 2          # == MNK_QN_BFGS / MNK_QN_DAMPED_BFGS of include/madnlp_hip.h
QN_KIND = {"bfgs": QN_BFGS, "damped_bfgs": QN_DAMPED_BFGS}
SKIP_TOL = 1e-8                          # quasi_newton.jl:114


def rho0(g0, f0):
    """The scale of the first approximation, `init!` quasi_newton.jl:195-203.  `f0 ≈ 0` is Julia's `isapprox` with its
    default tolerances (rtol = sqrt(eps), atol = 0), which against zero holds for `f0 == 0` only."""
    gg = float(np.dot(g0, g0))
    if gg < math.sqrt(np.finfo(np.float64).eps):
        return 1.0
    if f0 == 0.0:
        return 1.0 / gg
    return abs(f0) / gg


def symv_lower(B, s):
    """`Symmetric(B, :L) * s` from the lower triangle of B alone (dsymv 'L')."""
    return np.tril(B) @ s + np.tril(B, -1).T @ s


def _syr_lower(B, alpha, v):
    """B += alpha v v' on the lower triangle (dsyr 'L': column j receives v * (alpha v[j]))."""
    il = np.tril_indices(B.shape[0])
    B[il] += v[il[0]] * (alpha * v)[il[1]]


class _DenseQuasiNewton:
    kind = None

    def __init__(self, n):
        self.n = n
        self.is_instantiated = False       # the first PERFORMED update first resets the diagonal (quasi_newton.jl:118-122)
        self.updates = self.skipped = 0
        self.last = np.zeros(4)            # [s'y, s'Bs, theta, r's] of the last `update` (what mnk_dc_qn_status reports)
        # what the driver keeps between two calls (callbacks.jl:184-186); numpy arrays here, device vectors in ipm_dev
        self.last_x = self.last_g = self.last_jv = None

    def init(self, B, g0, f0):
        """`init!` quasi_newton.jl:194-206 (the reference's buffer is zero at this point: `initialize!(kkt)`)."""
        B[...] = 0.0
        B[np.diag_indices(self.n)] = 2.0 * rho0(g0, f0)

    def adopt(self):
        """Take the matrix as it is for the current approximation: no diagonal reset in front of the next update."""
        self.is_instantiated = True

    def _first(self, B, sy, s):
        if not self.is_instantiated:
            B[np.diag_indices(self.n)] = sy / float(np.dot(s, s))
            self.is_instantiated = True


class BFGS(_DenseQuasiNewton):
    """`BFGS` quasi_newton.jl:72-130."""
    kind = QN_BFGS

    def update(self, B, s, y):
        sy = float(np.dot(s, y))
        if sy < SKIP_TOL:
            self.skipped += 1
            self.last[:] = (sy, 0.0, 1.0, sy)
            return False
        self._first(B, sy, s)
        bs = symv_lower(B, s)
        sBs = float(np.dot(s, bs))
        _syr_lower(B, -(1.0 / sBs), bs)
        _syr_lower(B, 1.0 / sy, y)
        self.updates += 1
        self.last[:] = (sy, sBs, 1.0, sy)
        return True


class DampedBFGS(_DenseQuasiNewton):
    """`DampedBFGS` quasi_newton.jl:132-192."""
    kind = QN_DAMPED_BFGS

    def update(self, B, s, y):
        sy = float(np.dot(s, y))
        self._first(B, sy, s)
        bs = symv_lower(B, s)
        sBs = float(np.dot(s, bs))
        theta = 0.8 * sBs / (sBs - sy) if sy < 0.2 * sBs else 1.0
        r = theta * y + (1.0 - theta) * bs
        rs = float(np.dot(r, s))
        _syr_lower(B, -(1.0 / sBs), bs)
        _syr_lower(B, 1.0 / rs, r)
        self.updates += 1
        self.last[:] = (sy, sBs, theta, rs)
        return True


SCALAR1, SCALAR2, SCALAR3, SCALAR4 = 1, 2, 3, 4     # BFGSInitStrategy of the reference (the values of MNK_LBFGS_SCALAR1..4)
MAX_HISTORY_DEVICE = 32                             # the device handle's cap: E = [U V] is one chunk of the blocked solve


@dataclass
class QuasiNewtonOptions:
    """`QuasiNewtonOptions` quasi_newton.jl:63-69."""
    init_strategy: int = SCALAR1
    max_history: int = 6
    init_value: float = 1.0
    sigma_min: float = 1e-8
    sigma_max: float = 1e8


def odot(a, b):
    """a . b with the bits of the device reductions (`ipm.ordered_sum` over the products, each rounded on its own)."""
    from .ipm import ordered_sum      # (ipm imports this module)
    return ordered_sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def curvature(strategy, ss, sy, yy):
    """`curvature` quasi_newton.jl:48-61 from s's, s'y, y'y."""
    if strategy == SCALAR1:
        return sy / ss
    if strategy == SCALAR2:
        return yy / sy
    if strategy == SCALAR3:
        return ((sy / ss) + (yy / sy)) / 2
    if strategy == SCALAR4:
        return math.sqrt((sy / ss) * (yy / sy))
    raise ValueError(f"init_strategy must be SCALAR1 .. SCALAR4 (1 .. 4), not {strategy!r}")


def gram(A, B):
    """A' B (q_a x q_b), every entry an ordered sum: `lb_gram_kernel` of csrc/lbfgs.hip."""
    out = np.zeros((A.shape[1], B.shape[1]))
    for i in range(A.shape[1]):
        for j in range(B.shape[1]):
            out[i, j] = odot(A[:, i], B[:, j])
    return out


def lowrank_apply(y, alpha, A, M, B, x):
    """y += alpha A (M (B' x)) with A, B of n x q and M of q x q, in the operation order of the device pair
    `lb_gram_kernel` / `lb_apply_kernel`: t = B'x by ordered sums, c = M t and A c accumulated over ascending columns with one
    multiply and one add per term, one multiply by alpha and one add into y."""
    q = A.shape[1]
    t = gram(B, np.asarray(x, dtype=np.float64).reshape(-1, 1))[:, 0]
    c = np.zeros(q)
    for j in range(q):
        c = c + M[:, j] * t[j]
    acc = np.zeros(A.shape[0])
    for j in range(q):
        acc = acc + A[:, j] * c[j]
    y += alpha * acc
    return y


class CompactLBFGS:
    """`CompactLBFGS` quasi_newton.jl:210-437: S, Y hold the last `current_mem` <= `max_mem` accepted pairs, oldest first.
    After a performed update  B_k = sigma I - U U' + V V'  with  V = Y D^-1/2,  U = (sigma S + Y D^-1 L') J^-T,
    D = diag(S'Y), L = its strict lower triangle, J J' = M = sigma S'S + L D^-1 L'.
    Two things differ from the reference, neither where the reference gives an answer: S'S and L grow by one row per update
    instead of being recomputed (the same numbers), and a Cholesky breakdown of M (the reference raises PosDefException)
    resets the memory like a second skip."""
    kind = None

    def __init__(self, n, options: QuasiNewtonOptions | None = None):
        o = options or QuasiNewtonOptions()
        if o.max_history < 1:
            raise ValueError("max_history must be at least 1")
        curvature(o.init_strategy, 1.0, 1.0, 1.0)
        self.n, self.options = n, o
        self.max_mem, self.init_strategy = int(o.max_history), int(o.init_strategy)
        self.updates = self.skipped = self.resets = 0
        self.version = 0                    # bumped by every performed or resetting update: what caches of H, T are keyed on
        self.sigma = 0.0
        self.last_x = self.last_g = self.last_jv = None
        self._reset()

    # `size(qn)` of the reference is (n, current_mem)
    def _reset(self):
        """`_reset!` quasi_newton.jl:294-304."""
        n = self.n
        self.current_mem = self.skipped_iter = 0
        self.S, self.Y = np.zeros((n, 0)), np.zeros((n, 0))
        self.U, self.V = np.zeros((n, 0)), np.zeros((n, 0))
        self.StS, self.L, self.D = np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0)
        self.M = np.zeros((0, 0))

    @property
    def E(self):
        """[U V], n x 2p."""
        return np.hstack((self.U, self.V))

    @property
    def P(self):
        """diag(-I_p, I_p)."""
        p = self.current_mem
        return np.diag(np.concatenate((-np.ones(p), np.ones(p))))

    def init(self, B, g0, f0):
        """`init!` quasi_newton.jl:425-437: B .= 2 rho0 init_value."""
        gg = odot(g0, g0)
        if gg < math.sqrt(np.finfo(np.float64).eps):
            r = 1.0
        elif f0 == 0.0:
            r = 1.0 / gg
        else:
            r = abs(f0) / gg
        self.sigma = 2.0 * r * self.options.init_value
        B[:] = self.sigma

    def update(self, B, s, y):
        """`update!` quasi_newton.jl:366-423."""
        eps = np.finfo(np.float64).eps
        ss, sy, yy = odot(s, s), odot(s, y), odot(y, y)
        ns, ny = math.sqrt(ss), math.sqrt(yy)
        if ns < 100 * eps or ny < 100 * eps or sy < math.sqrt(eps) * ns * ny:
            self.skipped += 1
            self.skipped_iter += 1
            if self.skipped_iter >= 2:
                self._reset()
                self.resets += 1
                self.version += 1
            return False
        p = self.current_mem
        # the new row of S'S and of tril(S'Y, -1) against the stored pairs (before a shift drops the oldest)
        row_ss = np.array([odot(self.S[:, j], s) for j in range(p)])
        row_l = np.array([odot(self.Y[:, j], s) for j in range(p)])
        keep = slice(1, p) if p == self.max_mem else slice(0, p)     # `_update_S_and_Y!` / `_update_L_and_D!`
        self.S = np.column_stack((self.S[:, keep], s))
        self.Y = np.column_stack((self.Y[:, keep], y))
        k = self.S.shape[1]
        StS, Lk = np.zeros((k, k)), np.zeros((k, k))
        StS[:k - 1, :k - 1] = self.StS[keep, keep]
        StS[k - 1, :k - 1] = StS[:k - 1, k - 1] = row_ss[keep]
        StS[k - 1, k - 1] = ss
        Lk[:k - 1, :k - 1] = self.L[keep, keep]
        Lk[k - 1, :k - 1] = row_l[keep]
        D = np.concatenate((self.D[keep], [sy]))
        o = self.options
        sigma = curvature(self.init_strategy, ss, sy, yy)
        sigma = min(max(sigma, o.sigma_min), o.sigma_max)
        delta = 1.0 / np.sqrt(D)
        DkLk = delta[:, None] * Lk.T                      # D^-1/2 L'
        M = sigma * StS + DkLk.T @ DkLk
        try:
            J = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            self.skipped += 1
            self._reset()
            self.resets += 1
            self.version += 1
            return False
        from scipy.linalg import solve_triangular
        self.current_mem, self.StS, self.L, self.D, self.M = k, StS, Lk, D, M
        self.V = self.Y * delta[None, :]
        W = sigma * self.S + self.V @ DkLk
        self.U = solve_triangular(J, W.T, lower=True).T   # W J^-T
        self.sigma = sigma
        B[:] = sigma
        self.updates += 1
        self.version += 1
        return True


def create_quasi_newton(name, n, options=None):
    """`create_quasi_newton` quasi_newton.jl:94-110,144-161,242-277."""
    if name == "bfgs":
        return BFGS(n)
    if name == "damped_bfgs":
        return DampedBFGS(n)
    if name == "compact_lbfgs":
        return CompactLBFGS(n, options)
    raise ValueError(f"hessian_approximation must be one of {HESSIAN_APPROXIMATIONS}, not {name!r}")

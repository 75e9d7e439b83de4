"""Iterative refinement around `solve_kkt!`: Richardson -- host-side mirror of reference `src/LinearSolvers/backsolve.jl:27-76`
(the caller of `solve_linear_system!`) -- and restarted GMRES preconditioned by the factorization, the capability of the
reference's `lib/MadNLPKrylov` (solver option `iterator = "krylov"`; algorithm and its deviations in DESIGN.md section 17)."""
from __future__ import annotations

import math

import numpy as np

ITERATORS = ("richardson", "krylov")
KRYLOV_MAX_RESTART = 8     # columns one call of the device kernels takes (csrc/krylov.hip)


class RichardsonIterator:
    def __init__(self, kkt, tol=1e-8, max_iter=10):
        """defaults of reference `backsolve.jl:1-5,25`."""
        self.kkt = kkt
        self.richardson_tol = tol ** (5 / 4)
        self.richardson_acceptable_tol = tol ** (5 / 8)
        self.richardson_max_iter = max_iter
        self.ir = 0
        self.residual_ratio = 0.0

    def solve_refine(self, x, b, w):
        norm_b = np.linalg.norm(b.values, np.inf)
        residual_ratio = 0.0
        x.values[:] = 0.0
        if norm_b != 0:
            w.values[:] = b.values
            self.ir = 0
            while True:
                self.kkt.solve_kkt(w)
                x.values += w.values
                w.values[:] = b.values
                self.kkt.mul(w, x, -1.0, 1.0)
                norm_w = np.linalg.norm(w.values, np.inf)
                norm_x = np.linalg.norm(x.values, np.inf)
                residual_ratio = norm_w / (min(norm_x, 1e6 * norm_b) + norm_b)
                self.ir += 1
                if self.ir >= self.richardson_max_iter or residual_ratio < self.richardson_tol:
                    break
        self.residual_ratio = residual_ratio
        return residual_ratio < self.richardson_acceptable_tol


def _osum(v):
    from .ipm import ordered_sum      # (ipm imports this module)
    return ordered_sum(v)


class GmresCycle:
    """The host scalars of one GMRES cycle, shared by the host mirror and the device driver: the Hessenberg columns reduced
    to triangular form by Givens rotations, the rotated right-hand side g = beta e1 and the residual estimate rho = |g[j+1]|."""

    def __init__(self, beta, restart):
        self.R = np.zeros((restart + 1, restart))
        self.g = np.zeros(restart + 1)
        self.g[0] = beta
        self.cs, self.sn = np.zeros(restart), np.zeros(restart)
        self.k = 0
        self.rho = []

    def add_column(self, h1, h2, hn):
        """Column j of the Hessenberg matrix: h(1:j, j) = h1 + h2 (the two Gram-Schmidt passes), h(j+1, j) = hn.  Returns rho."""
        j = self.k
        col = np.zeros(j + 2)
        col[:j + 1] = np.asarray(h1, dtype=np.float64)[:j + 1] + np.asarray(h2, dtype=np.float64)[:j + 1]
        col[j + 1] = hn
        for i in range(j):
            a, b = col[i], col[i + 1]
            col[i], col[i + 1] = self.cs[i] * a + self.sn[i] * b, -self.sn[i] * a + self.cs[i] * b
        d = math.hypot(col[j], col[j + 1])
        self.cs[j], self.sn[j] = (col[j] / d, col[j + 1] / d) if d != 0 else (1.0, 0.0)
        col[j], col[j + 1] = d, 0.0
        self.R[:j + 2, j] = col
        self.g[j + 1] = -self.sn[j] * self.g[j]
        self.g[j] = self.cs[j] * self.g[j]
        self.k = j + 1
        self.rho.append(abs(self.g[j + 1]))
        return self.rho[-1]

    def solution(self):
        """y = R^-1 g over the k columns taken (a zero pivot -- a basis that broke down on a singular operator -- gives 0)."""
        k = self.k
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            t = self.g[i] - float(self.R[i, i + 1:k] @ y[i + 1:])
            y[i] = t / self.R[i, i] if self.R[i, i] != 0 else 0.0
        return y


class KrylovIterator:
    """Restarted GMRES on M^-1 A x = M^-1 b with A = `kkt.mul`, M^-1 = `kkt.solve_kkt` (left preconditioning), judged by
    Richardson's residual ratio so that the two iterators are interchangeable.  `ir` counts the `solve_kkt` calls (at most
    `max_iter`), `steps` the Arnoldi steps, `cycles` the GMRES cycles; `trace` holds (beta, [rho ...]) per cycle.  Every dot
    product and 2-norm is an `ordered_sum` and the Gram-Schmidt / solution updates take their terms in the order of the
    columns, one multiply and one add or subtract each: the operations of csrc/krylov.hip, bit for bit."""

    def __init__(self, kkt, tol=1e-8, restart=5, max_iter=10, krylov_tol=1e-10):
        if not 1 <= restart <= KRYLOV_MAX_RESTART:
            raise ValueError(f"krylov_restart must be in 1..{KRYLOV_MAX_RESTART}, not {restart!r}")
        if max_iter < 1:
            raise ValueError(f"krylov_max_iter must be at least 1, not {max_iter!r}")
        self.kkt = kkt
        self.richardson_tol = tol ** (5 / 4)
        self.richardson_acceptable_tol = tol ** (5 / 8)
        self.restart, self.max_iter, self.krylov_tol = int(restart), int(max_iter), float(krylov_tol)
        self.ir = self.steps = self.cycles = 0
        self.residual_ratio = 0.0
        self.trace = []
        self._V = self._cols = None

    @staticmethod
    def dots(V, k, u):
        """(V_j . u for j < k, u . u): `mnk_ipm_krylov_dots`."""
        return [_osum(V[j] * u) for j in range(k)] + [_osum(u * u)]

    @staticmethod
    def project(u, V, k, coef):
        """u -= sum_j coef[j] V_j: `mnk_ipm_krylov_project`."""
        for j in range(k):
            u -= coef[j] * V[j]

    @staticmethod
    def axpy(x, V, k, y):
        """x += sum_j y[j] V_j: `mnk_ipm_krylov_axpy`."""
        for j in range(k):
            x += y[j] * V[j]

    def _basis(self, w):
        n = len(w.values)
        if self._V is None or self._V.shape[1] != n:
            self._V = np.zeros((self.restart + 1, n))
            self._cols = []
            for j in range(self.restart + 1):
                c = w.copy()
                c.values = self._V[j]
                self._cols.append(c)
        return self._V, self._cols

    def _ratio(self, x, b, w, norm_b):
        w.values[:] = b.values
        self.kkt.mul(w, x, -1.0, 1.0)
        norm_w = np.linalg.norm(w.values, np.inf)
        norm_x = np.linalg.norm(x.values, np.inf)
        return norm_w / (min(norm_x, 1e6 * norm_b) + norm_b)

    def solve_refine(self, x, b, w):
        norm_b = np.linalg.norm(b.values, np.inf)
        r = 0.0
        x.values[:] = 0.0
        self.ir = self.steps = self.cycles = 0
        self.trace = []
        if norm_b != 0:
            w.values[:] = b.values
            self.kkt.solve_kkt(w)            # cycle 0: Richardson's first step
            self.ir = 1
            x.values[:] = w.values
            beta0 = math.sqrt(_osum(w.values * w.values))
            r = self._ratio(x, b, w, norm_b)
            while not (r < self.richardson_tol or self.ir >= self.max_iter):
                self._cycle(x, w, beta0)
                r = self._ratio(x, b, w, norm_b)
        self.residual_ratio = r
        return r < self.richardson_acceptable_tol

    def _cycle(self, x, w, beta0):
        """One GMRES cycle from the residual in w.  With a single solve left a cycle cannot take a step (it needs two: the
        preconditioned residual and one Arnoldi step), so that solve is spent on a Richardson step."""
        kkt = self.kkt
        kkt.solve_kkt(w)                     # z = M^-1 (b - A x)
        self.ir += 1
        if self.ir >= self.max_iter:
            x.values += w.values
            return
        V, cols = self._basis(w)
        u = w.values
        beta = math.sqrt(_osum(u * u))
        self.cycles += 1
        cyc = GmresCycle(beta, self.restart)
        self.trace.append((beta, cyc.rho))
        if not beta > 0:
            return
        V[0] = u / beta
        for j in range(self.restart):
            k = j + 1
            kkt.mul(w, cols[j], 1.0, 0.0)
            kkt.solve_kkt(w)                 # u = M^-1 A v_j
            self.ir += 1
            self.steps += 1
            h1 = self.dots(V, k, u)
            self.project(u, V, k, h1)
            h2 = self.dots(V, k, u)
            self.project(u, V, k, h2)
            hn = math.sqrt(_osum(u * u))
            if hn != 0:
                V[k] = u / hn
            rho = cyc.add_column(h1, h2, hn)
            if rho <= self.krylov_tol * beta0 or hn == 0 or self.ir >= self.max_iter:
                break
        self.axpy(x.values, V, cyc.k, cyc.solution())

"""Dense quasi-Newton Hessians of the dense KKT systems: `hessian_approximation = BFGS / DampedBFGS` of the reference
(`src/quasi_newton.jl:72-206`), restated in numpy.

This is the host specification of the update and the comparator of the device path (`csrc/qn.hip`,
`kkt._DenseBase.qn_update_device`).  The approximation `B` is the n x n Hessian buffer of a dense KKT system.  Like the
reference (dsymv / dsyr with `'L'`) every routine reads and writes the LOWER triangle only: the strict upper triangle keeps
whatever it held.

    init        src/quasi_newton.jl:194-206     B's diagonal = 2 rho0 (Gilbert & Lemarechal), the rest zero
    BFGS        src/quasi_newton.jl:112-130     B -= bs bs' / s'bs ; B += y y' / s'y ; skipped when s'y < 1e-8
    DampedBFGS  src/quasi_newton.jl:163-192     Powell's damping (Nocedal & Wright, procedure 18.2), never skipped

`CompactLBFGS` (sparse KKT systems only in the reference) is not part of this project.
"""
from __future__ import annotations

import math

import numpy as np

HESSIAN_APPROXIMATIONS = ("exact", "bfgs", "damped_bfgs")
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


def create_quasi_newton(name, n):
    """`create_quasi_newton` quasi_newton.jl:94-110,144-161."""
    if name == "bfgs":
        return BFGS(n)
    if name == "damped_bfgs":
        return DampedBFGS(n)
    raise ValueError(f"hessian_approximation must be one of {HESSIAN_APPROXIMATIONS}, not {name!r}")

"""Fixed variables (`lvar[i] == uvar[i]`) treated as parameters: the reference's `MakeParameter`
(src/Callbacks/nlpmodels.jl:266-353 the handlers, :580-591 the dense initialization, :665-690 the reduced getters and
un-reduction, :912-1087 the callback wrappers and `update_z!`), selected by `IPMOptions.fixed_variable_treatment =
"make_parameter"`.  The default, `"relax_bound"`, is the reference's `RelaxBound`: the bounds are widened by
`bound_relax_factor` like any other pair and the variable lives in an interval of width ~2e-8.

One host layer for both drivers.  `FixedVariableHandler.create(nlp, sparse)` returns None for a model without fixed
variables (the reference's `NoFixedVariables`); otherwise the handler holds `free`, `fixed`, `ind_jac_free`, `ind_hess_free`,
`x_full`, `g_full` and a `model`: the view of the user's model the solver evaluates.

  sparse=True   (SparseCallback) `ReducedModel`: n = len(free), the COO structure without the entries of fixed columns /
                rows, renumbered; every callback evaluates the user's model at `x_full` and gathers.
  sparse=False  (DenseCallback)  `FrozenModel`: n unchanged, x0[fixed] = lvar[fixed], free bounds there, zero Jacobian
                columns, zero Hessian rows and columns with a unit diagonal; the solver writes grad[fixed] = x[fixed] -
                lvar[fixed] after its scaling.

The views return the model's RAW values: NLP scaling and the objective sense stay where they are, in the solver's `eval_*`."""
from __future__ import annotations

import numpy as np

TREATMENTS = ("relax_bound", "make_parameter")
GATHER_FREE, GATHER_JAC, GATHER_HESS = 0, 1, 2     # `which` of mnk_fix_gather (include/madnlp_hip.h)


def structure(nlp, info):
    """(jac_I, jac_J, hess_I, hess_J), 0-based, of the problem a `kkt_factory(info)` builds a KKT system for: the reduced
    arrays the solver put into `info` when variables were made parameters, the model's own otherwise."""
    return tuple(np.asarray(info[k] if k in info else getattr(nlp, k)) for k in ("jac_I", "jac_J", "hess_I", "hess_J"))


class ReducedModel:
    """The user's model over its free variables (SparseCallback + MakeParameter)."""

    def __init__(self, h, nlp):
        self._h, self._nlp = h, nlp
        self.n, self.m = len(h.free), nlp.m
        self.x0 = np.asarray(nlp.x0, float)[h.free]
        self.y0 = nlp.y0
        self.lvar, self.uvar = np.asarray(nlp.lvar, float)[h.free], np.asarray(nlp.uvar, float)[h.free]
        self.lcon, self.ucon = nlp.lcon, nlp.ucon
        self.jac_I, self.jac_J, self.hess_I, self.hess_J = h.jac_I, h.jac_J, h.hess_I, h.hess_J
        if hasattr(nlp, "minimize"):
            self.minimize = nlp.minimize

    def obj(self, x):
        return self._nlp.obj(self._h.expand(x))

    def grad(self, x):
        h = self._h
        h.g_full[:] = self._nlp.grad(h.expand(x))
        return h.g_full[h.free]

    def cons(self, x):
        return self._nlp.cons(self._h.expand(x))

    def jac_coord(self, x):
        return np.asarray(self._nlp.jac_coord(self._h.expand(x)))[self._h.ind_jac_free]

    def hess_coord(self, x, y, w=1.0):
        return np.asarray(self._nlp.hess_coord(self._h.expand(x), y, w))[self._h.ind_hess_free]


class FrozenModel:
    """The user's model with its fixed variables frozen in place (DenseCallback + MakeParameter).  `grad` is the model's
    own: the solver overwrites the fixed entries after scaling, as the reference's wrapper does."""

    def __init__(self, h, nlp):
        self._h, self._nlp = h, nlp
        self.n, self.m = nlp.n, nlp.m
        self.x0 = np.array(nlp.x0, dtype=float)
        self.lvar, self.uvar = np.array(nlp.lvar, dtype=float), np.array(nlp.uvar, dtype=float)
        self.x0[h.fixed] = h.values
        self.lvar[h.fixed] = -np.inf
        self.uvar[h.fixed] = np.inf
        self.y0, self.lcon, self.ucon = nlp.y0, nlp.lcon, nlp.ucon
        for k in ("jac_I", "jac_J", "hess_I", "hess_J", "minimize"):
            if hasattr(nlp, k):
                setattr(self, k, getattr(nlp, k))

    def obj(self, x):
        return self._nlp.obj(x)

    def grad(self, x):
        return self._nlp.grad(x)

    def cons(self, x):
        return self._nlp.cons(x)

    def jac_dense(self, x):
        J = np.array(self._nlp.jac_dense(x), dtype=float, order="F")
        J[:, self._h.fixed] = 0.0
        return J

    def hess_dense(self, x, y, w=1.0):
        return self._h.mask_hessian(np.array(self._nlp.hess_dense(x, y, w), dtype=float, order="F"))


class FixedVariableHandler:
    """`MakeParameter` (nlpmodels.jl:319-327, :343-351).  Index arrays are 0-based int64; `values` = lvar[fixed]."""

    def __init__(self, nlp, sparse):
        lvar, uvar = np.asarray(nlp.lvar, float), np.asarray(nlp.uvar, float)
        isfree = lvar < uvar
        self.sparse = bool(sparse)
        self.n_full = int(nlp.n)
        self.fixed = np.nonzero(lvar == uvar)[0].astype(np.int64)
        self.free = np.nonzero(isfree)[0].astype(np.int64)
        self.values = lvar[self.fixed].copy()
        self.g_full = np.zeros(self.n_full)
        if len(self.free) == 0:
            raise ValueError("fixed_variable_treatment = 'make_parameter': the model has no free variable (every lvar[i] == "
                             "uvar[i]); there is nothing to optimize")
        empty = np.zeros(0, dtype=np.int64)
        if self.sparse:
            jI, jJ, hI, hJ = (np.asarray(getattr(nlp, k), dtype=np.int64) for k in ("jac_I", "jac_J", "hess_I", "hess_J"))
            self.nnzj_full, self.nnzh_full = len(jI), len(hI)
            map_full_to_free = np.full(self.n_full, -1, dtype=np.int64)
            map_full_to_free[self.free] = np.arange(len(self.free))
            self.ind_jac_free = np.nonzero(isfree[jJ])[0].astype(np.int64)
            self.ind_hess_free = np.nonzero(isfree[hI] & isfree[hJ])[0].astype(np.int64)
            self.jac_I, self.jac_J = jI[self.ind_jac_free], map_full_to_free[jJ[self.ind_jac_free]]
            self.hess_I, self.hess_J = map_full_to_free[hI[self.ind_hess_free]], map_full_to_free[hJ[self.ind_hess_free]]
            self.x_full = lvar.copy()          # the fixed entries are written here and never again
            self.x_full[self.free] = np.asarray(nlp.x0, float)[self.free]
            self.model = ReducedModel(self, nlp)
        else:
            self.nnzj_full = self.nnzh_full = 0
            self.ind_jac_free, self.ind_hess_free = empty, empty
            self.x_full = np.zeros(0)
            self.model = FrozenModel(self, nlp)

    @classmethod
    def create(cls, nlp, sparse):
        """The handler, or None when no variable is fixed (`NoFixedVariables`)."""
        if not (np.asarray(nlp.lvar, float) == np.asarray(nlp.uvar, float)).any():
            return None
        return cls(nlp, sparse)

    def expand(self, x):
        """`_update_x!`: x_full[free] = x; returns x_full (the fixed entries keep lvar)."""
        self.x_full[self.free] = x
        return self.x_full

    def mask_hessian(self, H):
        """Zero rows and columns of the fixed variables, a unit diagonal there (nlpmodels.jl:1053-1056); in place."""
        H[:, self.fixed] = 0.0
        H[self.fixed, :] = 0.0
        H[self.fixed, self.fixed] = 1.0
        return H

    def dense_grad(self, g, x):
        """g[fixed] = x[fixed] - lvar[fixed] (nlpmodels.jl:1026-1031), after the solver's scaling."""
        g[self.fixed] = x[self.fixed] - self.values

    def structure_info(self):
        """What the solver adds to the dict its `kkt_factory` receives (sparse: the reduced COO structure)."""
        if not self.sparse:
            return {}
        return dict(jac_I=self.jac_I, jac_J=self.jac_J, hess_I=self.hess_I, hess_J=self.hess_J)

    # ------------------------------------------------------------------ un-reduction of a solution
    def unpack(self, nlp, x, zl, zu, y, obj_sign):
        """Full-length x, zl, zu from the solver's un-scaled ones (`unpack_x!`, `unpack_z!` :683-690) and `update_z!`
        (:1075-1087, src/IPM/utils.jl:62) for the fixed entries: g = grad f(x) + J(x)' y with the model's raw callbacks and
        the unpacked y; zl = max(0, obj_sign g), zu = max(0, -obj_sign g)."""
        if self.sparse:
            xf = self.x_full.copy()
            xf[self.free] = x
            zlf, zuf = np.zeros(self.n_full), np.zeros(self.n_full)
            zlf[self.free], zuf[self.free] = zl, zu
        else:
            xf, zlf, zuf = np.array(x), np.array(zl), np.array(zu)
        g = np.asarray(nlp.grad(xf), dtype=float) + model_jtprod(nlp, xf, y)
        gf = g[self.fixed]
        zlf[self.fixed] = np.maximum(0.0, obj_sign * gf)
        zuf[self.fixed] = np.maximum(0.0, -obj_sign * gf)
        return xf, zlf, zuf


def model_jtprod(nlp, x, y):
    """J(x)' y through the model's `jtprod` where it has one, else from its COO or dense Jacobian."""
    y = np.asarray(y, dtype=float)
    if hasattr(nlp, "jtprod"):
        return np.asarray(nlp.jtprod(x, y), dtype=float)
    if hasattr(nlp, "jac_coord") and hasattr(nlp, "jac_I"):
        out = np.zeros(nlp.n)
        jI, jJ = np.asarray(nlp.jac_I, dtype=np.int64), np.asarray(nlp.jac_J, dtype=np.int64)
        np.add.at(out, jJ, np.asarray(nlp.jac_coord(x), dtype=float) * y[jI])
        return out
    return np.asarray(nlp.jac_dense(x), dtype=float).T @ y

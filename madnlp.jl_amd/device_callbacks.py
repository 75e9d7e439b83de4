"""The device NLP callbacks of `ipm_dev.DeviceMadNLPSolver` (reference `eval_*_wrapper!`, src/IPM/callbacks.jl:1-96) and the one
layer that applies NLP scaling and the objective sense to them (src/Callbacks/nlpmodels.jl:766-836).  The solver hands its
callbacks one `DeviceScaling` at the upload and then asks `eval_f`, `eval_grad`, `eval_cons`, `eval_jac`, `eval_lag_hess` and,
for dense quasi-Newton, `eval_jtprod_at`.  The classes differ in how they answer: `DeviceCallbacks` from data scaled once on the
host (the two QP classes), `DeviceCOOCallbacks` with a scaling launch behind the model's raw values (AC-OPF, tapes),
`DeviceFixedVariableCallbacks` with the scaling fused into its gather.  Imports without a GPU and without the built library."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _up(a, dev, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _empty(dev, k):
    return torch.empty(max(k, 1), dtype=torch.float64, device=dev)[:k]       # (never a null pointer)


def _zeros(K, dev, k):
    """A zero-filled device vector of length k (`hv0`, `P0_cm`, `ybuf`)."""
    v = _empty(dev, k)
    if k:
        K.vec_fill(v, 0.0)
    return v


class _LibraryHandle:
    """Owner of one library handle `_h`, released by the entry named `_destroy`."""
    _destroy = _h = None

    def close(self):
        if self._h:
            getattr(L.lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScaling:
    """What the solver hands its callbacks, once: the layout (`n`, `ns`, device `ind_ineq` and `rhs`) and, when `scaled` (NLP
    scaling is on or the model maximizes), `obj_sign` and `obj_scale` (apart: the objective is multiplied by one after the other),
    `ybuf` for y .* con_scale and `slack_pos`, the inverse of `ind_ineq`: a row's slack, -1 for an equality row; None when every
    row owns its slack.  Device `con_scale` and `jac_scale` = con_scale[jac_I] stay None unless raw-value callbacks are attached."""

    def __init__(self, K, dev, n, ns, ind_ineq, rhs, scaled=False, obj_sign=1.0, obj_scale=1.0, con_scale=None, jac_scale=None):
        self.n, self.ns, self.rhs, self.scaled, self.obj_sign, self.obj_scale = n, ns, rhs, scaled, obj_sign, obj_scale
        self.ind_ineq = _up(ind_ineq, dev, np.int64)
        self.host_scales = (con_scale, jac_scale)
        self.con_scale = self.jac_scale = self.ybuf = self.slack_pos = None
        if scaled:
            self.ybuf = _zeros(K, dev, rhs.numel())
            if 0 < ns < rhs.numel():
                pos = np.full(rhs.numel(), -1, dtype=np.int64)
                pos[ind_ineq] = np.arange(ns)
                self.slack_pos = _up(pos, dev, np.int64)

    def host_factors(self):
        """What prescaled callbacks multiply into their data: the constructor arguments of the two QP classes."""
        return dict(obj_factor=self.obj_sign * self.obj_scale, con_scale=self.host_scales[0]) if self.scaled else {}


class DeviceCallbacks(_LibraryHandle):
    """The solver-facing calls, as data that carry their factors already (`prescaled`) answer them: nothing is applied to what
    `obj`, `grad`, `cons`, `load_jac`, `load_hess` give.  `x` is the solver's iterate, slacks behind the `n` variables."""
    prescaled = True

    def attach(self, scaling):
        self.sc = s = scaling
        if s.scaled and not self.prescaled:            # raw values: the factors are applied on the device
            s.con_scale, s.jac_scale = (_up(a, s.rhs.device) for a in s.host_scales)

    def eval_f(self, x):
        return self.obj(x[:self.sc.n])

    def eval_grad(self, f, x):
        n = self.sc.n
        self.grad(f[:n], x[:n])
        self.K.vec_fill(f[n:], 0.0)

    def eval_cons(self, c, x):
        s, K = self.sc, self.K
        self.cons(c, x[:s.n])
        slack = x[s.n:]
        if s.scaled:                                   # c .* con_scale - slack - rhs in one launch
            return K.scale_cons(c, s.con_scale, slack, s.slack_pos, s.rhs)
        if s.ns == c.numel():
            K.vec_axpby(c, 1.0, c, -1.0, slack)        # ind_ineq = all constraints, in order
        else:
            K.vec_scatter_axpy(c, s.ind_ineq, -1.0, slack)
        K.vec_axpby(c, 1.0, c, -1.0, s.rhs)

    def eval_jac(self, x):
        self.load_jac(x[:self.sc.n])

    def eval_lag_hess(self, x, y, w):
        self.load_hess(x[:self.sc.n], y, w)

    def eval_jtprod_at(self, x, y, out_x):
        """out_x = J(x)' y for the quasi-Newton secant pair (`_eval_jtprod_wrapper!`, callbacks.jl:172)."""
        self.jtprod_at(x, self._model_y(y), out_x)

    def _model_y(self, y):
        return y


class DeviceCOOCallbacks(DeviceCallbacks):
    """Callbacks that compute the model's raw COO values (`jac_coord`, `hess_coord` into `jv`, `hv`) for the compressors of the
    sparse condensed handle, or of a dense handle with the COO structure attached (`kkt.coo_attached`, csrc/dense_coo.hip); J'y
    is the handle's transposed product on the Jacobian values it holds.  Scaling and the sense are launches behind the raw
    values: `scale_grad`, `vec_mul` by `jac_scale`; the model gets y .* con_scale (nlpmodels.jl:791-801) and w obj_sign obj_scale."""
    prescaled = False

    def jtprod_x(self, out_x, y):
        if getattr(self.kkt, "coo_attached", False):
            return self.kkt.jtprod_coo_device(L.MNK_DC_JAC_CURRENT, y, out_x)
        self.kkt.spmv_device(L.MNK_SC_JT, 0, 1.0, y, 0.0, out_x)

    def load_jac(self, x):
        self.kkt.compress_jacobian(self.jac_coord(x))

    def load_hess(self, x, y, sigma=1.0):
        self.kkt.compress_hessian(self.hess_coord(x, y, sigma))

    def zero_hess(self):
        self.kkt.compress_hessian(self.hv0)

    def eval_f(self, x):
        return self.sc.obj_sign * (self.obj(x[:self.sc.n]) * self.sc.obj_scale)

    def eval_grad(self, f, x):
        s = self.sc
        if not s.scaled:
            return super().eval_grad(f, x)
        self.grad(f[:s.n], x[:s.n])
        self.K.scale_grad(f, s.n, s.obj_sign * s.obj_scale)     # the factor and the zero slack part in one launch

    def eval_jac(self, x):
        jv = self.jac_coord(x[:self.sc.n])
        if self.sc.scaled:
            self.K.vec_mul(jv, jv, self.sc.jac_scale)
        self.kkt.compress_jacobian(jv)

    def eval_lag_hess(self, x, y, w):
        s = self.sc
        self.load_hess(x[:s.n], self._model_y(y), w * s.obj_sign * s.obj_scale)

    def _model_y(self, y):
        if not self.sc.scaled:
            return y
        self.K.vec_mul(self.sc.ybuf, y, self.sc.con_scale)
        return self.sc.ybuf


class DeviceHessianProduct(_LibraryHandle):
    """out = Symmetric(H, :L) x on the device for a fixed sparse H: a bare `mnk_sc` handle (no constraints, no solver) that is
    used for its compressed Hessian and `mnk_sc_spmv` only.  `DeviceQPCallbacks` evaluates the objective through the KKT
    handle's own Hessian; under a quasi-Newton method that handle holds the approximation, and the model's H lives here."""
    _destroy = "mnk_sc_destroy"

    def __init__(self, ctx, n, hess_I, hess_J, hv):
        hI, hJ = np.ascontiguousarray(hess_I, dtype=np.int32), np.ascontiguousarray(hess_J, dtype=np.int32)
        e = np.zeros(1, dtype=np.int32)
        self._h = C.c_void_p()
        L.check(L.lib().mnk_sc_create(ctx.handle, int(n), 0, 0, e.ctypes.data, e.ctypes.data, len(hI), hI.ctypes.data,
                                      hJ.ctypes.data, 0, C.byref(self._h)), "mnk_sc_create")
        L.check(L.lib().mnk_sc_compress_hessian(self._h, hv.data_ptr(), L.MNK_DEVICE), "mnk_sc_compress_hessian")

    def mul(self, x, out):
        L.check(L.lib().mnk_sc_spmv(self._h, L.MNK_SC_HESS, 0, 1.0, x.data_ptr(), 0.0, out.data_ptr()), "mnk_sc_spmv")


class _DevicePointer:
    """A device vector the library owns, as the callbacks take their arguments: by address."""

    def __init__(self, ptr, n):
        self._ptr, self._n = int(ptr), int(n)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


class DeviceFixedVariables(_LibraryHandle):
    """The `mnk_fix` handle (csrc/fixed_vars.hip) of a host `fixed_vars.FixedVariableHandler`: its index sets and the fixed
    values uploaded once, and the device `x_full` the handle owns.  Every call is one asynchronous launch on the context's
    stream."""
    _destroy = "mnk_fix_destroy"

    def __init__(self, ctx, handler):
        h = handler
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)   # noqa: E731
        free, fixed, ij, ih = i64(h.free), i64(h.fixed), i64(h.ind_jac_free), i64(h.ind_hess_free)
        val = np.ascontiguousarray(h.values, dtype=np.float64)
        self.n, self.nfree, self.nfixed, self.njac, self.nhess = h.n_full, len(free), len(fixed), len(ij), len(ih)
        self._h = C.c_void_p()
        L.check(L.lib().mnk_fix_create(ctx.handle, h.n_full, len(free), free.ctypes.data, len(fixed), fixed.ctypes.data,
                                       val.ctypes.data, h.nnzj_full, len(ij), ij.ctypes.data, h.nnzh_full, len(ih),
                                       ih.ctypes.data, C.byref(self._h)), "mnk_fix_create")
        self.x_full = _DevicePointer(L.lib().mnk_fix_x_full(self._h), h.n_full)

    def expand(self, x):
        assert x.numel() == self.nfree
        L.check(L.lib().mnk_fix_expand(self._h, x.data_ptr()), "mnk_fix_expand")
        return self.x_full

    def gather(self, which, src_full, dst, scale=None, factor=1.0):
        count = (self.nfree, self.njac, self.nhess)[which]
        assert dst.numel() == count and (scale is None or scale.numel() == count)
        L.check(L.lib().mnk_fix_gather(self._h, which, src_full.data_ptr(), None if scale is None else scale.data_ptr(),
                                       float(factor), dst.data_ptr()), "mnk_fix_gather")

    def dense_grad(self, g, x):
        assert g.numel() >= self.n and x.numel() >= self.n
        L.check(L.lib().mnk_fix_dense_grad(self._h, g.data_ptr(), x.data_ptr()), "mnk_fix_dense_grad")

    def x_full_host(self):
        """x_full downloaded (synchronizes; tests and reporting)."""
        out = np.empty(self.n)
        L.check(L.lib().mnk_fix_get_x_full(self._h, out.ctypes.data), "mnk_fix_get_x_full")
        return out


class _QuadraticCallbacks(DeviceCallbacks):
    """f = 0.5 x'Hx + q'x with linear constraints: `_hmul(x)` is the subclass's H x; the Lagrangian Hessian is sigma H: the
    uploaded H under objective weight 1, zero under 0, a scaled copy (`_weighted`, one launch into scratch) under any other
    weight.  `handle_has_H` says whether the KKT handle holds H itself, `_held` what it holds otherwise."""
    handle_has_H = True
    _held = _scratch = None
    H = fix = None                     # what a subclass owns besides its tensors: a `DeviceHessianProduct`, a `DeviceFixedVariables`

    def _weighted(self, sigma, full, zero, masked):
        """The source of the Lagrangian Hessian sigma H: `zero`, `full`, or sigma * `full` in scratch.  `masked`: `zero` carries
        the unit diagonal of frozen variables, which the weight must not touch: sigma (full - zero) + zero."""
        if sigma == 0.0 or sigma == 1.0:
            return zero if sigma == 0.0 else full
        if self._scratch is None:
            self._scratch = torch.empty_like(full)
        if masked:
            self.K.vec_axpby(self._scratch, sigma, full, -sigma, zero)
            self.K.vec_axpby(self._scratch, 1.0, self._scratch, 1.0, zero)
        else:
            self.K.vec_axpby(self._scratch, sigma, full)
        return self._scratch

    def obj(self, x):
        hx = self._hmul(x)
        with self.K.batch():
            a = self.K.get_dot(x, hx)
            b = self.K.get_dot(self.q, x)
        return 0.5 * a[0] + b[0]

    def zero_hess(self):
        self.load_hess(sigma=0.0)

    def close(self):
        for part in (self.H, self.fix):
            if part is not None:
                part.close()


class DeviceQPCallbacks(_QuadraticCallbacks):
    """f = 0.5 x'Hx + q'x, c = Jx with H = Symmetric(hess_com, :L) and J = jt_csc' held by the KKT handle.  The data ARE the
    handle's, so NLP scaling and the sense go into them once, on the host (`prescaled`): H and q times `obj_factor` = obj_sign
    obj_scale, the rows of J times `con_scale`."""

    def __init__(self, nlp, kkt, dev, K, obj_factor=1.0, con_scale=None, own_hessian=False):
        """`own_hessian`: the KKT handle's Hessian is a quasi-Newton approximation; H gets a `DeviceHessianProduct`."""
        self.kkt, self.K, self.n, self.m = kkt, K, nlp.n, nlp.m
        q, hv = np.asarray(nlp.q, float) * obj_factor, np.asarray(nlp.hess_coord(None, None, 1.0), float) * obj_factor
        jv = np.asarray(nlp.jac_coord(None), float)
        if con_scale is not None:
            jv = jv * con_scale[np.asarray(nlp.jac_I, dtype=np.int64)]
        self.q, self.jv, self.hv = _up(q, dev), _up(jv, dev), _up(hv, dev)
        self.hv0 = _zeros(K, dev, len(hv))
        self._hx = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.H = DeviceHessianProduct(kkt.ctx, nlp.n, nlp.hess_I, nlp.hess_J, self.hv) if own_hessian else None

    def _hmul(self, x):
        if self.H is not None:
            self.H.mul(x, self._hx)
            return self._hx
        # the SpMV runs on the handle's compressed Lagrangian Hessian: while that holds something else (zero after
        # initialize!(kkt), objective weight 0 in robust!, another weight) H is put back for the product, then what was held
        if not self.handle_has_H:
            self.kkt.compress_hessian(self.hv)
        self.kkt.spmv_device(L.MNK_SC_HESS, 0, 1.0, x, 0.0, self._hx)
        if not self.handle_has_H:
            self.kkt.compress_hessian(self._held)
        return self._hx

    def grad(self, g, x):
        self.K.vec_axpby(g, 1.0, self._hmul(x), 1.0, self.q)

    def cons(self, c, x):
        self.kkt.spmv_device(L.MNK_SC_JT, 1, 1.0, x, 0.0, c)

    def jtprod_x(self, out_x, y):
        self.kkt.spmv_device(L.MNK_SC_JT, 0, 1.0, y, 0.0, out_x)

    def load_jac(self, x=None):
        self.kkt.compress_jacobian(self.jv)

    def load_hess(self, x=None, y=None, sigma=1.0):
        self._held = self._weighted(sigma, self.hv, self.hv0, False)      # linear constraints: the Lagrangian Hessian is sigma H
        self.kkt.compress_hessian(self._held)
        self.handle_has_H = sigma == 1.0


class DeviceDenseQPCallbacks(_QuadraticCallbacks):
    """f = 0.5 x'Px + q'x, c = Ax with dense P, A on the device (`DenseQPModel`); Hessian / Jacobian of the KKT handle are
    loaded from these device copies (`mnk_dc_set_hess` / `mnk_dc_set_jac` with device pointers).  `prescaled` as
    `DeviceQPCallbacks`: P and q are uploaded times `obj_factor`, the rows of A times `con_scale`."""

    def __init__(self, nlp, kkt, dev, K, obj_factor=1.0, con_scale=None, fixed=None):
        """`fixed`: the host `FixedVariableHandler` of variables frozen in place (MakeParameter on a dense system).  The KKT
        handle is then loaded from masked copies made once, here -- zero Jacobian columns, zero Hessian rows and columns with a
        unit diagonal, also under objective weight 0 --, J'y uses the masked A, while f, grad f and c keep the model's own P
        and A and `grad` ends with `mnk_fix_dense_grad`."""
        self.kkt, self.K, self.n, self.m = kkt, K, nlp.n, nlp.m
        P, A, q = np.asarray(nlp.P, float) * obj_factor, np.asarray(nlp.A, float), np.asarray(nlp.q, float) * obj_factor
        if con_scale is not None:
            A = A * con_scale[:, None]
        # column-major device images (a row-major upload of the transpose IS the column-major matrix)
        self.P_cm = _up(P.T, dev)
        self.A_cm = _up(A.T, dev)        # (n, m) row-major == (m, n) column-major
        self.q = _up(q, dev)
        if fixed is None:
            self.P_kkt_cm, self.A_kkt_cm = self.P_cm, self.A_cm
            self.P0_cm = _zeros(K, dev, P.size).view(P.shape)
        else:
            Am = np.array(A)
            Am[:, fixed.fixed] = 0.0
            self.P_kkt_cm = _up(fixed.mask_hessian(np.array(P)).T, dev)
            self.A_kkt_cm = _up(Am.T, dev)
            self.P0_cm = _up(fixed.mask_hessian(np.zeros_like(P)), dev)
            self.fix = DeviceFixedVariables(K.ctx, fixed)
        self._px = torch.empty(self.n, dtype=torch.float64, device=dev)

    def _hmul(self, x, out=None):
        out = self._px if out is None else out
        self.K.gemv(0, self.n, self.n, 1.0, self.P_cm, self.n, x, 0.0, out)
        return out

    def grad(self, g, x):
        self._hmul(x, g)
        self.K.vec_axpby(g, 1.0, g, 1.0, self.q)
        if self.fix is not None:
            self.fix.dense_grad(g, x)

    def cons(self, c, x):
        if self.m > 0:
            self.K.gemv(0, self.m, self.n, 1.0, self.A_cm, self.m, x, 0.0, c)

    def jtprod_x(self, out_x, y):
        if self.m > 0:
            self.K.gemv(1, self.m, self.n, 1.0, self.A_kkt_cm, self.m, y, 0.0, out_x)
        else:
            self.K.vec_fill(out_x, 0.0)

    def jtprod_at(self, x, y, out_x):
        """out_x = J(x)' y; the constraints are linear: `x` is not used."""
        self.jtprod_x(out_x, y)

    def load_jac(self, x=None):
        if self.m > 0:
            L.check(L.lib().mnk_dc_set_jac(self.kkt._h, self.A_kkt_cm.data_ptr(), self.m, L.MNK_DEVICE), "mnk_dc_set_jac")

    def load_hess(self, x=None, y=None, sigma=1.0):
        src = self._held = self._weighted(sigma, self.P_kkt_cm, self.P0_cm, self.fix is not None)
        L.check(L.lib().mnk_dc_set_hess(self.kkt._h, src.data_ptr(), self.n, L.MNK_DEVICE), "mnk_dc_set_hess")
        self.handle_has_H = sigma == 1.0


class DeviceOPFCallbacks(DeviceCOOCallbacks):
    """Callbacks of `problems.ACOPFModel` on the device (`mnk_opf_*`, csrc/opf_eval.hip): objective, gradient, constraints,
    Jacobian and Lagrangian-Hessian COO values are computed from the device iterate and handed to the KKT handle's
    compressors without leaving HBM."""
    _destroy = "mnk_opf_destroy"

    def __init__(self, nlp, kkt, dev, K):
        self.kkt, self.K, self.n, self.m = kkt, K, nlp.n, nlp.m
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)   # noqa: E731
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        fr, to, gb, coef, bus, cost = i32(nlp.fr), i32(nlp.to), i32(nlp.gen_bus), f64(nlp.arc_coef), f64(nlp.bus_data), f64(nlp.gen_cost)
        self._h = C.c_void_p()
        L.check(L.lib().mnk_opf_create(K.ctx.handle, nlp.nbus, nlp.ngen, nlp.nbr, fr.ctypes.data, to.ctypes.data, gb.ctypes.data,
                                       coef.ctypes.data, bus.ctypes.data, cost.ctypes.data, C.byref(self._h)), "mnk_opf_create")
        sz = [C.c_int64() for _ in range(4)]
        L.check(L.lib().mnk_opf_sizes(self._h, *[C.byref(v) for v in sz]), "mnk_opf_sizes")
        assert (sz[0].value, sz[1].value, sz[2].value, sz[3].value) == (nlp.n, nlp.m, len(nlp.jac_I), len(nlp.hess_I))
        self.jv, self.hv, self.terms = _empty(dev, len(nlp.jac_I)), _empty(dev, len(nlp.hess_I)), _empty(dev, nlp.ngen)
        self.hv0 = _zeros(K, dev, len(nlp.hess_I))

    def obj(self, x):
        L.check(L.lib().mnk_opf_obj_terms(self._h, x.data_ptr(), self.terms.data_ptr()), "mnk_opf_obj_terms")
        return self.K.get_sum(self.terms)

    def grad(self, g, x):
        L.check(L.lib().mnk_opf_grad(self._h, x.data_ptr(), g.data_ptr()), "mnk_opf_grad")

    def cons(self, c, x):
        L.check(L.lib().mnk_opf_cons(self._h, x.data_ptr(), c.data_ptr()), "mnk_opf_cons")

    def jac_coord(self, x):
        L.check(L.lib().mnk_opf_jac_coord(self._h, x.data_ptr(), self.jv.data_ptr()), "mnk_opf_jac_coord")
        return self.jv

    def hess_coord(self, x, y, sigma=1.0):
        L.check(L.lib().mnk_opf_hess_coord(self._h, x.data_ptr(), y.data_ptr(), float(sigma), self.hv.data_ptr()),
                "mnk_opf_hess_coord")
        return self.hv


class DeviceTapeCallbacks(DeviceCOOCallbacks):
    """Callbacks of ANY model written as patterns (`tape_model.TapeModel`) on the device (`mnk_tape_*`, csrc/tape_eval.hip): the
    model's expression tapes are handed to the library once; objective terms, gradient, constraints, Jacobian and
    Lagrangian-Hessian COO values are then interpreted from the device iterate, in the model's own COO order (the KKT handle is
    created from the model's `jac_I .. hess_J`)."""
    _destroy = "mnk_tape_destroy"

    def __init__(self, nlp, kkt, dev, K):
        nlp.finalize()
        self.kkt, self.K, self.n, self.m = kkt, K, nlp.n, nlp.m
        lib = L.lib()
        self._h = C.c_void_p()
        L.check(lib.mnk_tape_create(K.ctx.handle, nlp.n, nlp.m, C.byref(self._h)), "mnk_tape_create")
        try:
            for p in nlp.patterns:
                args = []
                for t in p.tapes:
                    args += [len(t.code), t.code.ctypes.data, len(t.consts), t.consts.ctypes.data, t.nout, t.out_operand.ctypes.data,
                             t.out_j.ctypes.data, t.out_l.ctypes.data, t.nslot]
                L.check(lib.mnk_tape_add_pattern(self._h, p.kind, p.R, p.k, p.q, p.var_index.ctypes.data, p.params.ctypes.data,
                                                 p.rows.ctypes.data if p.kind == 1 else None, *args), "mnk_tape_add_pattern")
            L.check(lib.mnk_tape_finalize(self._h), "mnk_tape_finalize")
            sz = [C.c_int64() for _ in range(5)]
            L.check(lib.mnk_tape_sizes(self._h, *[C.byref(v) for v in sz]), "mnk_tape_sizes")
            nnzj, nnzh = len(nlp.jac_I), len(nlp.hess_I)
            if tuple(v.value for v in sz) != (nlp.n, nlp.m, nlp.nterms, nnzj, nnzh):
                raise RuntimeError(f"mnk_tape_sizes {tuple(v.value for v in sz)} differs from the host model's "
                                   f"{(nlp.n, nlp.m, nlp.nterms, nnzj, nnzh)}")
            st = [np.zeros(max(k, 1), dtype=np.int32) for k in (nnzj, nnzj, nnzh, nnzh)]
            L.check(lib.mnk_tape_get_structure(self._h, *[a.ctypes.data for a in st]), "mnk_tape_get_structure")
            for name, a, b in zip(("jac_I", "jac_J", "hess_I", "hess_J"), st, (nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J)):
                if not np.array_equal(a[:len(b)], b):   # (values would land in the wrong KKT entries)
                    raise RuntimeError(f"the library's COO structure ({name}) differs from the host model's")
        except Exception:
            self.close()
            raise
        self.jv, self.hv, self.terms = _empty(dev, nnzj), _empty(dev, nnzh), _empty(dev, nlp.nterms)
        self.hv0 = _zeros(K, dev, nnzh)

    EXT_OBJ, EXT_GRAD, EXT_CONS, EXT_JAC, EXT_HESS = 1, 2, 4, 8, 16

    def extended(self):
        """Which callback launches run the interpreter kernel that knows the opcodes from 16 on -- pow tan atan tanh abs sign step
        min max -- (`mnk_tape_extended`): the sum of EXT_OBJ .. EXT_HESS; 0 for a model that uses none of them."""
        mask = C.c_int(-1)
        L.check(L.lib().mnk_tape_extended(self._h, C.byref(mask)), "mnk_tape_extended")
        return mask.value

    def obj_terms(self, x):
        L.check(L.lib().mnk_tape_obj_terms(self._h, x.data_ptr(), self.terms.data_ptr()), "mnk_tape_obj_terms")
        return self.terms

    def obj(self, x):
        return self.K.get_sum(self.obj_terms(x)) if len(self.terms) else 0.0

    def grad(self, g, x):
        L.check(L.lib().mnk_tape_grad(self._h, x.data_ptr(), g.data_ptr()), "mnk_tape_grad")

    def cons(self, c, x):
        L.check(L.lib().mnk_tape_cons(self._h, x.data_ptr(), c.data_ptr()), "mnk_tape_cons")

    def jac_coord(self, x):
        L.check(L.lib().mnk_tape_jac_coord(self._h, x.data_ptr(), self.jv.data_ptr()), "mnk_tape_jac_coord")
        return self.jv

    def hess_coord(self, x, y, sigma=1.0):
        L.check(L.lib().mnk_tape_hess_coord(self._h, x.data_ptr(), y.data_ptr(), float(sigma), self.hv.data_ptr()),
                "mnk_tape_hess_coord")
        return self.hv


class DeviceFixedVariableCallbacks(DeviceCOOCallbacks):
    """Any `DeviceCOOCallbacks` object built on the FULL model, seen over the free variables of a
    `fixed_vars.FixedVariableHandler` (MakeParameter on the sparse condensed system; reference nlpmodels.jl:912-1013).  Every call
    expands the reduced iterate into the handle's `x_full` (one launch), runs the inner callback at full length into full-length
    scratch, and gathers the reduced values (one launch; objective and constraints need none).  `fused_scaling`: `grad` takes the
    objective factor and `jac_coord` the per-entry constraint scale, applied inside the gather: no `vec_mul` / `scale_grad` follows."""
    fused_scaling = True

    def __init__(self, inner, handler, kkt, dev, K):
        assert not inner.prescaled, "the wrapped callbacks must return the model's raw values"
        self.inner, self.kkt, self.K = inner, kkt, K
        self.n, self.m = len(handler.free), inner.m
        self.fix = DeviceFixedVariables(K.ctx, handler)
        self.g_full, self.jv, self.hv = _empty(dev, handler.n_full), _empty(dev, self.fix.njac), _empty(dev, self.fix.nhess)
        self.hv0 = _zeros(K, dev, self.fix.nhess)

    def obj(self, x):
        return self.inner.obj(self.fix.expand(x))

    def grad(self, g, x, factor=1.0):
        self.inner.grad(self.g_full, self.fix.expand(x))
        self.fix.gather(L.MNK_FIX_FREE, self.g_full, g, None, factor)

    def cons(self, c, x):
        self.inner.cons(c, self.fix.expand(x))

    def jac_coord(self, x, scale=None):
        self.fix.gather(L.MNK_FIX_JAC, self.inner.jac_coord(self.fix.expand(x)), self.jv, scale)
        return self.jv

    def hess_coord(self, x, y, sigma=1.0):
        self.fix.gather(L.MNK_FIX_HESS, self.inner.hess_coord(self.fix.expand(x), y, sigma), self.hv)
        return self.hv

    def eval_grad(self, f, x):
        s = self.sc
        self.grad(f[:s.n], x[:s.n], s.obj_sign * s.obj_scale if s.scaled else 1.0)
        self.K.vec_fill(f[s.n:], 0.0)

    def eval_jac(self, x):
        self.kkt.compress_jacobian(self.jac_coord(x[:self.sc.n], self.sc.jac_scale))

    def close(self):
        self.fix.close()
        self.inner.close()


def callbacks_class(nlp, sparse, callback="auto"):
    """The device callbacks of a model: by what the model is, not by what the run needs.  `callback` is `IPMOptions.callback`:
    with "sparse" the COO classes feed a dense handle too."""
    if getattr(nlp, "is_tape_model", False):
        return DeviceTapeCallbacks
    if hasattr(nlp, "arc_coef"):
        assert sparse or callback == "sparse", "the AC-OPF callbacks feed the sparse condensed handle, or a dense one with callback = 'sparse'"
        return DeviceOPFCallbacks
    return DeviceQPCallbacks if sparse else DeviceDenseQPCallbacks


def device_callbacks(nlp, kkt, dev, K, sparse, scaling, fixed=None, own_hessian=False, callback="auto"):
    """The callbacks object of a run, attached to the solver's `DeviceScaling`.  `nlp` is the FULL model; `fixed` (the host
    handler of variables made parameters) wraps raw-value callbacks and masks the dense QP's; `own_hessian`: compact L-BFGS."""
    cls = callbacks_class(nlp, sparse, callback)
    if cls is DeviceQPCallbacks:
        cb = cls(nlp, kkt, dev, K, own_hessian=own_hessian, **scaling.host_factors())
    elif cls is DeviceDenseQPCallbacks:
        cb = cls(nlp, kkt, dev, K, fixed=fixed, **scaling.host_factors())
    else:
        cb = cls(nlp, kkt, dev, K)
        if fixed is not None:
            cb = DeviceFixedVariableCallbacks(cb, fixed, kkt, dev, K)
    cb.attach(scaling)
    return cb

"""The scaling layer of `madnlp_jl_amd.device_callbacks` on CPU tensors: which launches the solver-facing calls (`eval_f`,
`eval_grad`, `eval_cons`, `eval_jac`, `eval_lag_hess`, `eval_jtprod_at`) make, in which order and on which buffers, for callbacks
of raw values, for prescaled data and for the fixed-variable wrapper, scaled and unscaled, with every row owning a slack
(ns == m) and with an equality row (ns < m).  `K`, the KKT handle and the `mnk_fix` handle are recording doubles: no library, no
GPU.  n = 3, m = 2."""
import types

import numpy as np
import pytest
import torch

from madnlp_jl_amd import _lib as L
from madnlp_jl_amd import device_callbacks as D

N, M = 3, 2
SIGN, SCALE = -1.0, 0.1
CON_SCALE = np.array([0.5, 0.25])
JAC_I = np.array([0, 0, 1, 1])
JAC_SCALE = CON_SCALE[JAC_I]


def key(a):
    """A tensor as (address, length) -- a slice is recognized by where it starts --, anything else as it is."""
    return ("tensor", a.data_ptr(), a.numel()) if hasattr(a, "data_ptr") else a


class Recorder:
    """Every method call lands in the shared `log` as (name, *arguments)."""

    def __init__(self, log, names):
        for name in names:
            setattr(self, name, lambda *a, _n=name: log.append((_n,) + tuple(key(v) for v in a)))


def doubles():
    log = []
    K = Recorder(log, ("vec_fill", "vec_axpby", "vec_scatter_axpy", "vec_mul", "scale_grad", "scale_cons", "gemv"))
    kkt = Recorder(log, ("compress_jacobian", "compress_hessian", "spmv_device"))
    return log, K, kkt


class RawStub(D.DeviceCOOCallbacks):
    """Raw values: every model callback is recorded; `jv`, `hv`, `hv0` as the real classes hold them."""

    def __init__(self, log, kkt, K):
        self.log, self.kkt, self.K, self.n, self.m, self.value = log, kkt, K, N, M, 3.0
        self.jv, self.hv, self.hv0 = torch.zeros(4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)

    def obj(self, x):
        self.log.append(("obj", key(x)))
        return self.value

    def grad(self, g, x):
        self.log.append(("grad", key(g), key(x)))

    def cons(self, c, x):
        self.log.append(("cons", key(c), key(x)))

    def jac_coord(self, x):
        self.log.append(("jac_coord", key(x)))
        return self.jv

    def hess_coord(self, x, y, sigma=1.0):
        self.log.append(("hess_coord", key(x), key(y), sigma))
        return self.hv


class TinyQP:
    """What the two QP callbacks read of a model."""
    n, m = N, M
    q = np.array([1.0, -2.0, 3.0])
    jac_I, jac_J = JAC_I, np.array([0, 1, 1, 2])
    hess_I, hess_J = np.array([0, 1, 2]), np.array([0, 1, 2])
    P = np.diag([2.0, 3.0, 4.0])
    A = np.array([[1.0, 2.0, 0.0], [0.0, -1.0, 5.0]])

    def jac_coord(self, x): return np.array([1.0, 2.0, -1.0, 5.0])
    def hess_coord(self, x, y, w): return np.array([2.0, 3.0, 4.0]) * w


class Setting:
    """The solver's vectors and the `DeviceScaling` it would hand over."""

    def __init__(self, K, ns, scaled):
        f64 = lambda k: torch.zeros(k, dtype=torch.float64)  # noqa: E731
        self.x, self.f, self.c, self.y, self.rhs, self.out = f64(N + ns), f64(N + ns), f64(M), f64(M), f64(M), f64(N)
        self.ns, self.ind_ineq = ns, np.arange(M)[M - ns:]
        self.sc = D.DeviceScaling(K, "cpu", N, ns, self.ind_ineq, self.rhs, scaled, *((SIGN, SCALE) if scaled else (1.0, 1.0)),
                                  CON_SCALE if scaled else np.ones(M), JAC_SCALE if scaled else np.ones(4))

    def cons_tail(self):
        """The launches behind `cons`, as DESIGN.md section 15 lists them."""
        s, c, slack = self.sc, key(self.c), key(self.x[N:])
        if s.scaled:
            return [("scale_cons", c, key(s.con_scale), slack, key(s.slack_pos), key(self.rhs))]
        first = ("vec_axpby", c, 1.0, c, -1.0, slack) if self.ns == M else ("vec_scatter_axpy", c, key(s.ind_ineq), -1.0, slack)
        return [first, ("vec_axpby", c, 1.0, c, -1.0, key(self.rhs))]


CASES = [(ns, scaled) for ns in (1, 2) for scaled in (True, False)]


@pytest.mark.parametrize("ns,scaled", CASES)
def test_scaling_object_holds_what_the_solver_hands_over(ns, scaled):
    log, K, _ = doubles()
    s = Setting(K, ns, scaled)
    sc = s.sc
    assert (sc.n, sc.ns, sc.scaled) == (N, ns, scaled) and sc.rhs is s.rhs
    assert sc.ind_ineq.dtype == torch.int64 and sc.ind_ineq.tolist() == list(s.ind_ineq)
    assert sc.con_scale is None and sc.jac_scale is None           # until callbacks of raw values are attached
    if not scaled:
        assert sc.ybuf is None and sc.slack_pos is None and log == [] and sc.host_factors() == {}
        return
    assert (sc.obj_sign, sc.obj_scale) == (SIGN, SCALE)             # kept apart
    assert sc.ybuf.numel() == M and log == [("vec_fill", key(sc.ybuf), 0.0)]
    assert (sc.slack_pos is None) if ns == M else (sc.slack_pos.tolist() == [-1, 0])
    hf = sc.host_factors()
    assert hf["obj_factor"] == SIGN * SCALE and hf["con_scale"] is CON_SCALE


@pytest.mark.parametrize("ns,scaled", CASES)
def test_raw_value_callbacks(ns, scaled):
    log, K, kkt = doubles()
    s = Setting(K, ns, scaled)
    cb = RawStub(log, kkt, K)
    cb.attach(s.sc)
    sc, x, xn = s.sc, s.x, key(s.x[:N])
    if scaled:
        assert sc.con_scale.tolist() == list(CON_SCALE) and sc.jac_scale.tolist() == list(JAC_SCALE)
    else:
        assert sc.con_scale is None and sc.jac_scale is None
    mark = len(log)
    cb.eval_grad(s.f, x)
    tail = ("scale_grad", key(s.f), N, SIGN * SCALE) if scaled else ("vec_fill", key(s.f[N:]), 0.0)
    assert log[mark:] == [("grad", key(s.f[:N]), xn), tail]
    mark = len(log)
    cb.eval_cons(s.c, x)
    assert log[mark:] == [("cons", key(s.c), xn)] + s.cons_tail()
    if scaled:
        assert log[-1][2] == key(sc.con_scale) != key(None) and (log[-1][4] is None) == (ns == M)
    mark = len(log)
    cb.eval_jac(x)
    scale = [("vec_mul", key(cb.jv), key(cb.jv), key(sc.jac_scale))] if scaled else []
    assert log[mark:] == [("jac_coord", xn)] + scale + [("compress_jacobian", key(cb.jv))]
    for w in (1.0, 0.0):
        mark = len(log)
        cb.eval_lag_hess(x, s.y, w)
        if scaled:
            assert log[mark:] == [("vec_mul", key(sc.ybuf), key(s.y), key(sc.con_scale)),
                                  ("hess_coord", xn, key(sc.ybuf), w * SIGN * SCALE), ("compress_hessian", key(cb.hv))]
        else:
            assert log[mark:] == [("hess_coord", xn, key(s.y), w), ("compress_hessian", key(cb.hv))]
    mark = len(log)
    cb.zero_hess()
    cb.jtprod_x(s.out, s.y)
    assert log[mark:] == [("compress_hessian", key(cb.hv0)), ("spmv_device", L.MNK_SC_JT, 0, 1.0, key(s.y), 0.0, key(s.out))]


@pytest.mark.parametrize("obj_scale", [0.1, 1.0 / 3.0])
def test_objective_is_multiplied_by_scale_then_sign(obj_scale):
    """obj_sign * (obj * obj_scale), bit for bit: two roundings at most, never one multiplication by the product."""
    log, K, kkt = doubles()
    s = Setting(K, 2, True)
    s.sc.obj_sign, s.sc.obj_scale = -1.0, obj_scale
    cb = RawStub(log, kkt, K)
    cb.attach(s.sc)
    for value in (3.0, 0.7, 1e-3 / 7.0):
        cb.value = value
        got = cb.eval_f(s.x)
        assert got.hex() == (-1.0 * (value * obj_scale)).hex()
    assert log[-1] == ("obj", key(s.x[:N]))
    # the order matters: with a factor that is no power of two in the place of the sign, the product of the two factors
    # first would round differently for some of these values
    s.sc.obj_sign, told_apart = 1.7, 0
    for value in (3.0, 0.7, 1e-3 / 7.0, 10.0, 2.3):
        cb.value = value
        assert cb.eval_f(s.x).hex() == (1.7 * (value * obj_scale)).hex()
        told_apart += 1.7 * (value * obj_scale) != (1.7 * obj_scale) * value
    assert told_apart > 0


@pytest.mark.parametrize("ns,scaled", CASES)
def test_prescaled_sparse_qp_callbacks(ns, scaled):
    log, K, kkt = doubles()
    s = Setting(K, ns, scaled)
    cb = D.device_callbacks(TinyQP(), kkt, "cpu", K, True, s.sc)
    assert type(cb) is D.DeviceQPCallbacks and cb.prescaled and cb.sc is s.sc
    assert s.sc.con_scale is None and s.sc.jac_scale is None        # the data carry the factors: nothing to apply on the device
    f = SIGN * SCALE if scaled else 1.0
    assert cb.q.tolist() == list(TinyQP.q * f) and cb.hv.tolist() == list(np.array([2.0, 3.0, 4.0]) * f)
    assert cb.jv.tolist() == list(TinyQP().jac_coord(None) * (JAC_SCALE if scaled else 1.0))
    x, xn = s.x, key(s.x[:N])
    cb.obj = lambda v: (log.append(("obj", key(v))), 3.0)[1]
    mark = len(log)
    assert cb.eval_f(x) == 3.0 and log[mark:] == [("obj", xn)]       # no factor, scaled or not
    mark = len(log)
    cb.eval_grad(s.f, x)
    assert [e[0] for e in log[mark:]] == ["spmv_device", "vec_axpby", "vec_fill"]
    assert log[-1] == ("vec_fill", key(s.f[N:]), 0.0) and log[-2][1] == key(s.f[:N])
    mark = len(log)
    cb.eval_cons(s.c, x)
    assert log[mark:] == [("spmv_device", L.MNK_SC_JT, 1, 1.0, xn, 0.0, key(s.c))] + s.cons_tail()
    if scaled:
        assert log[-1][2] is None                                   # con_scale of prescaled data
    mark = len(log)
    cb.eval_jac(x)
    assert log[mark:] == [("compress_jacobian", key(cb.jv))]
    for w, src in ((1.0, cb.hv), (0.0, cb.hv0)):
        mark = len(log)
        cb.eval_lag_hess(x, s.y, w)
        assert log[mark:] == [("compress_hessian", key(src))] and cb.handle_has_H == (w != 0.0)


@pytest.mark.parametrize("ns,scaled", CASES)
def test_prescaled_dense_qp_callbacks_and_the_quasi_newton_product(ns, scaled):
    log, K, kkt = doubles()
    s = Setting(K, ns, scaled)
    cb = D.device_callbacks(TinyQP(), kkt, "cpu", K, False, s.sc)
    assert type(cb) is D.DeviceDenseQPCallbacks and cb.prescaled
    A = TinyQP.A * (CON_SCALE[:, None] if scaled else 1.0)
    assert cb.A_cm.tolist() == A.T.tolist() and cb.P_cm.tolist() == (TinyQP.P * (SIGN * SCALE if scaled else 1.0)).T.tolist()
    last_x = torch.zeros(N, dtype=torch.float64)
    mark = len(log)
    cb.eval_jtprod_at(last_x, s.y, s.out)                           # y itself, never ybuf: the rows of A carry con_scale
    assert log[mark:] == [("gemv", 1, M, N, 1.0, key(cb.A_kkt_cm), M, key(s.y), 0.0, key(s.out))]
    mark = len(log)
    cb.eval_cons(s.c, s.x)
    assert log[mark:] == [("gemv", 0, M, N, 1.0, key(cb.A_cm), M, key(s.x[:N]), 0.0, key(s.c))] + s.cons_tail()
    loads = []
    cb.load_hess = lambda *a: loads.append(tuple(key(v) for v in a))  # (the real one calls the library: `mnk_dc_set_hess`)
    cb.eval_lag_hess(s.x, s.y, 1.0)
    assert loads == [(key(s.x[:N]), key(s.y), 1.0)]                   # an exact run loads through `load_hess`, weight unscaled


class FakeFix:
    """`DeviceFixedVariables` without the library: expand and gather are recorded."""
    njac, nhess = 4, 2

    def __init__(self, log):
        self.log, self.x_full = log, torch.zeros(N + 1, dtype=torch.float64)

    def expand(self, x):
        self.log.append(("expand", key(x)))
        return self.x_full

    def gather(self, which, src_full, dst, scale=None, factor=1.0):
        self.log.append(("gather", which, key(src_full), key(dst), key(scale), factor))


@pytest.mark.parametrize("ns,scaled", CASES)
def test_fixed_variable_wrapper_fuses_the_scaling_into_its_gather(ns, scaled):
    log, K, kkt = doubles()
    s = Setting(K, ns, scaled)
    inner = RawStub(log, None, K)
    cb = D.DeviceFixedVariableCallbacks.__new__(D.DeviceFixedVariableCallbacks)
    f64 = lambda k: torch.zeros(k, dtype=torch.float64)  # noqa: E731
    cb.__dict__.update(inner=inner, kkt=kkt, K=K, n=N, m=M, fix=FakeFix(log), g_full=f64(N + 1), jv=f64(4), hv=f64(2), hv0=f64(2))
    cb.close = types.MethodType(lambda self: None, cb)
    assert cb.fused_scaling and not cb.prescaled
    cb.attach(s.sc)
    sc, x, xn, xf = s.sc, s.x, key(s.x[:N]), key(cb.fix.x_full)
    mark = len(log)
    cb.eval_grad(s.f, x)
    assert log[mark:] == [("expand", xn), ("grad", key(cb.g_full), xf),
                          ("gather", L.MNK_FIX_FREE, key(cb.g_full), key(s.f[:N]), None, SIGN * SCALE if scaled else 1.0),
                          ("vec_fill", key(s.f[N:]), 0.0)]
    mark = len(log)
    cb.eval_cons(s.c, x)
    assert log[mark:] == [("expand", xn), ("cons", key(s.c), xf)] + s.cons_tail()
    mark = len(log)
    cb.eval_jac(x)
    assert log[mark:] == [("expand", xn), ("jac_coord", xf),
                          ("gather", L.MNK_FIX_JAC, key(inner.jv), key(cb.jv), key(sc.jac_scale), 1.0),
                          ("compress_jacobian", key(cb.jv))]
    assert (sc.jac_scale is not None) == scaled
    mark = len(log)
    cb.eval_lag_hess(x, s.y, 1.0)
    y_model = [("vec_mul", key(sc.ybuf), key(s.y), key(sc.con_scale))] if scaled else []
    assert log[mark:] == y_model + [("expand", xn), ("hess_coord", xf, key(sc.ybuf if scaled else s.y), SIGN * SCALE if scaled else 1.0),
                                    ("gather", L.MNK_FIX_HESS, key(inner.hv), key(cb.hv), None, 1.0),
                                    ("compress_hessian", key(cb.hv))]
    inner.value = 3.0
    assert cb.eval_f(x).hex() == (sc.obj_sign * (3.0 * sc.obj_scale)).hex()


def test_library_handles_are_released_once_by_their_destroy_entry(monkeypatch):
    calls = []
    lib = types.SimpleNamespace(mnk_tape_destroy=lambda h: calls.append(("tape", h)), mnk_opf_destroy=lambda h: calls.append(("opf", h)))
    monkeypatch.setattr(L, "lib", lambda: lib)
    for cls, name in ((D.DeviceTapeCallbacks, "tape"), (D.DeviceOPFCallbacks, "opf")):
        cb = cls.__new__(cls)
        cb._h = 1234
        cb.close()
        cb.close()
        assert calls == [(name, 1234)] and not cb._h
        calls.clear()
    assert (D.DeviceHessianProduct._destroy, D.DeviceFixedVariables._destroy) == ("mnk_sc_destroy", "mnk_fix_destroy")


def test_ipm_dev_keeps_exporting_the_callbacks_and_importing_loads_no_library(monkeypatch):
    import importlib.util
    import os
    import sys

    import madnlp_jl_amd
    from madnlp_jl_amd import ipm_dev as I

    def no_library():
        raise AssertionError("importing the module loaded the library")
    monkeypatch.setattr(L, "lib", no_library)
    pkg = os.path.dirname(os.path.abspath(madnlp_jl_amd.__file__))
    for module in ("device_callbacks", "ipm_dev"):                   # a second, private copy: executed from scratch
        name = f"madnlp_jl_amd._probe_{module}"
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, module + ".py"))
        mod = importlib.util.module_from_spec(spec)
        monkeypatch.setitem(sys.modules, name, mod)
        spec.loader.exec_module(mod)
        assert mod.DeviceTapeCallbacks.__name__ == "DeviceTapeCallbacks"
    names = ("_up _DevicePointer DeviceHessianProduct DeviceFixedVariables DeviceQPCallbacks DeviceDenseQPCallbacks "
             "DeviceOPFCallbacks DeviceTapeCallbacks DeviceFixedVariableCallbacks").split()
    assert all(getattr(I, n) is getattr(D, n) for n in names)
    assert I.DeviceMadNLPSolver.__dict__.get("_callbacks_class") is None and callable(D.callbacks_class)


def test_solver_close_is_safe_before_the_upload_and_closes_in_order():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    order = []
    part = lambda name: types.SimpleNamespace(close=lambda: order.append(name))  # noqa: E731
    s = DeviceMadNLPSolver.__new__(DeviceMadNLPSolver)
    s.kkt = part("kkt")
    s.close()
    assert order == ["kkt"]
    s.cb, s.K = part("cb"), part("K")
    s.close()
    assert order == ["kkt", "cb", "K", "kkt"]

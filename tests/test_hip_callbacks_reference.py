"""(-m gpu) The composition in `madnlp_jl_amd.device_callbacks` -- objective sense, NLP scaling, slack / rhs tail, fixed-variable
reduction on top of the model evaluators -- against `callback_cases.scaled_problem`, the mpmath statement of what the solver is
entitled to see, entry by entry and within the float64 bound derived there.  Every callbacks object is built by
`device_callbacks(...)` on a real KKT handle with a real `DeviceScaling`; the Jacobian and the Lagrangian Hessian are read back
from the HANDLE (compressed values of the sparse handle, the dense handle's buffers), not from the COO scratch vectors, so a scale
or gather applied by the wrong index shows even where the COO values look plausible.  The raw-value cells take their factors,
`jac_scale = con_scale[jac_I]`, the right-hand side and the fixed-variable handler from the host solver's own `initialize`."""
from fractions import Fraction as Fr

import numpy as np
import pytest

from madnlp_jl_amd import fixed_vars as FV
from tests import callback_cases as CC
from tests.test_hip_tape import gpu_ctx  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
OBJ_SCALE = 100.0 / 2406.0                 # the non-dyadic factor of tests/test_hip_nlp_scaling.py
NETWORK = (70, 20, 150)
_cache = {}


def every_seventh(n):
    return np.array(sorted({0, n - 1} | set(range(0, n, 7))))


def multipliers(m, seed):
    y = np.random.default_rng(seed).standard_normal(m)
    y[::7] = 0.0
    return y


def con_scale(m):
    return 10.0 ** np.random.default_rng(m).uniform(-3.0, 0.0, m)


# ------------------------------------------------------------------------------------------------- models and their references
def acopf_iterates():
    """(x_full A, x_full B, ModelRef A, ModelRef B): the random point, and the point on the voltage bounds with the entries
    that the fixed-variable cells fix taken from A (a handler holds ONE set of values)."""
    if "acopf" not in _cache:
        model, xa, _, ra = CC.acopf_case(NETWORK, "random")
        xb = CC.acopf_case(NETWORK, "bounds")[1].copy()
        where = every_seventh(model.n)
        xb[where] = xa[where]
        _cache["acopf"] = (xa, xb, ra, CC.acopf_model_reference(model, xb, CC.sampled_arcs(model)))
    return _cache["acopf"]


def tape_iterates():
    if "tape" not in _cache:
        M, terms, rows, owners = CC.small_tape_model()
        rng = np.random.default_rng(301)
        xa, xb = CC.on_grid(rng.uniform(0.5, 1.5, M.n)), CC.on_grid(rng.uniform(0.5, 1.5, M.n))
        where = every_seventh(M.n)
        xb[where] = xa[where]
        ref = lambda x: CC.model_reference(M.n, M.m, x, terms, rows, owners, M.jac_I, M.jac_J, M.hess_I, M.hess_J)  # noqa: E731
        _cache["tape"] = (xa, xb, ref(xa), ref(xb))
    return _cache["tape"]


def qp_iterates(nlp, key):
    if key not in _cache:
        rng = np.random.default_rng(nlp.n)
        xa, xb = rng.uniform(-1.0, 1.0, nlp.n), rng.uniform(-1.0, 1.0, nlp.n)
        where = every_seventh(nlp.n)
        xb[where] = xa[where]
        ref = lambda x: CC.qp_model_reference(nlp.n, nlp.m, nlp.hess_I, nlp.hess_J, nlp.hess_coord(None, None, 1.0), nlp.q,  # noqa: E731
                                              nlp.jac_I, nlp.jac_J, nlp.jac_coord(None), x)
        _cache[key] = (xa, xb, ref(xa), ref(xb))
    return _cache[key]


# ------------------------------------------------------------------------------------------------- cells
class Cell:
    """One callbacks object on its handle, and what `scaled_problem` needs to state the same problem."""

    def close(self):
        for h in (self.cb, self.K, self.kkt):
            h.close()


def _kernels(ctx, nt, ind_lb=None, ind_ub=None):
    from madnlp_jl_amd.ipm_device import IPMDeviceKernels
    return IPMDeviceKernels(nt, np.arange(1) if ind_lb is None else ind_lb, np.arange(1) if ind_ub is None else ind_ub, ctx=ctx)


def raw_cell(ctx, monkeypatch, nlp, scaled, fixed, relax, x_fixed=None, unit=False):
    """A raw-value model (AC-OPF, tape) the way the solver sets it up: the host `MadNLPSolver.initialize` forms obj_sign,
    obj_scale, con_scale, jac_scale = con_scale[jac_I], the scaled right-hand side, the index sets and the handler -- with the
    two `set_*_scale` rules replaced by this test's factors --, then the lines of `DeviceMadNLPSolver._upload` build the
    `DeviceScaling` and call `device_callbacks`.  The sparse condensed handle knows inequality rows only: it is created with all
    rows (it serves as the compressor), the `DeviceScaling` gets the solver's own `ind_ineq`."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import ipm
    from madnlp_jl_amd.device_callbacks import DeviceScaling, _up, device_callbacks
    cs = np.ones(nlp.m) if unit else con_scale(nlp.m)
    if scaled:
        monkeypatch.setattr(ipm, "set_con_scale_sparse", lambda m, jac_I, jac, max_gradient: cs.copy())
        monkeypatch.setattr(ipm, "set_obj_scale", lambda grad, max_gradient: 1.0 if unit else OBJ_SCALE)
        nlp.minimize = bool(unit)
    if fixed:
        where = every_seventh(nlp.n)
        nlp.lvar[where] = nlp.uvar[where] = x_fixed[where]
    opt = ipm.IPMOptions(tol=1e-6, nlp_scaling=scaled, fixed_variable_treatment="make_parameter")
    opt.relax_equality, opt.dual_initialization = relax, "zero"

    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], *FV.structure(nlp, info), np.arange(info["m"]), info["ind_lb"],
                                           info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    s = ipm.MadNLPSolver(nlp, factory, opt, sparse=True)
    s.initialize()
    c = Cell()
    c.kkt, c.n, c.ns, c.m, c.handler = s.kkt, s.n, s.ns, s.m, s.fixed_handler
    assert (c.handler is not None) == fixed and np.array_equal(s.jac_scale, s.con_scale[np.asarray(s.model.jac_I)])
    if scaled and not unit:
        assert s.obj_sign == -1.0 and s.obj_scale == OBJ_SCALE and np.array_equal(s.con_scale, cs)
    c.sign, c.scale, c.cs, c.ind_ineq, c.rhs = s.obj_sign, s.obj_scale, s.con_scale.copy(), s.ind_ineq, s.rhs.copy()
    c.scaled = bool(opt.nlp_scaling) or s.obj_sign != 1.0
    c.K = _kernels(ctx, s.n + s.ns, s.ind_lb, s.ind_ub)
    scaling = DeviceScaling(c.K, "cuda", s.n, s.ns, s.ind_ineq, _up(s.rhs, "cuda"), c.scaled, s.obj_sign, s.obj_scale, s.con_scale,
                            s.jac_scale)
    c.cb = device_callbacks(s.nlp, s.kkt, "cuda", c.K, True, scaling, fixed=s.fixed_handler)
    c.free = np.arange(nlp.n) if c.handler is None else c.handler.free
    return c


def acopf_cell(ctx, monkeypatch, scaled, fixed, unit=False):
    from madnlp_jl_amd.device_callbacks import DeviceFixedVariableCallbacks, DeviceOPFCallbacks
    from madnlp_jl_amd.problems import ACOPFModel
    c = raw_cell(ctx, monkeypatch, ACOPFModel(NETWORK), scaled, fixed, True, acopf_iterates()[0], unit)
    assert c.ns == c.m and isinstance(c.cb.inner if fixed else c.cb, DeviceOPFCallbacks)
    assert isinstance(c.cb, DeviceFixedVariableCallbacks) == fixed
    return c


def tape_cell(ctx, monkeypatch, scaled, fixed, rows="mixed", unit=False):
    from madnlp_jl_amd.device_callbacks import DeviceFixedVariableCallbacks, DeviceTapeCallbacks
    M = CC.small_tape_model(rows)[0]
    c = raw_cell(ctx, monkeypatch, M, scaled, fixed, False, tape_iterates()[0], unit)
    assert c.ns == {"mixed": M.m - len(range(0, M.m, 3)), "ineq": M.m, "eq": 0}[rows]
    assert isinstance(c.cb.inner if fixed else c.cb, DeviceTapeCallbacks) and isinstance(c.cb, DeviceFixedVariableCallbacks) == fixed
    if rows == "mixed":
        assert 0 < c.ns < c.m and (c.rhs != 0).any() and (c.cb.sc.slack_pos is not None) == c.scaled
    return c


def qp_cell(ctx, nlp, sparse, scaled, fixed=False, unit=False, own_hessian=False):
    """The two prescaled QP classes: the factors go into the data on the host (`host_factors`)."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.device_callbacks import DeviceDenseQPCallbacks, DeviceQPCallbacks, DeviceScaling, _up, device_callbacks
    n, m = nlp.n, nlp.m
    c = Cell()
    c.n, c.m = n, m
    c.ind_ineq = np.flatnonzero(np.asarray(nlp.lcon) < np.asarray(nlp.ucon)) if not sparse else np.flatnonzero(np.arange(m) % 3 != 0)
    c.ns = len(c.ind_ineq)
    rng = np.random.default_rng(m + 5)
    c.rhs = np.zeros(m)
    eq = np.setdiff1d(np.arange(m), c.ind_ineq)
    c.rhs[eq] = rng.integers(-8, 9, len(eq)) / 8.0
    c.scaled = scaled
    c.sign, c.scale = (1.0, 1.0) if unit or not scaled else (-1.0, OBJ_SCALE)
    c.cs = np.ones(m) if unit or not scaled else con_scale(m)
    c.handler = dense_handler = None
    if fixed:
        where = every_seventh(n)
        nlp.lvar[where] = nlp.uvar[where] = 0.5
        dense_handler = FV.FixedVariableHandler.create(nlp, False)
        c.handler = FV.FixedVariableHandler(nlp, True)                # the same index sets, with the COO subsets
        assert dense_handler.fixed.tolist() == c.handler.fixed.tolist() == where.tolist()
    none = np.zeros(0, dtype=np.int64)
    if sparse:
        c.kkt = mj.SparseCondensedKKTSystem(n, m, nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, np.arange(m), none, none, ctx=ctx,
                                            opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                            device_kkt_ops=True)
    else:
        c.kkt = mj.DenseKKTSystem(n, m, c.ind_ineq, none, none, ctx=ctx,
                                  opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)
    c.K = _kernels(ctx, n + c.ns)
    scaling = DeviceScaling(c.K, "cuda", n, c.ns, c.ind_ineq, _up(c.rhs, "cuda"), scaled, c.sign, c.scale, c.cs, None)
    c.cb = device_callbacks(nlp, c.kkt, "cuda", c.K, sparse, scaling, fixed=dense_handler, own_hessian=own_hessian)
    assert type(c.cb) is (DeviceQPCallbacks if sparse else DeviceDenseQPCallbacks) and c.cb.prescaled
    c.free = np.arange(n)                 # the dense class keeps all n variables: frozen ones stay in place
    c.sparse = sparse
    return c


# ------------------------------------------------------------------------------------------------- one evaluation
def handle_jacobian(c):
    """(values, positions (row, column)) the handle holds"""
    from madnlp_jl_amd import _lib as L
    k = c.kkt
    if hasattr(k, "jt_colptr"):
        vals = k._values(L.MNK_SC_JT, k.nnz_jt)
        rows = np.repeat(np.arange(k.m), np.diff(k.jt_colptr))
        return vals, list(zip(rows.tolist(), np.asarray(k.jt_rowval).tolist()))
    # dense: the Jacobian block of the augmented matrix [H + pr, 0, J'; 0, Sigma, -I; J, -I, du] built with zero diagonals
    lib = L.lib()
    npr = c.n + c.ns
    pr, du = np.zeros(npr), np.zeros(c.m)
    L.check(lib.mnk_dc_build(k._h, pr.ctypes.data, du.ctypes.data, L.MNK_HOST), "mnk_dc_build")
    order = npr + c.m
    aug = np.zeros((order, order), order="F")
    L.check(lib.mnk_dc_get_aug(k._h, aug.ctypes.data, L.MNK_HOST), "mnk_dc_get_aug")
    J = aug[npr:, :c.n]
    return J.ravel(), [(i, j) for i in range(c.m) for j in range(c.n)]


def handle_hessian(c):
    """(values, positions (row >= column)) the handle holds"""
    from madnlp_jl_amd import _lib as L
    k = c.kkt
    if hasattr(k, "hess_colptr"):
        vals = k._values(L.MNK_SC_HESS, k.nnz_hess)
        cols = np.repeat(np.arange(k.n), np.diff(k.hess_colptr))
        return vals, [(max(i, j), min(i, j)) for i, j in zip(np.asarray(k.hess_rowval).tolist(), cols.tolist())]
    H = k.get_hess()
    il, jl = np.tril_indices(c.n)
    return H[il, jl], list(zip(il.tolist(), jl.tolist()))


def evaluate(ctx, c, x, y, w):
    """All five solver-facing calls (and J'y of the dense class) at the iterate x = [variables | slacks]: host copies, the
    Jacobian and Hessian as the handle holds them.  Output vectors start as NaN."""
    import torch
    from madnlp_jl_amd.device_callbacks import _up
    xd, yd = _up(x, "cuda"), _up(y, "cuda")
    g = torch.full((c.n + c.ns,), np.nan, dtype=torch.float64, device="cuda")
    cons = torch.full((c.m,), np.nan, dtype=torch.float64, device="cuda")
    jt = torch.full((c.n,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()               # uploads and fills ran on torch's stream, the callbacks run on the context's
    c.cb.eval_jac(xd)                      # the loads first, as in the solver: a sparse QP evaluates f and grad f through the
    c.cb.eval_lag_hess(xd, yd, w)          # handle's Hessian, which holds H from its first load on (zero or w H: put back)
    out = {"f": c.cb.eval_f(xd)}
    c.cb.eval_grad(g, xd)
    c.cb.eval_cons(cons, xd)
    if not getattr(c, "sparse", True):
        c.cb.eval_jtprod_at(xd[:c.n], yd, jt)
    ctx.synchronize()
    out.update(g=g.cpu().numpy().copy(), c=cons.cpu().numpy().copy(), jt=jt.cpu().numpy().copy())
    out["hess"], out["hess_pos"] = handle_hessian(c)
    out["jac"], out["jac_pos"] = handle_jacobian(c)
    for k in ("g", "c", "jac", "hess"):
        assert not np.isnan(out[k]).any(), k
    return out


def stored(block, I, J, positions, lower, unit_diagonal=()):
    """The block's COO entries summed into the handle's positions: a Block aligned with the handle's values.  A stored
    position without a COO entry must hold exactly zero (exactly one on the diagonal of `unit_diagonal`: frozen variables);
    k summed duplicates add k - 1 roundings."""
    acc = {}
    for e, (i, j) in enumerate(zip(np.asarray(I).tolist(), np.asarray(J).tolist())):
        acc.setdefault((max(i, j), min(i, j)) if lower else (i, j), []).append(e)
    assert set(acc) <= set(positions), "a COO entry has no place in the handle"
    out = CC.Block()
    for pos in positions:
        es = acc.get(pos, [])
        if any(block.val[e] is None for e in es):
            out.skip()
        elif not es:
            out.add(CC.mpf(int(lower and pos[0] == pos[1] and pos[0] in unit_diagonal)), CC.mpf(0), 0)
        else:
            out.add(CC.mp.fsum(block.val[e] for e in es), CC.mp.fsum(block.mag[e] for e in es),
                    max(block.r[e] for e in es) + len(es) - 1, any(block.trig[e] for e in es))
    return out


def check(c, sp, out, s, y, w, what):
    """every output of one evaluation against the scaled problem; returns the largest ratios"""
    u = CC.U_DEVICE
    F = sp.objective()
    worst = {"eval_f": CC.assert_within([out["f"]], F, u, (what, "eval_f"))}
    G = sp.grad()
    frozen = sp.n != c.n                                        # the dense class keeps its frozen variables in place
    back = c.handler.free if frozen else np.arange(c.n)         # the scaled problem's column -> the handle's
    fixed = set(c.handler.fixed.tolist()) if frozen else ()
    worst["eval_grad"] = CC.assert_within(out["g"][np.concatenate((back, c.n + np.arange(c.ns)))], G, u, (what, "eval_grad"))
    assert (out["g"][c.n:] == 0.0).all() and not np.signbit(out["g"][c.n:]).any()
    worst["eval_cons"] = CC.assert_within(out["c"], sp.cons(s), u, (what, "eval_cons"))
    worst["eval_jac"] = CC.assert_within(out["jac"], stored(sp.jac(), sp.jac_I, back[sp.jac_J], out["jac_pos"], False), u,
                                         (what, "eval_jac"))
    worst["eval_lag_hess"] = CC.assert_within(out["hess"], stored(sp.hess(y, w), back[sp.hess_I], back[sp.hess_J], out["hess_pos"],
                                                                  True, fixed), u, (what, "eval_lag_hess"))
    print(what, "w =", w, {k: round(v, 3) for k, v in worst.items()})
    return worst


def run_raw(ctx, c, iterates, name):
    xa, xb, ra, rb = iterates
    for it, (x_full, ref) in enumerate(((xa, ra), (xb, rb))):
        sp = CC.scaled_problem(ref, c.sign, c.scale, c.cs if c.scaled else None, c.ind_ineq, c.rhs, c.handler)
        assert (sp.n, sp.ns) == (c.n, c.ns)
        s = np.random.default_rng(it).standard_normal(c.ns)
        y = multipliers(c.m, 40 + it)
        for w in CC.WEIGHTS:
            out = evaluate(ctx, c, np.concatenate((x_full[c.free], s)), y, w)
            check(c, sp, out, s, y, w, f"{name} iterate {it}")


# ------------------------------------------------------------------------------------------------- the cells
@pytest.mark.parametrize("fixed", [False, True], ids=["all_free", "fixed"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_acopf_callbacks_return_the_scaled_reduced_problem(gpu_ctx, monkeypatch, scaled, fixed):
    c = acopf_cell(gpu_ctx, monkeypatch, scaled, fixed)
    try:
        run_raw(gpu_ctx, c, acopf_iterates(), f"acopf scaled={scaled} fixed={fixed}")
    finally:
        c.close()


@pytest.mark.parametrize("rows,scaled,fixed", [("mixed", False, False), ("mixed", True, False), ("mixed", False, True),
                                               ("mixed", True, True), ("ineq", True, False), ("ineq", False, False),
                                               ("eq", True, False), ("eq", False, False)])
def test_tape_callbacks_return_the_scaled_reduced_problem(gpu_ctx, monkeypatch, rows, scaled, fixed):
    c = tape_cell(gpu_ctx, monkeypatch, scaled, fixed, rows)
    try:
        run_raw(gpu_ctx, c, tape_iterates(), f"tape {rows} scaled={scaled} fixed={fixed}")
    finally:
        c.close()


def run_qp(ctx, c, nlp, key, name):
    xa, xb, ra, rb = qp_iterates(nlp, key)
    for it, (x, ref) in enumerate(((xa, ra), (xb, rb))):
        x = x.copy()
        if c.handler is not None:
            x[c.handler.fixed] = 0.5 + (0.25 if it else 0.0)         # off the fixed value: grad[fixed] = x - lvar = 0.25
            ref = CC.qp_model_reference(nlp.n, nlp.m, nlp.hess_I, nlp.hess_J, nlp.hess_coord(None, None, 1.0), nlp.q, nlp.jac_I,
                                        nlp.jac_J, nlp.jac_coord(None), x)
        sp = CC.scaled_problem(ref, c.sign, c.scale, c.cs if c.scaled else None, c.ind_ineq, c.rhs, c.handler)
        s = np.random.default_rng(it).standard_normal(c.ns)
        y = multipliers(c.m, 50 + it)
        for w in CC.WEIGHTS:
            out = evaluate(ctx, c, np.concatenate((x, s)), y, w)
            check(c, sp, out, s, y, w, f"{name} iterate {it}")
            if c.handler is not None:                                  # frozen variables: masked in the handle, x - lvar in the gradient
                fx = c.handler.fixed
                assert np.array_equal(out["g"][fx], x[fx] - 0.5)
                H = c.kkt.get_hess()
                for k in fx:
                    assert H[k, k] == 1.0 and not H[k + 1:, k].any() and not H[k, :k].any()
                J = out["jac"].reshape(c.m, c.n)
                assert not J[:, fx].any()
            if not c.sparse:
                JT = sp.jtprod(y)
                if c.handler is None:
                    CC.assert_within(out["jt"], JT, CC.U_DEVICE, (name, "eval_jtprod_at"))
                else:
                    CC.assert_within(out["jt"][c.handler.free], JT, CC.U_DEVICE, (name, "eval_jtprod_at"))
                    assert not out["jt"][c.handler.fixed].any()


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_sparse_qp_callbacks_return_the_scaled_problem(gpu_ctx, scaled):
    from madnlp_jl_amd.problems import SparseQPModel
    nlp = SparseQPModel((2, 1, 1))
    c = qp_cell(gpu_ctx, nlp, True, scaled)
    try:
        run_qp(gpu_ctx, c, nlp, "sparse_qp", f"sparse qp scaled={scaled}")
    finally:
        c.close()


@pytest.mark.parametrize("fixed", [False, True], ids=["all_free", "frozen"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_dense_qp_callbacks_return_the_scaled_problem(gpu_ctx, scaled, fixed):
    from madnlp_jl_amd.problems import DenseQPModel
    nlp = DenseQPModel(n=70, m=33, n_eq=5)
    assert np.array_equal(nlp.P, nlp.P.T)
    c = qp_cell(gpu_ctx, nlp, False, scaled, fixed)
    assert 0 < c.ns < c.m
    try:
        run_qp(gpu_ctx, c, nlp, "dense_qp", f"dense qp scaled={scaled} frozen={fixed}")
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------- unit factors change no bit
@pytest.mark.parametrize("model", ["acopf", "tape", "sparse_qp", "dense_qp"])
def test_unit_factors_change_no_bit_of_a_callback(gpu_ctx, monkeypatch, model):
    """`scaled=True` with sign 1, scale 1 and con_scale all ones against `scaled=False`: the statement of
    test_hip_nlp_scaling.py::test_unit_factors_change_no_bit_of_a_device_run, at the callbacks."""
    from madnlp_jl_amd.problems import DenseQPModel, SparseQPModel
    outs = []
    for scaled in (True, False):
        if model == "acopf":
            c, x = acopf_cell(gpu_ctx, monkeypatch, scaled, False, unit=True), acopf_iterates()[0]
        elif model == "tape":
            c, x = tape_cell(gpu_ctx, monkeypatch, scaled, False, unit=True), tape_iterates()[0]
        else:
            nlp = SparseQPModel((2, 1, 1)) if model == "sparse_qp" else DenseQPModel(n=70, m=33, n_eq=5)
            c, x = qp_cell(gpu_ctx, nlp, model == "sparse_qp", scaled, unit=True), qp_iterates(nlp, model)[0]
        assert c.cb.sc.scaled == scaled and c.sign == 1.0 and c.scale == 1.0 and (c.cs == 1.0).all()
        try:
            s, y = np.random.default_rng(3).standard_normal(c.ns), multipliers(c.m, 60)
            outs.append([evaluate(gpu_ctx, c, np.concatenate((x, s)), y, w) for w in CC.WEIGHTS])
        finally:
            c.close()
    for a, b in zip(*outs):
        assert a["f"] == b["f"]
        for k in ("g", "c", "jac", "hess"):
            assert np.array_equal(a[k], b[k]), k
        if model == "dense_qp":
            assert np.array_equal(a["jt"], b["jt"])


# ------------------------------------------------------------------------------------------------- exact answers through the state of the QP classes
class IntegerQP:
    """H, q, J small integers; with a dyadic x every product and sum of f = 0.5 x'Hx + q'x is exact in any order."""
    n, m = 6, 3

    def __init__(self):
        rng = np.random.default_rng(66)
        L = np.tril(rng.integers(-3, 4, (6, 6))).astype(float)
        self.P = L + np.tril(L, -1).T
        self.q = rng.integers(-4, 5, 6).astype(float)
        self.A = rng.integers(-2, 3, (3, 6)).astype(float)
        self.hess_I, self.hess_J = np.tril_indices(6)
        self.jac_I, self.jac_J = np.nonzero(self.A)
        self.lvar, self.uvar, self.lcon, self.ucon = np.full(6, -4.0), np.full(6, 4.0), np.full(3, -9.0), np.full(3, 9.0)
        self.x = rng.integers(-8, 9, 6) / 4.0

    def hess_coord(self, x, y, w=1.0):
        return w * self.P[self.hess_I, self.hess_J]

    def jac_coord(self, x):
        return self.A[self.jac_I, self.jac_J]

    def answer(self):
        x, P, q = [Fr(float(v)) for v in self.x], self.P, self.q
        f = sum(Fr(float(P[i, j])) * x[i] * x[j] for i in range(6) for j in range(6)) / 2 + sum(Fr(float(q[i])) * x[i] for i in range(6))
        assert Fr(float(f)) == f
        return float(f)


@pytest.mark.parametrize("sparse,own_hessian", [(True, False), (False, False), (True, True)], ids=["sparse", "dense", "own_hessian"])
def test_qp_objective_and_handle_hessian_through_the_state_sequence(gpu_ctx, sparse, own_hessian):
    """eval_lag_hess(w = 1), eval_f, zero_hess(), eval_f, read the handle, eval_lag_hess(w = 1), eval_f: every objective is the
    integer answer, the handle holds zero after the second eval_f (`_hmul` puts it back) and H after the last load.  With
    `own_hessian` the objective never touches the handle's Hessian."""
    import torch
    from madnlp_jl_amd.device_callbacks import _up
    nlp = IntegerQP()
    c = qp_cell(gpu_ctx, nlp, sparse, False, own_hessian=own_hessian)
    try:
        xd, yd = _up(np.concatenate((nlp.x, np.zeros(c.ns))), "cuda"), _up(np.ones(3), "cuda")
        torch.cuda.synchronize()
        want, Hl = nlp.answer(), nlp.P[np.tril_indices(6)]

        def held():
            gpu_ctx.synchronize()
            vals, pos = handle_hessian(c)
            return np.array([vals[pos.index((i, j))] for i, j in zip(*np.tril_indices(6))])
        if own_hessian:
            mark = _up(np.arange(1.0, 22.0), "cuda")
            torch.cuda.synchronize()
            c.kkt.compress_hessian(mark)
            assert c.cb.eval_f(xd) == want and np.array_equal(held(), np.arange(1.0, 22.0))
            c.cb.handle_has_H = False                  # whatever the state says, H x comes from the callbacks' own product
            assert c.cb.eval_f(xd) == want and np.array_equal(held(), np.arange(1.0, 22.0))
            return
        c.cb.eval_lag_hess(xd, yd, 1.0)
        f1 = c.cb.eval_f(xd)
        assert np.array_equal(held(), Hl)
        c.cb.zero_hess()
        f2 = c.cb.eval_f(xd)
        assert not held().any()
        c.cb.eval_lag_hess(xd, yd, 1.0)
        f3 = c.cb.eval_f(xd)
        assert np.array_equal([f1, f2, f3], [want] * 3)
        assert np.array_equal(held(), Hl)
        c.cb.eval_lag_hess(xd, yd, 0.375)              # any other weight: 0.375 H in the handle, H x still from H
        assert c.cb.eval_f(xd) == want and np.array_equal(held(), 0.375 * Hl)
    finally:
        c.close()

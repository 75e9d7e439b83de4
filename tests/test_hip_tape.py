"""The device interpreter of expression tapes (`mnk_tape_*`, csrc/tape_eval.hip; `ipm_dev.DeviceTapeCallbacks`) against its host
mirror (`madnlp_jl_amd.tape_model`), against the hand-written device AC-OPF model (`mnk_opf_*`), on malformed tapes, and end to
end in `DeviceMadNLPSolver`."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.problems import ACOPFModel
from madnlp_jl_amd.tape_model import P, V, TapeModel
from tests.test_tape_model_cpu import (INT_POINTS, _options, acopf_points, check_integer_outputs, integer_model,
                                       slot_hungry_expr)

BS = 128          # rows per workgroup of the interpreter kernel (TAPE_BS in csrc/tape_eval.hip)


@pytest.fixture()
def gpu_ctx():
    torch = pytest.importorskip("torch")
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    st = torch.cuda.Stream()       # NOT torch's current stream: the callbacks must not depend on torch's stream order
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    yield ctx
    ctx.close()


def device_eval(ctx, cb, nlp, x, y, sigma):
    """The five callbacks into the caller's buffers on the context's stream; host copies after one synchronization."""
    import torch
    from madnlp_jl_amd.ipm_dev import _up
    xd, yd = _up(x, "cuda"), _up(y, "cuda")
    g = torch.full((nlp.n,), np.nan, dtype=torch.float64, device="cuda")
    c = torch.full((nlp.m,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()       # the uploads ran on torch's stream
    f = cb.obj(xd)
    terms = cb.obj_terms(xd) if hasattr(cb, "obj_terms") else None
    cb.grad(g, xd)
    cb.cons(c, xd)
    jv, hv = cb.jac_coord(xd), cb.hess_coord(xd, yd, sigma)
    ctx.synchronize()
    h = lambda t: None if t is None else t.cpu().numpy().copy()  # noqa: E731
    return f, h(terms), h(g), h(c), h(jv), h(hv)


def make_callbacks(ctx, nlp, cls):
    from madnlp_jl_amd.ipm_device import IPMDeviceKernels
    K = IPMDeviceKernels(nlp.n, np.arange(1), np.arange(1), ctx=ctx)
    return cls(nlp, None, "cuda", K), K


# ------------------------------------------------------------------------------------------------- 7. device vs host interpreter
def edge_model():
    """Patterns at the kernel's edges in ONE launch per callback: R = 1, BS, BS + 1, 3 BS - 1; k = 1 and 5; q = 0; a value tape
    exactly at SLOT_MAX; constraint rows fed by 3 / 2 / 1 / 0 patterns; variables without a gradient term.  Patterns 0 .. 5 use
    + - * / only, pattern 6 every transcendental function."""
    n, m = 700, 400
    rng = np.random.default_rng(21)
    M = TapeModel(n, m, np.ones(n), 0.0, 2.0, -np.inf, np.inf)
    distinct = lambda R, k, lo, hi: np.stack([rng.choice(np.arange(lo, hi), k, replace=False) for _ in range(R)])  # noqa: E731
    M.add_objective(V(0) * V(0), np.array([[0]]))                                                         # 0: R = 1, k = 1, q = 0
    M.add_objective(P(0) * V(0) * V(1) - V(1) / (V(0) * V(0) + 2.0), distinct(BS + 1, 2, 1, 300), rng.standard_normal((BS + 1, 1)))
    M.add_constraint(V(0) * V(1) - V(2) * V(3) / (V(4) * V(4) + 1.0) + P(0) * V(0) * V(4) - P(1), np.arange(BS),
                     distinct(BS, 5, 0, n), rng.standard_normal((BS, 2)))                                 # 2: R = BS, k = 5
    M.add_constraint(slot_hungry_expr(T.SLOT_MAX), np.arange(3 * BS - 1), distinct(3 * BS - 1, 1, 0, n))  # 3: SLOT_MAX slots
    M.add_constraint(V(0) - V(1) * 0.5, np.arange(BS), distinct(BS, 2, 0, n))                             # 4: rows 0 .. BS-1: 3 feeds
    M.add_constraint(V(0) * 3.0, np.array([5]), np.array([[699]]))                                        # 5: R = 1 (row 5: 4 feeds)
    d = V(0) - V(1)
    M.add_constraint(T.sin(V(0)) * T.exp(V(1) * P(0)) + T.log(V(2) * V(2) + 1.0) + T.sqrt(V(2) * V(2) + 0.5) * T.cos(d),
                     200 + np.arange(BS + 1), distinct(BS + 1, 3, 0, n), rng.standard_normal((BS + 1, 1)))  # 6: rows 200 .. 328
    return M.finalize()


def exact_masks(M, transcendental=(6,)):
    """which COO entries / rows / terms come from patterns without transcendental functions"""
    jm, hm = [], []
    rows_t = np.zeros(M.m, dtype=bool)
    for i, p in enumerate(M.patterns):
        ex = i not in transcendental
        if p.kind == 1:
            jm.append(np.full(p.R * p.tapes[1].nout, ex))
            if not ex:
                rows_t[p.rows] = True
        hm.append(np.full(p.R * p.tapes[2].nout, ex))
    return np.concatenate(jm), np.concatenate(hm), ~rows_t


@pytest.mark.gpu
def test_device_interpreter_matches_the_host_interpreter(gpu_ctx):
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M = edge_model()
    assert M.patterns[3].tapes[0].nslot == T.SLOT_MAX and max(p.k for p in M.patterns) == 5
    fed = np.bincount(np.concatenate([p.rows for p in M.patterns if p.kind == 1]), minlength=M.m)
    assert {0, 1, 3} <= set(fed.tolist())
    cb, K = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    jmask, hmask, rmask = exact_masks(M)
    assert jmask.sum() and hmask.sum() and (~jmask).sum() and (~hmask).sum() and rmask.sum() and (~rmask).sum()
    rng = np.random.default_rng(8)
    for sigma in (1.0, 0.0, 0.37):
        x, y = rng.uniform(0.5, 1.5, M.n), rng.standard_normal(M.m)
        y[::7] = 0.0
        f, terms, g, c, jv, hv = device_eval(gpu_ctx, cb, M, x, y, sigma)
        rt, rg, rc, rj, rh = M.obj_terms(x), M.grad(x), M.cons(x), M.jac_coord(x), M.hess_coord(x, y, sigma)
        # + - * / patterns: bit-identical in all five callbacks (the objective is the term vector; its sum is a device reduction)
        assert np.array_equal(terms, rt)
        assert abs(f - M.obj(x)) <= 1e-13 * np.abs(rt).sum()
        assert np.array_equal(g, rg) and (g[300:] == 0.0).all()          # variables without a gradient term: written as 0
        assert np.array_equal(c[rmask], rc[rmask]) and (c[fed == 0] == 0.0).all()
        assert np.array_equal(jv[jmask], rj[jmask])
        assert np.array_equal(hv[hmask], rh[hmask])
        # transcendental pattern: another math library
        for got, ref in ((c, rc), (jv, rj), (hv, rh)):
            assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    cb.close()
    K.close()


@pytest.mark.gpu
@pytest.mark.parametrize("x,y,w", INT_POINTS)
def test_integer_patterns_give_the_exact_answers_on_the_device(gpu_ctx, x, y, w):
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    M = integer_model()
    cb, K = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    f, terms, g, c, jv, hv = device_eval(gpu_ctx, cb, M, np.array(x, dtype=float), np.array(y, dtype=float), float(w))
    check_integer_outputs(M, x, y, w, f, g, c, jv, hv)
    cb.close()
    K.close()


# ------------------------------------------------------------------------------------------------- 8. against mnk_opf_*
def _csr(vals, I, J, shape):
    return sp.csr_matrix((vals, (np.maximum(I, J), np.minimum(I, J)) if shape[0] == shape[1] else (I, J)), shape=shape).toarray()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["case30", "case118"])
def test_tape_callbacks_match_the_hand_written_device_model(gpu_ctx, case):
    from madnlp_jl_amd.ipm_dev import DeviceOPFCallbacks, DeviceTapeCallbacks
    M, A = T.acopf_tape_model(case), ACOPFModel(case)
    cbt, Kt = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    cbo, Ko = make_callbacks(gpu_ctx, A, DeviceOPFCallbacks)
    for x, y, sigma in acopf_points(A):
        ft, _, gt, ct, jt, ht = device_eval(gpu_ctx, cbt, M, x, y, sigma)
        fo, _, go, co, jo, ho = device_eval(gpu_ctx, cbo, A, x, y, sigma)
        assert abs(ft - fo) <= 1e-13 * abs(fo)
        for got, ref in ((ct, co), (gt, go)):
            assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
        Jt, Jo = _csr(jt, M.jac_I, M.jac_J, (M.m, M.n)), _csr(jo, A.jac_I, A.jac_J, (A.m, A.n))
        assert np.abs(Jt - Jo).max() <= 1e-13 * np.abs(jo).max()
        Ht, Ho = _csr(ht, M.hess_I, M.hess_J, (M.n, M.n)), _csr(ho, A.hess_I, A.hess_J, (A.n, A.n))
        assert np.abs(Ht - Ho).max() <= 1e-13 * np.abs(ho).max()
    for h in (cbt, cbo, Kt, Ko):
        h.close()


# ------------------------------------------------------------------------------------------------- 9. malformed tapes
def _pattern_args(p, edit=None):
    """the argument list of mnk_tape_add_pattern for a compiled pattern; `edit(arrays)` may damage the copies first"""
    A = dict(var_index=p.var_index.copy(), params=p.params.copy(), rows=p.rows.copy(), k=p.k)
    for w, t in enumerate(p.tapes):
        A[f"code{w}"], A[f"consts{w}"], A[f"out{w}"] = t.code.copy(), t.consts.copy(), t.out_operand.copy()
        A[f"out_j{w}"], A[f"out_l{w}"], A[f"nslot{w}"] = t.out_j.copy(), t.out_l.copy(), t.nslot
    if edit:
        edit(A)
    args = [p.kind, p.R, A["k"], p.q, A["var_index"].ctypes.data, A["params"].ctypes.data, A["rows"].ctypes.data]
    for w in range(3):
        args += [len(A[f"code{w}"]), A[f"code{w}"].ctypes.data, len(A[f"consts{w}"]), A[f"consts{w}"].ctypes.data, len(A[f"out{w}"]),
                 A[f"out{w}"].ctypes.data, A[f"out_j{w}"].ctypes.data, A[f"out_l{w}"].ctypes.data, A[f"nslot{w}"]]
    return args, A


def _set(key, idx, value):
    def edit(A):
        if idx is None:
            A[key] = value
        else:
            A[key][idx] = value
    return edit


@pytest.mark.gpu
def test_malformed_tapes_are_refused_before_anything_is_launched(gpu_ctx):
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import _lib as L
    lib = mj.lib()
    M = TapeModel(6, 3, np.ones(6), 0.0, 2.0, 0.0, 0.0)
    M.add_constraint(V(0) * V(1) * P(0) + T.sin(V(2)) * V(0), np.array([0, 2]), np.array([[0, 1, 2], [3, 4, 5]]), np.array([[2.0], [3.0]]))
    M.finalize()
    p = M.patterns[0]
    assert p.tapes[0].nslot >= 2 and len(p.tapes[0].code) >= 3
    h = C.c_void_p()
    L.check(lib.mnk_tape_create(gpu_ctx.handle, M.n, M.m, C.byref(h)), "mnk_tape_create")
    slot = lambda s: T.KIND_SLOT << 24 | s  # noqa: E731
    bad = [
        (_set("code0", (0, 1), p.tapes[0].nslot), b"destination slot"),                # out-of-range slot (written)
        (_set("code0", (1, 2), slot(T.SLOT_MAX + 5)), b"out of range"),                 # out-of-range slot (read)
        (_set("code1", (0, 0), 10), b"bad opcode"),
        (_set("code0", (0, 0), -1), b"bad opcode"),
        (_set("code0", (0, 2), slot(p.tapes[0].nslot - 1)), b"read before it is written"),
        (_set("var_index", (1, 2), M.n), b"var_index[1, 2] = 6 is out of range"),
        (_set("rows", 1, M.m), b"rows[1] = 3 is out of range"),
        (_set("var_index", (0, 1), 0), b"twice"),
        (_set("nslot2", None, T.SLOT_MAX + 1), b"SLOT_MAX"),
        (_set("out1", 0, T.KIND_VAR << 24 | 3), b"local variable 3 is out of range"),
        (_set("out0", 0, T.KIND_CONST << 24 | 1000), b"constant 1000 is out of range"),
        (_set("code0", (0, 3), T.KIND_PAR << 24 | 1), b"parameter column 1 is out of range"),
        (_set("out_j2", 0, 3), b"local variable (pair)"),
        (_set("code0", (0, 2), 5 << 24), b"operand kind"),
    ]
    for edit, msg in bad:
        args, keep = _pattern_args(p, edit)
        rc = lib.mnk_tape_add_pattern(h, *args)
        err = lib.mnk_last_error_string()
        assert rc != 0 and msg in err, (msg, rc, err)
    # the evaluation entry points refuse a handle that was never finalized; the intact pattern is accepted
    x = np.zeros(1)
    assert lib.mnk_tape_cons(h, x.ctypes.data, x.ctypes.data) != 0 and b"mnk_tape_finalize" in lib.mnk_last_error_string()
    args, keep = _pattern_args(p)
    assert lib.mnk_tape_add_pattern(h, *args) == 0
    assert lib.mnk_tape_finalize(h) == 0
    assert lib.mnk_tape_add_pattern(h, *args) != 0 and b"finalized" in lib.mnk_last_error_string()
    sz = [C.c_int64() for _ in range(5)]
    assert lib.mnk_tape_sizes(h, *[C.byref(v) for v in sz]) == 0
    assert [v.value for v in sz] == [M.n, M.m, 0, len(M.jac_I), len(M.hess_I)]
    assert lib.mnk_tape_destroy(h) == 0


# ------------------------------------------------------------------------------------------------- 10. end to end
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["case30", "case118"])
def test_device_resident_tape_acopf_run(gpu_ctx, case):
    """`DeviceMadNLPSolver` on the tape AC-OPF against (1) the host driver with the numpy interpreter on the SAME HIP back-end --
    equal iteration, factorization and back-solve counts, the same history -- and (2) the device run of the hand-written model:
    the conditions of test_acopf.test_device_resident_acopf_run_matches_the_oracle_back_end."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.ipm import MadNLPSolver
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver, DeviceTapeCallbacks

    def factory_for(nlp):
        def factory(info):
            return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J,
                                               info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=gpu_ctx,
                                               opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                               device_kkt_ops=True)
        return factory
    M, A = T.acopf_tape_model(case), ACOPFModel(case)
    sh = MadNLPSolver(M, factory_for(M), _options(), sparse=True)
    sh.solve()
    sd = DeviceMadNLPSolver(M, factory_for(M), _options())
    sd.solve()
    sa = DeviceMadNLPSolver(A, factory_for(A), _options())
    sa.solve()
    assert isinstance(sd.cb, DeviceTapeCallbacks)
    assert sd.status == sh.status == sa.status == "SOLVE_SUCCEEDED"
    x, y, zl, zu = sd.host_state()
    assert (sd.cnt.k, sd.cnt.factorization_cnt, sd.cnt.backsolve_cnt) == (sh.cnt.k, sh.cnt.factorization_cnt, sh.cnt.backsolve_cnt)
    np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
    for a, b in zip(sd.history, sh.history):
        assert a.k == b.k and a.del_w == b.del_w
        for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
            va, vb = getattr(a, fld), getattr(b, fld)
            assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)
    assert abs(sd.cnt.k - sa.cnt.k) <= 2
    assert abs(sd.obj_val - sa.obj_val) <= 1e-6 * abs(sa.obj_val)
    xs = x[:A.n]
    c = A.cons(xs)                                  # feasibility judged by the hand-written host model
    assert (c >= A.lcon - 1e-5).all() and (c <= A.ucon + 1e-5).all()
    for s in (sd, sa):
        s.cb.close(); s.K.close(); s.kkt.close()
    sh.kkt.close()


def test_a_tape_model_on_the_dense_device_path_is_refused():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    with pytest.raises(NotImplementedError, match="sparse condensed KKT handle only"):
        DeviceMadNLPSolver(T.hs15_tape_model(), lambda info: None, sparse=False)

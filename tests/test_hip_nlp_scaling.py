"""NLP scaling and the objective sense on the device path: the three `mnk_ipm_*` kernels of csrc/nlp_scale.hip against numpy,
the statement that factors of one change no bit of a device run, device runs with non-trivial factors against the host mirror on
the same HIP KKT back-end, and the reference's `test_scaling` / `test_max_problem` LPs as tape models."""
import dataclasses

import numpy as np
import pytest

from nlp_scaling_cases import rescaled_dense_qp, solcmp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)  # torch ops and the library share ONE stream
    c = mj.HipContext(0, stream=st.cuda_stream)
    yield c
    torch.cuda.set_stream(torch.cuda.default_stream())
    c.close()


@pytest.fixture()
def K(ctx):
    from madnlp_jl_amd.ipm_device import IPMDeviceKernels
    k = IPMDeviceKernels(1, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), ctx=ctx)
    yield k
    k.close()


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


LENGTHS = [1, 63, 64, 65, 1000, 0]


# ------------------------------------------------------------------------------------------ G1. the kernels against numpy
@pytest.mark.parametrize("n", LENGTHS)
def test_vec_mul(ctx, K, n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n), rng.standard_normal(n)
    da, db, out = _dev(a), _dev(b), _dev(np.full(n, np.nan))
    K.vec_mul(out, da, db)
    assert np.array_equal(_host(ctx, out), a * b)
    assert np.array_equal(_host(ctx, da), a)
    K.vec_mul(da, da, db)                                # out aliases a
    assert np.array_equal(_host(ctx, da), a * b)


def _cons_mirror(c, cs, slack, ind, rhs):
    c = c.copy()
    if cs is not None:
        c *= cs
    if len(slack):
        c[ind] -= slack
    c -= rhs
    return c


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("m", LENGTHS)
def test_scale_cons_with_every_row_an_inequality_or_none(ctx, K, m, with_scale):
    rng = np.random.default_rng(100 + m)
    c, cs, rhs, slack = rng.standard_normal(m), 10.0 ** rng.uniform(-4, 0, m), rng.standard_normal(m), rng.standard_normal(m)
    for s in (slack, slack[:0]):                         # ind_ineq = the identity (NULL), then ns = 0
        dc = _dev(c)
        K.scale_cons(dc, _dev(cs) if with_scale else None, _dev(s), None, _dev(rhs))
        assert np.array_equal(_host(ctx, dc), _cons_mirror(c, cs if with_scale else None, s, np.arange(m), rhs))


@pytest.mark.parametrize("with_scale", [True, False])
def test_scale_cons_with_equalities(ctx, K, with_scale):
    m, ns = 1000, 37
    rng = np.random.default_rng(7)
    ind = np.sort(rng.choice(m, ns, replace=False))
    pos = np.full(m, -1, dtype=np.int64)
    pos[ind] = np.arange(ns)
    c, cs, rhs, slack = rng.standard_normal(m), 10.0 ** rng.uniform(-4, 0, m), rng.standard_normal(m), rng.standard_normal(ns)
    dc = _dev(c)
    K.scale_cons(dc, _dev(cs) if with_scale else None, _dev(slack), _dev(pos, np.int64), _dev(rhs))
    assert np.array_equal(_host(ctx, dc), _cons_mirror(c, cs if with_scale else None, slack, ind, rhs))


@pytest.mark.parametrize("factor", [1.0, -1.0, 100.0 / 2406.0])
@pytest.mark.parametrize("ntot", LENGTHS)
def test_scale_grad(ctx, K, ntot, factor):
    rng = np.random.default_rng(200 + ntot)
    f = rng.standard_normal(ntot)
    for n in sorted({ntot, ntot // 3}):                  # n < ntot (where there is room) and n == ntot
        df = _dev(f)
        K.scale_grad(df, n, factor)
        want = np.concatenate((f[:n] * factor, np.zeros(ntot - n)))
        assert np.array_equal(_host(ctx, df), want)


def test_bad_arguments_are_refused(ctx, K):
    import madnlp_jl_amd as mj
    lib = mj.lib()
    v, idx = _dev(np.ones(8)), _dev(np.arange(8), np.int64)
    p, q = v.data_ptr(), idx.data_ptr()
    bad = [
        lib.mnk_ipm_vec_mul(K._h, None, p, p, 8), lib.mnk_ipm_vec_mul(K._h, p, p, p, -1), lib.mnk_ipm_vec_mul(None, p, p, p, 8),
        lib.mnk_ipm_scale_cons(K._h, None, p, p, None, 8, p, 8),      # NULL c
        lib.mnk_ipm_scale_cons(K._h, p, p, p, None, 8, None, 8),      # NULL rhs
        lib.mnk_ipm_scale_cons(K._h, p, p, p, None, 8, p, -1), lib.mnk_ipm_scale_cons(K._h, p, p, p, None, -1, p, 8),
        lib.mnk_ipm_scale_cons(K._h, p, p, p, None, 9, p, 8),         # more slacks than rows
        lib.mnk_ipm_scale_cons(K._h, p, p, p, None, 3, p, 8),         # 0 < ns < m without the rows' slack positions
        lib.mnk_ipm_scale_cons(K._h, p, p, None, q, 3, p, 8),         # NULL slack
        lib.mnk_ipm_scale_grad(K._h, None, 4, 8, 1.0), lib.mnk_ipm_scale_grad(K._h, p, -1, 8, 1.0),
        lib.mnk_ipm_scale_grad(K._h, p, 9, 8, 1.0),
    ]
    assert all(rc != 0 for rc in bad), bad
    assert b"mnk_ipm_scale_grad" in lib.mnk_last_error_string()
    assert np.array_equal(_host(ctx, v), np.ones(8))                 # nothing was launched


# ------------------------------------------------------------------------------------------ drivers
def _options(tol=1e-6, **kw):
    from madnlp_jl_amd.ipm import IPMOptions
    o = IPMOptions(tol=tol, **kw)
    o.relax_equality, o.dual_initialization = True, "zero"       # the preset of SparseCondensedKKTSystem
    return o


def _sparse_factory(nlp, ctx):
    import madnlp_jl_amd as mj

    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                           info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    return factory


def _dense_factory(ctx):
    import madnlp_jl_amd as mj

    def factory(info):
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                          device_kkt_ops=True)
    return factory


def _close(*solvers):
    for s in solvers:
        (s if hasattr(s, "cb") else s.kkt).close()       # a device solver closes its callbacks, kernels and KKT handle


# ------------------------------------------------------------------------------------------ G2. factors of one change no bit
@pytest.mark.parametrize("model", ["hs15_tape", "acopf_case30"])
def test_unit_factors_change_no_bit_of_a_device_run(ctx, model):
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import ACOPFModel
    from madnlp_jl_amd.tape_model import hs15_tape_model
    nlp = hs15_tape_model() if model == "hs15_tape" else ACOPFModel("case30")
    runs = []
    for scaling in (True, False):
        s = DeviceMadNLPSolver(nlp, _sparse_factory(nlp, ctx), _options(nlp_scaling=scaling))
        s.solve()
        assert s.status == "SOLVE_SUCCEEDED", s.status
        assert s._scaled == scaling                       # the fused launches ran in the first run, the plain ones in the second
        runs.append((s.host_state(), dataclasses.asdict(s.cnt), s.obj_val))
        assert s.obj_scale == 1.0 and (s.con_scale == 1.0).all()
        _close(s)
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert runs[0][1:] == runs[1][1:]


# ------------------------------------------------------------------------------------------ G3. non-trivial factors, device against host
def _compare(sd, sh):
    """The comparisons of tests/test_ipm_dev_driver.py."""
    assert sd.status == sh.status == "SOLVE_SUCCEEDED", (sd.status, sh.status)
    print("counts (k, factorizations, back-solves): device", (sd.cnt.k, sd.cnt.factorization_cnt, sd.cnt.backsolve_cnt),
          "host", (sh.cnt.k, sh.cnt.factorization_cnt, sh.cnt.backsolve_cnt))
    assert sd.obj_scale == sh.obj_scale and np.array_equal(sd.con_scale, sh.con_scale)
    assert (sd.cnt.k, sd.cnt.factorization_cnt, sd.cnt.backsolve_cnt) == (sh.cnt.k, sh.cnt.factorization_cnt, sh.cnt.backsolve_cnt)
    x, y, zl, zu = sd.host_state()
    np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
    np.testing.assert_allclose(y, sh.y, rtol=0, atol=1e-6 * max(1.0, np.abs(sh.y).max()))
    assert len(sd.history) == len(sh.history)
    for a, b in zip(sd.history, sh.history):
        assert a.k == b.k
        for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
            va, vb = getattr(a, fld), getattr(b, fld)
            assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)  # rtol 1e-5 above 1e-9
    rd, rh = sd.solution(), sh.solution()
    assert abs(rd.objective - rh.objective) <= 1e-8 * max(1.0, abs(rh.objective))
    np.testing.assert_allclose(rd.multipliers, rh.multipliers, rtol=0, atol=1e-6 * max(1.0, np.abs(rh.multipliers).max()))


@pytest.mark.parametrize("model", ["acopf", "acopf_tape"])
def test_scaled_acopf_device_run_reproduces_the_host_mirror(ctx, model):
    """max_gradient = 10 puts both kinds of factor below one on the model as it is (gradient maximum 44.9, Jacobian row maxima up
    to 30.7)."""
    from madnlp_jl_amd.ipm import MadNLPSolver
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver, DeviceOPFCallbacks, DeviceTapeCallbacks
    from madnlp_jl_amd.problems import ACOPFModel
    from madnlp_jl_amd.tape_model import acopf_tape_model
    nlp = ACOPFModel("case30") if model == "acopf" else acopf_tape_model("case30")
    opt = lambda: _options(nlp_scaling=True, nlp_scaling_max_gradient=10.0)  # noqa: E731
    sh = MadNLPSolver(nlp, _sparse_factory(nlp, ctx), opt(), sparse=True)
    sh.solve()
    sd = DeviceMadNLPSolver(nlp, _sparse_factory(nlp, ctx), opt())
    sd.solve()
    assert isinstance(sd.cb, DeviceOPFCallbacks if model == "acopf" else DeviceTapeCallbacks)
    assert sh.obj_scale < 1.0 and sh.con_scale.min() < 1.0 and sh.con_scale.max() == 1.0
    _compare(sd, sh)
    _close(sd, sh)


@pytest.mark.parametrize("approx", ["exact", "bfgs"])
def test_scaled_dense_qp_device_run_reproduces_the_host_mirror(ctx, approx):
    """Equalities (ind_ineq is not the identity: the rows' slack positions), the prescaled QP callbacks, and the quasi-Newton
    path under scaling."""
    from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
    from madnlp_jl_amd.ipm_dev import DeviceDenseQPCallbacks, DeviceMadNLPSolver
    nlp = rescaled_dense_qp(20, 15, 2)
    opt = lambda: IPMOptions(tol=1e-8, nlp_scaling=True, hessian_approximation=approx)  # noqa: E731
    sh = MadNLPSolver(nlp, _dense_factory(ctx), opt(), sparse=False)
    sh.solve()
    sd = DeviceMadNLPSolver(nlp, _dense_factory(ctx), opt(), sparse=False)
    sd.solve()
    assert isinstance(sd.cb, DeviceDenseQPCallbacks) and sd.cb.prescaled and sd.slack_pos_t is not None
    assert sh.obj_scale < 1.0 and sh.con_scale.min() == 100.0 / 1e4
    _compare(sd, sh)
    _close(sd, sh)


# ------------------------------------------------------------------------------------------ G4. the reference's two LPs as tape models
@pytest.mark.parametrize("case", ["test_scaling", "test_max_problem", "test_max_problem_scaled"])
def test_reference_lps_as_tape_models_on_the_device(ctx, case):
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.tape_model import simplex_lp_tape_model
    if case == "test_scaling":
        big, nlp, scaling = 1e6, simplex_lp_tape_model(1e6), True
        want = dict(solution=[1.0, 0.0, 0.0], multipliers=[-1.0], multipliers_L=[0.0, big, 2 * big], objective=[big])
    else:
        nlp, scaling = simplex_lp_tape_model(1.0, minimize=False), case.endswith("scaled")
        want = dict(solution=[0.0, 0.0, 1.0], multipliers=[-3.0], multipliers_L=[2.0, 1.0, 0.0], objective=[3.0])
    s = DeviceMadNLPSolver(nlp, _sparse_factory(nlp, ctx), _options(nlp_scaling=scaling))
    s.solve()
    assert s.status == "SOLVE_SUCCEEDED", s.status
    r = s.solution()
    print(case, s.cnt.k, r)
    if case == "test_scaling":
        assert s.obj_scale == 100.0 / 3e6 and s.con_scale[0] == 100.0 / 1e6
    tol = np.sqrt(s.opt.tol)
    for name, w in want.items():
        assert solcmp(np.atleast_1d(getattr(r, name)), w, tol), (name, getattr(r, name))
    _close(s)

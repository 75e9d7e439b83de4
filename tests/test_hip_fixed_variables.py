"""`fixed_variable_treatment = "make_parameter"` on the device: the `mnk_fix_*` kernels behind
`device_callbacks.DeviceFixedVariableCallbacks` against the host layer (`madnlp_jl_amd.fixed_vars`), and `DeviceMadNLPSolver` against
`MadNLPSolver` on the same HIP back-end, sparse (reduced) and dense (frozen)."""
import dataclasses

import numpy as np
import pytest

from madnlp_jl_amd import fixed_vars as FV
from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.problems import LootsmaModel
from tests.test_fixed_variables_cpu import acopf_fixed, factory, fix, qp_fixed, sparse_options, QP_FIXED, QP_VALUES
from tests.test_hip_tape import edge_model, exact_masks, gpu_ctx, make_callbacks  # noqa: F401  (gpu_ctx is a fixture)

THREADS = 256     # FIX_THREADS in csrc/fixed_vars.hip


def sparse_factory(ctx, nlp):
    import madnlp_jl_amd as mj

    def make(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], *FV.structure(nlp, info), info["ind_ineq"], info["ind_lb"],
                                           info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    return make


def close(*solvers):
    for s in solvers:
        (s if hasattr(s, "cb") else s.kkt).close()       # a device solver closes its callbacks, kernels and KKT handle


def assert_same_run(sd, sh):
    """The conditions of tests/test_hip_tape.py::test_device_resident_tape_acopf_run between a device and a host run."""
    assert sd.status == sh.status == "SOLVE_SUCCEEDED", (sd.status, sh.status)
    assert (sd.cnt.k, sd.cnt.factorization_cnt, sd.cnt.backsolve_cnt) == (sh.cnt.k, sh.cnt.factorization_cnt, sh.cnt.backsolve_cnt)
    x = sd.host_state()[0]
    np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
    for a, b in zip(sd.history, sh.history):
        assert a.k == b.k and a.del_w == b.del_w
        for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
            va, vb = getattr(a, fld), getattr(b, fld)
            assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)


# ------------------------------------------------------------------------------------------------- 1. callback level
@pytest.mark.gpu
def test_device_callbacks_match_the_host_handler(gpu_ctx):
    import torch
    from madnlp_jl_amd.ipm_dev import DeviceFixedVariableCallbacks, DeviceTapeCallbacks, _up
    M = edge_model()
    rng = np.random.default_rng(12)
    where = np.array(sorted({0, M.n - 1} | set(range(0, M.n, 7))
                            | {int(a[i]) for a in (M.jac_J, M.hess_I, M.hess_J) for i in (0, -1)}))
    fix(M, where, rng.uniform(0.2, 1.8, len(where)))
    h = FV.FixedVariableHandler.create(M, True)
    R = h.model
    assert h.fixed.tolist() == where.tolist()
    for count in (len(h.free), len(h.ind_jac_free), len(h.ind_hess_free)):   # more than one workgroup, the last one ragged
        assert count > THREADS and count % THREADS != 0, count
    assert len(h.ind_jac_free) < len(M.jac_I) and len(h.ind_hess_free) < len(M.hess_I)
    inner, K = make_callbacks(gpu_ctx, M, DeviceTapeCallbacks)
    cb = DeviceFixedVariableCallbacks(inner, h, None, "cuda", K)
    assert (cb.n, cb.m) == (len(h.free), M.m)
    jmask, hmask, rmask = exact_masks(M)
    jmask, hmask = jmask[h.ind_jac_free], hmask[h.ind_hess_free]
    assert jmask.sum() and hmask.sum() and (~jmask).sum() and (~hmask).sum()

    def untouched(x):
        xf = cb.fix.x_full_host()
        assert np.array_equal(xf[h.fixed], h.values) and np.array_equal(xf[h.free], x)

    dl = lambda t: t.cpu().numpy().copy()  # noqa: E731
    for sigma, scaled in ((1.0, False), (0.0, True), (0.37, True)):
        x, y = rng.uniform(0.5, 1.5, cb.n), rng.standard_normal(M.m)
        factor = -0.3125 * 1.37 if scaled else 1.0
        scale = rng.uniform(0.25, 4.0, len(h.ind_jac_free)) if scaled else None
        xd, yd = _up(x, "cuda"), _up(y, "cuda")
        sc = None if scale is None else _up(scale, "cuda")
        g = torch.full((cb.n,), np.nan, dtype=torch.float64, device="cuda")
        c = torch.full((M.m,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()       # the uploads ran on torch's stream
        f = cb.obj(xd)
        untouched(x)
        cb.grad(g, xd, factor)
        untouched(x)
        cb.cons(c, xd)
        untouched(x)
        jv = cb.jac_coord(xd, sc)
        untouched(x)
        hv = cb.hess_coord(xd, yd, sigma)
        untouched(x)
        gpu_ctx.synchronize()          # the callbacks ran on the context's stream, the downloads run on torch's
        g, c, jv, hv = dl(g), dl(c), dl(jv), dl(hv)
        rg, rc = R.grad(x) * factor, R.cons(x)
        rj = R.jac_coord(x) if scale is None else R.jac_coord(x) * scale
        rh = R.hess_coord(x, y, sigma)
        assert abs(f - R.obj(x)) <= 1e-13 * np.abs(M.obj_terms(h.expand(x))).sum()
        assert np.array_equal(g, rg)
        assert np.array_equal(c[rmask], rc[rmask])
        assert np.array_equal(jv[jmask], rj[jmask])
        assert np.array_equal(hv[hmask], rh[hmask])
        for got, ref in ((c, rc), (jv, rj), (hv, rh)):
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    cb.close()
    K.close()


# ------------------------------------------------------------------------------------------------- 2. device runs, sparse
@pytest.mark.gpu
def test_device_resident_run_with_fixed_variables_case30(gpu_ctx):
    from madnlp_jl_amd.ipm_dev import DeviceFixedVariableCallbacks, DeviceMadNLPSolver, DeviceTapeCallbacks
    M0 = T.acopf_tape_model("case30")
    s0 = MadNLPSolver(M0, factory("sparse_condensed", M0), sparse_options(), sparse=True)     # CPU oracle: the unfixed optimum
    assert s0.solve() == "SOLVE_SUCCEEDED"
    r0 = s0.solution()
    M, where = acopf_fixed("case30", r0.solution)
    opt = lambda: sparse_options(fixed_variable_treatment="make_parameter")  # noqa: E731
    sh = MadNLPSolver(M, sparse_factory(gpu_ctx, M), opt(), sparse=True)
    sh.solve()
    sd = DeviceMadNLPSolver(M, sparse_factory(gpu_ctx, M), opt())
    sd.solve()
    assert isinstance(sd.cb, DeviceFixedVariableCallbacks) and isinstance(sd.cb.inner, DeviceTapeCallbacks)
    assert sd.n == sh.n == M.n - len(where)
    assert_same_run(sd, sh)
    rd, rh = sd.solution(), sh.solution()
    assert np.array_equal(rd.solution[where], r0.solution[where]) and rd.solution.shape == (M.n,)
    assert abs(rd.objective - r0.objective) <= 1e-6 * abs(r0.objective)
    for zd, zh in ((rd.multipliers_L, rh.multipliers_L), (rd.multipliers_U, rh.multipliers_U)):
        assert zd.shape == (M.n,)
        print("fixed multipliers: max", np.abs(zh[where]).max(), "device - host", np.abs(zd[where] - zh[where]).max())
        assert np.abs(zd[where] - zh[where]).max() <= 1e-7 * np.abs(zh[where]).max()
    close(sd, sh)


@pytest.mark.gpu
def test_device_resident_lootsma_with_its_fixed_parameter(gpu_ctx):
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    M = T.lootsma_fixed_tape_model()
    sd = DeviceMadNLPSolver(M, sparse_factory(gpu_ctx, M), sparse_options(fixed_variable_treatment="make_parameter"))
    sd.solve()
    assert sd.status == "SOLVE_SUCCEEDED" and sd.n == 3
    r = sd.solution()
    tol = np.sqrt(sd.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731  (solcmp)
    assert r.solution[0] == 6.0
    assert cmp(r.solution[1:], LootsmaModel.LOOTSMA_X), r.solution
    assert cmp(r.multipliers, LootsmaModel.LOOTSMA_Y), r.multipliers
    close(sd)


@pytest.mark.gpu
def test_without_fixed_variables_the_device_history_is_identical(gpu_ctx):
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver, DeviceTapeCallbacks
    M = T.acopf_tape_model("case30")
    runs = []
    for treatment in ("make_parameter", "relax_bound"):
        s = DeviceMadNLPSolver(M, sparse_factory(gpu_ctx, M), sparse_options(fixed_variable_treatment=treatment))
        s.solve()
        assert s.fixed_handler is None and type(s.cb) is DeviceTapeCallbacks
        runs.append(([dataclasses.astuple(r) for r in s.history], s.host_state()))
        close(s)
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ------------------------------------------------------------------------------------------------- 3. device run, dense
@pytest.mark.gpu
def test_device_resident_dense_run_with_frozen_variables(gpu_ctx):
    """The comparison of tests/test_ipm_dev_driver.py::test_device_resident_ipm_on_the_dense_condensed_system."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    nlp = qp_fixed(2)

    def dense_factory(info):
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=gpu_ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                          device_kkt_ops=True)
    opt = lambda: IPMOptions(tol=1e-8, fixed_variable_treatment="make_parameter")  # noqa: E731
    sh = MadNLPSolver(nlp, dense_factory, opt(), sparse=False)
    sh.solve()
    sd = DeviceMadNLPSolver(nlp, dense_factory, opt(), sparse=False)
    sd.solve()
    assert sd.status == sh.status == "SOLVE_SUCCEEDED"
    assert (sd.cnt.k, sd.cnt.factorization_cnt) == (sh.cnt.k, sh.cnt.factorization_cnt)
    x, y, zl, zu = sd.host_state()
    np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
    np.testing.assert_allclose(y, sh.y, rtol=0, atol=1e-6 * max(1.0, np.abs(sh.y).max()))
    for a, b in zip(sd.history, sh.history):
        assert a.k == b.k
        for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
            va, vb = getattr(a, fld), getattr(b, fld)
            assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)
    assert sd.solution().solution[QP_FIXED].tolist() == QP_VALUES == sh.solution().solution[QP_FIXED].tolist()
    close(sd, sh)

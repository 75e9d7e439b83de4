"""The adaptive barrier updates (`barrier = "loqo" / "quality_function"`) on the device-resident driver: the control flow is
`MadNLPSolver`'s, `DeviceMadNLPSolver` supplies the primitives -- the two complementarity reductions, the affine and centering
right-hand sides, the plain KKT solve and `mnk_ipm_quality_function`.  As tests/test_ipm_dev_driver.py: one stream, the HIP KKT
back-end for both drivers, the same margins.  On these inputs the closest pair of quality values inside any one golden-section
search of the host run differs by 2.5e-5 relative (case30) and 1.1e-5 (the dense QP), so the ~1e-15 difference between the
host's and the device's order of summation cannot flip a decision of the search."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)      # torch ops and the library share ONE stream
    c = mj.HipContext(0, stream=st.cuda_stream)
    yield c
    torch.cuda.set_stream(torch.cuda.default_stream())
    c.close()


def sparse_factory(nlp, ctx):
    import madnlp_jl_amd as mj

    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                           info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    return factory


def dense_factory(ctx):
    import madnlp_jl_amd as mj

    def factory(info):
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                          device_kkt_ops=True)
    return factory


def sparse_options(**kw):
    from madnlp_jl_amd.ipm import IPMOptions
    o = IPMOptions(tol=1e-6, **kw)
    o.relax_equality, o.dual_initialization = True, "zero"       # the preset of SparseCondensedKKTSystem
    return o


def close(*solvers):
    for s in solvers:
        if hasattr(s, "cb"):
            s.cb.close()
            s.K.close()
        s.kkt.close()


@pytest.mark.parametrize("barrier", ["loqo", "quality_function"])
@pytest.mark.parametrize("system", ["sparse_case30", "dense_20_15_2"])
def test_device_driver_reproduces_the_host_driver(ctx, system, barrier):
    """Same status, k, factorization and update counts, x within 1e-7 max(1, |x|max), residual and mu histories within 1e-5
    relative above 1e-9.  Under the adaptive rules mu is a multiple of the average complementarity, a SUM that enters the
    iterate: the host takes it in the device reduction's order (`ipm.ordered_sum`), so mu starts out bit-identical on both
    drivers.  Summed in numpy's order instead, mu differed by 2e-15 relative on case30 with the quality function, and the
    un-refined solve error of the following full step (inf_du = 1.5e-8 at k = 4, after an iteration at mu = 4.6e-7) came out
    2.4e-9 apart, outside the 1e-9 floor of these margins."""
    from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import DenseQPModel, SparseQPModel
    if system == "sparse_case30":
        nlp = SparseQPModel("case30")
        make = lambda cls: cls(nlp, sparse_factory(nlp, ctx), sparse_options(barrier=barrier), sparse=True)  # noqa: E731
    else:
        nlp = DenseQPModel(20, 15, 2)
        make = lambda cls: cls(nlp, dense_factory(ctx), IPMOptions(tol=1e-8, barrier=barrier), sparse=False)  # noqa: E731
    sh = make(MadNLPSolver)
    sh.solve()
    sd = make(DeviceMadNLPSolver)
    sd.solve()
    counts = lambda s: (s.cnt.k, s.cnt.factorization_cnt, s.cnt.barrier_update_cnt)  # noqa: E731
    print("status, (k, factorizations, barrier updates): device", sd.status, counts(sd), "host", sh.status, counts(sh))
    assert sd.status == sh.status == "SOLVE_SUCCEEDED", (sd.status, sh.status)
    assert counts(sd) == counts(sh)
    assert sd.cnt.probe_solve_cnt == sh.cnt.probe_solve_cnt == (2 * sh.cnt.barrier_update_cnt if barrier == "quality_function" else 0)
    if barrier == "quality_function":
        assert sh.cnt.barrier_update_cnt > 0 and sd.cnt.quality_eval_cnt == sh.cnt.quality_eval_cnt
    x = sd.host_state()[0]
    np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
    assert len(sd.history) == len(sh.history)
    for a, b in zip(sd.history, sh.history):
        assert a.k == b.k
        for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
            va, vb = getattr(a, fld), getattr(b, fld)
            assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)  # rtol 1e-5 above 1e-9
    close(sh, sd)


@pytest.mark.parametrize("n", [0, 1, 3, 255, 257, 65536, 65537, 200001])
def test_ordered_sum_has_the_bits_of_the_device_sum(ctx, n):
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.ipm import ordered_sum
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)       # both signs, 16 decades: every order gives other bits
    K = mj.IPMDeviceKernels(max(n, 1), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), ctx=ctx)
    t = torch.from_numpy(np.ascontiguousarray(v if n else np.zeros(1))).cuda()
    got = K.get_sum(t[:n])
    K.close()
    assert np.float64(got).view(np.int64) == np.float64(ordered_sum(v)).view(np.int64), (got, ordered_sum(v), float(v.sum()))


def test_average_complementarity_has_the_same_bits_on_both_back_ends(ctx):
    """ntot = 70001 with 65537 lower bounds: the second trip of the grid-stride loop."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.ipm import ordered_sum
    rng = np.random.default_rng(7)
    ntot, nlb, nub = 70001, 65537, 300
    lb, ub = np.sort(rng.choice(ntot, nlb, replace=False)), np.sort(rng.choice(ntot, nub, replace=False))
    xl, xu = np.full(ntot, -np.inf), np.full(ntot, np.inf)
    xl[lb], xu[ub] = -rng.uniform(0.5, 2.0, nlb), rng.uniform(0.5, 2.0, nub)
    x = rng.uniform(-0.45, 0.45, ntot)
    zl, zu = np.zeros(ntot), np.zeros(ntot)
    zl[lb], zu[ub] = 10.0 ** rng.uniform(-9, 3, nlb), 10.0 ** rng.uniform(-9, 3, nub)
    K = mj.IPMDeviceKernels(ntot, lb, ub, ctx=ctx)
    g = [torch.from_numpy(a).cuda() for a in (x, xl, xu, zl, zu)]
    got = K.get_average_complementarity(*g)
    K.close()
    want = (ordered_sum((x[lb] - xl[lb]) * zl[lb]) + ordered_sum((xu[ub] - x[ub]) * zu[ub])) / (nlb + nub)
    assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), (got, want)


_monotone = {}


@pytest.mark.parametrize("config", ["loqo", "quality_function", "quality_function_no_globalization"])
def test_hs15_tape_model_on_the_device_reaches_the_monotone_solution(ctx, config):
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.tape_model import hs15_tape_model

    def solve(**kw):
        nlp = hs15_tape_model()
        nlp.x0 = np.array([1.0, 1.0])      # from (0, 0) the adaptive rules reach HS15's other local optimum
        s = DeviceMadNLPSolver(nlp, sparse_factory(nlp, ctx), sparse_options(**kw))
        s.solve()
        x, y = s.host_state()[:2]
        out = (s.status, s.cnt.k, x[:s.n].copy(), y.copy(), s.opt.tol)
        close(s)
        return out

    if not _monotone:
        _monotone["run"] = solve()
    status0, _, x0, y0, _ = _monotone["run"]
    assert status0 == "SOLVE_SUCCEEDED"
    kw = dict(barrier=config.replace("_no_globalization", ""), barrier_globalization=not config.endswith("_no_globalization"))
    status, k, x, y, tol = solve(**kw)
    print(config, status, k, "max |x - x_monotone|", np.abs(x - x0).max(), "max |y - y_monotone|", np.abs(y - y0).max())
    assert status == "SOLVE_SUCCEEDED", status
    approx = lambda a, b: np.linalg.norm(a - b) <= max(math.sqrt(tol), math.sqrt(tol) * max(np.linalg.norm(a), np.linalg.norm(b)))  # noqa: E731
    assert approx(x, x0) and approx(y, y0)

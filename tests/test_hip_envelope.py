"""The envelope skip of the task-DAG schedule (-m gpu): the bulk kernel starts every K-loop behind the
structurally zero tile columns of its operands and closes the tiles left of a row's envelope without computing them.  The
products it drops are exact zeros, so the factor, D, the inertia and the solves are those of the dense order -- checked here
against the same solver with the option "envelope" = 0."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd.problems import OPF_CASES, opf_shaped  # noqa: E402

# (nbus, ngen, nbranch) -> order n = 2 nbus + 2 ngen + 4 nbranch: the schedule's window 1280 .. 30 720 with the band-only
# shape (every row in the chain's band) and the band + bulk shape
SHAPES = {
    "n1504": (160, 32, 280),      # 1504: deep band (bulk tasks accumulate band tiles only)
    "n5808": (600, 104, 1100),    # band + bulk
    "case1354pegase": OPF_CASES["case1354pegase"],   # 11 192: the bench system (C3)
    "n19680": (2400, 440, 3500),  # 19 680
}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def _kkt(P, ctx, alg=mj.BUNCHKAUFMAN):
    k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                    opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=alg))
    return k


def _load(k, P, hess=None):
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess if hess is None else hess
    k.compress_jacobian()
    k.compress_hessian()
    k.set_aug_diagonal()
    k.build_kkt()


def _factor(k, envelope):
    ls = k.linear_solver
    ls.set_option("envelope", envelope)
    ls.factorize()
    inertia = ls.inertia()
    Lf, D = ls.get_factor_device()
    rng = np.random.default_rng(7)
    xs = [ls.solve_linear_system(rng.standard_normal(k.n)) for _ in range(2)]
    stats = {s: ls.get_stat(s) for s in ("panel_algo", "pp_fallbacks", "env_ksteps", "env_ksteps_skipped", "early_reject_col")}
    return dict(L=torch.tril(Lf).clone(), D=D.clone(), inertia=inertia, info=ls.info, xs=xs, stats=stats)


def _assert_same(a, b, what, same_solver=True):
    assert a["inertia"] == b["inertia"] and a["info"] == b["info"], what
    assert torch.equal(a["L"], b["L"]) and torch.equal(a["D"], b["D"]), what   # (== : +0 and -0 compare equal)
    for xa, xb in zip(a["xs"], b["xs"]):
        np.testing.assert_array_equal(xa, xb, err_msg=what)
    if same_solver:   # (a statistic of the solver's history)
        assert a["stats"]["early_reject_col"] == b["stats"]["early_reject_col"], what


def _bytes_equal(a, b):
    return (torch.equal(a["L"].view(torch.int64), b["L"].view(torch.int64)) and torch.equal(a["D"].view(torch.int64), b["D"].view(torch.int64))
            and all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a["xs"], b["xs"])))


@pytest.mark.parametrize("shape,seed", [("n1504", 1), ("n5808", 2), ("case1354pegase", None), ("case1354pegase", 77),
                                        ("n19680", 3)])
def test_envelope_keeps_the_factor_and_the_solves(ctx, shape, seed):
    P = opf_shaped(SHAPES[shape], seed=seed, du=1e-8)
    k = _kkt(P, ctx)
    try:
        _load(k, P)
        on = _factor(k, 1)
        off = _factor(k, 0)
        on2 = _factor(k, 1)   # (after a dense factorization of the same solver: V of the skipped tiles is rewritten)
        for r in (on, off, on2):
            assert r["stats"]["panel_algo"] == 5.0 and r["stats"]["pp_fallbacks"] == 0.0
        assert on["inertia"] == (P.n, 0, 0)
        _assert_same(on, off, shape)
        _assert_same(on2, off, shape)
        assert off["stats"]["env_ksteps_skipped"] == 0.0
        assert on["stats"]["env_ksteps"] == off["stats"]["env_ksteps"]
        if shape != "n1504":   # (band-only shape: the band tiles' accumulation may lie inside the envelope entirely)
            assert on["stats"]["env_ksteps_skipped"] > 0.0
        print(f"{shape} n={P.n}: k-steps {on['stats']['env_ksteps']:.0f}, skipped {on['stats']['env_ksteps_skipped']:.0f}, "
              f"byte-equal {_bytes_equal(on, off)}")
    finally:
        k.close()


def test_envelope_with_early_rejection(ctx):
    """An indefinite matrix under early rejection (accept_only_pd): the same rejection column and inertia bound."""
    P = opf_shaped("case1354pegase", indefinite=True, du=1e-8)
    k = _kkt(P, ctx)
    try:
        _load(k, P)
        ls = k.linear_solver
        ls.set_option("accept_only_pd", 1)
        ls.set_option("early_reject", 1)
        res = []
        for env in (1, 0):
            ls.set_option("envelope", env)
            ls.factorize()
            res.append((ls.inertia(), ls.info, ls.get_stat("early_reject_col"), ls.get_stat("early_rejects")))
        assert res[0][:3] == res[1][:3] and res[0][3] + 1 == res[1][3], res
        assert res[0][0] != (P.n, 0, 0)
    finally:
        k.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_entry_turns_the_envelope_off(ctx, bad):
    """A NaN / Inf spreads through 0 * NaN into rows outside the envelope in the dense order: with one in the transferred matrix
    the bulk kernel skips nothing, and info, inertia and pivots are exactly those of envelope = 0.  The next finite matrix on the
    same solver skips again."""
    P = opf_shaped("case1354pegase", du=1e-8)
    hess = P.hess.copy()
    hess[len(hess) // 3] = bad
    k = _kkt(P, ctx)
    try:
        _load(k, P, hess)
        ls = k.linear_solver
        res = []
        for env in (1, 0):
            ls.set_option("envelope", env)
            ls.factorize()
            _, D = ls.get_factor_device()
            res.append((ls.inertia(), ls.info, ls.get_stat("env_ksteps_skipped"), D.cpu().numpy()))
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1], (res[0][:3], res[1][:3])
        assert res[0][2] == 0.0
        np.testing.assert_array_equal(res[0][3], res[1][3])
        _load(k, P)
        ls.set_option("envelope", 1)
        ls.factorize()
        assert ls.inertia() == (P.n, 0, 0) and ls.get_stat("env_ksteps_skipped") > 0.0
    finally:
        k.close()


def test_stale_v_cannot_leak(ctx):
    """V = L D is never refilled: a solver that has just factored a matrix with a NaN (dense order, NaN in V everywhere) and then
    factors the finite one with the envelope gives exactly what a fresh solver gives."""
    P = opf_shaped("case1354pegase", seed=5, du=1e-8)
    hess = P.hess.copy()
    hess[7] = np.nan
    k1, k2 = _kkt(P, ctx), _kkt(P, ctx)
    try:
        _load(k1, P, hess)
        k1.linear_solver.factorize()
        k1.linear_solver.inertia()
        _load(k1, P)
        a = _factor(k1, 1)
        _load(k2, P)
        b = _factor(k2, 1)
        assert a["stats"]["env_ksteps_skipped"] > 0.0
        _assert_same(a, b, "stale V", same_solver=False)
        assert np.isfinite(a["L"].cpu().numpy()).all()
    finally:
        k1.close()
        k2.close()


def test_batch_of_16_different_graphs_matches_lone_calls(ctx):
    """16 instances with 16 different graphs (and envelopes) in one merged launch: bit-identical to one-by-one factorizations."""
    base = OPF_CASES["case1354pegase"][0]
    Ps = [opf_shaped("case1354pegase", seed=base + 300 + i, du=1e-8) for i in range(16)]
    ks = [_kkt(P, ctx) for P in Ps]
    try:
        ref = []
        for P, k in zip(Ps, ks):
            _load(k, P)
            k.linear_solver.factorize()
            assert k.linear_solver.inertia() == (P.n, 0, 0)
            Lf, D = k.linear_solver.get_factor_device()
            ref.append((torch.tril(Lf).clone(), D.clone()))
            assert k.linear_solver.get_stat("env_ksteps_skipped") > 0.0
        with mj.factorize_batch():
            for P, k in zip(Ps, ks):
                k.linear_solver.factorize_async()
        for i, (P, k) in enumerate(zip(Ps, ks)):
            ls = k.linear_solver
            assert ls.inertia() == (P.n, 0, 0)
            assert ls.get_stat("panel_algo") == 5.0 and ls.get_stat("pp_fallbacks") == 0.0
            assert ls.get_stat("env_ksteps_skipped") > 0.0
            Lf, D = ls.get_factor_device()
            assert torch.equal(torch.tril(Lf), ref[i][0]) and torch.equal(D, ref[i][1]), i
    finally:
        for k in ks:
            k.close()


def test_probe_child_keeps_the_interior_point_run(ctx):
    """The AC-OPF run of case1354pegase with the leading-block probe (its child solver factors a leading block of the same handle
    with the truncated envelope): the same iterations, trials, perturbations and optimum with the envelope on and off."""
    from madnlp_jl_amd.ipm import IPMOptions
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import ACOPFModel
    nlp = ACOPFModel("case1354pegase")
    runs = {}
    for env in (0, 1):
        def factory(info):
            k = mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                            info["ind_lb"], info["ind_ub"], ctx=ctx,
                                            opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                            device_kkt_ops=True)
            k.linear_solver.set_option("envelope", env)
            return k
        o = IPMOptions(tol=1e-6)
        o.relax_equality, o.dual_initialization = True, "zero"
        s = DeviceMadNLPSolver(nlp, factory, o)
        s.probe = True
        s.initialize(); s._upload(); torch.cuda.synchronize()
        s.solve(); torch.cuda.synchronize()
        runs[env] = (s.status, s.cnt.k, s.cnt.factorization_cnt, s.obj_val, [h.del_w for h in s.history], s.probe_hits)
        s.cb.close(); s.K.close(); s.kkt.close()
    assert runs[0][0] == "SOLVE_SUCCEEDED"
    assert runs[0] == runs[1], (runs[0][:4], runs[1][:4])
    print(f"iterations {runs[1][1]}, factorizations {runs[1][2]}, probe hits {runs[1][5]}")

"""The half-tile skip of the task-DAG bulk kernel (-m gpu): inside the tile envelope the waves of a chunk's
K-loop skip the k-tiles left of the envelopes of their own 64-row halves and never multiply the upper quadrant of a diagonal tile.
What they drop are products with an exact zero factor (or entries nobody reads), so the factor, D, the inertia and the solves are
those of the tile-level skip -- checked here with the option "envelope_half" on against off, "envelope" = 1 both times, at the
smallest orders of the schedule."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd.problems import opf_shaped  # noqa: E402

# (nbus, ngen, nbranch) -> order n = 2 nbus + 2 ngen + 4 nbranch
SHAPES = {
    "n1336": (140, 28, 250),    # 1336 = 10 * 128 + 56: the lower half of the last tile row is padding only
    "n1504": (192, 32, 264),    # 1504: variable blocks end at rows 192 = 3 * 64 and 448 = 7 * 64, inside a tile
    "n2624": (280, 52, 490),    # 2624 = 20.5 tiles
}
STATS = ("panel_algo", "pp_fallbacks", "env_ksteps", "env_ksteps_skipped", "envh_ksteps", "envh_ksteps_skipped", "early_reject_col")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def _kkt(P, ctx, alg=mj.BUNCHKAUFMAN):
    return mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                       opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=alg))


def _load(k, P, hess=None):
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.jac[:] = P.jac
    k.hess[:] = P.hess if hess is None else hess
    k.compress_jacobian()
    k.compress_hessian()
    k.set_aug_diagonal()
    k.build_kkt()


def _result(ls, n):
    inertia = ls.inertia()
    Lf, D = ls.get_factor_device()
    rng = np.random.default_rng(7)
    xs = [ls.solve_linear_system(rng.standard_normal(n)) for _ in range(2)]
    return dict(L=torch.tril(Lf).clone(), D=D.clone(), inertia=inertia, info=ls.info, xs=xs, stats={s: ls.get_stat(s) for s in STATS})


def _factor(ls, n, half):
    ls.set_option("envelope", 1)
    ls.set_option("envelope_half", half)
    ls.factorize()
    return _result(ls, n)


def _assert_same(a, b, what):
    assert a["inertia"] == b["inertia"] and a["info"] == b["info"], what
    assert torch.equal(a["L"], b["L"]) and torch.equal(a["D"], b["D"]), what   # (== : +0 and -0 compare equal)
    for xa, xb in zip(a["xs"], b["xs"]):
        np.testing.assert_array_equal(xa, xb, err_msg=what)


def _assert_skipped(on, off, what):
    for r in (on, off):
        assert r["stats"]["panel_algo"] == 5.0 and r["stats"]["pp_fallbacks"] == 0.0, what
    assert on["stats"]["envh_ksteps_skipped"] > 0.0 and off["stats"]["envh_ksteps_skipped"] == 0.0, what
    assert on["stats"]["envh_ksteps"] == off["stats"]["envh_ksteps"] > 0.0, what
    assert on["stats"]["env_ksteps_skipped"] == off["stats"]["env_ksteps_skipped"], what   # (the tile-level skip is the same)


@pytest.mark.parametrize("alg", [mj.BUNCHKAUFMAN, mj.CHOLESKY])
@pytest.mark.parametrize("shape,seed", [("n1336", 11), ("n1504", 12), ("n2624", 13)])
def test_half_skip_keeps_the_factor_and_the_solves(ctx, shape, seed, alg):
    P = opf_shaped(SHAPES[shape], seed=seed, du=1e-8)
    assert P.n == int(shape[1:])
    k = _kkt(P, ctx, alg)
    try:
        _load(k, P)
        ls = k.linear_solver
        on = _factor(ls, P.n, 1)
        off = _factor(ls, P.n, 0)
        on2 = _factor(ls, P.n, 1)
        assert on["inertia"] == (P.n, 0, 0)
        _assert_skipped(on, off, shape)
        _assert_same(on, off, shape)
        _assert_same(on2, off, shape)
        print(f"{shape} {alg}: half-tile k-steps {on['stats']['envh_ksteps']:.0f}, skipped {on['stats']['envh_ksteps_skipped']:.0f}")
    finally:
        k.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_entry_turns_the_half_skip_off(ctx, bad):
    """The gate of the tile envelope (a NaN / Inf entry in the transferred matrix) closes the half-tile skip with it: the same info,
    inertia and D with the option on and off (NaN positions included), and both skips report nothing skipped for that call."""
    P = opf_shaped(SHAPES["n2624"], seed=21, du=1e-8)
    hess = P.hess.copy()
    hess[len(hess) // 3] = bad
    k = _kkt(P, ctx)
    try:
        _load(k, P, hess)
        ls = k.linear_solver
        ls.set_option("envelope", 1)
        res = []
        for half in (1, 0):
            ls.set_option("envelope_half", half)
            ls.factorize()
            _, D = ls.get_factor_device()
            res.append((ls.inertia(), ls.info, ls.get_stat("envh_ksteps_skipped"), ls.get_stat("env_ksteps_skipped"), D.cpu().numpy()))
        assert res[0][:2] == res[1][:2], (res[0][:4], res[1][:4])
        assert res[0][2] == 0.0 and res[0][3] == 0.0 and res[1][2] == 0.0
        np.testing.assert_array_equal(np.isnan(res[0][4]), np.isnan(res[1][4]))
        np.testing.assert_array_equal(res[0][4], res[1][4])   # (NaN == NaN here)
        # the next finite matrix on the same solver skips again
        _load(k, P)
        ls.set_option("envelope_half", 1)
        ls.factorize()
        assert ls.inertia() == (P.n, 0, 0) and ls.get_stat("envh_ksteps_skipped") > 0.0
    finally:
        k.close()


@pytest.mark.parametrize("alg", [mj.BUNCHKAUFMAN, mj.CHOLESKY])
def test_sparse_after_dense_on_the_same_solver(ctx, alg):
    """A dense source fills what the sparse one leaves structurally zero -- the upper quadrants of diagonal tiles, V left of the
    envelope -- with numbers.  The sparse factorization that follows must not see them, with the half-tile skip or without."""
    P = opf_shaped(SHAPES["n1504"], seed=31, du=1e-8)
    k = _kkt(P, ctx, alg)
    try:
        _load(k, P)
        ls = k.linear_solver
        sparse = ls.A
        rng = np.random.default_rng(3)
        G = rng.standard_normal((P.n, 16))
        dense = np.asfortranarray(G @ G.T + 0.5 * rng.random((P.n, P.n)) + P.n * np.eye(P.n))
        dense = np.asfortranarray(0.5 * (dense + dense.T))
        res = {}
        for half in (1, 0):
            ls.A = dense
            ls.set_option("envelope_half", half)
            ls.factorize()
            assert ls.inertia() == (P.n, 0, 0) and ls.get_stat("envh_ksteps_skipped") == 0.0   # (a dense source has no envelope)
            ls.A = sparse
            res[half] = _factor(ls, P.n, half)
        _assert_skipped(res[1], res[0], "after dense")
        _assert_same(res[1], res[0], "after dense")
        assert res[1]["inertia"] == (P.n, 0, 0) and np.isfinite(res[1]["L"].cpu().numpy()).all()
    finally:
        k.close()


def test_half_skip_with_early_rejection(ctx):
    """An indefinite matrix under early rejection (accept_only_pd): the same rejection column and inertia bound on and off."""
    P = opf_shaped(SHAPES["n2624"], seed=41, indefinite=True, du=1e-8)
    k = _kkt(P, ctx)
    try:
        _load(k, P)
        ls = k.linear_solver
        ls.set_option("accept_only_pd", 1)
        ls.set_option("early_reject", 1)
        ls.set_option("envelope", 1)
        res = []
        for half in (1, 0):
            ls.set_option("envelope_half", half)
            ls.factorize()
            res.append((ls.inertia(), ls.info, ls.get_stat("early_reject_col"), ls.get_stat("early_rejects")))
        assert res[0][:3] == res[1][:3] and res[0][3] + 1 == res[1][3], res
        assert res[0][0] != (P.n, 0, 0)
    finally:
        k.close()


def test_batch_of_4_different_graphs_matches_lone_calls(ctx):
    """Four instances with four different graphs in one merged launch (tile-level skip) against lone factorizations with the
    half-tile skip: bit-identical lower factors and pivots."""
    Ps = [opf_shaped(SHAPES["n2624"], seed=500 + i, du=1e-8) for i in range(4)]
    ks = [_kkt(P, ctx) for P in Ps]
    try:
        ref = []
        for P, k in zip(Ps, ks):
            _load(k, P)
            ls = k.linear_solver
            ls.set_option("envelope_half", 1)
            ls.factorize()
            assert ls.inertia() == (P.n, 0, 0) and ls.get_stat("envh_ksteps_skipped") > 0.0
            Lf, D = ls.get_factor_device()
            ref.append((torch.tril(Lf).clone(), D.clone()))
        with mj.factorize_batch():
            for k in ks:
                k.linear_solver.factorize_async()
        for i, (P, k) in enumerate(zip(Ps, ks)):
            ls = k.linear_solver
            assert ls.inertia() == (P.n, 0, 0)
            assert ls.get_stat("pp_fallbacks") == 0.0
            Lf, D = ls.get_factor_device()
            assert torch.equal(torch.tril(Lf), ref[i][0]) and torch.equal(D, ref[i][1]), i
    finally:
        for k in ks:
            k.close()


def test_probe_child_of_a_smaller_order(ctx):
    """A solver of a smaller order on the leading block of the same handle (the probe's child) uses the leading part of the
    half-tile envelope; 1472 = 23 * 64 rows: the lower half of its last tile row is padding where the parent has matrix rows."""
    P = opf_shaped(SHAPES["n2624"], seed=51, du=1e-8)
    k = _kkt(P, ctx)
    try:
        _load(k, P)
        m = 1472
        ps = k.probe_solver(m)
        ps.set_option("accept_only_pd", 0)
        ps.set_option("early_reject", 0)
        on = _factor(ps, m, 1)
        off = _factor(ps, m, 0)
        assert on["inertia"] == (m, 0, 0)
        _assert_skipped(on, off, "child")
        _assert_same(on, off, "child")
    finally:
        k.close()

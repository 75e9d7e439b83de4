"""Compact L-BFGS Hessians on the sparse condensed KKT system, host specification (`madnlp_jl_amd.quasi_newton.CompactLBFGS`,
`kkt.LowRankHessianKKT`, the `"compact_lbfgs"` option of `MadNLPSolver`) on the CPU oracle.  No GPU.

Error rule of the comparisons with the longdouble BFGS recursion: U = W J^-T with J J' = M, so U U' = W M^-1 W' carries a
relative error of about cond(M) eps, where the three terms of an entry of sigma I - U U' + V V' have the sizes sigma, |U U'| and
|V V'|:  err <= 100 eps cond(M) max(sigma, max|U U'|, max|V V'|)  with cond(M) computed from the mirror's own M."""
import ctypes as C

import numpy as np
import pytest

import madnlp_jl_amd as mj
from lbfgs_cases import EPS, compact_dense, ld_bfgs, random_pairs, scripted_sequence
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.kkt import LowRankHessianKKT
from madnlp_jl_amd.problems import ACOPFModel, HS15Model, LootsmaModel
from madnlp_jl_amd.quasi_newton import (SCALAR1, SCALAR2, SCALAR3, SCALAR4, CompactLBFGS, QuasiNewtonOptions, curvature,
                                        odot)
from oracle import hs15
from oracle.kernels import UnreducedKKTVector, set_aug_diagonal
from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver
from oracle.sparse_condensed import SparseCondensedKKTSystem


def solcmp(x, sol, atol=1e-4, rtol=1e-4):
    """reference `solcmp` lib/MadNLPTests/src/MadNLPTests.jl:18-22."""
    aerr = np.linalg.norm(x - sol, np.inf)
    return aerr < atol or aerr / np.linalg.norm(sol, np.inf) < rtol


def run_updates(n, history, k, seed, strategy=SCALAR1):
    S, Y = random_pairs(n, k, seed)
    qn = CompactLBFGS(n, QuasiNewtonOptions(max_history=history, init_strategy=strategy))
    B = np.zeros(n)
    for i in range(k):
        assert qn.update(B, S[:, i], Y[:, i])
    return qn, B, S, Y


def bound(qn):
    scale = max(qn.sigma, np.abs(qn.U @ qn.U.T).max(), np.abs(qn.V @ qn.V.T).max())
    return 100 * EPS * np.linalg.cond(qn.M) * scale


# ------------------------------------------------------------------------------------------ 1. the update
@pytest.mark.parametrize("n", [1, 2, 7, 65])
@pytest.mark.parametrize("history", [1, 2, 6])
@pytest.mark.parametrize("kk", ["one", "history", "history+3"])
def test_compact_representation_equals_the_longdouble_bfgs_recursion(n, history, kk):
    k = {"one": 1, "history": history, "history+3": history + 3}[kk]
    qn, B, S, Y = run_updates(n, history, k, 100 * n + 10 * history + k)
    p = min(k, history)
    assert qn.current_mem == p and qn.updates == k and qn.skipped == 0
    assert np.array_equal(qn.S, S[:, k - p:k]) and np.array_equal(qn.Y, Y[:, k - p:k])      # the shift keeps the newest pairs
    assert np.all(B == qn.sigma)
    ref = ld_bfgs(qn.sigma, qn.S, qn.Y)
    err = float(np.abs(compact_dense(qn.sigma, qn.U, qn.V) - ref).max())
    print(f"n={n} history={history} k={k}: err {err:.3e} bound {bound(qn):.3e} cond(M) {np.linalg.cond(qn.M):.3e}")
    assert err <= bound(qn)


@pytest.mark.parametrize("n,history,k", [(2, 1, 3), (7, 2, 5), (65, 6, 9), (65, 6, 3)])
def test_secant_equation(n, history, k):
    qn, B, S, Y = run_updates(n, history, k, 7 * n + k)
    s, y = S[:, k - 1], Y[:, k - 1]
    Bs = qn.sigma * s - qn.U @ (qn.U.T @ s) + qn.V @ (qn.V.T @ s)
    err = np.abs(Bs - y).max()
    print(f"n={n} history={history} k={k}: |B s - y| {err:.3e} bound {bound(qn) * np.abs(s).sum():.3e}")
    assert err <= bound(qn) * np.abs(s).sum()


@pytest.mark.parametrize("strategy", [SCALAR1, SCALAR2, SCALAR3, SCALAR4])
def test_curvature_rules_and_the_clamp(strategy):
    S, Y = random_pairs(7, 1, 5)
    s, y = S[:, 0], Y[:, 0]
    ss, sy, yy = odot(s, s), odot(s, y), odot(y, y)
    want = {SCALAR1: sy / ss, SCALAR2: yy / sy, SCALAR3: ((sy / ss) + (yy / sy)) / 2,
            SCALAR4: np.sqrt((sy / ss) * (yy / sy))}[strategy]
    assert curvature(strategy, ss, sy, yy) == want
    for lo, hi, expect in ((1e-8, 1e8, want), (2 * want, 1e8, 2 * want), (1e-8, want / 2, want / 2)):
        qn = CompactLBFGS(7, QuasiNewtonOptions(init_strategy=strategy, sigma_min=lo, sigma_max=hi))
        B = np.zeros(7)
        assert qn.update(B, s, y)
        assert qn.sigma == expect and np.all(B == expect)
    with pytest.raises(ValueError, match="init_strategy"):
        CompactLBFGS(3, QuasiNewtonOptions(init_strategy=5))


def test_init_branches():
    """`init!` quasi_newton.jl:425-437: the three rho0 branches, times init_value."""
    g = np.array([3.0, 4.0])
    for g0, f0, rho in ((g * 1e-5, 7.0, 1.0), (g, 0.0, 1.0 / 25.0), (g, -50.0, 2.0)):
        for init_value in (1.0, 0.25):
            qn = CompactLBFGS(2, QuasiNewtonOptions(init_value=init_value))
            B = np.zeros(2)
            qn.init(B, g0, f0)
            assert np.all(B == 2.0 * rho * init_value) and qn.current_mem == 0


# ------------------------------------------------------------------------------------------ 2. skip and reset
def test_skip_keeps_the_history_and_the_second_skip_resets():
    n = 7
    qn = CompactLBFGS(n, QuasiNewtonOptions(max_history=3))
    B = np.zeros(n)
    log = []
    for s, y, ok in scripted_sequence(n):
        before = (qn.current_mem, qn.S.copy(), qn.U.copy(), B.copy())
        assert qn.update(B, s, y) == ok
        log.append(qn.current_mem)
        if not ok and qn.current_mem:          # an isolated skip: nothing moves
            assert qn.current_mem == before[0] and np.array_equal(qn.S, before[1]) and np.array_equal(qn.U, before[2])
        if not ok:
            assert np.array_equal(B, before[3])
    assert log == [1, 2, 3, 3, 3, 3, 3, 0, 0, 1]
    assert (qn.updates, qn.skipped, qn.resets) == (7, 3, 1)
    # tiny vectors are skipped too (100 eps)
    qn2 = CompactLBFGS(n)
    assert not qn2.update(B, np.full(n, 1e-15), np.ones(n)) and not qn2.update(B, np.ones(n), np.full(n, 1e-15))
    assert qn2.resets == 1 and qn2.skipped == 2


def _hs15_system(qn):
    """The oracle's sparse condensed system at the point of `test_kkt_system` (tests/test_oracle_golden.py), with the diagonal
    Hessian pattern holding sigma, factorized; wrapped."""
    n = hs15.N
    diag = np.arange(n)
    kkt = SparseCondensedKKTSystem(n, hs15.M, hs15.JAC_I, hs15.JAC_J, diag, diag, hs15.IND_INEQ, hs15.IND_LB, hs15.IND_UB,
                                   lambda A: LapackCPUSolver(A, BUNCHKAUFMAN))
    kkt.initialize()
    kkt.get_jacobian()[:] = hs15.jac_coord(np.zeros(2))
    kkt.get_hessian()[:] = qn.sigma
    kkt.compress_jacobian()
    kkt.compress_hessian()
    kkt.l_lower[:] = 1e-3
    kkt.u_lower[:] = 1e-3
    set_aug_diagonal(kkt)
    w = LowRankHessianKKT(kkt, qn)
    w.build_kkt()
    kkt.linear_solver.factorize()
    return kkt, w


def _count_inner_solves(kkt):
    calls = [0]
    inner = kkt.solve_kkt

    def counted(v):
        calls[0] += 1
        return inner(v)
    kkt.solve_kkt = counted
    return calls


def test_wrapper_identity_on_the_oracle_at_the_hs15_point():
    """reference `test_kkt_system` (lib/MadNLPTests/src/MadNLPTests.jl:53-110): mul!(solve_kkt!(1)) ~ 1 by `solcmp` (1e-4), here
    with a non-empty memory."""
    qn, B, S, Y = run_updates(hs15.N, 6, 2, 11)
    kkt, w = _hs15_system(qn)
    x = UnreducedKKTVector.from_kkt(kkt)
    x.values[:] = 1.0
    assert w.solve_kkt(x) is x
    y = x.copy()
    y.values[:] = 0.0
    w.mul(y, x)
    res = np.abs(y.values - 1.0).max()
    print(f"|K K^-1 1 - 1| = {res:.3e}, T =\n{w.T}")
    assert solcmp(y.values, np.ones(len(y.values)))
    assert res < 1e-10
    # the low-rank term is really there: the inner system alone gives another answer
    z = x.copy()
    z.values[:] = 1.0
    kkt.solve_kkt(z)
    assert np.abs(z.values - x.values).max() > 1e-3
    # mul_hess_blk: (B + pr_diag) t on the primal block
    t = np.arange(1.0, len(kkt.pr_diag) + 1)
    out = w.mul_hess_blk(np.zeros_like(t), t)
    Bd = np.asarray(compact_dense(qn.sigma, qn.U, qn.V), dtype=float)
    want = t * kkt.pr_diag
    want[:hs15.N] += Bd @ t[:hs15.N]
    np.testing.assert_allclose(out, want, rtol=1e-12)
    assert kkt.linear_solver.inertia() == w.linear_solver.inertia()


def test_no_rebuild_without_cause_and_bit_identity_after_a_reset():
    qn, B, S, Y = run_updates(hs15.N, 6, 2, 11)
    kkt, w = _hs15_system(qn)
    calls = _count_inner_solves(kkt)
    q = 2 * qn.current_mem
    x = UnreducedKKTVector.from_kkt(kkt)
    for _ in range(3):
        x.values[:] = 1.0
        w.solve_kkt(x)
    assert (calls[0], w.builds) == (3 + q, 1)                  # one build of HH for three solves
    w.build_kkt()
    kkt.linear_solver.factorize()
    x.values[:] = 1.0
    w.solve_kkt(x)
    assert (calls[0], w.builds) == (4 + 2 * q, 2)              # build_kkt: one more
    S2, Y2 = random_pairs(hs15.N, 1, 99)
    assert qn.update(B, S2[:, 0], Y2[:, 0])
    q2 = 2 * qn.current_mem
    x.values[:] = 1.0
    w.solve_kkt(x)
    assert (calls[0], w.builds) == (5 + 2 * q + q2, 3)         # a performed update: one more
    assert not qn.update(B, S2[:, 0], -Y2[:, 0])               # one skip: the cache stays
    x.values[:] = 1.0
    w.solve_kkt(x)
    assert (calls[0], w.builds) == (6 + 2 * q + q2, 3)
    assert not qn.update(B, S2[:, 0], -Y2[:, 0]) and qn.current_mem == 0 and qn.resets == 1
    a, b = UnreducedKKTVector.from_kkt(kkt), UnreducedKKTVector.from_kkt(kkt)
    a.values[:] = b.values[:] = np.linspace(1.0, 2.0, len(a.values))
    w.solve_kkt(a)
    kkt.solve_kkt(b)
    assert a.values.tobytes() == b.values.tobytes()            # p = 0: the inner solve, bit for bit
    assert w.builds == 3


# ------------------------------------------------------------------------------------------ 3. end to end on the oracle
def oracle_factory(nlp):
    def make(info):
        return SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, info.get("hess_I", nlp.hess_I),
                                        info.get("hess_J", nlp.hess_J), info["ind_ineq"], info["ind_lb"], info["ind_ub"],
                                        lambda A: LapackCPUSolver(A, BUNCHKAUFMAN))
    return make


def run(nlp, approx="compact_lbfgs", **kw):
    opt = IPMOptions(tol=1e-6, hessian_approximation=approx, **kw)
    opt.relax_equality, opt.dual_initialization = True, "zero"      # the sparse-condensed preset (options.jl:146-147,160,226)
    s = MadNLPSolver(nlp, oracle_factory(nlp), opt, sparse=True)
    s.solve()
    return s


def check_run(s, tag):
    print(f"{tag}: {s.status} k={s.cnt.k} updates={s.qn.updates} skipped={s.qn.skipped} resets={s.qn.resets} "
          f"obj={s.obj_val:.10g}")
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.cnt.lag_hess_cnt == 0
    assert isinstance(s.kkt, LowRankHessianKKT)
    assert max(s.inf_pr, s.inf_du, s.inf_compl_v) <= s.opt.tol


def test_hs15_end_to_end():
    s = run(HS15Model())
    check_run(s, "HS15")
    near = lambda p: np.abs(s.x[:2] - np.array(p)).max() < 2e-3  # noqa: E731  (both documented optima, docs/src/quickstart.md)
    assert near([0.5, 2.0]) or near([-0.7921, -1.2624]), s.x[:2]
    assert s.qn.updates + s.qn.skipped == s.cnt.k - 1


def test_lootsma_end_to_end():
    nlp = LootsmaModel()
    s = run(nlp)
    check_run(s, "lootsma")
    tol = np.sqrt(s.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731  (solcmp)
    assert cmp(s.x[:3], nlp.LOOTSMA_X), s.x[:3]
    assert cmp(s.y, nlp.LOOTSMA_Y), s.y
    assert s.qn.updates + s.qn.skipped == s.cnt.k - 1


def test_acopf_case30_end_to_end():
    nlp = ACOPFModel("case30")
    s = run(nlp)
    check_run(s, "ACOPF case30")
    ex = run(nlp, "exact")
    print(f"exact: k={ex.cnt.k} obj={ex.obj_val:.10g}; |obj - obj_exact| / |obj_exact| = "
          f"{abs(s.obj_val - ex.obj_val) / abs(ex.obj_val):.3e}")
    assert abs(s.obj_val - ex.obj_val) <= 1e-5 * abs(ex.obj_val)      # two runs to tol 1e-6 of the same problem
    assert s.qn.updates + s.qn.skipped == s.cnt.k - 1


def test_regular_line_search_gives_three_second_chances():
    """reference line_search.jl:79-96: a line search that backtracks below 10 eps / |d| restarts the regular phase from the
    current iterate with y = 0, z = 1 and an empty filter, three times; the fourth time ends the run.  Scripted with a filter
    that accepts nothing and no restoration threshold (the device QP run of tests/test_hip_compact_lbfgs.py reaches it by
    itself)."""
    nlp = HS15Model()
    opt = IPMOptions(tol=1e-6, hessian_approximation="compact_lbfgs", relax_equality=True, dual_initialization="zero")
    s = MadNLPSolver(nlp, oracle_factory(nlp), opt, sparse=True)
    seen = []
    real = s.filter_line_search

    def watched():
        st = real()
        seen.append((st, s.cnt.k, s.y.copy(), s.zl_r.copy(), s.zu_r.copy(), list(s.filter)))
        return st
    s._filter_ok = lambda theta, varphi: False
    s._alpha_min = lambda theta, varphi_d: 0.0
    s.filter_line_search = watched
    assert s.solve() == "SEARCH_DIRECTION_BECOMES_TOO_SMALL"
    assert [st for st, *_ in seen] == ["REGULAR"] * 3 + ["SEARCH_DIRECTION_BECOMES_TOO_SMALL"]
    assert s.cnt.restoration_fail_count == 4 and s.cnt.k == 3
    for i, (st, k, y, zl, zu, flt) in enumerate(seen[:3]):
        assert k == i + 1 and not y.any() and np.all(zl == 1.0) and np.all(zu == 1.0)
        assert flt == [(s.theta_max, -np.inf)]
    # no step was ever taken (one gradient evaluated): every restart ran init! again, no pair was formed
    assert s.cnt.obj_grad_cnt == 1 and s.qn.updates == 0 and s.qn.skipped == 0 and s.cnt.lag_hess_cnt == 0


# ------------------------------------------------------------------------------------------ 4. options
def test_option_validation():
    nlp = HS15Model()
    assert "compact_lbfgs" in mj.HESSIAN_APPROXIMATIONS and mj.HESSIAN_COMPACT_LBFGS == "compact_lbfgs"
    o = IPMOptions()
    assert (o.qn_max_history, o.qn_init_strategy, o.qn_init_value, o.qn_sigma_min, o.qn_sigma_max) == (6, 1, 1.0, 1e-8, 1e8)
    with pytest.raises(ValueError, match="sparse=True"):
        MadNLPSolver(nlp, oracle_factory(nlp), IPMOptions(hessian_approximation="compact_lbfgs"), sparse=False)
    for approx in ("bfgs", "damped_bfgs"):
        with pytest.raises(ValueError, match="needs a dense KKT system"):
            MadNLPSolver(nlp, oracle_factory(nlp), IPMOptions(hessian_approximation=approx), sparse=True)
    opt = IPMOptions(hessian_approximation="compact_lbfgs", qn_max_history=4, qn_init_strategy=SCALAR3, qn_init_value=0.5,
                     qn_sigma_min=1e-3, qn_sigma_max=1e3, relax_equality=True, dual_initialization="zero")
    s = MadNLPSolver(nlp, oracle_factory(nlp), opt, sparse=True)
    q = s.qn.options
    assert (q.max_history, q.init_strategy, q.init_value, q.sigma_min, q.sigma_max) == (4, SCALAR3, 0.5, 1e-3, 1e3)
    assert len(s.kkt.get_hessian()) == nlp.n                    # the diagonal pattern


# ------------------------------------------------------------------------------------------ 5. ABI
def test_null_handles_are_reported_not_crashed():
    lib = mj.lib()
    v = np.zeros(4)
    p = v.ctypes.data
    i, d, h = C.c_int(), C.c_double(), C.c_void_p()
    out8 = (C.c_int64 * 8)()
    for rc in (lib.mnk_lbfgs_create(None, 4, 6, 1, 1.0, 1e-8, 1e8, C.byref(h)), lib.mnk_lbfgs_init(None, p, 0.0, C.byref(d)),
               lib.mnk_lbfgs_update(None, p, p, C.byref(i), C.byref(d)), lib.mnk_lbfgs_status(None, out8),
               lib.mnk_lbfgs_get(None, 0, p, 4), lib.mnk_lbfgs_gram(None, p, 4, 1, p, 4, 1, 4, p),
               lib.mnk_lbfgs_apply(None, p, 1.0, p, 4, p, p, 4, p, 1, 4), lib.mnk_sc_attach_lbfgs(None, None),
               lib.mnk_sc_keep_jacobian(None), lib.mnk_sc_qn_secant(None, *([p] * 8))):
        assert rc < 0 and b"NULL argument" in lib.mnk_last_error_string()
    assert lib.mnk_lbfgs_destroy(None) == 0


def test_max_history_above_32_is_an_error():
    lib = mj.lib()
    h = C.c_void_p()
    assert lib.mnk_lbfgs_create(None, 4, 33, 1, 1.0, 1e-8, 1e8, C.byref(h)) < 0
    assert b"max_history must be 1 to 32" in lib.mnk_last_error_string()
    assert lib.mnk_lbfgs_create(None, 4, 0, 1, 1.0, 1e-8, 1e8, C.byref(h)) < 0
    assert lib.mnk_lbfgs_create(None, 4, 6, 5, 1.0, 1e-8, 1e8, C.byref(h)) < 0
    assert b"init_strategy" in lib.mnk_last_error_string()

"""NLP scaling (`nlp_scaling`, reference src/IPM/solver.jl:37-49, src/Callbacks/nlpmodels.jl:222-264,649-661,693-906) and the
objective sense (`minimize`, src/IPM/callbacks.jl:9,28-30,82) in the host driver, on the CPU oracle back-end: the two tests of
the reference's own suite that pin them (`test_scaling`, `test_max_problem`, lib/MadNLPTests/src/MadNLPTests.jl:334-379), the
factor functions, and the statement that factors of one change no bit."""
import dataclasses
import json
import os

import numpy as np
import pytest

from madnlp_jl_amd import ipm
from madnlp_jl_amd.ipm import IPMOptions, set_con_scale_dense, set_con_scale_sparse, set_obj_scale
from madnlp_jl_amd.problems import ACOPFModel, DenseQPModel, HS15Model, SimplexLPModel
from nlp_scaling_cases import hs15_from, jl_isapprox, rescaled_dense_qp, solcmp
from test_ipm_oracle import run
from test_quasi_newton_cpu import run as run_qn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["dense", "dense_condensed", "sparse_condensed"]


def _tol(kind):
    return 1e-8 if kind != "sparse_condensed" else 1e-6     # RelaxEquality runs at 1e-6, as tests/test_ipm_oracle.py does


# ------------------------------------------------------------------------------------------ C1. the reference's test_scaling
@pytest.mark.parametrize("kind", KINDS)
def test_scaling_lp_returns_the_unscaled_solution(kind):
    big = 1e6
    s = run(kind, SimplexLPModel(big), nlp_scaling=True, tol=_tol(kind))
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.obj_scale == 100.0 / 3e6 and s.con_scale[0] == 100.0 / 1e6
    r = s.solution()
    print(kind, s.cnt.k, r.solution, r.multipliers, r.multipliers_L)
    if kind == "sparse_condensed":
        # the relaxed equality leaves multipliers_L[0] at the size of its relaxation: the suite's solcmp rule at sqrt(tol)
        tol = np.sqrt(s.opt.tol)
        assert solcmp(r.solution, [1.0, 0.0, 0.0], tol), r.solution
        assert solcmp(r.multipliers, [-1.0], tol), r.multipliers
        assert solcmp(r.multipliers_L, [0.0, big, 2 * big], tol), r.multipliers_L
        return
    assert jl_isapprox(r.solution, [1.0, 0.0, 0.0], rtol=1e-7), r.solution
    assert jl_isapprox(r.multipliers, [-1.0], rtol=1e-7), r.multipliers
    assert abs(r.multipliers_L[0]) <= 1e-3, r.multipliers_L
    assert jl_isapprox(r.multipliers_L[1], big, rtol=1e-7) and jl_isapprox(r.multipliers_L[2], 2 * big, rtol=1e-7), r.multipliers_L


# ------------------------------------------------------------------------------------------ C2. the reference's test_max_problem
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_max_problem(kind, scaling):
    s = run(kind, SimplexLPModel(1.0, minimize=False), nlp_scaling=scaling)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.obj_sign == -1.0
    r = s.solution()
    print(kind, scaling, s.cnt.k, r.objective, r.solution, r.multipliers, r.multipliers_L)
    assert jl_isapprox(r.objective, 3.0, rtol=np.sqrt(np.finfo(float).eps)), r.objective     # Julia's default for `≈`
    assert jl_isapprox(r.solution, [0.0, 0.0, 1.0], rtol=1e-7), r.solution
    assert jl_isapprox(r.multipliers[0], -3.0, rtol=1e-7), r.multipliers
    assert jl_isapprox(r.multipliers_L[0], 2.0, rtol=1e-7) and jl_isapprox(r.multipliers_L[1], 1.0, rtol=1e-7), r.multipliers_L
    assert abs(r.multipliers_L[2]) <= 1e-7, r.multipliers_L


# ------------------------------------------------------------------------------------------ C3. the factor functions
def test_factor_functions():
    jac_I = np.array([0, 0, 0, 1, 1, 2])
    jac = np.array([150.0, -150.0, 20.0, 0.5, -0.25, 400.0])        # per row the largest |entry|, starting from 1
    cs = set_con_scale_sparse(4, jac_I, jac, 100.0)
    assert np.array_equal(cs, [100.0 / 150.0, 1.0, 100.0 / 400.0, 1.0])   # row 1: all below 1; row 3: no entry at all
    # a duplicated COO entry (the same (i, j) twice) counts with its own value, not the sum 2 x 60 = 120
    assert np.array_equal(set_con_scale_sparse(1, np.array([0, 0]), np.array([60.0, 60.0]), 100.0), [1.0])
    assert set_obj_scale(np.zeros(3), 100.0) == 1.0
    assert set_obj_scale(np.array([1.0, -2406.0]), 100.0) == 100.0 / 2406.0
    assert set_obj_scale(np.array([3.0, -4.0]), 100.0) == 1.0
    nlp = rescaled_dense_qp()                                         # no duplicates in its COO Jacobian
    x = np.full(nlp.n, 0.01)
    dense = set_con_scale_dense(nlp.jac_dense(x), 100.0)
    assert np.array_equal(dense, set_con_scale_sparse(nlp.m, nlp.jac_I, nlp.jac_coord(x), 100.0))
    assert dense.min() == 100.0 / 1e4 and dense.max() == 1.0
    s = run("sparse_condensed", SimplexLPModel(1e6), nlp_scaling=True, tol=1e-6)
    assert np.array_equal(s.jac_scale, s.con_scale[s.nlp.jac_I])


# ------------------------------------------------------------------------------------------ C4. HS15 from (-2, 1)
@pytest.mark.parametrize("kind", KINDS)
def test_hs15_from_a_steep_start(kind):
    s = run(kind, hs15_from([-2.0, 1.0]), nlp_scaling=True, tol=_tol(kind))
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.obj_scale == 100.0 / 2406.0
    assert np.array_equal(s.con_scale, [1.0, 1.0])
    assert abs(s.history[0].obj - 909.0) <= 1e-9, s.history[0].obj      # the record shows the un-scaled objective
    r = s.solution()
    print(kind, s.cnt.k, r.solution, r.objective)
    assert np.abs(r.solution - [0.5, 2.0]).max() < 2e-3, r.solution
    assert abs(r.objective - 306.5) < 1e-4, r.objective


# ------------------------------------------------------------------------------------------ C5. factors of one change nothing
def _same_run(a, b):
    for u, v in zip((a.x, a.y, a.zl, a.zu), (b.x, b.y, b.zl, b.zu)):
        assert np.array_equal(u, v)
    assert dataclasses.asdict(a.cnt) == dataclasses.asdict(b.cnt)
    assert [dataclasses.astuple(h) for h in a.history] == [dataclasses.astuple(h) for h in b.history]
    assert a.obj_scale == 1.0 and (a.con_scale == 1.0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_unit_factors_change_no_bit_hs15(kind):
    assert HS15Model.x0.tolist() == [0.0, 0.0]
    _same_run(run(kind, HS15Model(), nlp_scaling=True, tol=_tol(kind)), run(kind, HS15Model(), tol=_tol(kind)))


@pytest.mark.parametrize("kind", KINDS)
def test_unit_factors_change_no_bit_dense_qp(kind):
    nlp = DenseQPModel(50, 10, 0)
    _same_run(run(kind, nlp, nlp_scaling=True, tol=_tol(kind)), run(kind, nlp, tol=_tol(kind)))


@pytest.mark.parametrize("case", ["case30", "case118", "case1354pegase"])
def test_acopf_cases_have_unit_factors(case):
    """What lets the recorded AC-OPF trajectories stand for runs with `nlp_scaling` on as well."""
    nlp = ACOPFModel(case)
    x0, lvar, uvar = nlp.x0.copy(), nlp.lvar.copy(), nlp.uvar.copy()
    o = IPMOptions()
    ipm._set_initial_bounds(lvar, uvar, o.bound_relax_factor)
    ipm._initialize_variables(x0, lvar, uvar, o.bound_push, o.bound_fac)
    assert (set_con_scale_sparse(nlp.m, nlp.jac_I, nlp.jac_coord(x0), o.nlp_scaling_max_gradient) == 1.0).all()
    assert set_obj_scale(nlp.grad(x0), o.nlp_scaling_max_gradient) == 1.0


# ------------------------------------------------------------------------------------------ C6. quasi-Newton under scaling
def test_bfgs_reaches_the_exact_hessian_answer_under_scaling():
    """The comparison and tolerances of test_quasi_newton_cpu.test_dense_qp_against_the_exact_hessian_run (objective 1e-6,
    solution and multipliers 10 x what profiles/qn_host_vs_exact.json records for this size), on `solution()`."""
    n, m, n_eq = 20, 15, 2
    rec = {tuple(r["size"]): r for r in json.load(open(os.path.join(ROOT, "profiles", "qn_host_vs_exact.json")))["sizes"]}[(n, m, n_eq)]
    nlp = rescaled_dense_qp(n, m, n_eq)
    ex = run_qn("dense", nlp, "exact", nlp_scaling=True)
    assert ex.status == "SOLVE_SUCCEEDED"
    assert ex.obj_scale < 1.0 and ex.con_scale.min() == 100.0 / 1e4 and ex.con_scale.max() == 1.0
    e = ex.solution()
    for kind in ("dense", "dense_condensed"):
        s = run_qn(kind, nlp, "bfgs", nlp_scaling=True)
        r = s.solution()
        dx, dy = np.abs(r.solution - e.solution).max(), np.abs(r.multipliers - e.multipliers).max()
        print(f"{kind}: k {s.cnt.k} (exact {ex.cnt.k}) dobj {abs(r.objective - e.objective):.2e} dx {dx:.3e} dy {dy:.3e}")
        assert s.status == "SOLVE_SUCCEEDED", (kind, s.status)
        assert s.cnt.lag_hess_cnt == 0
        assert abs(r.objective - e.objective) < 1e-6
        assert dx <= 10 * rec["max_dx"], (kind, dx)
        assert dy <= 10 * rec["max_dy"], (kind, dy)

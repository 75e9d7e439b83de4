"""Quasi-Newton Hessians of the dense KKT systems, host mirror (`madnlp_jl_amd.quasi_newton`, `ipm.MadNLPSolver` with
`hessian_approximation = "bfgs" / "damped_bfgs"`) on the CPU oracle's KKT systems: the update rule against a direct
longdouble formula, the reference's hard-coded answers without second derivatives, and the reference's own acceptance
shape (test/madnlp_quasi_newton.jl:8-35) against the exact-Hessian run."""
import json
import os

import numpy as np
import pytest

import madnlp_jl_amd as mj
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.problems import DenseQPModel, HS15Model, LootsmaModel
from madnlp_jl_amd.quasi_newton import BFGS, DampedBFGS, create_quasi_newton, rho0, symv_lower
from oracle.dense import DenseCondensedKKTSystem, DenseKKTSystem
from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver
from qn_cases import EPS, LD, exact_case, formula, random_case, tril_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("dense", "dense_condensed")
APPROX = ("bfgs", "damped_bfgs")


def _adopted(kind, n):
    qn = create_quasi_newton(kind, n)
    qn.adopt()
    return qn


# ------------------------------------------------------------------------------------------ 1. update / init
@pytest.mark.parametrize("n", [7, 64, 130, 501])
@pytest.mark.parametrize("mode", ["bfgs", "damped", "damped_lt1", "damped_neg"])
def test_update_against_the_longdouble_formula(n, mode):
    B, s, y, kind = random_case(n, 100 + n, mode)
    ref = formula(B, s, y, kind)
    theta = float(ref["theta"])
    assert (theta < 1.0) == (mode in ("damped_lt1", "damped_neg"))
    B0 = B.copy()
    qn = _adopted(kind, n)
    assert qn.update(B, s, y) is True
    err = tril_err(B, ref["B1"])
    bound = 8 * n * EPS * ref["scale"]
    print(f"n={n} {mode}: err {err:.3e} bound {bound:.3e} theta {theta:.4f}")
    assert err <= bound
    iu = np.triu_indices(n, 1)
    assert np.isnan(B[iu]).all() and np.isnan(B0[iu]).all()      # the strict upper triangle: neither read nor written
    np.testing.assert_allclose(qn.last, [float(ref[k]) for k in ("sy", "sBs", "theta", "rs")], rtol=64 * n * EPS)
    assert (qn.updates, qn.skipped) == (1, 0)


@pytest.mark.parametrize("n", [7, 130])
def test_bfgs_skips_and_damped_does_not(n):
    B, s, y, _ = random_case(n, 7 + n, "skip")
    assert s @ y < 1e-8
    B0 = B.copy()
    qn = _adopted("bfgs", n)
    assert qn.update(B, s, y) is False
    assert B.tobytes() == B0.tobytes()                            # bit-identical, NaNs of the upper triangle included
    assert (qn.updates, qn.skipped) == (0, 1)
    assert not create_quasi_newton("bfgs", n).update(B, s, y) and B.tobytes() == B0.tobytes()   # ... not instantiated either
    qd = _adopted("damped_bfgs", n)
    assert qd.update(B, s, y) is True
    ref = formula(B0, s, y, "damped_bfgs")
    assert float(ref["theta"]) < 1.0
    assert tril_err(B, ref["B1"]) <= 8 * n * EPS * ref["scale"]


@pytest.mark.parametrize("kind", APPROX)
def test_first_update_resets_the_diagonal_only(kind):
    n = 40
    B, s, y, _ = random_case(n, 5, "bfgs")
    ref = formula(B, s, y, kind, first=True)
    with_reset = B.copy()
    with_reset[np.diag_indices(n)] = (s @ y) / (s @ s)
    qn = create_quasi_newton(kind, n)
    assert not qn.is_instantiated
    assert qn.update(B, s, y) and qn.is_instantiated
    assert tril_err(B, ref["B1"]) <= 8 * n * EPS * ref["scale"]
    # the same result as an ordinary update of the matrix whose DIAGONAL ALONE was replaced
    B2 = with_reset.copy()
    _adopted(kind, n).update(B2, s, y)
    assert np.array_equal(np.tril(B), np.tril(B2))
    # and the second update resets nothing
    B3, ref2 = B.copy(), formula(B, s, y, kind)
    qn.update(B3, s, y)
    assert tril_err(B3, ref2["B1"]) <= 8 * n * EPS * ref2["scale"]


def test_init_rho0_branches():
    eps = np.finfo(np.float64).eps
    g = np.array([3.0, 4.0])
    assert rho0(g * 1e-6, 5.0) == 1.0                      # g'g = 2.5e-11 < sqrt(eps)
    assert rho0(g, 0.0) == 1.0 / 25.0                      # f0 == 0
    assert rho0(g, -50.0) == 2.0                           # |f0| / g'g
    assert rho0(g, 1e-300) == 1e-300 / 25.0                # isapprox(f0, 0) with atol = 0 holds for f0 == 0 only
    assert rho0(np.array([np.sqrt(np.sqrt(eps)) * 1.01, 0.0]), 0.0) != 1.0
    for cls in (BFGS, DampedBFGS):
        B = np.full((3, 3), 7.0, order="F")
        cls(3).init(B, np.array([1.0, 2.0, 2.0]), 18.0)
        assert np.array_equal(B, 4.0 * np.eye(3))


# ------------------------------------------------------------------------------------------ 2. secant equation
@pytest.mark.parametrize("n", [7, 130, 501])
def test_secant_equation_after_a_bfgs_update(n):
    B, s, y, kind = random_case(n, 300 + n, "bfgs")
    scale = formula(B, s, y, kind)["scale"]
    assert _adopted("bfgs", n).update(B, s, y)
    res = np.abs(symv_lower(B, s) - y).max()
    assert res <= 64 * n * EPS * scale * np.abs(s).max() * n


# ------------------------------------------------------------------------------------------ exact-answer inputs (GPU item 7)
@pytest.mark.parametrize("n", [5, 64, 65, 257, 1000])
@pytest.mark.parametrize("kind", APPROX)
@pytest.mark.parametrize("first", [False, True])
def test_exact_cases_are_exact_on_the_host(n, kind, first):
    """The inputs of the device's exact-answer test: host mirror == longdouble formula, bit for bit."""
    B, s, y = exact_case(n, 11 * n + first, kind, first)
    ref = formula(B, s, y, kind, first)
    assert float(ref["theta"]) == 1.0 and float(ref["sy"]) == float(ref["sBs"])
    assert np.log2(float(ref["sy"])) % 1 == 0
    qn = create_quasi_newton(kind, n) if first else _adopted(kind, n)
    assert qn.update(B, s, y)
    assert np.array_equal(np.tril(B).astype(LD), np.tril(ref["B1"]))
    assert np.isnan(B[np.triu_indices(n, 1)]).all()


# ------------------------------------------------------------------------------------------ 3. known answers
def oracle_factory(kind):
    fac = lambda A: LapackCPUSolver(A, BUNCHKAUFMAN)  # noqa: E731

    def make(info):
        if kind == "dense_condensed":
            return DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                           info["ind_ub"], fac)
        return DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], fac)
    return make


def run(kind, nlp, approx, **kw):
    s = MadNLPSolver(nlp, oracle_factory(kind), IPMOptions(hessian_approximation=approx, **kw), sparse=False)
    s.solve()
    return s


@pytest.mark.parametrize("approx", APPROX)
@pytest.mark.parametrize("kind", KINDS)
def test_lootsma_without_second_derivatives(kind, approx):
    """The answers the reference's suite pins (lib/MadNLPTests/src/MadNLPTests.jl:153-194), same `solcmp` rule and
    tolerance sqrt(tol) as tests/test_ipm_oracle.py."""
    nlp = LootsmaModel()
    s = run(kind, nlp, approx, tol=1e-8)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    tol = np.sqrt(s.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731  (solcmp)
    assert cmp(s.x[:3], nlp.LOOTSMA_X), s.x[:3]
    assert cmp(s.y, nlp.LOOTSMA_Y), s.y
    assert s.cnt.lag_hess_cnt == 0
    assert s.qn.updates + s.qn.skipped == s.cnt.k - 1      # init! at k = 0, one update per later iteration (no restoration here)


@pytest.mark.parametrize("approx", APPROX)
@pytest.mark.parametrize("kind", KINDS)
def test_hs15_without_second_derivatives(kind, approx):
    s = run(kind, HS15Model(), approx, tol=1e-8)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    near = lambda p: np.abs(s.x[:2] - np.array(p)).max() < 2e-3  # noqa: E731
    assert near([0.5, 2.0]) or near([-0.7921, -1.2624]), s.x[:2]     # the two documented optima (docs/src/quickstart.md:32,202)
    assert max(s.inf_pr, s.inf_du, s.inf_compl_v) <= s.opt.tol
    assert s.cnt.lag_hess_cnt == 0


def test_exact_run_counts_its_hessians():
    s = run("dense", HS15Model(), "exact", tol=1e-8)
    assert s.cnt.lag_hess_cnt == s.cnt.k and s.qn is None


# ------------------------------------------------------------------------------------------ 4. the reference's acceptance shape
MEASURED = os.path.join(ROOT, "profiles", "qn_host_vs_exact.json")     # written by tools/qn_host_vs_exact.py


@pytest.mark.parametrize("n,m,n_eq", [(10, 5, 0), (50, 10, 0), (20, 15, 2)])
def test_dense_qp_against_the_exact_hessian_run(n, m, n_eq):
    """test/madnlp_quasi_newton.jl:8-35 on this project's DenseQPModel.  Objective: the reference's 1e-6.  Solution and
    multipliers: 10 x what profiles/qn_host_vs_exact.json records for this size (this project's QP generator is not the
    reference's; both runs converge to tol = 1e-8, one decade is left for platform BLAS differences)."""
    rec = {tuple(r["size"]): r for r in json.load(open(MEASURED))["sizes"]}[(n, m, n_eq)]
    nlp = DenseQPModel(n, m, n_eq)
    ex = run("dense", nlp, "exact")
    assert ex.status == "SOLVE_SUCCEEDED"
    for kind in KINDS:
        for approx in APPROX:
            s = run(kind, nlp, approx)
            dx, dy = np.abs(s.x[:n] - ex.x[:n]).max(), np.abs(s.y - ex.y).max()
            print(f"({n},{m},{n_eq}) {kind} {approx}: k {s.cnt.k} (exact {ex.cnt.k}) dobj {abs(s.obj_val - ex.obj_val):.2e} "
                  f"dx {dx:.3e} dy {dy:.3e}")
            assert s.status == "SOLVE_SUCCEEDED", (kind, approx, s.status)
            assert s.cnt.lag_hess_cnt == 0
            assert abs(s.obj_val - ex.obj_val) < 1e-6
            assert dx <= 10 * rec["max_dx"], (kind, approx, dx)
            assert dy <= 10 * rec["max_dy"], (kind, approx, dy)


@pytest.mark.parametrize("kind", KINDS)
def test_damped_bfgs_on_the_200_60_8_qp(kind):
    """Plain BFGS ends SOLVED_TO_ACCEPTABLE_LEVEL here (about half of its updates are skipped) and is left out on purpose;
    the damped update must succeed."""
    s = run(kind, DenseQPModel(200, 60, 8), "damped_bfgs")
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.cnt.lag_hess_cnt == 0 and s.qn.skipped == 0


# ------------------------------------------------------------------------------------------ 5. options
def test_option_validation():
    nlp = HS15Model()
    with pytest.raises(ValueError, match="hessian_approximation"):
        MadNLPSolver(nlp, oracle_factory("dense"), IPMOptions(hessian_approximation="sr1"), sparse=False)
    for approx in APPROX:
        with pytest.raises(ValueError, match="dense"):
            MadNLPSolver(nlp, oracle_factory("dense"), IPMOptions(hessian_approximation=approx), sparse=True)
    assert IPMOptions().hessian_approximation == "exact"
    assert (mj.HESSIAN_EXACT, mj.HESSIAN_BFGS, mj.HESSIAN_DAMPED_BFGS) == ("exact", "bfgs", "damped_bfgs")
    assert (mj.MNK_QN_BFGS, mj.MNK_QN_DAMPED_BFGS) == (1, 2)


# ------------------------------------------------------------------------------------------ 6. ABI
def test_null_handle_is_reported_not_crashed():
    """(the call in front of mnk_dc_qn_init needs a handle, hence a device: tests/test_hip_quasi_newton.py)"""
    lib = mj.lib()
    v = np.zeros(4)
    for rc in (lib.mnk_dc_qn_update(None, v.ctypes.data, v.ctypes.data), lib.mnk_dc_qn_init(None, 1, None, 0.0),
               lib.mnk_dc_qn_status(None, None, None, None), lib.mnk_dc_get_hess(None, v.ctypes.data, 2, 0),
               lib.mnk_dc_qn_secant(None, *([v.ctypes.data] * 8))):
        assert rc < 0 and b"NULL argument" in lib.mnk_last_error_string()

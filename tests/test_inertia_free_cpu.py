"""Inertia-free and inertia-ignoring correction of the IPM mirror (reference src/IPM/solver.jl:672-788, IPM.jl:203-207) on the CPU
oracle: a linear solver that reveals no inertia (the oracle's LapackCPUSolver(LU): `is_inertia()` is False, `inertia()` raises)
selects `inertia_free` under the default `inertia_correction_method = "auto"` and solves the problems the inertia-based runs
solve; the Julia glue maps QR and reports no inertia for it."""
import os
import re

import numpy as np
import pytest

from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver, curv_test
from madnlp_jl_amd.problems import DenseQPModel, HS15Model, LootsmaModel
from oracle.dense import DenseCondensedKKTSystem, DenseKKTSystem
from oracle.lapack_cpu import BUNCHKAUFMAN, LU, LapackCPUSolver
from oracle.sparse_condensed import SparseCondensedKKTSystem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["dense", "dense_condensed", "sparse_condensed"]


def factory(kind, nlp, alg):
    fac = lambda A: LapackCPUSolver(A, alg)  # noqa: E731

    def make(info):
        if kind == "sparse_condensed":
            return SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J,
                                            info["ind_ineq"], info["ind_lb"], info["ind_ub"], fac)
        if kind == "dense_condensed":
            return DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                           info["ind_ub"], fac)
        return DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], fac)
    return make


def make_solver(kind, nlp, alg=LU, **kw):
    sparse = kind == "sparse_condensed"
    opt = IPMOptions(tol=1e-8 if not sparse else 1e-6)
    for k, v in kw.items():
        setattr(opt, k, v)
    if sparse:  # preset of SparseCondensedKKTSystem (reference src/IPM/options.jl:146-147,160,226)
        opt.relax_equality, opt.dual_initialization = True, "zero"
    return MadNLPSolver(nlp, factory(kind, nlp, alg), opt, sparse=sparse)


def run(kind, nlp, alg=LU, **kw):
    s = make_solver(kind, nlp, alg, **kw)
    s.solve()
    return s


def assert_hs15_optimum(s):
    assert s.status == "SOLVE_SUCCEEDED", s.status
    near = lambda p: np.abs(s.x[:2] - np.array(p)).max() < 2e-3  # noqa: E731
    assert near([0.5, 2.0]) or near([-0.7921, -1.2624]), s.x[:2]
    if near([0.5, 2.0]):
        assert abs(s.obj_val - 306.5) < 1e-4
    else:
        assert abs(s.obj_val - 360.3797) < 1e-3
    assert max(s.inf_pr, s.inf_du, s.inf_compl_v) <= s.opt.tol


def test_auto_resolves_by_the_solver():
    """IPM.jl:203-207: InertiaBased when the solver reveals the inertia, InertiaFree otherwise; explicit choices stand."""
    nlp = HS15Model()
    assert make_solver("dense", nlp, LU).inertia_correction_method == "inertia_free"
    assert make_solver("dense", nlp, BUNCHKAUFMAN).inertia_correction_method == "inertia_based"
    assert make_solver("dense", nlp, BUNCHKAUFMAN, inertia_correction_method="ignore").inertia_correction_method == "ignore"
    assert IPMOptions().inertia_correction_method == "auto" and IPMOptions().inertia_free_tol == 0.0
    with pytest.raises(ValueError):
        make_solver("dense", nlp, LU, inertia_correction_method="inertia_revealing")


@pytest.mark.parametrize("kind", KINDS)
def test_hs15_inertia_free_on_a_solver_without_inertia(kind):
    s = run(kind, HS15Model())
    assert s.inertia_correction_method == "inertia_free"
    assert_hs15_optimum(s)


@pytest.mark.parametrize("kind", KINDS)
def test_lootsma_inertia_free_reproduces_the_reference_answers(kind):
    """reference lib/MadNLPTests/src/MadNLPTests.jl:153-194 at atol = rtol = sqrt(tol)."""
    nlp = LootsmaModel()
    s = run(kind, nlp)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    tol = np.sqrt(s.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731
    assert cmp(s.x[:3], nlp.LOOTSMA_X), s.x[:3]
    assert cmp(s.y, nlp.LOOTSMA_Y), s.y


@pytest.mark.parametrize("kind", KINDS)
def test_explicit_inertia_free_matches_inertia_based(kind):
    """With BUNCHKAUFMAN (inertia available) the inertia-free correction, asked for explicitly, reaches the optimum of the
    inertia-based run."""
    a = run(kind, HS15Model(), BUNCHKAUFMAN)
    b = run(kind, HS15Model(), BUNCHKAUFMAN, inertia_correction_method="inertia_free")
    assert a.inertia_correction_method == "inertia_based" and b.inertia_correction_method == "inertia_free"
    assert_hs15_optimum(a)
    assert_hs15_optimum(b)
    np.testing.assert_allclose(b.x[:2], a.x[:2], atol=1e-6)
    assert abs(b.obj_val - a.obj_val) < 1e-6 * max(1.0, abs(a.obj_val))


@pytest.mark.parametrize("n,m,n_eq", [(10, 5, 0), (50, 10, 0), (20, 15, 2)])
def test_dense_formulations_agree_inertia_free(n, m, n_eq):
    """reference test/madnlp_dense.jl:105-119 with inertia = InertiaFree: same iteration count, same solution."""
    nlp = DenseQPModel(n, m, n_eq)
    a = run("dense", nlp, LU)
    b = run("dense_condensed", nlp, LU)
    assert a.inertia_correction_method == b.inertia_correction_method == "inertia_free"
    assert a.status == b.status == "SOLVE_SUCCEEDED"
    assert a.cnt.k == b.cnt.k
    np.testing.assert_allclose(a.x[:n], b.x[:n], atol=1e-6)
    np.testing.assert_allclose(a.y, b.y, atol=1e-6)


@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_ignore_runs_hs15(kind):
    s = run(kind, HS15Model(), LU, inertia_correction_method="ignore")
    assert s.inertia_correction_method == "ignore"
    assert_hs15_optimum(s)


class _Diag2:
    """A KKT stand-in whose Hessian block is diag(h) (mul_hess_blk, reference src/IPM/factorization.jl:326-338)."""

    def __init__(self, h):
        self.h = np.asarray(h, float)

    def mul_hess_blk(self, wx, t):
        wx[:] = self.h * t
        return wx


def test_curv_test_verdicts_on_both_sides_of_the_threshold():
    """solver.jl:785-788: t'Wt + max(t'Wn - g'n, 0) - tol t't >= 0."""
    wx = np.zeros(2)
    t = np.array([1.0, 1.0])
    n = np.zeros(2)
    g = np.zeros(2)
    assert curv_test(t, n, g, _Diag2([1.0, -0.5]), wx, 0.0)          # t'Wt = 0.5
    assert not curv_test(t, n, g, _Diag2([1.0, -1.5]), wx, 0.0)      # t'Wt = -0.5
    assert curv_test(t, n, g, _Diag2([1.0, -1.0]), wx, 0.0)          # = 0: accepted (>=)
    assert not curv_test(t, n, g, _Diag2([1.0, -0.5]), wx, 0.3)      # 0.5 - 0.3 * 2 < 0
    assert curv_test(t, n, g, _Diag2([1.0, -0.5]), wx, 0.2)          # 0.5 - 0.4 >= 0
    # the normal component: max(t'Wn - g'n, 0) lifts a negative t'Wt, never lowers it
    n2 = np.array([1.0, 0.0])
    assert curv_test(t, n2, np.array([-1.0, 0.0]), _Diag2([1.0, -1.5]), wx, 0.0)    # -0.5 + (1 + 1) >= 0
    assert not curv_test(t, n2, np.array([5.0, 0.0]), _Diag2([1.0, -1.5]), wx, 0.0)  # -0.5 + max(1 - 5, 0) < 0


def test_device_driver_refuses_a_method_other_than_inertia_based():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    nlp = DenseQPModel(10, 5, 0)
    with pytest.raises(NotImplementedError, match="inertia"):
        DeviceMadNLPSolver(nlp, factory("dense_condensed", nlp, LU), IPMOptions(), sparse=False)
    with pytest.raises(NotImplementedError, match="inertia"):
        DeviceMadNLPSolver(nlp, factory("dense_condensed", nlp, BUNCHKAUFMAN),
                           IPMOptions(inertia_correction_method="ignore"), sparse=False)


def test_julia_glue_maps_qr_and_reports_no_inertia_for_it():
    jl = open(os.path.join(ROOT, "julia", "MadNLPHIP.jl")).read()
    algo = dict(re.findall(r"(\w+) => Cint\((\d+)\)", re.search(r"const MNK_ALGO = Dict\((.*?)\)\n", jl).group(1)))
    assert algo["QR"] == "3" and algo["BUNCHKAUFMAN"] == "1" and algo["CHOLESKY"] == "4" and algo["LDL"] == "5"
    hdr = open(os.path.join(ROOT, "include", "madnlp_hip.h")).read()
    assert "MNK_QR = 3" in hdr
    assert re.search(r"^MadNLP\.is_inertia\(M::HipLinearSolver\) = M\.opt\.lapack_algorithm != QR$", jl, flags=re.M)
    body = jl.split("function MadNLP.inertia(M::HipLinearSolver)")[1].split("\nend")[0]
    assert "throw(InertiaException())" in body
    assert re.search(r"import MadNLP:[^\n]*(\n[^\n]*)*?\bQR\b", jl.split("import LinearAlgebra")[0])


def test_python_mirror_knows_qr_without_a_device():
    from madnlp_jl_amd import _lib as L
    from madnlp_jl_amd.linear_solver import _ALGO, QR
    assert _ALGO[QR] == L.MNK_QR == 3

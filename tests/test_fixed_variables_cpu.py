"""`fixed_variable_treatment = "make_parameter"` (reference `MakeParameter`, src/Callbacks/nlpmodels.jl:266-353, 580-591,
665-690, 912-1087; the reference's own "Fixed variables" test set, test/madnlp_test.jl:162-188) in the host driver on the CPU
oracle back-end: the handler's structure against a brute-force dense construction, exact fixed values and `update_z!`
multipliers, the reduced (sparse) and frozen (dense) runs against each other and against `"relax_bound"`, the refused
combinations, and the statement that a model without fixed variables runs bit for bit as before."""
import dataclasses

import numpy as np
import pytest

from madnlp_jl_amd import fixed_vars as FV
from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.problems import DenseQPModel, HS15Model, LootsmaModel, SimplexLPModel, SparseQPModel
from oracle.dense import DenseCondensedKKTSystem, DenseKKTSystem
from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver
from oracle.sparse_condensed import SparseCondensedKKTSystem

KINDS = ["dense", "dense_condensed", "sparse_condensed"]


def factory(kind, nlp):
    """tests/test_ipm_oracle.py::oracle_factory with the structure taken through `fixed_vars.structure`."""
    fac = lambda A: LapackCPUSolver(A, BUNCHKAUFMAN)  # noqa: E731

    def make(info):
        if kind == "sparse_condensed":
            return SparseCondensedKKTSystem(info["n"], info["m"], *FV.structure(nlp, info), info["ind_ineq"], info["ind_lb"],
                                            info["ind_ub"], fac)
        if kind == "dense_condensed":
            return DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                           info["ind_ub"], fac)
        return DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], fac)
    return make


def _tol(kind):
    return 1e-8 if kind != "sparse_condensed" else 1e-6     # RelaxEquality runs at 1e-6, as tests/test_ipm_oracle.py::run


def run(kind, nlp, treatment="make_parameter", **kw):
    sparse = kind == "sparse_condensed"
    opt = IPMOptions(tol=_tol(kind), fixed_variable_treatment=treatment, **kw)
    if sparse:  # preset of SparseCondensedKKTSystem, as tests/test_ipm_oracle.py::run
        opt.relax_equality, opt.dual_initialization = True, "zero"
    s = MadNLPSolver(nlp, factory(kind, nlp), opt, sparse=sparse)
    s.solve()
    return s


def fix(nlp, where, values):
    """`nlp` with lvar = uvar = values at `where` (its own bound arrays are replaced, not written)."""
    nlp.lvar, nlp.uvar = np.array(nlp.lvar, dtype=float), np.array(nlp.uvar, dtype=float)
    nlp.lvar[where] = nlp.uvar[where] = values
    return nlp


def hs15_fixed():
    return fix(HS15Model(), [0], 0.5)


# ------------------------------------------------------------------------------------------------- 1. HS15, x[0] fixed at 0.5
@pytest.fixture(scope="module")
def hs15_runs():
    return {kind: run(kind, hs15_fixed()) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_hs15_fixed_variable_is_exact_and_gets_its_multiplier(hs15_runs, kind):
    s = hs15_runs[kind]
    tol = np.sqrt(s.opt.tol)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.n == (1 if kind == "sparse_condensed" else 2)
    r = s.solution()
    print(kind, s.cnt.k, repr(r.solution), r.objective, r.multipliers, r.multipliers_L, r.multipliers_U)
    assert r.solution.shape == r.multipliers_L.shape == r.multipliers_U.shape == (2,)
    assert r.solution[0] == 0.5                         # (the relaxed bound returns 0.50000001)
    assert abs(r.solution[1] - 2.0) <= tol and abs(r.objective - 306.5) <= tol
    # update_z!: grad f = (-351, 350), y = (-700, 0), J'y = (-1400, -350): g[0] = -1751
    assert r.multipliers_L[0] == 0.0
    assert abs(r.multipliers_U[0] - 1751.0) <= tol * 1751.0


def test_hs15_relaxed_bound_is_not_exact():
    r = run("dense", hs15_fixed(), treatment="relax_bound").solution()
    assert r.solution[0] != 0.5 and abs(r.solution[0] - 0.5) < 1e-7


def test_hs15_dense_and_sparse_runs_agree(hs15_runs):
    """The reference demands equality of its two runs (test/madnlp_test.jl:162-188); here they factor different matrices."""
    a, b, c = (hs15_runs[k].solution() for k in KINDS)
    tol = np.sqrt(1e-6)
    for other in (b, c):
        assert np.abs(a.solution - other.solution).max() <= tol
        assert abs(a.objective - other.objective) <= tol
        assert np.abs(a.multipliers - other.multipliers).max() <= tol * 700.0
        assert np.abs(a.multipliers_U - other.multipliers_U).max() <= tol * 1751.0


# ------------------------------------------------------------------------------------------------- 2. Lootsma with `par`
def test_lootsma_with_its_fixed_parameter():
    """reference lib/MadNLPTests/src/MadNLPTests.jl:155-196 as written there: `par == 6` is a variable; the comparison of
    tests/test_ipm_oracle.py::test_lootsma_reproduces_the_reference_hard_coded_answers."""
    M = T.lootsma_fixed_tape_model()
    s = run("sparse_condensed", M)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.n == 3 and s.fixed_handler.fixed.tolist() == [0]
    r = s.solution()
    tol = np.sqrt(s.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731  (solcmp)
    assert r.solution[0] == 6.0
    assert cmp(r.solution[1:], LootsmaModel.LOOTSMA_X), r.solution
    assert cmp(r.multipliers, LootsmaModel.LOOTSMA_Y), r.multipliers
    assert np.abs(r.multipliers_L[1:]).max() < tol and np.abs(r.multipliers_U[1:]).max() < tol


# ------------------------------------------------------------------------------------------------- 3. dense QP, three frozen
QP_FIXED, QP_VALUES = [0, 17, 49], [0.25, 0.5, 0.75]


def qp_fixed(n_eq):
    return fix(DenseQPModel(50, 10, n_eq, seed=1), QP_FIXED, QP_VALUES)


@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
@pytest.mark.parametrize("n_eq", [0, 2])
def test_dense_qp_frozen_variables(kind, n_eq):
    a, b = run(kind, qp_fixed(n_eq)), run(kind, qp_fixed(n_eq), treatment="relax_bound")
    assert a.status == b.status == "SOLVE_SUCCEEDED"
    assert a.n == 50 and not set(QP_FIXED) & (set(a.ind_lb.tolist()) | set(a.ind_ub.tolist()))
    ra, rb = a.solution(), b.solution()
    tol = np.sqrt(a.opt.tol)
    print(kind, n_eq, a.cnt.k, b.cnt.k, np.abs(ra.solution - rb.solution).max())
    assert ra.solution[QP_FIXED].tolist() == QP_VALUES
    assert rb.solution[QP_FIXED].tolist() != QP_VALUES
    assert np.abs(ra.solution - rb.solution).max() <= tol
    assert abs(ra.objective - rb.objective) <= tol
    # (the multipliers of this QP are not compared between the runs: its active set is degenerate and they move by 1e-3 under
    # the 1e-8 relaxation.)  Stationarity of what is returned, over ALL variables: the free ones by the solver's own
    # criterion inf_du <= tol (its scaling factor s_d is 1 for multipliers of this size), the frozen ones by update_z!
    M = qp_fixed(n_eq)
    res = M.grad(ra.solution) + M.A.T @ ra.multipliers - ra.multipliers_L + ra.multipliers_U
    assert np.abs(res).max() <= 2 * a.opt.tol and np.abs(res[QP_FIXED]).max() <= 1e-15
    assert (np.minimum(ra.multipliers_L[QP_FIXED], ra.multipliers_U[QP_FIXED]) == 0).all()


# ------------------------------------------------------------------------------------------------- 4. AC-OPF case30 as tapes
def acopf_fixed_set(n, also=()):
    return np.array(sorted(set(range(5, n, 29)) | {n - 1} | set(also)))


def acopf_fixed(case, x_opt, also=()):
    M = T.acopf_tape_model(case)
    where = acopf_fixed_set(M.n, also)
    return fix(M, where, x_opt[where]), where


def sparse_options(**kw):
    o = IPMOptions(tol=1e-6, **kw)
    o.relax_equality, o.dual_initialization = True, "zero"
    return o


@pytest.fixture(scope="module")
def case30_optimum():
    M = T.acopf_tape_model("case30")
    s = MadNLPSolver(M, factory("sparse_condensed", M), sparse_options(), sparse=True)
    assert s.solve() == "SOLVE_SUCCEEDED"
    r = s.solution()
    return r.solution, r.objective


def test_case30_fixed_set_exercises_every_kind_of_dropped_entry(case30_optimum):
    M, where = acopf_fixed("case30", case30_optimum[0])
    h = FV.FixedVariableHandler.create(M, True)
    assert h.fixed.tolist() == where.tolist()
    assert len(np.unique(h.jac_I)) == len(np.unique(M.jac_I)) == M.m == 348        # no Jacobian row loses all its entries
    isfixed = np.zeros(M.n, dtype=bool)
    isfixed[where] = True
    fi, fj = isfixed[M.hess_I], isfixed[M.hess_J]
    assert ((fi ^ fj).sum(), (fi & fj).sum()) == (84, 31)
    assert (len(M.jac_I), len(M.hess_I)) == (1303, 1706)
    assert (len(h.ind_jac_free), len(h.ind_hess_free)) == (1250, 1706 - 84 - 31)   # several workgroups of 256, none full


@pytest.mark.parametrize("also", [(), (0,)], ids=["every29th", "va_ref_row_emptied"])
def test_case30_with_fixed_variables(case30_optimum, also):
    """`also = (0,)` fixes the reference angle too: the `va_ref = 0` row keeps no Jacobian entry (its constraint value is the
    constant 0 = its right-hand side)."""
    x_opt, f_opt = case30_optimum
    M, where = acopf_fixed("case30", x_opt, also)
    s = MadNLPSolver(M, factory("sparse_condensed", M), sparse_options(fixed_variable_treatment="make_parameter"), sparse=True)
    s.solve()
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.n == M.n - len(where)
    if also:
        assert 0 not in s.fixed_handler.jac_I            # row 0 is the va_ref row (tape_model.acopf_tape_model)
    r = s.solution()
    print(also, "iterations", s.cnt.k, "objective", r.objective, "relative difference", abs(r.objective - f_opt) / abs(f_opt))
    assert np.array_equal(r.solution[where], x_opt[where])
    assert abs(r.objective - f_opt) <= 1e-6 * abs(f_opt)
    assert r.multipliers_L.shape == r.multipliers_U.shape == (M.n,)
    assert (r.multipliers_L >= 0).all() and (r.multipliers_U >= 0).all()
    assert (np.minimum(r.multipliers_L[where], r.multipliers_U[where]) == 0).all()     # max(0, g), max(0, -g)


# ------------------------------------------------------------------------------------------------- 5. structure of the handler
class _Structure:
    """A model that is nothing but bounds and a COO structure with duplicate entries and an upper-triangular Hessian entry."""
    def __init__(self, n, m, fixed, seed):
        rng = np.random.default_rng(seed)
        self.n, self.m = n, m
        self.x0 = rng.standard_normal(n)
        self.lvar, self.uvar = np.full(n, -1.0), np.full(n, 1.0)
        self.lvar[fixed] = self.uvar[fixed] = rng.uniform(-1, 1, len(fixed))
        self.jac_I, self.jac_J = rng.integers(0, m, 4 * n), rng.integers(0, n, 4 * n)
        self.hess_I, self.hess_J = rng.integers(0, n, 5 * n), rng.integers(0, n, 5 * n)
        self.y0, self.lcon, self.ucon = np.zeros(m), np.zeros(m), np.ones(m)


@pytest.mark.parametrize("fixed", [[0], [11], [0, 11], [0, 3, 4, 11], list(range(1, 12))], ids=str)
def test_reduced_structure_against_a_dense_construction(fixed):
    """Values scattered through the reduced structure give the dense matrix of the full structure with the fixed columns
    (Jacobian) / rows and columns (Hessian) deleted: renumbering, dropped entries, a fixed first and last variable."""
    n, m = 12, 7
    S = _Structure(n, m, fixed, seed=len(fixed))
    h = FV.FixedVariableHandler.create(S, True)
    free = np.setdiff1d(np.arange(n), fixed)
    assert h.fixed.tolist() == fixed and h.free.tolist() == free.tolist()
    assert np.array_equal(h.values, S.lvar[fixed]) and np.array_equal(h.x_full[fixed], S.lvar[fixed])
    rng = np.random.default_rng(1)
    jv, hv = rng.standard_normal(len(S.jac_I)), rng.standard_normal(len(S.hess_I))
    J, H = np.zeros((m, n)), np.zeros((n, n))
    np.add.at(J, (S.jac_I, S.jac_J), jv)
    np.add.at(H, (S.hess_I, S.hess_J), hv)
    Jr, Hr = np.zeros((m, len(free))), np.zeros((len(free), len(free)))
    np.add.at(Jr, (h.jac_I, h.jac_J), jv[h.ind_jac_free])
    np.add.at(Hr, (h.hess_I, h.hess_J), hv[h.ind_hess_free])
    assert np.array_equal(Jr, J[:, free]) and np.array_equal(Hr, H[np.ix_(free, free)])
    assert len(h.ind_jac_free) == (~np.isin(S.jac_J, fixed)).sum()
    assert len(h.ind_hess_free) == (~np.isin(S.hess_I, fixed) & ~np.isin(S.hess_J, fixed)).sum()
    assert h.structure_info().keys() == {"jac_I", "jac_J", "hess_I", "hess_J"}
    info = dict(n=len(free), m=m, **h.structure_info())
    assert all(np.array_equal(a, b) for a, b in zip(FV.structure(S, info), (h.jac_I, h.jac_J, h.hess_I, h.hess_J)))
    assert all(np.array_equal(a, b) for a, b in zip(FV.structure(S, dict(n=n, m=m)), (S.jac_I, S.jac_J, S.hess_I, S.hess_J)))
    x = rng.standard_normal(len(free))
    xf = h.expand(x)
    assert np.array_equal(xf[free], x) and np.array_equal(xf[fixed], S.lvar[fixed])


def test_reduced_and_frozen_callbacks_of_hs15():
    M = hs15_fixed()
    x, y = np.array([0.5, 1.7]), np.array([0.3, -1.1])
    hs, hd = FV.FixedVariableHandler.create(M, True), FV.FixedVariableHandler.create(M, False)
    R, F = hs.model, hd.model
    assert (R.n, F.n) == (1, 2) and R.lvar.tolist() == [-np.inf] and F.lvar.tolist() == [-np.inf, -np.inf]
    assert F.uvar.tolist() == [np.inf, np.inf] and F.x0.tolist() == [0.5, 0.0]
    assert R.obj(x[1:]) == M.obj(x) and np.array_equal(R.cons(x[1:]), M.cons(x))
    assert np.array_equal(R.grad(x[1:]), M.grad(x)[1:])
    assert np.array_equal(R.jac_coord(x[1:]), M.jac_coord(x)[[1, 3]]) and (R.jac_I.tolist(), R.jac_J.tolist()) == ([0, 1], [0, 0])
    assert np.array_equal(R.hess_coord(x[1:], y, 0.7), M.hess_coord(x, y, 0.7)[[2]])
    assert (R.hess_I.tolist(), R.hess_J.tolist()) == ([0], [0])
    J, H = M.jac_dense(x), M.hess_dense(x, y, 0.7)
    assert np.array_equal(F.jac_dense(x), np.array([[0.0, J[0, 1]], [0.0, J[1, 1]]]))
    assert np.array_equal(F.hess_dense(x, y, 0.7), np.array([[1.0, 0.0], [0.0, H[1, 1]]]))
    g = M.grad(x)
    hd.dense_grad(g, np.array([0.625, 1.7]))
    assert g.tolist() == [0.125, M.grad(x)[1]]


# ------------------------------------------------------------------------------------------------- 6. nothing fixed: nothing changes
@pytest.mark.parametrize("kind", KINDS)
def test_without_fixed_variables_the_history_is_identical(kind):
    a, b = run(kind, HS15Model()), run(kind, HS15Model(), treatment="relax_bound")
    assert a.fixed_handler is None and a.model is a.nlp
    assert a.status == b.status == "SOLVE_SUCCEEDED"
    assert [dataclasses.astuple(r) for r in a.history] == [dataclasses.astuple(r) for r in b.history]
    assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y) and np.array_equal(a.zl, b.zl) and np.array_equal(a.zu, b.zu)


# ------------------------------------------------------------------------------------------------- 7. refused combinations
def test_unknown_treatment_is_refused():
    with pytest.raises(ValueError, match="fixed_variable_treatment must be one of"):
        MadNLPSolver(HS15Model(), lambda info: None, IPMOptions(fixed_variable_treatment="MakeParameter"))


@pytest.mark.parametrize("approx,sparse", [("bfgs", False), ("damped_bfgs", False), ("compact_lbfgs", True)])
def test_quasi_newton_with_fixed_variables_is_refused(approx, sparse):
    opt = IPMOptions(fixed_variable_treatment="make_parameter", hessian_approximation=approx)
    with pytest.raises(ValueError, match="needs hessian_approximation = 'exact'"):
        MadNLPSolver(hs15_fixed(), lambda info: None, opt, sparse=sparse)


def test_the_sparse_qp_device_callbacks_with_fixed_variables_are_refused():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    M = SparseQPModel("case30")
    fix(M, [0, M.n - 1], [M.lvar[0], M.uvar[M.n - 1]])
    with pytest.raises(NotImplementedError, match="DeviceQPCallbacks.*constant offsets"):
        DeviceMadNLPSolver(M, lambda info: None, sparse_options(fixed_variable_treatment="make_parameter"))


@pytest.mark.parametrize("sparse", [True, False])
def test_a_model_without_a_free_variable_is_refused(sparse):
    M = fix(HS15Model(), [0, 1], [0.5, 2.0])
    with pytest.raises(ValueError, match="no free variable"):
        MadNLPSolver(M, lambda info: None, IPMOptions(fixed_variable_treatment="make_parameter"), sparse=sparse)


# ------------------------------------------------------------------------------------------------- 8. with NLP scaling
@pytest.mark.parametrize("kind", KINDS)
def test_nlp_scaling_with_a_fixed_variable(kind):
    """The `big = 1e6` simplex LP (reference test_scaling) with x3 fixed at 0.25: x = (0.75, 0, 0.25), y = -1, and from
    grad f + J'y = big (0, 1, 2): zl = (0, big, 2 big) -- the last one from update_z!, un-scaled.  `set_scaling!` sees the
    reduced gradient big (1, 2) in the sparse run and the model's own big (1, 2, 3) in the dense ones."""
    big = 1e6
    s = run(kind, fix(SimplexLPModel(big), [2], 0.25), nlp_scaling=True)
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.obj_scale == 100.0 / (2e6 if kind == "sparse_condensed" else 3e6) and s.con_scale[0] == 100.0 / 1e6
    r = s.solution()
    tol = np.sqrt(s.opt.tol)
    print(kind, s.cnt.k, r.solution, r.multipliers, r.multipliers_L, r.multipliers_U)
    assert r.solution[2] == 0.25
    assert np.abs(r.solution - [0.75, 0.0, 0.25]).max() <= tol
    assert abs(r.multipliers[0] + 1.0) <= tol
    assert abs(r.objective - 1.5 * big) <= tol * 1.5 * big
    assert np.abs(r.multipliers_L - [0.0, big, 2 * big]).max() <= tol * 2 * big
    assert r.multipliers_U[2] == 0.0 and np.abs(r.multipliers_U).max() <= tol

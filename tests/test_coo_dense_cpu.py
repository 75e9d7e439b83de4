"""`IPMOptions.callback` on the host driver: with "sparse" and `sparse=False` the model's COO callbacks are scattered, in COO
order, into the dense Jacobian and Hessian of the oracle's `DenseKKTSystem` / `DenseCondensedKKTSystem` (the reference's
SparseCallback on a dense KKT system, src/Callbacks/nlpmodels.jl:829-842, :863-881).  No GPU."""
import numpy as np
import pytest

from madnlp_jl_amd import ipm, tape_model as T
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.problems import ACOPFModel, DenseQPModel, HS15Model, LootsmaModel
from tests.coo_dense_cases import (HYPERBOLA_F, HYPERBOLA_X, HYPERBOLA_Y, SIZES, host_scatter_hess, host_scatter_jac,
                                   hyperbola_model, random_structure)
from tests.test_quasi_newton_cpu import oracle_factory

KINDS = ("dense", "dense_condensed")
APPROX = ("bfgs", "damped_bfgs")


def solve(nlp, kind, **kw):
    s = MadNLPSolver(nlp, oracle_factory(kind), IPMOptions(callback="sparse", tol=1e-8, **kw), sparse=False)
    s.solve()
    return s


def solcmp(a, b, tol):
    """The reference suite's rule (lib/MadNLPTests/src/MadNLPTests.jl: `solcmp`): absolute or relative to the largest entry."""
    d = np.abs(np.asarray(a) - np.asarray(b)).max()
    return d < tol or d / np.abs(b).max() < tol


# ------------------------------------------------------------------------------------------ 1. the scatter itself
class ThreeByThree:
    """Constant COO callbacks with duplicates, an upper-triangular Hessian entry and both orientations of one pair."""
    n = m = 3
    x0, y0 = np.ones(3), np.zeros(3)
    lvar, uvar = -np.ones(3), 2.0 * np.ones(3)
    lcon, ucon = -np.ones(3), np.ones(3)
    jac_I, jac_J = np.array([0, 2, 0, 1, 0]), np.array([1, 2, 1, 0, 1])
    JV = np.array([1.0, 4.0, 1e-20, -3.0, -1.0])
    hess_I, hess_J = np.array([0, 0, 2, 1, 2, 1]), np.array([0, 2, 0, 1, 0, 1])
    HV = np.array([5.0, 1.0, 1e-20, 7.0, -1.0, 0.5])

    def jac_coord(self, x):
        return self.JV.copy()

    def hess_coord(self, x, y, w=1.0):
        return w * self.HV


def test_host_scatter_against_hand_written_matrices():
    s = MadNLPSolver(ThreeByThree(), oracle_factory("dense"), IPMOptions(callback="sparse"), sparse=False)
    s.eval_jac(s.x)
    # (0, 1) receives 1, 1e-20, -1 in that order: (1 + 1e-20) - 1 = 0 exactly; another order would leave 1e-20
    assert np.array_equal(s.kkt.jac, np.array([[0.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [0.0, 0.0, 4.0]]))
    s.eval_lag_hess(s.x, s.y)
    # the pair {0, 2} receives 1 (upper), 1e-20 (lower), -1 (lower): 0 in both triangles; (1, 1) receives 7 + 0.5
    assert np.array_equal(s.kkt.hess, np.array([[5.0, 0.0, 0.0], [0.0, 7.5, 0.0], [0.0, 0.0, 0.0]]))
    s.eval_lag_hess(s.x, s.y, is_resto=True)
    assert np.array_equal(s.kkt.hess, np.zeros((3, 3)))


@pytest.mark.parametrize("m,n", SIZES)
def test_host_scatter_on_random_structures(m, n):
    """The driver's two scatters against the plain loops of coo_dense_cases, on integer values: exact."""
    S = random_structure(m, n)
    rng = np.random.default_rng(m + n)
    model = ThreeByThree()
    model.n, model.m = n, m
    model.x0, model.y0, model.lvar, model.uvar = np.ones(n), np.zeros(m), -np.ones(n), 2.0 * np.ones(n)
    model.lcon, model.ucon = -np.ones(m), np.ones(m)
    model.jac_I, model.jac_J, model.hess_I, model.hess_J = S["jac_I"], S["jac_J"], S["hess_I"], S["hess_J"]
    model.JV = rng.integers(-9, 10, len(S["jac_I"])).astype(float)
    model.HV = rng.integers(-9, 10, len(S["hess_I"])).astype(float)
    s = MadNLPSolver(model, oracle_factory("dense"), IPMOptions(callback="sparse"), sparse=False)
    s.eval_jac(s.x)
    s.eval_lag_hess(s.x, s.y)
    assert np.array_equal(s.kkt.jac, host_scatter_jac(m, n, S["jac_I"], S["jac_J"], model.JV))
    H = host_scatter_hess(n, S["hess_I"], S["hess_J"], model.HV)
    assert np.array_equal(s.kkt.hess, H) and np.array_equal(H, H.T)


# ------------------------------------------------------------------------------------------ 2. the option
def test_the_option_is_validated():
    assert ipm.CALLBACKS == ("auto", "sparse", "dense") and IPMOptions().callback == "auto"
    with pytest.raises(ValueError, match="callback must be one of"):
        MadNLPSolver(HS15Model(), oracle_factory("dense"), IPMOptions(callback="coo"), sparse=False)


@pytest.mark.parametrize("kind", KINDS)
def test_auto_and_dense_leave_the_dense_path_untouched(kind):
    """"auto" and "dense" call the model's `jac_dense` / `hess_dense` as before: a model whose COO callbacks raise runs, and the
    history is the one of a solver built without the option."""
    class DenseOnly(HS15Model):
        def jac_coord(self, x):
            raise AssertionError("COO callback on the dense path")
        hess_coord_ = HS15Model.hess_coord

        def hess_dense(self, x, y, w=1.0):
            h = self.hess_coord_(x, y, w)
            return np.array([[h[0], h[1]], [h[1], h[2]]], order="F")

        def hess_coord(self, x, y, w=1.0):
            raise AssertionError("COO callback on the dense path")
    ref = MadNLPSolver(HS15Model(), oracle_factory(kind), None, sparse=False)
    ref.solve()
    # what the commit before the option gave (there: 360.37976240508465 at (-0.7921232178, -1.2624298436); not compared bit
    # for bit, the host LAPACK may differ from machine to machine)
    assert (ref.cnt.k, ref.cnt.factorization_cnt) == (18, 24) and abs(ref.obj_val - 360.37976240508465) <= 1e-9
    assert np.abs(ref.x[:2] - np.array([-0.7921232178, -1.2624298436])).max() <= 1e-9
    for cb in ("auto", "dense"):
        s = MadNLPSolver(DenseOnly(), oracle_factory(kind), IPMOptions(callback=cb), sparse=False)
        s.solve()
        assert s.status == ref.status == "SOLVE_SUCCEEDED" and not s.coo_dense and s.jac_scale is None
        assert [tuple(vars(r).values()) for r in s.history] == [tuple(vars(r).values()) for r in ref.history]
        assert np.array_equal(s.x, ref.x) and np.array_equal(s.y, ref.y)


def test_sparse_callbacks_give_the_dense_callbacks_run():
    """HS15 has both sets of callbacks: COO order and dense evaluation agree entry for entry there, so the two runs do."""
    a = MadNLPSolver(HS15Model(), oracle_factory("dense"), IPMOptions(callback="sparse"), sparse=False)
    b = MadNLPSolver(HS15Model(), oracle_factory("dense"), IPMOptions(callback="dense"), sparse=False)
    a.solve(), b.solve()
    assert a.coo_dense and not b.coo_dense
    assert (a.status, a.cnt.k, a.cnt.factorization_cnt) == (b.status, b.cnt.k, b.cnt.factorization_cnt)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)


# ------------------------------------------------------------------------------------------ 3. known answers
@pytest.mark.parametrize("kind", KINDS)
def test_hs15_tape_exact(kind):
    s = solve(T.hs15_tape_model(), kind)
    sol = s.solution()
    print(kind, s.status, s.cnt.k, s.cnt.factorization_cnt, sol.solution, sol.objective)
    assert s.status == "SOLVE_SUCCEEDED"
    tol = np.sqrt(s.opt.tol)
    assert solcmp(sol.solution, [-0.7921, -1.2624], tol)        # the second documented optimum (docs/src/quickstart.md:202)
    assert solcmp([sol.objective], [360.3798], tol)
    assert (s.cnt.k, s.cnt.factorization_cnt) == (18, 24) and s.cnt.lag_hess_cnt == s.cnt.k


@pytest.mark.parametrize("approx", APPROX)
@pytest.mark.parametrize("kind", KINDS)
def test_hs15_tape_without_second_derivatives(kind, approx):
    M = T.hs15_tape_model()
    M.hess_coord = None                                          # never evaluated
    s = solve(M, kind, hessian_approximation=approx)
    sol = s.solution()
    print(kind, approx, s.status, s.cnt.k, s.cnt.factorization_cnt, sol.solution, sol.objective, s.qn.updates, s.qn.skipped)
    assert s.status == "SOLVE_SUCCEEDED"
    tol = np.sqrt(s.opt.tol)
    assert solcmp(sol.solution, [0.5, 2.0], tol) and solcmp([sol.objective], [306.49998], tol)
    assert s.cnt.lag_hess_cnt == 0 and s.qn.updates + s.qn.skipped == s.cnt.k - 1
    assert (s.cnt.k, s.cnt.factorization_cnt) == (11, 12)


@pytest.mark.parametrize("kind", KINDS)
def test_lootsma_tape_exact(kind):
    s = solve(T.lootsma_tape_model(), kind)
    sol = s.solution()
    print(kind, s.status, s.cnt.k, s.cnt.factorization_cnt, sol.solution, sol.objective, sol.multipliers)
    assert s.status == "SOLVE_SUCCEEDED"
    tol = np.sqrt(s.opt.tol)
    assert solcmp(sol.solution, LootsmaModel.LOOTSMA_X, tol) and solcmp(sol.multipliers, LootsmaModel.LOOTSMA_Y, tol)
    assert solcmp([sol.objective], [3.18222774], tol)
    assert (s.cnt.k, s.cnt.factorization_cnt) == (16, 21)


@pytest.mark.parametrize("approx,counts", [("exact", (7, 8)), ("bfgs", (11, 12)), ("damped_bfgs", (9, 10))])
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_hyperbola(kind, scaling, approx, counts):
    s = solve(hyperbola_model(), kind, hessian_approximation=approx, nlp_scaling=scaling)
    sol = s.solution()
    print(kind, scaling, approx, s.status, s.cnt.k, s.cnt.factorization_cnt, sol.solution, sol.objective, sol.multipliers)
    assert s.status == "SOLVE_SUCCEEDED"
    tol = np.sqrt(s.opt.tol)
    assert np.abs(sol.solution - HYPERBOLA_X).max() < tol and abs(sol.objective - HYPERBOLA_F) < tol
    assert np.abs(sol.multipliers - HYPERBOLA_Y).max() < tol
    assert (s.cnt.k, s.cnt.factorization_cnt) == counts
    if approx == "exact":
        assert s.cnt.lag_hess_cnt == s.cnt.k
    else:
        assert s.cnt.lag_hess_cnt == 0 and s.qn.updates + s.qn.skipped == s.cnt.k - 1


def test_scaled_coo_run_uses_the_sparse_scaling_factors():
    """A model whose constraint gradients exceed `nlp_scaling_max_gradient`: con_scale comes from `set_con_scale_sparse`, and
    jac_scale = con_scale[jac_I] exists in this mode; the un-scaled answer is the same."""
    def big():
        M = T.TapeModel(2, 2, np.array([2.0, 0.3]), 0.1, 10.0, np.array([1000.0, -np.inf]), np.array([1000.0, 3.0]), name="hyperbola1000")
        xy = np.array([[0, 1]])
        M.add_objective(T.V(0) * T.V(0) + T.V(1) * T.V(1), xy)
        M.add_constraint(1000.0 * T.V(0) * T.V(1), np.array([0]), xy)
        M.add_constraint(T.V(0) + T.V(1) * T.V(1), np.array([1]), xy)
        return M.finalize()
    s = solve(big(), "dense_condensed", nlp_scaling=True)
    sol = s.solution()
    assert s.status == "SOLVE_SUCCEEDED"
    assert s.con_scale[0] < 1.0 and s.con_scale[1] == 1.0
    assert np.array_equal(s.jac_scale, s.con_scale[np.asarray(s.model.jac_I)])
    tol = np.sqrt(s.opt.tol)
    assert np.abs(sol.solution - HYPERBOLA_X).max() < tol and abs(sol.multipliers[0] + 2e-3) < tol * 1e-3


# ------------------------------------------------------------------------------------------ 4. AC-OPF with its equalities
def test_acopf_case30_with_equalities_enforced():
    M, A = T.acopf_tape_model("case30"), ACOPFModel("case30")
    assert (M.n, M.m, int((M.lcon == M.ucon).sum()), len(M.jac_I), len(M.hess_I)) == (236, 348, 225, 1303, 1706)
    s = solve(M, "dense_condensed")
    r = solve(T.acopf_tape_model("case30"), "dense_condensed", relax_equality=True)
    h = solve(A, "dense_condensed")                  # the hand-written model through the same path
    print(s.status, s.cnt.k, s.cnt.factorization_cnt, s.solution().objective, r.cnt.k, r.cnt.factorization_cnt,
          r.solution().objective, h.cnt.k, h.solution().objective)
    assert s.status == r.status == h.status == "SOLVE_SUCCEEDED"
    assert s.m - s.ns == 225 and r.ns == r.m
    c = A.cons(s.solution().solution)
    assert (c >= A.lcon - 1e-5).all() and (c <= A.ucon + 1e-5).all()
    fs, fr, fh = s.solution().objective, r.solution().objective, h.solution().objective
    assert abs(fs - fr) <= 1e-5 * abs(fr) and abs(fh - fs) <= 1e-5 * abs(fs)
    assert (s.cnt.k, s.cnt.factorization_cnt) == (11, 12) and (r.cnt.k, r.cnt.factorization_cnt) == (13, 16)


# ------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("kind", KINDS)
def test_make_parameter_on_this_path_is_refused(kind):
    with pytest.raises(NotImplementedError, match="callback = 'sparse'.*make_parameter"):
        MadNLPSolver(T.lootsma_fixed_tape_model(), oracle_factory(kind),
                     IPMOptions(callback="sparse", fixed_variable_treatment="make_parameter"), sparse=False)
    # ... with fixed variables PRESENT: a model without any runs
    s = solve(hyperbola_model(), kind, fixed_variable_treatment="make_parameter")
    assert s.status == "SOLVE_SUCCEEDED" and s.fixed_handler is None


def test_dense_callbacks_of_a_model_without_them_are_refused():
    with pytest.raises(NotImplementedError, match="callback = 'dense'.*jac_dense"):
        MadNLPSolver(T.hs15_tape_model(), oracle_factory("dense"), IPMOptions(callback="dense"), sparse=False)
    assert hasattr(DenseQPModel(4, 2, 0), "jac_dense")
    MadNLPSolver(DenseQPModel(4, 2, 0), oracle_factory("dense"), IPMOptions(callback="dense"), sparse=False)

"""The adaptive barrier updates (`barrier = "loqo" / "quality_function"`, reference src/IPM/barrier.jl:95-316) of the host
driver on the CPU oracle back-end.  The reference's own test (test/madnlp_test.jl:262-276) solves HS15 with each rule and
compares with the default run at its `≈` (atol = rtol = sqrt(tol)); the same comparison runs here on every KKT formulation
and on further models, next to the rules' own behaviour and the golden-section search on its own."""
import math

import numpy as np
import pytest

from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver, golden_section, ordered_sum
from madnlp_jl_amd.problems import CubicDiskModel, DenseQPModel, HS15Model, LootsmaModel
from test_ipm_oracle import oracle_factory, run

KINDS = ["dense", "dense_condensed", "sparse_condensed"]
CONFIGS = {"loqo": dict(barrier="loqo"), "quality_function": dict(barrier="quality_function"),
           "quality_function_no_globalization": dict(barrier="quality_function", barrier_globalization=False)}


def hs15():
    """HS15 from (1, 1): from the class default (0, 0) the adaptive rules reach the problem's other local optimum."""
    nlp = HS15Model()
    nlp.x0 = np.array([1.0, 1.0])
    return nlp


MODELS = {"hs15": hs15, "lootsma": LootsmaModel, "cubic_disk": lambda: CubicDiskModel(1.5, [0.5, 0.5]),
          "qp_20_15_2": lambda: DenseQPModel(20, 15, 2), "qp_50_10_0": lambda: DenseQPModel(50, 10, 0)}
_runs = {}


def solved(model, kind, config):
    """One run per (model, formulation, configuration), shared by the tests below and never modified."""
    key = (model, kind, config)
    if key not in _runs:
        kw = {} if config == "monotone" else CONFIGS[config]
        _runs[key] = run(kind, MODELS[model](), tol=1e-8 if kind != "sparse_condensed" else 1e-6, **kw)
    return _runs[key]


def approx(a, b, tol):
    """The reference's `≈` with atol = rtol = tol on vectors: norm(a - b) <= max(tol, tol max(norm a, norm b))."""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    return np.linalg.norm(a - b) <= max(tol, tol * max(np.linalg.norm(a), np.linalg.norm(b)))


def model_kinds(model):
    return ["dense", "dense_condensed"] if model.startswith("qp_") else KINDS    # the dense QPs: dense formulations


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", ["hs15", "lootsma", "cubic_disk"])
def test_adaptive_rules_reach_the_monotone_solution(model, kind, config):
    s, ref = solved(model, kind, config), solved(model, kind, "monotone")
    assert ref.status == "SOLVE_SUCCEEDED"
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.cnt.k <= 100, s.cnt.k
    tol = math.sqrt(s.opt.tol)
    n = s.n
    assert approx(s.x[:n], ref.x[:n], tol), np.abs(s.x[:n] - ref.x[:n]).max()
    assert approx(s.y, ref.y, tol), np.abs(s.y - ref.y).max()
    assert approx(s.obj_val, ref.obj_val, tol), (s.obj_val, ref.obj_val)
    if model == "lootsma":     # the reference's pinned answers, as test_ipm_oracle.py checks them
        nlp = s.nlp
        cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731
        assert cmp(s.x[:3], nlp.LOOTSMA_X), s.x[:3]
        assert cmp(s.y, nlp.LOOTSMA_Y), s.y
        assert np.abs(s.zl[:3]).max() < tol and np.abs(s.zu[:3]).max() < tol


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
@pytest.mark.parametrize("model", ["qp_20_15_2", "qp_50_10_0"])
def test_adaptive_rules_reach_the_monotone_solution_of_the_dense_qps(model, kind, config):
    """x and the objective only: the multipliers of these QPs are not unique to that accuracy."""
    s, ref = solved(model, kind, config), solved(model, kind, "monotone")
    assert ref.status == "SOLVE_SUCCEEDED"
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.cnt.k <= 100, s.cnt.k
    tol = math.sqrt(s.opt.tol)
    assert approx(s.x[:s.n], ref.x[:s.n], tol), np.abs(s.x[:s.n] - ref.x[:s.n]).max()
    assert approx(s.obj_val, ref.obj_val, tol), (s.obj_val, ref.obj_val)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_rules_raise_mu_at_least_once(kind, config):
    mu = [h.mu for h in solved("hs15", kind, config).history]
    assert any(b > a for a, b in zip(mu, mu[1:])), mu


@pytest.mark.parametrize("kind", KINDS)
def test_monotone_never_raises_mu(kind):
    mu = [h.mu for h in solved("hs15", kind, "monotone").history]
    assert all(b <= a for a, b in zip(mu, mu[1:])), mu
    s = solved("hs15", kind, "monotone")
    assert s.cnt.barrier_update_cnt == s.cnt.probe_solve_cnt == s.cnt.quality_eval_cnt == 0


@pytest.mark.parametrize("config", ["quality_function", "quality_function_no_globalization"])
@pytest.mark.parametrize("kind", KINDS)
def test_quality_function_counts_two_probe_solves_per_update(kind, config):
    s = solved("hs15", kind, config)
    assert s.cnt.barrier_update_cnt > 0
    assert s.cnt.probe_solve_cnt == 2 * s.cnt.barrier_update_cnt
    # 2 values to place the interval, 4 to start the search, 1 to `qf_max_gs_iter` steps
    assert 7 * s.cnt.barrier_update_cnt <= s.cnt.quality_eval_cnt <= (6 + s.opt.qf_max_gs_iter) * s.cnt.barrier_update_cnt


def test_quality_function_keeps_mu_init_while_nothing_is_factorized():
    """sparse_condensed initializes the multipliers with zero: no factorization exists at iteration 0, the rule keeps mu."""
    s = solved("hs15", "sparse_condensed", "quality_function")
    assert s.history[0].mu == s.history[1].mu == s.opt.mu_init
    d = solved("hs15", "dense", "quality_function")          # least-squares multipliers: a factor exists, the rule runs
    assert d.history[1].mu != d.opt.mu_init


def test_unknown_barrier_is_rejected():
    nlp = hs15()
    with pytest.raises(ValueError, match="barrier"):
        MadNLPSolver(nlp, oracle_factory("dense", nlp), IPMOptions(barrier="mehrotra"), sparse=False)


# ---------------------------------------------------------------------------------------------- golden_section
def counted(f):
    calls = []

    def q(sigmas):
        calls.append(len(sigmas))
        return [f(s) for s in sigmas]
    return q, calls


def test_golden_section_returns_the_lower_end_of_an_increasing_function():
    q, calls = counted(lambda s: s)
    assert golden_section(q, 0.1, 1.0, 8, 1e-2) == 0.1
    assert sum(calls) <= 4 + 8 and calls[0] == 4 and all(c == 1 for c in calls[1:])


def test_golden_section_returns_the_upper_end_of_a_decreasing_function():
    q, calls = counted(lambda s: -s)
    assert golden_section(q, 0.1, 1.0, 8, 1e-2) == 1.0      # the end-point correction
    assert sum(calls) <= 4 + 8


@pytest.mark.parametrize("max_iter", [0, 1, 3, 8, 20])
def test_golden_section_evaluation_count(max_iter):
    q, calls = counted(lambda s: (s - 0.3) ** 2)
    golden_section(q, 1e-6, 1.0, max_iter, 0.0)
    assert sum(calls) == 4 + max_iter


def test_golden_section_brackets_an_interior_minimum():
    g = (3.0 - math.sqrt(5.0)) / 2
    q, calls = counted(lambda s: (s - 0.3) ** 2)
    bracket = []
    sigma = golden_section(q, 1e-6, 1.0, 8, 1e-2, bracket)
    (lo, hi), = bracket
    assert lo <= sigma <= hi
    assert hi - lo <= (1 - g) ** 8 * (1.0 - 1e-6) * (1 + 1e-12)
    # (the bracket need not hold the minimizer 0.3: with phi_mid2 = phi_mid1 after an else-branch step the next comparison
    # is between equal values and takes the else branch again -- the reference's search, restated as written)
    assert sum(calls) <= 12


# ---------------------------------------------------------------------------------------------- ordered_sum
def test_ordered_sum_adds_lanes_by_a_halving_tree():
    assert ordered_sum([]) == 0.0
    assert ordered_sum([1e16, 1.0, -1e16]) == 1.0            # (v0 + v2) + v1; left to right gives 0
    assert ordered_sum([1e16, -1e16, 1.0]) == 0.0            # (v0 + v2) + v1: the 1 is absorbed; left to right gives 1 ...
    v = np.zeros(65537)
    v[0], v[1], v[65536] = 1e16, 1.0, -1e16                  # ... and a second-trip element joins its lane before the tree
    assert ordered_sum(v) == 1.0
    ints = np.arange(1.0, 100001.0)
    assert ordered_sum(ints) == 100000 * 100001 / 2          # exact whatever the order

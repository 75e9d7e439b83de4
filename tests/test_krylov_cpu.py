"""The GMRES refinement iterator (`iterator = "krylov"`, madnlp_jl_amd/backsolve.py `KrylovIterator`) on
the host: exact-answer operators, restarts, trivial inputs, a stale factorization on the CPU oracle, whole IPM runs on the
oracle back-end against the Richardson runs, and the options.  No GPU."""
import numpy as np
import pytest

from madnlp_jl_amd import KrylovIterator, RichardsonIterator
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.kkt import UnreducedKKTVector
from madnlp_jl_amd.problems import ACOPFModel, HS15Model, LootsmaModel
from test_ipm_oracle import oracle_factory, run

TOL = 1e-8


class Vec:
    def __init__(self, n):
        self.values = np.zeros(n)

    def copy(self):
        c = Vec(len(self.values))
        c.values[:] = self.values
        return c


class StubKKT:
    """`mul` applies a dense A, `solve_kkt` an exact M^-1; the solves are counted and the preconditioned residual recorded."""

    def __init__(self, A, Minv):
        self.A, self.Minv, self.solves = A, Minv, 0

    def mul(self, w, x, alpha=1.0, beta=0.0):
        w.values[:] = alpha * (self.A @ x.values) + beta * w.values
        return w

    def solve_kkt(self, w):
        self.solves += 1
        w.values[:] = self.Minv @ w.values
        return w


def integer_similarity(n):
    """Unit lower-triangular P with small integer entries and its (integer) inverse."""
    P = np.eye(n)
    for i in range(1, n):
        P[i, i - 1] = (-1.0) ** i * (1 + i % 2)
    Pinv = np.round(np.linalg.inv(P))
    assert np.array_equal(P @ Pinv, np.eye(n))
    return P, Pinv


def stub(eigs):
    """A = P diag(eigs) P^-1 in small integers (or dyadic fractions), M = I: M^-1 A has exactly the eigenvalues `eigs`."""
    n = len(eigs)
    P, Pinv = integer_similarity(n)
    A = P @ np.diag(np.asarray(eigs, float)) @ Pinv
    return StubKKT(A, np.eye(n)), A


def refine(it, b):
    n = len(b)
    x, bb, w = Vec(n), Vec(n), Vec(n)
    bb.values[:] = b
    ok = it.solve_refine(x, bb, w)
    return ok, x.values


def ratio(A, x, b):
    nb = np.abs(b).max()
    return np.abs(b - A @ x).max() / (min(np.abs(x).max(), 1e6 * nb) + nb)


# ------------------------------------------------------------------------------------------------- exact-answer operator
def test_two_eigenvalues_richardson_diverges_gmres_ends_in_two_steps():
    """M^-1 A diagonalizable with the eigenvalues {1, 3}, order 12: Richardson's iteration matrix I - M^-1 A has the eigenvalue
    -2, so its residual ratio grows from step to step; the minimal polynomial has degree 2, so GMRES is exact after two Arnoldi
    steps.  x* = A^-1 b is known exactly: A^-1 = P diag(1, 1/3) P^-1 and b = A x* for an integer x*."""
    eigs = [1.0, 3.0] * 6
    kkt, A = stub(eigs)
    xs = np.arange(1.0, 13.0) * np.where(np.arange(12) % 3 == 0, -1.0, 1.0)
    b = A @ xs                                    # exact: small integers
    ratios = []
    for steps in range(1, 7):
        rich = RichardsonIterator(kkt, tol=TOL, max_iter=steps)
        ok, _ = refine(rich, b)
        assert not ok and rich.ir == steps
        ratios.append(rich.residual_ratio)
    assert all(q > p for p, q in zip(ratios, ratios[1:])), ratios           # grows from step to step
    ok, _ = refine(RichardsonIterator(kkt, tol=TOL), b)
    assert not ok
    kkt.solves = 0
    it = KrylovIterator(kkt, tol=TOL)
    ok, x = refine(it, b)
    assert ok and it.ir <= 4 and it.steps <= 2, (it.ir, it.steps)
    assert it.ir == kkt.solves
    assert np.abs(x - xs).max() <= 1e-12 * np.abs(xs).max()
    assert it.residual_ratio == ratio(A, x, b) < TOL ** (5 / 4)


# ------------------------------------------------------------------------------------------------------------ restart
def test_restarted_cycles_decrease_monotonically():
    eigs = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0] * 2
    kkt, A0 = stub(eigs)
    scale = 2.0 ** (np.arange(12) % 3)            # M = diag(scale), A = M A0: M^-1 A = A0 exactly, eigenvalues `eigs`
    A = kkt.A = np.diag(scale) @ A0
    kkt.Minv = np.diag(1.0 / scale)
    b = np.arange(1.0, 13.0)
    it = KrylovIterator(kkt, tol=TOL, restart=2, max_iter=12)
    pre = []                                                                 # |M^-1 (b - A x)|_2 at every cycle's start
    orig = it._cycle

    def cycle(x, w, beta0):
        pre.append(np.linalg.norm(kkt.Minv @ (b - A @ x.values)))
        orig(x, w, beta0)
    it._cycle = cycle
    ok, x = refine(it, b)
    pre.append(np.linalg.norm(kkt.Minv @ (b - A @ x)))
    assert it.cycles >= 2 and it.ir <= 12 and it.ir == kkt.solves, (it.cycles, it.ir)
    assert it.steps <= 2 * it.cycles
    for beta, rho in it.trace:
        assert len(rho) >= 1 and rho[0] <= beta * (1 + 1e-14)
        assert all(q <= p * (1 + 1e-14) for p, q in zip(rho, rho[1:])), rho
    assert all(q <= p * (1 + 1e-12) for p, q in zip(pre, pre[1:])), pre
    assert [t[0] for t in it.trace] == pytest.approx(pre[:len(it.trace)], rel=1e-9)


def test_a_single_remaining_solve_is_a_richardson_step():
    kkt, A = stub([0.5, 1.0, 1.5, 2.0, 2.5, 3.0] * 2)
    it = KrylovIterator(kkt, tol=TOL, restart=2, max_iter=2)
    refine(it, np.arange(1.0, 13.0))
    assert it.ir == kkt.solves == 2 and it.steps == 0


# ------------------------------------------------------------------------------------------------------ trivial inputs
def test_zero_right_hand_side_and_exact_factor():
    kkt, A = stub([1.0, 2.0] * 6)
    it = KrylovIterator(kkt, tol=TOL)
    ok, x = refine(it, np.zeros(12))
    assert ok and it.ir == 0 and kkt.solves == 0 and not x.any()
    P, Pinv = integer_similarity(12)
    exact = StubKKT(A, P @ np.diag([1.0, 0.5] * 6) @ Pinv)                    # M = A: A^-1 in dyadic fractions, exact
    assert np.array_equal(exact.Minv @ A, np.eye(12))
    xs = np.arange(1.0, 13.0)
    it = KrylovIterator(exact, tol=TOL)
    ok, x = refine(it, A @ xs)
    assert ok and it.ir == 1 and it.steps == 0 and it.cycles == 0
    assert np.abs(x - xs).max() <= 1e-13 * np.abs(xs).max()


# ---------------------------------------------------------------------------------------- stale factor on the oracle
def acopf_options(**kw):
    o = IPMOptions(tol=1e-6, **kw)
    o.relax_equality, o.dual_initialization = True, "zero"
    return o


@pytest.fixture(scope="module")
def stale_case30():
    """AC-OPF case30, sparse condensed, oracle back-end: the state after 8 iterations, the KKT matrix built and factorized
    there, then the compressed Hessian multiplied by 1 + theta = 3 WITHOUT a new factorization."""
    nlp = ACOPFModel("case30")
    s = MadNLPSolver(nlp, oracle_factory("sparse_condensed", nlp), acopf_options(max_iter=8), sparse=True)
    assert s.solve() == "MAXIMUM_ITERATIONS_EXCEEDED" and s.cnt.k == 8
    s.eval_lag_hess(s.x, s.y)
    s.set_aug_diagonal()
    s.factorize_wrapper()
    s.kkt.hess_com.nzval *= 3.0
    return s


@pytest.mark.parametrize("seed", [3, 4])
def test_stale_factor_richardson_fails_gmres_succeeds(stale_case30, seed):
    """Measured on the oracle: Richardson ratio 2.2e-2 / 1.2e-2 after 10 solves, GMRES 6.6e-9 / 2.4e-9
    with 10 solves (5 Arnoldi steps in 3 cycles); the bounds leave more than two decades on Richardson's side and more than one
    on GMRES's."""
    s = stale_case30
    V = lambda: UnreducedKKTVector.from_kkt(s.kkt)      # noqa: E731
    b = V()
    b.values[:] = np.random.default_rng(seed).standard_normal(len(b.values))
    x, w = V(), V()
    rich = RichardsonIterator(s.kkt, tol=1e-8)
    ok = rich.solve_refine(x, b, w)
    print("richardson", seed, rich.ir, rich.residual_ratio)
    assert not ok and rich.residual_ratio > 1e-4
    it = KrylovIterator(s.kkt, tol=1e-8)
    ok = it.solve_refine(x, b, w)
    print("krylov", seed, it.ir, it.steps, it.cycles, it.residual_ratio)
    assert ok and it.residual_ratio < 1e-7 and it.ir <= 10
    w.values[:] = b.values                              # the ratio again, outside the iterator
    s.kkt.mul(w, x, -1.0, 1.0)
    nb = np.abs(b.values).max()
    assert np.abs(w.values).max() / (min(np.abs(x.values).max(), 1e6 * nb) + nb) == it.residual_ratio


# ------------------------------------------------------------------------------------- IPM runs on the oracle back-end
KINDS = ["dense", "dense_condensed", "sparse_condensed"]
_runs = {}


def solved(model, kind, iterator):
    key = (model, kind, iterator)
    if key not in _runs:
        nlp = {"hs15": HS15Model, "lootsma": LootsmaModel}[model]()
        _runs[key] = run(kind, nlp, tol=1e-8 if kind != "sparse_condensed" else 1e-6, iterator=iterator)
    return _runs[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", ["hs15", "lootsma"])
def test_ipm_with_gmres_follows_the_richardson_run(model, kind):
    s, ref = solved(model, kind, "krylov"), solved(model, kind, "richardson")
    assert isinstance(s.iterator, KrylovIterator) and isinstance(ref.iterator, RichardsonIterator)
    assert ref.status == "SOLVE_SUCCEEDED" and s.status == "SOLVE_SUCCEEDED", s.status
    assert abs(s.obj_val - ref.obj_val) <= 1e-6 * abs(ref.obj_val), (s.obj_val, ref.obj_val)
    assert s.cnt.k == ref.cnt.k, (s.cnt.k, ref.cnt.k)
    assert s.cnt.backsolve_cnt > 0


@pytest.mark.parametrize("case", ["case30", "case118"])
def test_acopf_with_gmres_follows_the_richardson_run(case):
    nlp = ACOPFModel(case)
    out = {}
    for iterator in ("richardson", "krylov"):
        s = MadNLPSolver(nlp, oracle_factory("sparse_condensed", nlp), acopf_options(iterator=iterator), sparse=True)
        total = []
        inner = s.solve_refine_wrapper
        s.solve_refine_wrapper = lambda *a, _f=inner, _s=s: (_f(*a), total.append(_s.iterator.ir))[0]
        assert s.solve() == "SOLVE_SUCCEEDED"
        assert s.cnt.backsolve_cnt == sum(total)
        out[iterator] = s
    s, ref = out["krylov"], out["richardson"]
    print(case, "k", s.cnt.k, ref.cnt.k, "factorizations", s.cnt.factorization_cnt, ref.cnt.factorization_cnt, "backsolves",
          s.cnt.backsolve_cnt, ref.cnt.backsolve_cnt)
    assert abs(s.obj_val - ref.obj_val) <= 1e-6 * abs(ref.obj_val), (s.obj_val, ref.obj_val)
    assert s.cnt.k == ref.cnt.k, (s.cnt.k, ref.cnt.k)
    x = s.x[:nlp.n]
    c = nlp.cons(x)                                     # feasibility as in tests/test_acopf.py
    assert (c >= nlp.lcon - 1e-5).all() and (c <= nlp.ucon + 1e-5).all()
    assert (x >= nlp.lvar - 1e-7).all() and (x <= nlp.uvar + 1e-7).all()
    assert abs(nlp.obj(x) - s.obj_val) <= 1e-9 * abs(s.obj_val)


# ------------------------------------------------------------------------------------------------------------ options
def test_options():
    assert IPMOptions().iterator == "richardson"
    assert (IPMOptions().krylov_restart, IPMOptions().krylov_max_iter, IPMOptions().krylov_tol) == (5, 10, 1e-10)
    nlp = HS15Model()
    make = lambda **kw: MadNLPSolver(nlp, oracle_factory("dense", nlp), IPMOptions(**kw), sparse=False)   # noqa: E731
    with pytest.raises(ValueError, match="richardson.*krylov"):
        make(iterator="cg")
    for bad in (0, 9):
        with pytest.raises(ValueError, match="krylov_restart"):
            make(iterator="krylov", krylov_restart=bad)
    with pytest.raises(ValueError, match="krylov_max_iter"):
        make(iterator="krylov", krylov_max_iter=0)
    assert isinstance(make().iterator, RichardsonIterator)
    it = make(iterator="krylov", krylov_restart=8, krylov_max_iter=3, krylov_tol=1e-6).iterator
    assert (it.restart, it.max_iter, it.krylov_tol) == (8, 3, 1e-6)

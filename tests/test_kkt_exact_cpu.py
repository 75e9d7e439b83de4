"""The exact KKT cases of tests/kkt_exact.py are what they claim to be, and the oracle agrees with them (runs anywhere).

For every (kind, shape): H, b and the condensed matrix A are exact (scaled integers everywhere, `fractions.Fraction` on the small
shape and on sampled entries of the large ones) and `bit_budget` stays below 53 bits; A[n:, n:] is diagonal; every Sigma_s and
every D is a power of four; the inertia of A by the signs of d is (n, 0, n_eq); the fp64 `solve_kkt!` chain returns x* under three
summation orders; the `oracle/` classes' `mul` and `build_kkt` give the exact answers bit for bit (which pins `unreduced_matrix`
against an independent restatement, and the oracle against the definition).  On the rounded cases the oracle alone meets both
per-entry bounds and its residual stays below 1e-12, so that the acceptance of the GPU test (100 x the oracle's residual) is not
vacuous."""
from fractions import Fraction

import numpy as np
import pytest

from tests import kkt_exact as ke

CASES = [(k, s) for k in ke.KINDS for s in ke.SHAPES[k]]
ORDERS = ("forward", "backward", "random")


def _id(v):
    return v if isinstance(v, str) else "-".join(map(str, v))


_CACHE = {}


def _case(param):
    if param not in _CACHE:
        _CACHE[param] = ke.exact_kkt_case(param[0], *param[1])
    return _CACHE[param]


@pytest.fixture(params=CASES, ids=lambda p: f"{p[0]}-{_id(p[1])}")
def case(request):
    return _case(request.param)


@pytest.fixture(params=[p for p in CASES if p[0] != "dense"], ids=lambda p: f"{p[0]}-{_id(p[1])}")
def condensed_case(request):
    """(The augmented system has no exact factorization: its solve_kkt! is checked on rounded data.)"""
    return _case(request.param)


def _frac(a):
    return [Fraction(float(v)) for v in a]


def _pow4(v):
    e = np.log2(v)
    return np.all(v > 0) and np.array_equal(e, np.rint(e)) and np.all(e.astype(np.int64) % 2 == 0)


def test_the_data_are_dyadic_and_the_budget_holds(case):
    c = case
    n, npr = c.n, c.npr
    assert ke.bit_budget(c) < 53, ke.bit_budget(c)
    for name in ("reg", "du_diag", "l_diag", "u_diag", "l_lower", "u_lower", "H", "jac", "xstar", "pr_diag", "D"):
        ke.to_int(getattr(c, name))                                      # multiples of 2^-8
    assert (c.l_diag < 0).all() and (c.u_diag < 0).all() and (c.l_lower > 0).all() and (c.u_lower > 0).all()
    for v in (-c.l_diag, -c.u_diag, c.l_lower, c.u_lower, c.reg[:n]):
        assert np.array_equal(np.log2(v), np.rint(np.log2(v)))           # powers of two
    assert not c.reg[n:].any()
    assert _pow4(c.pr_diag[n:]) and _pow4(c.D), "Sigma_s and D are powers of four"
    assert np.array_equal(np.sqrt(c.D) ** 2, c.D)
    # the index sets: interleaved rows, every kind of bound on x, every slack bounded
    assert np.array_equal(np.sort(np.concatenate((c.ind_eq, c.ind_ineq))), np.arange(c.m))
    if c.n_eq and c.ns:
        assert c.ind_eq.min() < c.ind_ineq.max() and c.ind_ineq.min() < c.ind_eq.max() or min(c.n_eq, c.ns) == 1
    lb, ub = np.isin(np.arange(npr), c.ind_lb), np.isin(np.arange(npr), c.ind_ub)
    assert (lb | ub)[n:].all(), "a slack without a bound"
    for pattern in ((True, True), (True, False), (False, True), (False, False)):
        assert ((lb[:n] == pattern[0]) & (ub[:n] == pattern[1])).any(), pattern
    # the condensed matrix and its factors
    A = c.A
    assert np.array_equal(A, A.T)
    assert np.array_equal(A[n:, n:], np.diag(np.diagonal(A)[n:])), "A[n:, n:] is not diagonal"
    assert (c.d[:n] > 0).all() and (c.d[n:] < 0).all() and c.inertia() == (n, 0, c.n_eq)
    assert abs(c.Nmat @ c.Nmat).nnz == 0 or not (c.Nmat @ c.Nmat).toarray().any()
    assert np.array_equal(np.abs(np.log2(np.abs(c.d))) % 2, np.zeros(len(c.d)))
    if c.kind != "dense":
        assert np.array_equal(ke.reduced_matrix(c), A), "build_kkt!'s matrix is not A"


def test_hessian_right_hand_side_and_matrix_are_exact_in_fractions(case):
    """H = A[:n, :n] - diag(pr_x) - J_i' D J_i, b = K_u x* and A = (I + N) diag(d) (I + N)' entry by entry in rationals: all of
    the small shape, sampled rows of the others."""
    c = case
    n = c.n
    rng = np.random.default_rng(5)
    rows = np.arange(n) if n <= 5 else rng.choice(n, size=3, replace=False)
    A, Ji, D, pr = c.A, c.jac[c.ind_ineq], c.D, c.pr_diag
    M = np.eye(c.n + c.n_eq) + c.Nmat.toarray()
    for i in rows:
        cols = np.arange(n) if n <= 5 else rng.choice(n, size=12, replace=False)
        for j in cols:
            want = Fraction(float(A[i, j])) - (Fraction(float(pr[i])) if i == j else 0) \
                - sum(Fraction(float(Ji[k, i])) * Fraction(float(D[k])) * Fraction(float(Ji[k, j])) for k in range(c.ns))
            assert Fraction(float(c.H[i, j])) == want, (i, j)
            a = sum(Fraction(float(M[i, k])) * Fraction(float(c.d[k])) * Fraction(float(M[j, k])) for k in range(len(c.d)))
            assert Fraction(float(A[i, j])) == a, (i, j)
    K, b, xs = ke.unreduced_matrix(c), c.b, _frac(c.xstar)
    for i in (np.arange(c.lw) if c.lw <= 40 else rng.choice(c.lw, size=25, replace=False)):
        nz = np.flatnonzero(K[i])
        assert Fraction(float(b[i])) == sum(Fraction(float(K[i, j])) * xs[j] for j in nz), i
    # ... and all of b in scaled integers
    assert np.array_equal(b, ke.exact_mul(c, c.xstar, np.zeros(c.lw), 1.0, 0.0))


def test_the_fp64_chain_returns_the_solution_in_every_order(condensed_case):
    case = condensed_case
    for order in ORDERS:
        got = ke.solve_chain(case, case.b, order, seed=11)
        assert np.array_equal(got, case.xstar), order


def test_the_oracle_gives_the_exact_answers(case):
    """`mul` for every (alpha, beta) and `build_kkt` of the oracle class, bit for bit."""
    c = case
    ko = ke.oracle_system(c)
    for name in ("pr_diag",):
        assert np.array_equal(getattr(ko, name), getattr(c, name))
    for k, (alpha, beta) in enumerate(ke.ALPHA_BETA):
        x, w = ke.draw_vector(c, 2 * k), ke.draw_vector(c, 2 * k + 1)
        got = ko.mul(ke.oracle_vector(ko, w), ke.oracle_vector(ko, x), alpha, beta).values
        assert np.array_equal(got, ke.exact_mul(c, x, w, alpha, beta)), (alpha, beta)
    want = ke.reduced_matrix(c)
    if c.kind == "sparse_condensed":
        cols = np.repeat(np.arange(c.n), np.diff(ko.aug_com.colptr))
        assert np.array_equal(ko.aug_com.nzval, want[ko.aug_com.rowval, cols])
        full = ko.aug_com.to_dense()
        assert np.array_equal(full, np.tril(want)), "the pattern of aug_com misses a nonzero of A"
    else:
        assert np.array_equal(np.tril(ko.aug_com), np.tril(want))      # (the oracle's upper triangle mirrors the garbage of hess)


def test_the_scaled_case_is_the_base_case_in_other_units():
    c = ke.exact_kkt_case("dense_condensed", 130, 97, 14)
    s = ke.scaled_case(c, 20, 0, 40)
    units = ke.solution_units(s)
    assert units.min() == 0 and units.max() == 40
    assert {int(units[v][0]) for v in s.blocks().values()} == {0, 20, 40}
    assert np.array_equal(s.b, np.ldexp(c.b, ke.rhs_units(s)))
    assert np.array_equal(ke.reduced_matrix(s), s.A) and s.inertia() == c.inertia()
    assert _pow4(s.pr_diag[s.n:]) and _pow4(s.D)
    assert ke.bit_budget(s) == ke.bit_budget(c) < 53
    for order in ORDERS:
        assert np.array_equal(ke.solve_chain(s, s.b, order, seed=12), s.xstar), order
    ko = ke.oracle_system(s)
    got = ko.mul(ke.oracle_vector(ko, 0.0), ke.oracle_vector(ko, s.xstar), 1.0, 0.0).values
    assert np.array_equal(got, s.b)


# ------------------------------------------------------------------------------------------------ rounded data
@pytest.mark.parametrize("shape", ke.ROUNDED_SHAPES, ids=_id)
@pytest.mark.parametrize("kind", ke.KINDS)
def test_the_oracle_meets_the_bounds_on_rounded_data(kind, shape):
    c = ke.random_kkt_case(kind, *shape)
    ko = ke.oracle_system(c)
    rng = np.random.default_rng(3)
    for alpha, beta in ke.ALPHA_BETA:
        x, w = rng.standard_normal(c.lw), rng.standard_normal(c.lw)
        got = ko.mul(ke.oracle_vector(ko, w), ke.oracle_vector(ko, x), alpha, beta).values
        ref, bound = ke.mul_bound(c, x, w, alpha, beta)
        assert (np.abs(got - ref) <= bound).all(), (alpha, beta, float((np.abs(got - ref) / bound).max()))
    if kind == "dense_condensed":
        ref, bound = ke.build_bound(c)
        i, j = np.tril_indices(c.order)
        assert (np.abs(ko.aug_com - ref)[i, j] <= bound[i, j]).all()
    b = rng.standard_normal(c.lw)
    x, res = ke.oracle_residual(c, b)
    print(f"{kind} {shape}: oracle residual {res:.2e}")
    assert res <= 1e-12, res

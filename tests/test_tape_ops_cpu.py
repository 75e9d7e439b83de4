"""The tape vocabulary beyond + - * / and sin cos exp log sqrt (`madnlp_jl_amd.tape_model`), host half: real powers, tan atan
tanh and the piecewise abs_ sign step minimum maximum -- exact values and derivative tapes at signed zeros and ties written out
by hand, how powers fold, that existing tapes did not change, finite differences, and three NLPs with closed-form optima on the
host driver.  `tests/test_hip_tape_ops.py` runs the device interpreter against this one."""
import numpy as np
import pytest

from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.tape_model import P, V, TapeModel
from tests import tape_ops_cases as K
from tests.test_tape_model_cpu import _dense_hess, _dense_jac, _options, integer_model


# ------------------------------------------------------------------------------------------------- 1. exact values
def _same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


def test_selection_operations_give_the_hand_written_values_at_zeros_and_ties():
    M = K.selection_model()
    x = np.array(K.SEL_A + K.SEL_B)
    c = M.cons(x).reshape(5, 5)          # (0.0 + v keeps v's bits except for v = -0.0, which the sum order turns into +0.0)
    assert c[0].tolist() == [0.0, 0.0, 2.0, 1.5, 3.0]                     # abs_
    assert c[1].tolist() == [0.0, 0.0, 1.0, 1.0, -1.0]                    # sign: 0 for both zeros
    assert c[2].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]                     # step: 1 for both zeros
    assert c[3].tolist() == [0.0, 0.0, 2.0, -2.5, -3.0]                   # minimum
    assert c[4].tolist() == [0.0, 0.0, 2.0, 1.5, 4.0]                     # maximum
    # the value tapes themselves, sign bits included: a tie -- and +0 against -0 is one -- returns `a`
    xv = [np.array(K.SEL_A), np.array(K.SEL_B)]
    val = lambda i: M.patterns[i].tapes[0].run(xv, [], 5)[0]  # noqa: E731
    _same_bits(val(0), [0.0, 0.0, 2.0, 1.5, 3.0])
    _same_bits(val(3), [0.0, -0.0, 2.0, -2.5, -3.0])
    _same_bits(val(4), [0.0, -0.0, 2.0, 1.5, 4.0])
    # first-derivative tapes: abs_ -> sign(a); minimum -> (step(b - a), 1 - step(b - a)); maximum -> (step(a - b), 1 - step(a - b));
    # sign and step have none.  At a tie the derivative is the one of `a`, like the value.
    assert [p.tapes[1].nout for p in M.patterns] == [1, 0, 0, 2, 2]
    assert [p.tapes[2].nout for p in M.patterns] == [0, 0, 0, 0, 0] and len(M.hess_I) == 0
    assert M.jac_coord(x).tolist() == [0.0, 0.0, 1.0, 1.0, -1.0,
                                       1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0,
                                       1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert M.jac_I.tolist() == list(range(5)) + 2 * list(range(15, 20)) + 2 * list(range(20, 25))
    assert M.jac_J.tolist() == list(range(5)) + 2 * list(range(10))


def test_a_nan_in_b_returns_a_and_sign_of_nan_is_zero():
    nan = float("nan")
    a, b = [np.array([1.0, nan, -2.0])], [np.array([nan, 1.0, nan])]
    run = lambda e: Tape1(e).run(a, b, 3)[0]  # noqa: E731
    Tape1 = lambda e: T.Tape([e])  # noqa: E731
    np.testing.assert_array_equal(run(T.minimum(V(0), P(0))), [1.0, nan, -2.0])
    np.testing.assert_array_equal(run(T.maximum(V(0), P(0))), [1.0, nan, -2.0])
    np.testing.assert_array_equal(run(T.sign(V(0))), [1.0, 0.0, -1.0])
    np.testing.assert_array_equal(run(T.step(V(0))), [1.0, 0.0, 0.0])
    assert not np.signbit(run(T.abs_(P(0) * -1.0))).any()


def test_sign_and_step_drop_out_of_the_sparsity_pattern():
    M = TapeModel(3, 1, np.zeros(3), -1.0, 1.0, 0.0, 0.0)
    M.add_constraint(T.sign(V(0)) + T.step(V(1)) * 3.0 + V(2) * V(2), np.array([0]), np.array([[0, 1, 2]]))
    M.add_objective(T.step(V(0) * V(1)) + T.sign(V(2) - 1.0), np.array([[0, 1, 2]]))
    M.finalize()
    assert M.patterns[0].tapes[1].out_j.tolist() == [2] and M.patterns[0].tapes[2].out_j.tolist() == [2]
    assert M.patterns[1].tapes[1].nout == 0 and M.patterns[1].tapes[2].nout == 0
    assert (M.jac_I.tolist(), M.jac_J.tolist(), M.hess_I.tolist(), M.hess_J.tolist()) == ([0], [2], [2], [2])
    assert M.cons(np.array([-0.5, 0.0, 2.0]))[0] == -1.0 + 3.0 + 4.0 and M.obj(np.array([-0.5, 0.5, 2.0])) == 0.0 + 1.0
    assert (M.grad(np.ones(3)) == 0.0).all()


def test_the_hinge_penalty_has_one_hessian_output_and_exact_values():
    M = TapeModel(4, 0, np.zeros(4), -10.0, 10.0, 0.0, 0.0)
    M.add_objective(T.maximum(V(0) - 1, 0) ** 2, np.arange(4)[:, None])
    M.finalize()
    assert M.patterns[0].tapes[2].nout == 1
    x = np.array([0.5, 1.0, 3.0, -2.0])                    # below the kink, on it (a tie: the `a` branch, whose value is 0), above
    assert M.obj_terms(x).tolist() == [0.0, 0.0, 4.0, 0.0]
    assert M.grad(x).tolist() == [0.0, 0.0, 4.0, 0.0]
    assert M.hess_coord(x, np.zeros(0), 1.0).tolist() == [0.0, 2.0, 2.0, 0.0]


def test_new_functions_fold_constants_and_leave_domain_errors_to_run_time():
    import math
    assert T.tan(0.5).value == math.tan(0.5) and T.atan(2.0).value == math.atan(2.0) and T.tanh(-1.0).value == math.tanh(-1.0)
    assert T.abs_(-3.0).value == 3.0 and not np.signbit(T.abs_(-0.0).value)
    assert [T.sign(v).value for v in (2.0, -2.0, 0.0, -0.0)] == [1.0, -1.0, 0.0, 0.0]
    assert [T.step(v).value for v in (2.0, -2.0, 0.0, -0.0)] == [1.0, 0.0, 1.0, 1.0]
    assert T.minimum(2.0, -1).value == -1.0 and T.maximum(2.0, -1).value == 2.0
    assert T.pow_(2.0, 1.5).value == math.pow(2.0, 1.5)
    e = T.pow_(-2.0, 1.5)                                   # math.pow raises: not folded, NaN at run time
    with np.errstate(invalid="ignore"):
        assert e.op == T.OP_POW and np.isnan(T.Tape([e]).run([], [], 1)[0][0])
    assert (2.0 ** V(0)).op == T.OP_POW and (2.0 ** V(0)).a.value == 2.0
    assert T.minimum(V(0), 1).op == T.OP_MIN and T.maximum(P(0), V(1) * 2.0).op == T.OP_MAX
    assert T.OP_NAMES[16:25] == ("pow", "tan", "atan", "tanh", "abs", "sign", "step", "min", "max") and T.OP_NAMES[10:16] == (None,) * 6


# ------------------------------------------------------------------------------------------------- 2. powers
def _ops(e, seen=None):
    seen = {} if seen is None else seen
    if id(e) not in seen and e.op not in ("const", "var", "par"):
        seen[id(e)] = e.op
        _ops(e.a, seen)
        _ops(e.b, seen)
    return list(seen.values())


def test_powers_fold_to_products_quotients_and_square_roots():
    e = V(0) * P(0) + 1.0
    assert e ** 2.0 is e * e and e ** 3 is e * e * e and e ** np.int64(2) is e * e
    assert e ** 0.5 is T.sqrt(e)
    assert e ** -2 is 1 / (e * e) and e ** -1.0 is 1 / e
    assert (e ** 0).value == 1.0 and (e ** 0.0).value == 1.0 and e ** 1 is e and e ** 1.0 is e
    assert (e ** 1.5).op == T.OP_POW and (e ** V(1)).op == T.OP_POW and (e ** T.const(2)) is e * e
    d = T.diff(T.pow_(V(0), 1.5), 0)                       # 1.5 pow(v, 0.5) -> 1.5 sqrt(v)
    assert T.OP_SQRT in _ops(d) and T.OP_POW not in _ops(d)
    d = T.diff(V(0) ** 2.5, 0)                             # 2.5 pow(v, 1.5): stays a pow
    assert _ops(d).count(T.OP_POW) == 1 and d.a.value == 2.5 and d.b.b.value == 1.5
    d = T.diff(T.pow_(P(0), V(0)), 0)                      # d/dv p^v = p^v log p: nothing divides by the base
    assert sorted(_ops(d)) == sorted([T.OP_MUL, T.OP_POW, T.OP_LOG])


# digests of the `code` arrays as the commit before the new operations compiled them (tape_ops_cases.code_digest)
PARENT_DIGESTS = {"integer": "f86f57cb478e1b6858bfd80afbdef2edf9a461b1ecb1c6cdcb7b977e5b36b498",
                  "case30": "1448ec622a750923f38dba50043bd3b99830212f046f6ea5ac689397cb80cce2"}


def test_existing_models_compile_to_the_same_instructions_as_before():
    assert K.code_digest(integer_model()) == PARENT_DIGESTS["integer"]
    assert K.code_digest(T.acopf_tape_model("case30")) == PARENT_DIGESTS["case30"]


# ------------------------------------------------------------------------------------------------- 3. finite differences
def test_derivatives_of_every_new_operation_match_finite_differences():
    """central differences in the manner (and with the tolerances) of test_tape_acopf_derivatives_match_finite_differences"""
    M = K.fd_model()
    used = {op for p in M.patterns for op in p.tapes[0].code[:, 0].tolist()}
    assert set(range(T.OP_POW, T.OP_MAX + 1)) <= used
    x, y = K.FD_X, np.array([-1.3])
    h = 1e-6
    E = np.eye(M.n) * h
    Jfd = np.stack([(M.cons(x + e) - M.cons(x - e)) / (2 * h) for e in E], axis=1)
    assert np.abs(_dense_jac(M, x) - Jfd).max() <= 1e-7
    gfd = np.array([(M.obj(x + e) - M.obj(x - e)) / (2 * h) for e in E])
    assert np.abs(gfd - M.grad(x)).max() <= 1e-6

    def lag_grad(z):
        return 0.7 * M.grad(z) + _dense_jac(M, z).T @ y
    Hfd = np.stack([(lag_grad(x + e) - lag_grad(x - e)) / (2 * h) for e in E], axis=1)
    H = _dense_hess(M, x, y, 0.7)
    assert np.abs(H).max() > 0.1
    assert np.abs(H - Hfd).max() <= 1e-6


# ------------------------------------------------------------------------------------------------- 4. closed-form NLPs
@pytest.mark.parametrize("name", list(K.NLPS))
def test_host_ipm_reaches_the_closed_form_optimum_on_the_oracle_back_end(name):
    """tolerance sqrt(tol) = 1e-3: the rule of test_lootsma_reproduces_the_reference_hard_coded_answers"""
    from madnlp_jl_amd.ipm import MadNLPSolver
    from tests.test_ipm_oracle import oracle_factory
    M, xstar = K.NLPS[name]()
    assert M.n == 129
    s = MadNLPSolver(M, oracle_factory("sparse_condensed", M), _options(tol=1e-6), sparse=True)
    status = s.solve()
    err = np.abs(s.x[:M.n] - xstar).max()
    print(name, status, "iterations", s.cnt.k, "error", err)
    assert status == "SOLVE_SUCCEEDED"
    assert err <= 1e-3

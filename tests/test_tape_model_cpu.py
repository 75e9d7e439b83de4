"""The expression-tape NLP evaluator (`madnlp_jl_amd.tape_model`), host half: exact integer answers written out by hand,
the dropped structural zeros, finite differences, the hand-written models (`ACOPFModel`, `HS15Model`, `LootsmaModel`) as
references, the error paths, and host interior-point runs on the oracle back-end.  `tests/test_hip_tape.py` runs the device
interpreter against this one."""
import numpy as np
import pytest
import scipy.sparse as sp

from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.problems import ACOPFModel, HS15Model, LootsmaModel
from madnlp_jl_amd.tape_model import P, V, TapeModel


# ------------------------------------------------------------------------------------------------- 1. exact integers
INT_N, INT_M = 5, 4
_OBJ_A_VI, _OBJ_A_P = [[0, 1], [1, 2], [2, 0]], [2, -3, 5]      # V0*V0*V1 - P0*V1 + 3
_OBJ_B_VI = [[3]]                                                # V0*V0*V0                     (R = 1)
_C1_ROWS, _C1_VI, _C1_P = [0, 1], [[0, 4], [1, 3]], [7, -2]      # V0*V1 + P0
_C2_ROWS, _C2_VI = [0], [[2, 1]]                                 # V0*V0*V0 - V1                (R = 1)
_C3_ROWS, _C3_VI, _C3_P = [0, 3], [[4], [0]], [4, -6]            # P0*V0                        (linear: no Hessian)


def integer_model():
    """Polynomial patterns on small integers: row 0 is fed by three patterns, row 2 by none, variable 4 by no objective
    pattern; two patterns have R = 1."""
    M = TapeModel(INT_N, INT_M, np.zeros(INT_N), -4.0, 4.0, -np.inf, np.inf)
    f64 = lambda a: np.array(a, dtype=float).reshape(-1, 1)  # noqa: E731
    M.add_objective(V(0) * V(0) * V(1) - P(0) * V(1) + 3, np.array(_OBJ_A_VI), f64(_OBJ_A_P))
    M.add_objective(V(0) * V(0) * V(0), np.array(_OBJ_B_VI))
    M.add_constraint(V(0) * V(1) + P(0), np.array(_C1_ROWS), np.array(_C1_VI), f64(_C1_P))
    M.add_constraint(V(0) ** 3 - V(1), np.array(_C2_ROWS), np.array(_C2_VI))
    M.add_constraint(P(0) * V(0), np.array(_C3_ROWS), np.array(_C3_VI), f64(_C3_P))
    return M.finalize()


def integer_reference(x, y, w):
    """f, grad, cons, dense Jacobian and dense lower Lagrangian Hessian in Python integers, from derivatives taken by hand."""
    n, m = INT_N, INT_M
    f, g, c = 0, [0] * n, [0] * m
    J = [[0] * n for _ in range(m)]
    H = [[0] * n for _ in range(n)]

    def h_add(i, j, v):
        H[max(i, j)][min(i, j)] += v
    for (a, b), p in zip(_OBJ_A_VI, _OBJ_A_P):
        f += x[a] * x[a] * x[b] - p * x[b] + 3
        g[a] += 2 * x[a] * x[b]
        g[b] += x[a] * x[a] - p
        h_add(a, a, w * 2 * x[b])
        h_add(a, b, w * 2 * x[a])
    (a,), = _OBJ_B_VI
    f += x[a] ** 3
    g[a] += 3 * x[a] ** 2
    h_add(a, a, w * 6 * x[a])
    for r, (a, b), p in zip(_C1_ROWS, _C1_VI, _C1_P):
        c[r] += x[a] * x[b] + p
        J[r][a] += x[b]
        J[r][b] += x[a]
        h_add(a, b, y[r] * 1)
    for r, (a, b) in zip(_C2_ROWS, _C2_VI):
        c[r] += x[a] ** 3 - x[b]
        J[r][a] += 3 * x[a] ** 2
        J[r][b] += -1
        h_add(a, a, y[r] * 6 * x[a])
    for r, (a,), p in zip(_C3_ROWS, _C3_VI, _C3_P):
        c[r] += p * x[a]
        J[r][a] += p
    return f, g, c, J, H


INT_POINTS = [([3, -2, 4, -1, 2], [2, 0, -3, 5], 3), ([-4, 4, 0, 3, -3], [0, 1, 7, -2], 0), ([1, 1, -1, 0, 4], [-1, 2, 0, 0], 1)]


def summed(vals, I, J, shape):
    A = np.zeros(shape)
    np.add.at(A, (I, J), vals)
    return A


def check_integer_outputs(M, x, y, w, f, g, c, jv, hv):
    rf, rg, rc, rJ, rH = integer_reference(x, y, w)
    assert f == rf
    assert (np.asarray(g) == np.array(rg)).all()
    assert (np.asarray(c) == np.array(rc)).all()
    assert (summed(jv, M.jac_I, M.jac_J, (M.m, M.n)) == np.array(rJ)).all()
    assert (M.hess_I >= M.hess_J).all()
    assert (summed(hv, M.hess_I, M.hess_J, (M.n, M.n)) == np.array(rH)).all()


@pytest.mark.parametrize("x,y,w", INT_POINTS)
def test_integer_patterns_give_the_exact_hand_computed_answers(x, y, w):
    M = integer_model()
    xf, yf = np.array(x, dtype=float), np.array(y, dtype=float)
    check_integer_outputs(M, x, y, w, M.obj(xf), M.grad(xf), M.cons(xf), M.jac_coord(xf), M.hess_coord(xf, yf, float(w)))
    assert M.cons(xf)[2] == 0.0 and M.grad(xf)[4] == 0.0            # the row no pattern feeds, the variable no objective touches
    assert len(M.jac_I) == 2 * 2 + 2 * 1 + 1 * 2 and len(M.hess_I) == 2 * 3 + 1 + 1 * 2 + 1      # pattern-major, output-major, row
    # layout: entry = base[pattern] + o * R + r
    assert M.jac_I[:4].tolist() == [0, 1, 0, 1] and M.jac_J[:4].tolist() == [0, 1, 4, 3]


# ------------------------------------------------------------------------------------------------- 2. structural zeros
def test_structurally_zero_derivatives_are_not_part_of_the_pattern():
    d = V(3) - V(4)
    flow = V(0) - (P(0) * V(1) ** 2 + V(1) * V(2) * (P(1) * T.cos(d) + P(2) * T.sin(d)))
    M = TapeModel(5, 1, np.ones(5), -np.inf, np.inf, 0.0, 0.0)
    M.add_constraint(flow, np.array([0]), np.arange(5)[None, :], np.array([[1.5, -2.0, 0.5]]))
    M.finalize()
    _, d1, d2 = M.patterns[0].tapes
    assert d1.nout == 5 and d1.out_j.tolist() == [0, 1, 2, 3, 4]
    pairs = list(zip(d2.out_j.tolist(), d2.out_l.tolist()))
    assert len(pairs) == 9                                           # not 15: nothing with v0, no (v2, v2)
    assert all(0 not in p for p in pairs) and (2, 2) not in pairs
    assert sorted(pairs) == sorted((j, l) for j in range(1, 5) for l in range(1, j + 1) if (j, l) != (2, 2))
    # common subexpressions are shared across the outputs of a tape: one sine and one cosine for nine second derivatives
    ops = d2.code[:, 0].tolist()
    assert ops.count(T.OP_SIN) == 1 and ops.count(T.OP_COS) == 1
    assert max(t.nslot for t in M.patterns[0].tapes) <= T.SLOT_MAX


# ------------------------------------------------------------------------------------------------- 3. finite differences
def _dense_jac(M, x):
    return sp.csr_matrix((M.jac_coord(x), (M.jac_I, M.jac_J)), shape=(M.m, M.n)).toarray()


def _lower_hess(M, x, y, w):
    I, J = np.maximum(M.hess_I, M.hess_J), np.minimum(M.hess_I, M.hess_J)
    return sp.csr_matrix((M.hess_coord(x, y, w), (I, J)), shape=(M.n, M.n)).toarray()


def _dense_hess(M, x, y, w):
    L = _lower_hess(M, x, y, w)
    return L + np.tril(L, -1).T


@pytest.fixture(scope="module")
def tape_opf():
    return {case: T.acopf_tape_model(case) for case in ("case30", "case118")}


def test_tape_acopf_derivatives_match_finite_differences(tape_opf):
    M = tape_opf["case30"]
    rng = np.random.default_rng(0)
    x = M.x0 + 0.05 * rng.standard_normal(M.n)
    y = rng.standard_normal(M.m)
    h = 1e-6
    E = np.eye(M.n) * h
    Jfd = np.stack([(M.cons(x + e) - M.cons(x - e)) / (2 * h) for e in E], axis=1)
    assert np.abs(_dense_jac(M, x) - Jfd).max() <= 1e-7
    gfd = np.array([(M.obj(x + e) - M.obj(x - e)) / (2 * h) for e in E])
    assert np.abs(gfd - M.grad(x)).max() <= 1e-6

    def lag_grad(z):
        return 0.7 * M.grad(z) + _dense_jac(M, z).T @ y
    Hfd = np.stack([(lag_grad(x + e) - lag_grad(x - e)) / (2 * h) for e in E], axis=1)
    assert np.abs(_dense_hess(M, x, y, 0.7) - Hfd).max() <= 1e-6


# ------------------------------------------------------------------------------------------------- 4. hand-written models
def acopf_points(nlp):
    """the points, multipliers and objective weights of test_acopf.test_device_callbacks_match_the_host_model"""
    rng = np.random.default_rng(5)
    for trial in range(3):
        x = nlp.x0 + (0.0 if trial == 0 else 0.1) * rng.standard_normal(nlp.n)
        yield x, rng.standard_normal(nlp.m), [1.0, 0.0, 0.37][trial]


def assert_models_agree(M, A, x, y, w):
    fa = A.obj(x)
    assert abs(M.obj(x) - fa) <= 1e-13 * abs(fa)
    for got, ref in ((M.cons(x), A.cons(x)), (M.grad(x), A.grad(x))):
        assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    Jm, Ja = _dense_jac(M, x), _dense_jac(A, x)
    assert np.abs(Jm - Ja).max() <= 1e-13 * np.abs(A.jac_coord(x)).max()
    Hm, Ha = _lower_hess(M, x, y, w), _lower_hess(A, x, y, w)
    assert np.abs(Hm - Ha).max() <= 1e-13 * np.abs(A.hess_coord(x, y, w)).max()


@pytest.mark.parametrize("case", ["case30", "case118"])
def test_tape_acopf_matches_the_hand_written_model(tape_opf, case):
    M, A = tape_opf[case], ACOPFModel(case)
    assert (M.n, M.m) == (A.n, A.m)
    for f in ("x0", "lvar", "uvar", "lcon", "ucon"):
        assert np.array_equal(getattr(M, f), getattr(A, f))
    assert len(M.jac_I) == len(A.jac_I)                          # no structural zero in the hand-written Jacobian
    # its Hessian stores one explicit 0 per flow row; the two balance patterns of a bus each bring their own vm^2 entry
    assert len(M.hess_I) == len(A.hess_I) - 2 * A.narc + A.nbus
    for x, y, w in acopf_points(A):
        assert_models_agree(M, A, x, y, w)


@pytest.mark.parametrize("make,ref", [(T.hs15_tape_model, HS15Model), (T.lootsma_tape_model, LootsmaModel)])
def test_small_tape_models_match_the_hand_written_ones(make, ref):
    M, A = make(), ref()
    rng = np.random.default_rng(3)
    for w in (1.0, 0.0, 0.37):
        x = rng.uniform(0.3, 2.0, M.n)                           # (sqrt and its derivatives: positive points)
        assert_models_agree(M, A, x, rng.standard_normal(M.m), w)


# ------------------------------------------------------------------------------------------------- 5. error paths
def test_errors_are_reported_when_a_pattern_is_added():
    M = TapeModel(4, 2, np.zeros(4), -1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="names the same variable twice"):
        M.add_constraint(V(0) * V(1), np.array([0, 1]), np.array([[0, 1], [2, 2]]))
    with pytest.raises(ValueError, match=r"var_index\[1, 0\] = 4 is out of range"):
        M.add_objective(V(0), np.array([[0], [4]]))
    with pytest.raises(ValueError, match=r"rows\[0\] = 2 is out of range"):
        M.add_constraint(V(0), np.array([2]), np.array([[0]]))
    with pytest.raises(ValueError, match=r"uses V\(1\) but var_index has 1 columns"):
        M.add_objective(V(0) * V(1), np.array([[0]]))
    with pytest.raises(ValueError, match=r"uses P\(0\) but params has 0 columns"):
        M.add_objective(V(0) * P(0), np.array([[0]]))
    assert M.patterns == []


def slot_hungry_expr(nterms):
    """t_0 + (t_1 + (t_2 + ...)) with distinct products t_i: all of them are alive before the first sum is taken, so the value
    tape needs exactly `nterms` slots."""
    t = [V(0) * float(i + 2) for i in range(nterms)]
    e = t[-1]
    for ti in t[-2::-1]:
        e = ti + e
    return e


def test_a_tape_over_slot_max_is_refused_at_finalize():
    M = TapeModel(1, 1, np.zeros(1), -1.0, 1.0, 0.0, 0.0)
    M.add_constraint(slot_hungry_expr(T.SLOT_MAX), np.array([0]), np.array([[0]]))
    M.finalize()
    assert M.patterns[0].tapes[0].nslot == T.SLOT_MAX
    assert M.cons(np.array([1.0]))[0] == sum(range(2, T.SLOT_MAX + 2))
    M = TapeModel(1, 1, np.zeros(1), -1.0, 1.0, 0.0, 0.0)
    M.add_constraint(slot_hungry_expr(T.SLOT_MAX + 1), np.array([0]), np.array([[0]]))
    with pytest.raises(ValueError, match=f"needs {T.SLOT_MAX + 1} slots, SLOT_MAX is {T.SLOT_MAX}"):
        M.finalize()


# ------------------------------------------------------------------------------------------------- 6. host IPM, oracle back-end
def _options(tol=1e-6):            # test_acopf._options
    from madnlp_jl_amd.ipm import IPMOptions
    o = IPMOptions(tol=tol)
    o.relax_equality, o.dual_initialization = True, "zero"
    return o


@pytest.mark.parametrize("case,iters", [("case30", 10), ("case118", 13)])
def test_host_ipm_solves_the_tape_acopf_on_the_oracle_back_end(tape_opf, case, iters):
    from madnlp_jl_amd.ipm import MadNLPSolver
    from tests.test_ipm_oracle import oracle_factory
    M, A = tape_opf[case], ACOPFModel(case)
    s = MadNLPSolver(M, oracle_factory("sparse_condensed", M), _options(), sparse=True)
    assert s.solve() == "SOLVE_SUCCEEDED"
    ref = MadNLPSolver(A, oracle_factory("sparse_condensed", A), _options(), sparse=True)
    assert ref.solve() == "SOLVE_SUCCEEDED"
    print(case, "tape iterations", s.cnt.k, "hand-written", ref.cnt.k)
    assert s.cnt.k == iters                   # regression value of the tape model's own trajectory (hand-written model: 10 / 13)
    x = s.x[:A.n]
    c = A.cons(x)                             # feasibility judged by the hand-written model
    assert (c >= A.lcon - 1e-5).all() and (c <= A.ucon + 1e-5).all()
    assert (x >= A.lvar - 1e-7).all() and (x <= A.uvar + 1e-7).all()
    assert abs(s.obj_val - ref.obj_val) <= 1e-6 * abs(ref.obj_val)


def test_host_ipm_solves_the_tape_hs15_like_the_hand_written_model():
    from tests.test_ipm_oracle import run
    a, b = run("sparse_condensed", T.hs15_tape_model(), tol=1e-6), run("sparse_condensed", HS15Model(), tol=1e-6)
    assert a.status == b.status == "SOLVE_SUCCEEDED"
    assert a.cnt.k == b.cnt.k
    np.testing.assert_allclose(a.x[:2], b.x[:2], rtol=0, atol=1e-8)
    assert abs(a.obj_val - b.obj_val) <= 1e-8 * abs(b.obj_val)


def test_expressions_are_interned_weakly_and_constant_folding_leaves_overflow_to_run_time():
    import gc
    assert V(0) * P(1) + 2.0 is V(0) * P(1) + 2.0                 # (held by the comparison: the same node)
    e = T.exp(T.const(1000.0))                                     # math.exp overflows: not folded, inf at run time
    assert e.op == T.OP_EXP
    del e
    gc.collect()
    before = len(T.Expr._pool)
    M = T.hs15_tape_model()
    assert len(T.Expr._pool) > before
    del M
    gc.collect()
    assert len(T.Expr._pool) <= before                             # a model's nodes and derivatives go with the model

"""Model builders shared by tests/test_tape_ops_cpu.py and tests/test_hip_tape_ops.py: the tape vocabulary beyond
+ - * / and sin cos exp log sqrt -- real powers, tan atan tanh, abs_ sign step minimum maximum."""
import hashlib

import numpy as np

from madnlp_jl_amd import tape_model as T
from madnlp_jl_amd.tape_model import P, V, TapeModel

BS = 128          # rows per workgroup of the interpreter kernel (TAPE_BS in csrc/tape_eval.hip)
NLP_N = 129       # the three closed-form NLPs: one full workgroup and one row


def code_digest(M):
    """sha256 over the `code` arrays of a model's tapes (pattern order, value | first | second), little-endian int32"""
    h = hashlib.sha256()
    for p in M.patterns:
        for t in p.tapes:
            h.update(np.ascontiguousarray(t.code, dtype="<i4").tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------- exact values
# (a, b) per row: signed zeros on both sides, a tie, b below a, b above a
SEL_A = [0.0, -0.0, 2.0, 1.5, -3.0]
SEL_B = [-0.0, 0.0, 2.0, -2.5, 4.0]


def selection_model():
    """One constraint pattern per selection operation on the rows (SEL_A[r], SEL_B[r]) = (x[r], x[5 + r]); pattern p feeds
    rows 5 p .. 5 p + 4."""
    R = len(SEL_A)
    M = TapeModel(2 * R, 5 * R, np.zeros(2 * R), -10.0, 10.0, -np.inf, np.inf)
    vi = np.stack([np.arange(R), R + np.arange(R)], axis=1)
    for i, e in enumerate((T.abs_(V(0)), T.sign(V(0)), T.step(V(0)), T.minimum(V(0), V(1)), T.maximum(V(0), V(1)))):
        M.add_constraint(e, i * R + np.arange(R), vi)
    return M.finalize()


def fd_expr():
    """every new operation in one three-variable expression, away from every kink at x = FD_X"""
    return (T.pow_(V(0), V(1)) + T.minimum(V(0) * V(1), V(2)) * T.tan(V(2)) + T.abs_(V(0) - V(2)) ** 1.7
            + T.tanh(V(1)) * T.atan(V(0)) + T.maximum(V(1), V(2)) * V(0) * T.step(V(0)) + T.sign(V(1)) * V(2) * V(2))


FD_X = np.array([1.3, 0.7, 0.4])


def fd_model():
    M = TapeModel(3, 1, FD_X, -np.inf, np.inf, -np.inf, np.inf)
    M.add_objective(fd_expr(), np.array([[0, 1, 2]]))
    M.add_constraint(fd_expr(), np.array([0]), np.array([[2, 0, 1]]))
    return M.finalize()


# ------------------------------------------------------------------------------------------------- closed-form NLPs
def nlp_data(n=NLP_N):
    """t, b, u, a drawn in this order from one generator"""
    rng = np.random.default_rng(3)
    t = rng.uniform(-1.0, 3.0, n)
    t[::10] = 1.0                         # exactly on the kink of the hinge
    b, u = rng.uniform(0.5, 3.0, n), rng.uniform(0.5, 3.0, n)
    a = rng.uniform(-0.8, 0.8, n)
    return t, b, u, a


def hinge_model(n=NLP_N):
    """A: min sum maximum(x_i - 1, 0)^2 + (x_i - t_i)^2, |x| <= 10, x_i + x_{i+1} <= 50 (inactive).
    Optimum t_i where t_i <= 1, else (t_i + 1) / 2.  Selection operations and + - * / only."""
    t = nlp_data(n)[0]
    M = TapeModel(n, n - 1, np.zeros(n), -10.0, 10.0, -np.inf, 50.0, name="hinge")
    own = np.arange(n)[:, None]
    M.add_objective(T.maximum(V(0) - 1.0, 0.0) ** 2 + (V(0) - P(0)) ** 2, own, t[:, None])
    M.add_constraint(V(0) + V(1), np.arange(n - 1), np.stack([np.arange(n - 1), np.arange(1, n)], axis=1))
    return M.finalize(), np.where(t <= 1.0, t, (t + 1.0) / 2.0)


def power_model(n=NLP_N):
    """B: min sum x_i^2.7 / 2.7 - b_i x_i, x_i^1.7 <= u_i, x >= 1e-3, x0 = 1.  Optimum min(b_i, u_i)^(1 / 1.7)."""
    _, b, u, _ = nlp_data(n)
    M = TapeModel(n, n, np.ones(n), 1e-3, np.inf, -np.inf, u, name="powers")
    own = np.arange(n)[:, None]
    M.add_objective(V(0) ** 2.7 / 2.7 - P(0) * V(0), own, b[:, None])
    M.add_constraint(V(0) ** 1.7, np.arange(n), own)
    return M.finalize(), np.minimum(b, u) ** (1.0 / 1.7)


def tanh_model(n=NLP_N):
    """C: min sum (tanh(x_i) - a_i)^2, atan(x_i) + 0.1 |x_i + 3| + tan(0.1 x_i) <= 2 (inactive), |x| <= 5.
    Optimum atanh(a_i)."""
    a = nlp_data(n)[3]
    M = TapeModel(n, n, np.zeros(n), -5.0, 5.0, -np.inf, 2.0, name="tanh")
    own = np.arange(n)[:, None]
    M.add_objective((T.tanh(V(0)) - P(0)) ** 2, own, a[:, None])
    M.add_constraint(T.atan(V(0)) + 0.1 * T.abs_(V(0) + 3.0) + T.tan(0.1 * V(0)), np.arange(n), own)
    return M.finalize(), np.arctanh(a)


NLPS = {"hinge": hinge_model, "powers": power_model, "tanh": tanh_model}


# ------------------------------------------------------------------------------------------------- device vs host
SEL_PATTERNS, EXT_PATTERNS, ARITH_PATTERNS = (0, 1, 2), (3, 4, 5), (6, 7)


def ops_edge_model():
    """Patterns at the interpreter's edges in ONE launch per callback: R = 1, BS, BS + 1, 3 BS - 1 rows, k = 1 .. 5.
      0 .. 2  (a) selection operations and + - * / only; the parameters of 0 and 2 place exact ties (P == V is not possible
                  without knowing x, so ties are between two parameter columns and between a parameter and a constant) and zeros
      3 .. 5  (b) pow with the constant exponents 1.7 and -0.3 and with a variable exponent, tan(0.5 V), atan, tanh
      6 .. 7  (c) + - * / patterns that existed before
    Constraint rows 0 .. BS - 1 are fed by patterns 3 and 6 together (extended, arithmetic), rows 250 .. 277 by patterns 0 and 4
    (selection, extended), rows 150 .. 249 by the selection pattern 0 alone; the objective has a pattern of each kind."""
    n, m = 600, 700
    rng = np.random.default_rng(33)
    M = TapeModel(n, m, np.ones(n), 0.0, 2.0, -np.inf, np.inf)
    distinct = lambda R, k, lo, hi: np.stack([rng.choice(np.arange(lo, hi), k, replace=False) for _ in range(R)])  # noqa: E731
    par = rng.uniform(0.5, 1.5, (BS, 3))
    par[::4, 1] = par[::4, 0]             # ties between two parameters
    par[1::4, 2] = 0.0                    # zeros, of both signs
    par[2::8, 2] = -0.0
    M.add_constraint(T.minimum(P(0), P(1)) * V(0) + T.maximum(P(1), P(0)) * V(1) - T.abs_(V(2) - V(3)) * T.sign(P(2))
                     + T.step(P(2)) * T.maximum(V(4) * V(0), P(2)) + T.minimum(V(1) - 1.0, 0.0) * T.minimum(V(1) - 1.0, 0.0),
                     150 + np.arange(BS), distinct(BS, 5, 0, n), par)                                             # 0: R = BS, k = 5
    M.add_objective(T.maximum(V(0) - 1.0, 0.0) ** 2 + T.abs_(V(0) - P(0)) * V(0), distinct(3 * BS - 1, 1, 0, 400),
                    rng.uniform(0.5, 1.5, (3 * BS - 1, 1)))                                                       # 1: R = 3 BS - 1
    M.add_constraint(T.minimum(V(0) * V(1), P(0)) / T.maximum(V(1), 1.0) + T.sign(V(0) - 1.0) * V(1) * V(1) + T.step(P(0) - 1.0) * V(0),
                     np.array([130]), np.array([[7, 9]]), np.array([[1.0]]))                                      # 2: R = 1 (tie P0 == 1)
    M.add_constraint(V(0) ** 1.7 + V(1) ** -0.3 * V(2) + T.pow_(V(0), V(3)), np.arange(BS + 1), distinct(BS + 1, 4, 0, n))   # 3: R = BS + 1
    M.add_constraint(T.tan(0.5 * V(0)) * T.atan(V(1)) + T.tanh(V(2)) * P(0), 250 + np.arange(3 * BS - 1),
                     distinct(3 * BS - 1, 3, 0, n), rng.standard_normal((3 * BS - 1, 1)))                         # 4: R = 3 BS - 1
    M.add_objective(T.tanh(V(0)) * V(1) ** 2.5 + T.atan(V(0) * V(1)), distinct(BS, 2, 0, 400))                    # 5: R = BS, k = 2
    M.add_constraint(V(0) * V(1) - V(2) / (V(1) * V(1) + 1.0) + P(0) * V(0), np.arange(BS), distinct(BS, 3, 0, n),
                     rng.standard_normal((BS, 1)))                                                                # 6: rows 0 .. BS - 1
    M.add_objective(P(0) * V(0) * V(1) - V(1) / (V(0) * V(0) + 2.0), distinct(BS + 1, 2, 0, 400), rng.standard_normal((BS + 1, 1)))  # 7
    return M.finalize()


def ops_edge_masks(M):
    """which Jacobian / Hessian COO entries, constraint rows, objective terms and gradient entries no extended pattern feeds"""
    jm, hm, tm = [], [], []
    rows_x, vars_x = np.zeros(M.m, dtype=bool), np.zeros(M.n, dtype=bool)
    for i, p in enumerate(M.patterns):
        ex = i not in EXT_PATTERNS
        if p.kind == 1:
            jm.append(np.full(p.R * p.tapes[1].nout, ex))
            if not ex:
                rows_x[p.rows] = True
        else:
            tm.append(np.full(p.R, ex))
            if not ex:
                vars_x[p.var_index.ravel()] = True
        hm.append(np.full(p.R * p.tapes[2].nout, ex))
    return np.concatenate(jm), np.concatenate(hm), ~rows_x, np.concatenate(tm), ~vars_x


def tanh_in_one_constraint_model():
    """the only opcode from 16 on is tanh in ONE constraint pattern: the cons, jac and hess launches are extended, obj and grad not"""
    M = TapeModel(4, 2, np.ones(4), -2.0, 2.0, -np.inf, 1.0)
    M.add_objective(V(0) * V(0) * V(0) - T.sin(V(0)), np.arange(4)[:, None])
    M.add_constraint(V(0) * V(1), np.array([0]), np.array([[0, 1]]))
    M.add_constraint(T.tanh(V(0)) + V(1), np.array([0, 1]), np.array([[2, 3], [1, 0]]))
    return M.finalize()

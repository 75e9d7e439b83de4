"""An independent reference for the expression-tape evaluator (`madnlp_jl_amd.tape_model`, csrc/tape_eval.hip); a helper module,
no tests in it.  tests/test_tape_reference_cpu.py and tests/test_hip_tape_reference.py use it.

  trees        nested tuples -- ("mul", ("var", 0), ("sin", ("par", 1))) -- drawn by `random_tree`; `to_expr` builds the project's
               expression through the public front end, `evaluate` computes the tree in mpmath from the mathematical definitions
               (the documented comparison rules for the selection operations) and calls nothing in `tape_model`
  derivatives  `mpmath.diff` on `evaluate`: no differentiation rule is shared with the code under test
  guard        `evaluate(..., guard=True)` raises `Reject` at a point where a node is near a kink or a domain edge
  bound        `run_tape` interprets a COMPILED tape (the documented format: (op, dst, a, b), operand = kind << 24 | index) in
               mpmath and carries, next to every slot, a first-order bound on the float64 error of that slot.  The value a test
               compares with comes from `evaluate` / `mpmath.diff`, never from the tape (the edge-argument test, where no tree
               exists, compares with the tape's own 60-digit value).
A slot of `run_tape` is (value, sign of a zero, bound from the folded constants alone, full float64 bound): mpmath has no
signed zero, so the sign of an exact zero follows the IEEE rules by hand, and every value is brought into float64's range after
every instruction (overflow to +-Inf, underflow to a signed zero, a domain error to NaN)."""
import math
import random

import numpy as np
from mpmath import mp, mpf

from madnlp_jl_amd import tape_model as T

mp.dps = 60

# The two measured constants of the bound (tools/tape_ulp_survey.py -> profiles/tape_accuracy.json; the unit is 2^-52 |value|
# for a function, 2^-53 |constant| for a folded constant):
C_FUN = 2        # profiles/tape_accuracy.json "c_fun": twice the largest error of a library function on either side, rounded up
C_CONST = 3      # profiles/tape_accuracy.json "c_const": twice the largest error ratio of the folded constants, rounded up

U = mpf(2) ** -52
DIFF_NOISE = mpf(10) ** -30          # what mpmath.diff leaves of a derivative that is exactly zero
X_RANGE, P_RANGE = (0.3, 1.7), (0.5, 1.5)
REAL_POWERS = (1.7, -0.3, 2.5, 0.5, 3.0, -2.0)
TREE_CONSTS = (2.0, 0.5, 1.5, -1.0, 3.0, 0.7, 1.3, -0.4, 2.5)
UNARY = ("neg", "sin", "cos", "exp", "log", "sqrt", "tan", "atan", "tanh", "abs", "sign", "step")


class Reject(Exception):
    """the point is near a kink or a domain edge of some node of the tree"""


# ------------------------------------------------------------------------------------------------- (a) trees
def random_tree(rng, depth, k, q):
    """A tree over the whole vocabulary; `rng` is a `random.Random`."""
    if depth == 0 or rng.random() < 0.12:
        u = rng.random()
        if u < 0.62 or (q == 0 and u < 0.85):
            return ("var", rng.randrange(k))
        if u < 0.85:
            return ("par", rng.randrange(q))
        return ("const", rng.choice(TREE_CONSTS))
    u = rng.random()
    if u < 0.40:
        return (rng.choice(("add", "sub", "mul", "mul", "div")), random_tree(rng, depth - 1, k, q), random_tree(rng, depth - 1, k, q))
    if u < 0.70:
        return (rng.choice(UNARY), random_tree(rng, depth - 1, k, q))
    if u < 0.82:
        return (rng.choice(("min", "max")), random_tree(rng, depth - 1, k, q), random_tree(rng, depth - 1, k, q))
    if u < 0.94:
        return ("powc", random_tree(rng, depth - 1, k, q), rng.choice(REAL_POWERS))
    return ("pow", random_tree(rng, depth - 1, k, q), random_tree(rng, depth - 1, k, q))


def wide_tree(rng, k, q):
    """A tree that couples all k = 8 local variables: a full binary tree of depth 3 over the variables in random order (every
    other one scaled by a parameter) under one function, so that Hessians with all 36 pairs reach the checks (a Hessian tape
    with 36 outputs fits SLOT_MAX only where outputs share nodes: most draws are refused at finalize())."""
    level = [("var", j) for j in rng.sample(range(k), k)]
    level = [("mul", ("par", rng.randrange(q)), v) if rng.random() < 0.5 else v for v in level]
    while len(level) > 1:
        level = [(rng.choice(("add", "add", "sub", "mul", "div", "min", "max")), a, b) for a, b in zip(level[::2], level[1::2])]
    u = rng.choice(("sin", "cos", "exp", "log", "sqrt", "tan", "atan", "tanh", "powc"))
    return ("powc", level[0], rng.choice(REAL_POWERS)) if u == "powc" else (u, level[0])


_FRONT = {"sin": T.sin, "cos": T.cos, "exp": T.exp, "log": T.log, "sqrt": T.sqrt, "tan": T.tan, "atan": T.atan, "tanh": T.tanh,
          "abs": T.abs_, "sign": T.sign, "step": T.step}


def to_expr(tree):
    """the project's `Expr` of a tree, through the public front end only"""
    op = tree[0]
    if op == "var":
        return T.V(tree[1])
    if op == "par":
        return T.P(tree[1])
    if op == "const":
        return T.const(tree[1])
    a = to_expr(tree[1])
    if op == "neg":
        return -a
    if op in _FRONT:
        return _FRONT[op](a)
    if op == "powc":
        return a ** tree[2]
    b = to_expr(tree[2])
    return {"add": lambda: a + b, "sub": lambda: a - b, "mul": lambda: a * b, "div": lambda: a / b, "min": lambda: T.minimum(a, b),
            "max": lambda: T.maximum(a, b), "pow": lambda: T.pow_(a, b)}[op]()


def evaluate(tree, x, p, guard=False):
    """The tree's value in mpmath at the current precision, from the definitions.  With `guard`, `Reject` where a node is within
    the thresholds of a kink or a domain edge."""
    def need(ok):
        if guard and not ok:
            raise Reject

    def ev(t):
        op = t[0]
        if op == "var":
            return +x[t[1]]
        if op == "par":
            return +p[t[1]]
        if op == "const":
            return mpf(t[1])
        a = ev(t[1])
        if op == "neg":
            return -a
        if op == "sin":
            return mp.sin(a)
        if op == "cos":
            return mp.cos(a)
        if op == "exp":
            need(abs(a) <= 20)
            return mp.exp(a)
        if op == "log":
            need(a > 0.05)
            return mp.log(a)
        if op == "sqrt":
            need(a > 0.05)
            return mp.sqrt(a)
        if op == "tan":
            need(abs(mp.cos(a)) >= 0.05)
            return mp.sin(a) / mp.cos(a)
        if op == "atan":
            return mp.atan(a)
        if op == "tanh":
            return mp.tanh(a)
        if op in ("abs", "sign", "step"):
            need(abs(a) >= 1e-3)
            return abs(a) if op == "abs" else mpf(1 if a > 0 else -1 if a < 0 else 0) if op == "sign" else mpf(1 if a >= 0 else 0)
        if op == "powc":
            c = t[2]
            if c == math.floor(c):                       # an integer power is a product (and holds for any base but 0 ** -k)
                need(c > 0 or abs(a) >= 0.05)
                return a ** int(c)
            need(a > 0.05)
            return mp.exp(mpf(c) * mp.log(a))
        b = ev(t[2])
        if op == "add":
            return a + b
        if op == "sub":
            return a - b
        if op == "mul":
            return a * b
        if op == "div":
            need(abs(b) >= 0.05)
            return a / b
        if op in ("min", "max"):
            need(abs(a - b) >= 1e-3)
            return b if (b < a if op == "min" else b > a) else a
        assert op == "pow", op
        need(a > 0.05)
        need(abs(b * mp.log(a)) <= 20)
        return mp.exp(b * mp.log(a))

    return ev(tree)


# ------------------------------------------------------------------------------------------------- (b) reference derivatives
def derivative(tree, x, p, orders):
    """the partial derivative of the orders `orders` (one per local variable) by mpmath.diff on `evaluate`"""
    x = [mpf(v) for v in x]
    p = [mpf(v) for v in p]
    if not any(orders):
        return evaluate(tree, x, p)
    return mp.diff(lambda *xs: evaluate(tree, xs, p), tuple(x), tuple(orders))


def orders_of(k, j, l=None):
    o = [0] * k
    o[j] += 1
    if l is not None:
        o[l] += 1
    return o


# ------------------------------------------------------------------------------------------------- (d) the bound
def _is_inf(v):
    return mp.isinf(v)


def ieee_range(v, neg):
    """(value, sign of zero) with the value brought into float64's range"""
    if mp.isnan(v) or mp.isinf(v):
        return v, False
    if v == 0:
        return v, neg
    if abs(v) >= mpf(2) ** 1024 * (1 - mpf(2) ** -54):
        return (mp.inf if v > 0 else -mp.inf), False
    if abs(v) <= mpf(2) ** -1075:
        return mpf(0), bool(v < 0)
    return v, False


def _sb(v, neg):
    """the sign bit of a slot"""
    return neg if v == 0 else bool(v < 0)


def _pe(partial, e):
    """partial * e, where an operand without error contributes nothing (its partial may be infinite)"""
    return mpf(0) if e == 0 else abs(partial) * e


def _odd_integer(b):
    return mp.isint(b) and int(b) % 2 == 1


def _op(op, a, b):
    """(value, sign of zero, partial wrt a, partial wrt b, c_op) of one instruction on the slots a, b = (value, sign of zero);
    a partial of None stands for a selection that passes operand errors through (handled by the caller)."""
    (av, an), (bv, bn) = a, b
    nan = mp.nan
    if mp.isnan(av) or (mp.isnan(bv) and op in (T.OP_ADD, T.OP_SUB, T.OP_MUL, T.OP_DIV)):
        if op in (T.OP_SIGN, T.OP_STEP):
            return mpf(0), False, 0, 0, 0
        if op == T.OP_POW and bv == 0:
            return mpf(1), False, 0, 0, 0
        return nan, False, 0, 0, 0
    if op in (T.OP_ADD, T.OP_SUB):
        if op == T.OP_SUB:
            bv, bn = -bv, not _sb(bv, bn) if bv == 0 else False
        v = av + bv
        neg = (an and bn) if (av == 0 and bv == 0) else False
        return v, neg, 1, 1, 0.5
    if op == T.OP_MUL:
        if (av == 0 and _is_inf(bv)) or (bv == 0 and _is_inf(av)):
            return nan, False, 0, 0, 0
        return av * bv, _sb(av, an) != _sb(bv, bn), bv, av, 0.5
    if op == T.OP_DIV:
        s = _sb(av, an) != _sb(bv, bn)
        if bv == 0:
            return (nan if av == 0 else -mp.inf if s else mp.inf), False, 0, 0, 0
        if _is_inf(bv):
            return (nan if _is_inf(av) else mpf(0)), s, 0, 0, 0
        return av / bv, s, 1 / bv, av / (bv * bv), 0.5
    if op == T.OP_NEG:
        return -av, not an, 1, 0, 0
    if op == T.OP_SIN:
        return (nan if _is_inf(av) else mp.sin(av)), an, (0 if _is_inf(av) else mp.cos(av)), 0, C_FUN
    if op == T.OP_COS:
        return (nan if _is_inf(av) else mp.cos(av)), False, (0 if _is_inf(av) else mp.sin(av)), 0, C_FUN
    if op == T.OP_EXP:
        v = mp.exp(av)
        return v, False, (0 if _is_inf(av) else v), 0, C_FUN
    if op == T.OP_LOG:
        if av < 0:
            return nan, False, 0, 0, 0
        if av == 0:
            return -mp.inf, False, 0, 0, 0
        return mp.log(av), False, (0 if _is_inf(av) else 1 / av), 0, C_FUN
    if op == T.OP_SQRT:
        if av < 0:
            return nan, False, 0, 0, 0
        v = mp.sqrt(av)
        return v, an, (0 if av == 0 or _is_inf(av) else 1 / (2 * v)), 0, 0.5
    if op == T.OP_TAN:
        if _is_inf(av):
            return nan, False, 0, 0, 0
        v = mp.sin(av) / mp.cos(av)
        return v, an, 1 + v * v, 0, C_FUN
    if op == T.OP_ATAN:
        return mp.atan(av), an, (0 if _is_inf(av) else 1 / (1 + av * av)), 0, C_FUN
    if op == T.OP_TANH:
        v = mp.tanh(av)
        return v, an, (0 if _is_inf(av) else 1 - v * v), 0, C_FUN
    if op == T.OP_ABS:
        return abs(av), False, 1, 0, 0
    if op == T.OP_SIGN:
        return mpf(1 if av > 0 else -1 if av < 0 else 0), False, None, 0, 0
    if op == T.OP_STEP:
        return mpf(1 if av >= 0 else 0), False, None, 0, 0
    if op in (T.OP_MIN, T.OP_MAX):
        take_b = (bv < av) if op == T.OP_MIN else (bv > av)
        return (bv, bn, None, None, 0) if take_b else (av, an, None, None, 0)
    assert op == T.OP_POW, op
    return _pow(av, an, bv)


def _pow(av, an, bv):
    """IEEE pow on (value, sign of zero) ** value"""
    nan, inf = mp.nan, mp.inf
    if bv == 0 or av == 1:
        return mpf(1), False, 0, 0, 0
    if mp.isnan(bv):
        return nan, False, 0, 0, 0
    odd = (not _is_inf(bv)) and _odd_integer(bv)
    if av == 0:
        s = an and odd
        return (mpf(0), s, 0, 0, 0) if bv > 0 else ((-inf if s else inf), False, 0, 0, 0)
    if _is_inf(bv):
        if av == -1:
            return mpf(1), False, 0, 0, 0
        big = abs(av) > 1
        return (inf if big == (bv > 0) else mpf(0)), False, 0, 0, 0
    if _is_inf(av):
        if av > 0:
            return (inf if bv > 0 else mpf(0)), False, 0, 0, 0
        return ((-inf if odd else inf), False, 0, 0, 0) if bv > 0 else (mpf(0), odd, 0, 0, 0)
    if av < 0:
        if not mp.isint(bv):
            return nan, False, 0, 0, 0
        v = mp.exp(bv * mp.log(-av))
        v = -v if odd else v
        return v, bool(v < 0), bv * v / av, mp.inf, C_FUN          # (the exponent's own error would leave the integers)
    v = mp.exp(bv * mp.log(av))
    return v, False, bv * v / av, v * mp.log(av), C_FUN


def run_tape(tape, x, p, weight=None):
    """The compiled `tape` at the local variables `x` and parameters `p` (floats): per output (value, sign of zero, bound from
    the folded constants alone, full float64 bound), all mpmath but the sign.  `weight`: the multiplier a Hessian output is
    stored with (one more rounding)."""
    tiny = mpf(2) ** -1075

    def load(f):
        f = float(f)
        if math.isnan(f) or math.isinf(f):
            return (mp.nan if math.isnan(f) else mpf(f)), False, mpf(0), mpf(0)
        return mpf(f), (f == 0.0 and math.copysign(1.0, f) < 0), mpf(0), mpf(0)

    def rounding(c_op, v):
        """of the exact result `v` (before it is brought into range): relative, or half the smallest subnormal"""
        if not c_op or mp.isnan(v) or _is_inf(v) or v == 0:
            return mpf(0)
        return c_op * U * abs(v) + (max(1, 2 * c_op) * tiny if abs(v) < mpf(2) ** -1021 else 0)

    slots = [None] * tape.nslot

    def get(o):
        kind, idx = o >> 24, o & 0xFFFFFF
        if kind == T.KIND_SLOT:
            return slots[idx]
        if kind != T.KIND_CONST:
            return load(x[idx] if kind == T.KIND_VAR else p[idx])
        c = float(tape.consts[idx])
        v, neg, _, _ = load(c)
        e = mpf(0) if (math.isinf(c) or math.isnan(c) or c == math.floor(c)) else C_CONST * (U / 2) * abs(v)
        return v, neg, e, e

    def step(op, a, b):
        exact, neg, da, db, c_op = _op(op, a[:2], b[:2])
        v, neg = ieee_range(exact, neg)
        if da is None:                                    # a selection: the error of what it selected, unless the choice is in doubt
            if op in (T.OP_SIGN, T.OP_STEP):
                doubt = a[3] > 0 and a[3] >= abs(a[0])
                ec = ef = mp.inf if doubt else mpf(0)
            else:
                doubt = (a[3] + b[3]) > 0 and (a[3] + b[3]) >= abs(a[0] - b[0])
                pick = b if ((b[0] < a[0]) if op == T.OP_MIN else (b[0] > a[0])) else a
                ec, ef = (mp.inf, mp.inf) if doubt else (pick[2], pick[3])
            return v, neg, ec, ef
        ec = _pe(da, a[2]) + _pe(db, b[2])
        ef = _pe(da, a[3]) + _pe(db, b[3]) + rounding(c_op, exact)
        return v, neg, ec, ef

    for op, dst, a, b in tape.code.tolist():
        slots[dst] = step(op, get(a), get(b))
    outs = [get(o) for o in tape.out_operand.tolist()]
    if weight is not None:
        outs = [step(T.OP_MUL, load(weight), o) for o in outs]
    return outs


def classify(v, neg=False):
    """"nan", "+inf", "-inf", "+0", "-0" or "finite" of a float or of an (mpmath value, sign of zero) of `run_tape`"""
    if isinstance(v, (float, np.floating)):
        v = float(v)
        if math.isnan(v):
            return "nan"
        if math.isinf(v):
            return "+inf" if v > 0 else "-inf"
        if v == 0.0:
            return "-0" if math.copysign(1.0, v) < 0 else "+0"
        return "finite"
    if mp.isnan(v):
        return "nan"
    if mp.isinf(v):
        return "+inf" if v > 0 else "-inf"
    if v == 0:
        return "-0" if neg else "+0"
    return "finite"


def within(got, ref, bound):
    """|got - ref| <= bound, where `ref` may carry mpmath.diff's noise: 1e-40 relative, never as much as one bit of a float64"""
    ref = mpf(ref)
    slack = abs(ref) * mpf(10) ** -40 if abs(ref) > DIFF_NOISE else DIFF_NOISE * mpf(10) ** -10
    return abs(mpf(float(got)) - ref) <= bound + slack


# ------------------------------------------------------------------------------------------------- folded constants
# A constant subtree is folded in float64 when the expression is built, and so is log(a) in the derivative of a ** b with a
# constant base.  The bound gives a folded constant c the error C_CONST 2^-53 |c|, which an ill-conditioned fold -- tan(27 ** 2.5),
# log(atan(1.5)) -- exceeds by orders of magnitude through no fault of the evaluator.  A tree is therefore kept only if the
# first-order error analysis of each of its constant subtrees (0.5 2^-52 per arithmetic operation, 2^-52 per function, the
# rules of `_op`) stays within CONST_GUARD 2^-53 |c|; what the folds then really lose is measured (C_CONST).
CONST_GUARD = 8
_TREE_OPS = {"add": T.OP_ADD, "sub": T.OP_SUB, "mul": T.OP_MUL, "div": T.OP_DIV, "neg": T.OP_NEG, "sin": T.OP_SIN, "cos": T.OP_COS,
             "exp": T.OP_EXP, "log": T.OP_LOG, "sqrt": T.OP_SQRT, "pow": T.OP_POW, "tan": T.OP_TAN, "atan": T.OP_ATAN,
             "tanh": T.OP_TANH, "abs": T.OP_ABS, "sign": T.OP_SIGN, "step": T.OP_STEP, "min": T.OP_MIN, "max": T.OP_MAX}


def _fold(op, a, b):
    """(value, bound) of one folded operation on constants given as (value, bound)"""
    v, _, da, db, c_op = _op(op, (a[0], False), (b[0], False))
    if da is None:
        pick = b if op in (T.OP_MIN, T.OP_MAX) and v == b[0] and v != a[0] else a
        return v, (mpf(0) if op in (T.OP_SIGN, T.OP_STEP) else pick[1])
    return v, _pe(da, a[1]) + _pe(db, b[1]) + min(c_op, 1) * U * abs(v)


def folded_constants_ok(tree):
    """True where every constant the compiler folds out of `tree` is well conditioned (see above)"""
    def well(c):
        return mp.isfinite(c[0]) and c[1] <= CONST_GUARD * (U / 2) * abs(c[0])

    def walk(t):
        """(value, bound) of a constant subtree, None of any other; raises Reject at an ill-conditioned fold"""
        op = t[0]
        if op in ("var", "par"):
            return None
        if op == "const":
            return mpf(t[1]), mpf(0)
        kids = [walk(c) for c in t[1:] if isinstance(c, tuple)]
        if op == "pow" and kids[0] is not None and kids[1] is None and kids[0][0] > 0 and not well(_fold(T.OP_LOG, kids[0], kids[0])):
            raise Reject
        if any(c is None for c in kids):
            if not all(c is None or well(c) for c in kids):
                raise Reject
            return None
        a = kids[0]
        if op == "powc":
            c = t[2]
            if c == math.floor(c):
                v = a[0] ** int(c)
                return v, abs(c) * abs(v / a[0]) * a[1] + abs(c) * (U / 2) * abs(v)
            return _fold(T.OP_SQRT, a, a) if c == 0.5 else _fold(T.OP_POW, a, (mpf(c), mpf(0)))
        return _fold(_TREE_OPS[op], a, kids[-1])

    try:
        root = walk(tree)
        return root is None or well(root)
    except (Reject, ZeroDivisionError, ValueError, TypeError):
        return False


# ------------------------------------------------------------------------------------------------- (c) kept patterns
class Kept:
    """a generated tree that passed: its expression, its compiled tapes and `rows` guarded sample points (x, p)"""

    def __init__(self, tree, k, q, expr, tapes, points):
        self.tree, self.k, self.q, self.expr, self.tapes, self.points = tree, k, q, expr, tapes, points
        self.x = np.array([pt[0] for pt in points])
        self.p = np.array([pt[1] for pt in points]).reshape(len(points), q)


def compile_tapes(expr, k, q):
    """the three tapes of `expr` as `TapeModel.finalize()` compiles them, or None where one does not fit SLOT_MAX"""
    M = T.TapeModel(k, 1, np.ones(k), -np.inf, np.inf, -np.inf, np.inf)
    M.add_constraint(expr, np.array([0]), np.arange(k)[None, :], np.ones((1, q)))
    try:
        M.finalize()
    except ValueError:
        return None
    return M.patterns[0].tapes


def draw_point(rng, k, q):
    return [rng.uniform(*X_RANGE) for _ in range(k)], [rng.uniform(*P_RANGE) for _ in range(q)]


def try_tree(rng, tree, k, q, rows, fixed_x=None):
    """`Kept` or None: not constant, well-conditioned folded constants, a non-zero first derivative, three tapes within
    SLOT_MAX, `rows` guarded points within 6 * rows draws (`fixed_x`: the local variables of every point are these, only the
    parameters are drawn)"""
    expr = to_expr(tree)
    if expr.is_const or not folded_constants_ok(tree):
        return None
    tapes = compile_tapes(expr, k, q)
    if tapes is None or tapes[1].nout == 0:
        return None
    points = []
    for _ in range(6 * rows):
        x, p = draw_point(rng, k, q)
        x = x if fixed_x is None else list(fixed_x)
        try:
            evaluate(tree, [mpf(v) for v in x], [mpf(v) for v in p], guard=True)
        except Reject:
            continue
        points.append((x, p))
        if len(points) == rows:
            return Kept(tree, k, q, expr, tapes, points)
    return None


def kept_patterns(seed, count, k, q, depth, rows, wide=False):
    """`count` kept patterns of one seed and the number of trees generated for them (`wide`: trees of `wide_tree`)"""
    rng = random.Random(seed)
    kept, generated = [], 0
    while len(kept) < count:
        generated += 1
        assert generated <= (400 if wide else 20) * count, "the generator keeps too few of its trees"
        pat = try_tree(rng, wide_tree(rng, k, q) if wide else random_tree(rng, depth, k, q), k, q, rows)
        if pat is not None:
            kept.append(pat)
    return kept, generated


def opcodes(tape):
    return set(tape.code[:, 0].tolist())


def kept_patterns_sized(seed, sizes, k, q, depth, fixed_x=None):
    """one kept pattern per entry of `sizes` (its number of guarded points); `fixed_x(i, kept)`: None or the local variables
    every point of pattern i must have"""
    rng = random.Random(seed)
    kept, generated = [], 0
    while len(kept) < len(sizes):
        generated += 1
        assert generated <= 40 * len(sizes), "the generator keeps too few of its trees"
        fx = fixed_x(len(kept), kept) if fixed_x else None
        pat = try_tree(rng, random_tree(rng, depth, k, q), k, q, sizes[len(kept)], fx)
        if pat is not None:
            kept.append(pat)
    return kept


# ------------------------------------------------------------------------------------------------- the device model of random patterns
BS = 128          # rows per workgroup of the interpreter kernel (TAPE_BS in csrc/tape_eval.hip)
NREF = 16         # rows of a pattern that get the mpmath reference
LIBRARY_OPS = frozenset((T.OP_SIN, T.OP_COS, T.OP_EXP, T.OP_LOG, T.OP_SQRT, T.OP_POW, T.OP_TAN, T.OP_ATAN, T.OP_TANH))


def reference_rows(rng, nrow):
    """the first, the last, both sides of every multiple of BS, the rest at random: at most NREF rows, sorted"""
    rows = {0, nrow - 1}
    for edge in range(BS, nrow, BS):
        rows |= {edge - 1, edge}
    rest = [r for r in range(nrow) if r not in rows]
    rng.shuffle(rest)
    return sorted(rows | set(rest[:max(0, NREF - len(rows))]))


def random_device_model(seed=8):
    """ONE TapeModel of 24 kept patterns, k = 3, q = 2: objective and constraint patterns alternate, R cycles through
    1, BS, BS + 1, 3 BS - 1.  Every pattern row has variables of its own, so every row sits at a guarded point, except that the
    objective patterns 8 and 16 (R = 1) use the variables of row 0 of the objective pattern before them (gradient entries with
    two contributions).  Constraint patterns write to disjoint rows, except that pattern 9 feeds a row of pattern 7 and pattern
    13 (R = BS + 1) the BS rows of pattern 11 (its first row twice).  Returns the model, x and per pattern its `Kept` with
    `.kind, .rows, .var_index, .ref_rows`."""
    k, q = 3, 2
    sizes = [(1, BS, BS + 1, 3 * BS - 1)[(i // 2) % 4] for i in range(24)]
    pats = kept_patterns_sized(seed, sizes, k, q, 4, lambda i, kept: kept[i - 2].points[0][0] if i in (8, 16) else None)
    rng = random.Random(seed + 1)
    nvar = sum(s for i, s in enumerate(sizes) if i not in (8, 16)) * k
    perm = list(range(nvar))
    rng.shuffle(perm)
    x, vbase, cbase, blocks = np.zeros(nvar), 0, 0, {}
    for i, pat in enumerate(pats):
        nrow = sizes[i]
        pat.kind, pat.R, pat.ref_rows = i % 2, nrow, reference_rows(rng, nrow)
        if i in (8, 16):
            pat.var_index = pats[i - 2].var_index[:1].copy()
        else:
            pat.var_index = np.array(perm[vbase:vbase + nrow * k]).reshape(nrow, k)
            vbase += nrow * k
        x[pat.var_index] = pat.x
        pat.rows = None
        if pat.kind == 1:
            if i == 9:
                pat.rows = blocks[7][:1].copy()
            elif i == 13:
                pat.rows = blocks[11][np.arange(nrow) % len(blocks[11])]
            else:
                pat.rows = cbase + np.arange(nrow)
                cbase += nrow
            blocks[i] = pat.rows
    M = T.TapeModel(nvar, cbase + 3, x, -np.inf, np.inf, -np.inf, np.inf)          # (the last three rows: fed by no pattern)
    for pat in pats:
        if pat.kind == 0:
            M.add_objective(pat.expr, pat.var_index, pat.p)
        else:
            M.add_constraint(pat.expr, pat.rows, pat.var_index, pat.p)
    return M.finalize(), x, pats


# ------------------------------------------------------------------------------------------------- the kernel's full footprint
# K8 without the perfect matching below splits into these eight triangles: every pair of local variables is in exactly one term
FP_TRIANGLES = ((0, 2, 4), (0, 3, 6), (0, 5, 7), (1, 2, 7), (1, 3, 5), (1, 4, 6), (2, 5, 6), (3, 4, 7))
FP_MATCHING = ((0, 1), (2, 3), (4, 5), (6, 7))
FP_R, FP_N, FP_M = 2 * BS + 1, 40, 100


def footprint_terms():
    """The polynomial as monomials (parameter columns, local variables):
      cheap   P_j V_j V_j (8), P_c V_a V_b V_c over the triangles (8), P_c V_a V_b over the matching (4); each of the 36 second
              derivatives comes from exactly one term and is one instruction or a parameter: P_j + P_j (8), P_c V_m (24),
              P_c (4) -- 32 distinct slots that live to the end of the Hessian tape
      hungry  (q_0 + (q_1 + ... q_27)) V_0 with 28 distinct products q = P_a P_b: all 28 are alive before the first sum is taken
    and the expression is  t_7 + (t_6 + (t_5 + (LOW + hungry)))  with LOW the other 17 cheap terms summed left to right: while
    the 28 products wait, the value tape holds t_7, t_6, t_5 and LOW (32 slots), the first-derivative tape the V_0 derivative
    of LOW and three products it shares with later outputs (32 slots)."""
    cheap = [((j,), (j, j)) for j in range(8)] + [((c,), t) for c, t in enumerate(FP_TRIANGLES)] + \
            [((c,), e) for c, e in enumerate(FP_MATCHING)]
    products = [(a, b) for a in range(8) for b in range(a, 8)][:28]
    return cheap, products


def footprint_expr():
    cheap, products = footprint_terms()

    def monomial(pars, vars_):
        fac = [T.P(c) for c in pars] + [T.V(j) for j in vars_]
        e = fac[0]
        for f in fac[1:]:
            e = e * f
        return e
    rest = cheap[:5] + cheap[8:]
    low = monomial(*rest[0])
    for t in rest[1:]:
        low = low + monomial(*t)
    q = [monomial(ab, ()) for ab in products]
    big = q[-1]
    for t in q[-2::-1]:
        big = t + big
    e = low + big * T.V(0)
    for j in (5, 6, 7):
        e = monomial(*cheap[j]) + e
    return e


def footprint_model():
    """The full-footprint polynomial as an objective AND a constraint pattern (k = q = 8, R = 2 BS + 1, variables shared between
    rows, several pattern rows per constraint row), a one-slot k = 1 objective pattern, and the extended constraint pattern
    tanh(V0 - P0) V1 + V1 V1 whose parameter IS its first variable's value: tanh(0) = 0 on any library, so its value v1^2, its
    derivatives (v1, 2 v1) and (0, 1, 2) are integers too.  obj and grad run the base kernel, cons, jac and hess the extended
    one, each launch with the LDS of the full-footprint tape.  All data are small integers."""
    rng = np.random.default_rng(40)
    x = rng.integers(-3, 4, FP_N).astype(float)
    M = T.TapeModel(FP_N, FP_M, x, -np.inf, np.inf, -np.inf, np.inf)
    distinct = lambda R, k: np.stack([rng.choice(FP_N, k, replace=False) for _ in range(R)])  # noqa: E731
    vi, par = distinct(FP_R, 8), rng.integers(-2, 3, (FP_R, 8)).astype(float)
    M.add_objective(footprint_expr(), vi, par)
    M.add_constraint(footprint_expr(), np.arange(FP_R) % (FP_M - 10), vi[::-1].copy(), par)
    M.add_objective(T.V(0) * T.V(0), np.array([[5], [17], [5]]))
    vt = distinct(BS + 3, 2)
    M.add_constraint(T.tanh(T.V(0) - T.P(0)) * T.V(1) + T.V(1) * T.V(1), 50 + np.arange(BS + 3) % 45, vt, x[vt[:, :1]])
    M.fp_x = x
    return M.finalize()


def assert_footprint_shape(M):
    for p in M.patterns[:2]:
        assert (p.k, p.q, p.R) == (T.K_MAX, T.Q_MAX, 2 * BS + 1)
        assert [t.nslot for t in p.tapes] == [T.SLOT_MAX] * 3, [t.nslot for t in p.tapes]
        assert [t.nout for t in p.tapes] == [1, 8, 36]
        assert not any(opcodes(t) & T.OP_EXTENDED for t in p.tapes)
    one = M.patterns[2]
    assert one.k == 1 and [t.nslot for t in one.tapes] == [1, 1, 0]
    assert T.OP_TANH in opcodes(M.patterns[3].tapes[0]) and M.patterns[3].kind == 1


def footprint_points(M):
    rng = np.random.default_rng(41)
    y = rng.integers(-3, 4, M.m).astype(float)
    y[::5] = 0.0
    return [(M.fp_x, y, 2.0), (M.fp_x, -y, 0.0)]


def _monomial_derivative(pars, vars_, p, v, wrt):
    """the integer value of the derivative of prod p[c] prod v[j] with respect to the local variables in `wrt` (power rule)"""
    vars_, coef = list(vars_), 1
    for j in wrt:
        coef *= vars_.count(j)
        if coef == 0:
            return 0
        vars_.remove(j)
    for c in pars:
        coef *= p[c]
    for j in vars_:
        coef *= v[j]
    return coef


def footprint_reference(M, x, y, w):
    """f, grad, cons, dense Jacobian and dense lower Lagrangian Hessian in Python integers; the scatter by (rows[r], var_index[r, j])
    is this function's own"""
    cheap, products = footprint_terms()
    monomials = cheap + [(ab, (0,)) for ab in products]
    xi, yi, wi = [int(v) for v in x], [int(v) for v in y], int(w)
    n, m = M.n, M.m
    f, g, c = 0, [0] * n, [0] * m
    J = [[0] * n for _ in range(m)]
    H = [[0] * n for _ in range(n)]
    for ip, pat in enumerate(M.patterns):
        for r in range(pat.R):
            gv = [int(i) for i in pat.var_index[r]]
            v, p = [xi[i] for i in gv], [int(t) for t in pat.params[r]]
            if ip < 2:
                d = lambda *wrt: sum(_monomial_derivative(a, b, p, v, wrt) for a, b in monomials)  # noqa: E731
            elif ip == 2:
                d = lambda *wrt: (v[0] * v[0], 2 * v[0], 2)[len(wrt)]  # noqa: E731
            else:
                assert p[0] == v[0]
                d = lambda *wrt: {(): v[1] * v[1], (0,): v[1], (1,): 2 * v[1], (0, 0): 0, (1, 0): 1, (1, 1): 2}[wrt]  # noqa: E731
            weight = wi if pat.kind == 0 else yi[pat.rows[r]]
            if pat.kind == 0:
                f += d()
            else:
                c[pat.rows[r]] += d()
            for j in range(pat.k):
                if pat.kind == 0:
                    g[gv[j]] += d(j)
                else:
                    J[pat.rows[r]][gv[j]] += d(j)
                for l in range(j + 1):
                    H[max(gv[j], gv[l])][min(gv[j], gv[l])] += weight * d(j, l)
    return f, g, c, J, H


def check_footprint_outputs(M, x, y, w, f, g, c, jv, hv, structure=None):
    """all five callbacks against the integers; `structure`: (jac_I, jac_J, hess_I, hess_J) to sum the COO values by (the model's
    own by default)"""
    jI, jJ, hI, hJ = structure or (M.jac_I, M.jac_J, M.hess_I, M.hess_J)
    rf, rg, rc, rJ, rH = footprint_reference(M, x, y, w)
    assert f == rf, (f, rf)
    assert (np.asarray(g) == np.array(rg, dtype=float)).all()
    assert (np.asarray(c) == np.array(rc, dtype=float)).all()
    Jd, Hd = np.zeros((M.m, M.n)), np.zeros((M.n, M.n))
    np.add.at(Jd, (jI, jJ), jv)
    np.add.at(Hd, (hI, hJ), hv)
    assert (np.asarray(hI) >= np.asarray(hJ)).all()
    assert (Jd == np.array(rJ, dtype=float)).all()
    assert (Hd == np.array(rH, dtype=float)).all()


# ------------------------------------------------------------------------------------------------- edge arguments of the library functions
_INF, _NAN, _PI2 = math.inf, math.nan, math.pi / 2          # (math.pi / 2 is pi/2 rounded down)
EDGE_ARGS = [0.0, -0.0, 5e-324, 2.0 ** -1022, 1e-300, -1e-300, 1 + 2.0 ** -52, 1 - 2.0 ** -52, 20.0, -20.0, 710.0, -710.0, 709.78,
             1e5, 1e10, 1e15, 1e300, _INF, -_INF, _NAN, _PI2, math.nextafter(_PI2, _INF), -1.5, -2.0]
EDGE_POW = [(0.0, 2.5), (0.0, 3.0), (-0.0, 3.0), (0.0, -1.5), (-0.0, -3.0), (0.0, 0.0), (-0.0, 0.0), (-2.0, 3.0), (-2.0, 2.0),
            (-2.0, 0.5), (-1.5, -1.0), (2.0, 0.5), (1.0, _NAN), (_NAN, 0.0), (2.0, _INF), (0.5, _INF), (2.0, -_INF), (_INF, 2.0),
            (_INF, -1.0), (-_INF, 3.0), (1.5, 1e3), (10.0, 308.5), (10.0, -320.0), (1 + 2.0 ** -52, 1e15), (1e300, 1.7),
            (5e-324, 0.5), (1 - 2.0 ** -52, -1e15), (1e-300, -1.0)]


def edge_model():
    """One constraint pattern per library function on rows of edge arguments; value, first and second derivatives are read
    back through cons, jac_coord and hess_coord (y = 1).  Returns the model, x and the function names in pattern order."""
    V0, V1 = T.V(0), T.V(1)
    funcs = [("sin", T.sin(V0)), ("cos", T.cos(V0)), ("exp", T.exp(V0)), ("log", T.log(V0)), ("sqrt", T.sqrt(V0)), ("tan", T.tan(V0)),
             ("atan", T.atan(V0)), ("tanh", T.tanh(V0)), ("pow 1.7", V0 ** 1.7), ("pow -0.3", V0 ** -0.3), ("pow", T.pow_(V0, V1))]
    nrow = [len(EDGE_POW) if name == "pow" else len(EDGE_ARGS) for name, _ in funcs]
    M = T.TapeModel(2 * sum(nrow), sum(nrow), np.ones(2 * sum(nrow)), -np.inf, np.inf, -np.inf, np.inf)
    x, base = np.zeros(M.n), 0
    for (name, expr), R_ in zip(funcs, nrow):
        vi = 2 * base + np.arange(2 * R_).reshape(R_, 2)
        x[vi] = np.array(EDGE_POW) if name == "pow" else np.stack([EDGE_ARGS, np.ones(R_)], axis=1)
        M.add_constraint(expr, base + np.arange(R_), vi)
        base += R_
    return M.finalize(), x, [name for name, _ in funcs]


def edge_entries(M, x, c, jv, hv):
    """every entry of one side's cons / jac_coord / hess_coord (y = 1) beside the 60-digit value of the same tape:
    (function pattern, tape, output, row, value, (reference, sign of zero, bound)); the entry of output o and row r of a
    pattern is base + o R + r (the documented COO layout)"""
    base = [None, 0, 0]
    for ip, pat in enumerate(M.patterns):
        for r in range(pat.R):
            xs = x[pat.var_index[r]]
            for w, tape in enumerate(pat.tapes):
                for o, (v, neg, _, bound) in enumerate(run_tape(tape, xs, [], weight=1.0 if w == 2 else None)):
                    if w == 0:
                        got, neg = c[pat.rows[r]], (False if v == 0 else neg)          # the ordered sum starts from +0: 0 + -0 = +0
                    else:
                        got = (jv, hv)[w - 1][base[w] + o * pat.R + r]
                    yield ip, w, o, r, float(got), (v, neg, bound)
        base[1] += pat.R * pat.tapes[1].nout
        base[2] += pat.R * pat.tapes[2].nout


def edge_findings(M, x, c, jv, hv, names):
    """(class differences, value misses) of one side: {(function, tape, output, arguments): (class there, class of the
    reference)} and a list of finite entries outside the bound"""
    classes, misses = {}, []
    for ip, w, o, r, got, (v, neg, bound) in edge_entries(M, x, c, jv, hv):
        args = tuple(float(t) for t in x[M.patterns[ip].var_index[r]][:2 if names[ip] == "pow" else 1])
        here, there = classify(got), classify(v, neg)
        number = ("finite", "+0", "-0")      # a zero beside a non-zero reference (1 - tanh(20)^2 in float64) is a VALUE to compare
        if here != there and not (here in number and there in number and "finite" in (here, there)):
            classes[(names[ip], w, o, repr(args))] = (here, there)
        elif "finite" in (here, there) and not abs(mpf(got) - v) <= bound:
            misses.append((names[ip], w, o, args, got, mp.nstr(v, 20), mp.nstr(bound, 3)))
    return classes, misses

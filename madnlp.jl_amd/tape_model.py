"""Model-agnostic NLP evaluator: an NLP written as a list of PATTERNS, each one scalar expression applied to many rows of
index and parameter data (the way ExaModels compiles the models of the reference's GPU benchmarks), compiled to straight-line
expression TAPES that one interpreter evaluates -- here in numpy (the host mirror and oracle), in `csrc/tape_eval.hip` on the
device (`mnk_tape_*`, `ipm_dev.DeviceTapeCallbacks`).  DESIGN.md section 14 documents the format.

  expression   V(j) local variable j of the row, P(c) parameter column c, float constants; + - * / unary minus, powers (integer
               exponents expanded to products, 0.5 a square root, anything else `pow_`), sin cos exp log sqrt tan atan tanh, and
               the piecewise abs_ sign step minimum maximum (defined by comparisons, see `minimum`)
  pattern      objective:  f   += sum_r expr(x[var_index[r, :]], params[r, :])
               constraint: c[rows[r]] += expr(x[var_index[r, :]], params[r, :])      (several patterns may feed one row)
  tapes        per pattern three: value | first derivatives per local variable | second derivatives per local pair j >= l;
               derivatives that fold to the constant 0 are not part of the sparsity pattern
  instruction  (op, dst_slot, a, b); an operand is kind << 24 | index with kind 0 slot, 1 local variable, 2 parameter column,
               3 entry of the tape's constant pool; unary operations carry their operand twice
  COO layout   pattern-major, output-major, then row: entry = base[pattern] + o * R + r; Jacobian (rows[r], var_index[r, j_o]);
               Hessian of the pair (j, l) at (max, min) of the two global indices.  Duplicates across patterns are expected.
  summation    objective = sum of the term vector; cons[i], grad[i] = their contributions added one after the other in term
               order (np.add.at)"""
from __future__ import annotations

import heapq
import math
import struct
import weakref

import numpy as np

SLOT_MAX = 32    # slots of one tape (its live intermediate values); the device keeps one LDS column per slot and lane
K_MAX = 8        # local variables of a pattern
Q_MAX = 8        # parameter columns of a pattern
OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_SIN, OP_COS, OP_EXP, OP_LOG, OP_SQRT = range(10)
OP_POW, OP_TAN, OP_ATAN, OP_TANH, OP_ABS, OP_SIGN, OP_STEP, OP_MIN, OP_MAX = range(16, 25)      # 10 .. 15 are unassigned
OP_NAMES = ("add", "sub", "mul", "div", "neg", "sin", "cos", "exp", "log", "sqrt") + (None,) * 6 + \
           ("pow", "tan", "atan", "tanh", "abs", "sign", "step", "min", "max")
OP_EXTENDED = frozenset(range(OP_POW, OP_MAX + 1))      # what the device keeps in the second instantiation of its kernel
KIND_SLOT, KIND_VAR, KIND_PAR, KIND_CONST = range(4)


# The selection operations are these comparisons on both interpreters (not fmin / fmax / copysign, whose NaN and signed-zero
# rules differ between libraries): a NaN in `b` returns `a`, sign(NaN) = 0, a tie returns `a`.
def _np_min(a, b): return np.where(np.less(b, a), b, a)
def _np_max(a, b): return np.where(np.greater(b, a), b, a)
def _np_step(a): return np.where(np.greater_equal(a, 0.0), 1.0, 0.0)
def _np_sign(a): return np.where(np.greater(a, 0.0), 1.0, np.where(np.less(a, 0.0), -1.0, 0.0))
def _py_min(a, b): return b if b < a else a
def _py_max(a, b): return b if b > a else a
def _py_step(a): return 1.0 if a >= 0.0 else 0.0
def _py_sign(a): return 1.0 if a > 0.0 else -1.0 if a < 0.0 else 0.0


_UNARY = {OP_NEG: np.negative, OP_SIN: np.sin, OP_COS: np.cos, OP_EXP: np.exp, OP_LOG: np.log, OP_SQRT: np.sqrt,
          OP_TAN: np.tan, OP_ATAN: np.arctan, OP_TANH: np.tanh, OP_ABS: np.abs, OP_SIGN: _np_sign, OP_STEP: _np_step}
_BINARY = {OP_ADD: np.add, OP_SUB: np.subtract, OP_MUL: np.multiply, OP_DIV: np.divide,
           OP_POW: np.power, OP_MIN: _np_min, OP_MAX: _np_max}
_FOLD = {OP_SIN: math.sin, OP_COS: math.cos, OP_EXP: math.exp, OP_LOG: math.log, OP_SQRT: math.sqrt,
         OP_TAN: math.tan, OP_ATAN: math.atan, OP_TANH: math.tanh, OP_ABS: abs, OP_SIGN: _py_sign, OP_STEP: _py_step}
_FOLD2 = {OP_POW: math.pow, OP_MIN: _py_min, OP_MAX: _py_max}


class Expr:
    """A node of an expression DAG.  Nodes are interned: building the same expression twice gives the same object, which is
    what shares common subexpressions across the outputs of a tape.  The intern table holds its nodes weakly and a node's
    derivatives are memoized on the node itself, so expressions live exactly as long as something (a model's patterns, the
    caller) refers to them; the table's keys name operand nodes by `id`, which is safe because an entry exists only while its
    node -- and with it the operands the node refers to -- is alive."""
    __slots__ = ("op", "a", "b", "value", "_d", "__weakref__")
    _pool: "weakref.WeakValueDictionary" = weakref.WeakValueDictionary()

    def __init__(self, op, a=None, b=None, value=None):
        self.op, self.a, self.b, self.value, self._d = op, a, b, value, None

    @staticmethod
    def _get(key, *args):
        e = Expr._pool.get(key)
        if e is None:
            e = Expr._pool[key] = Expr(*args)
        return e

    @property
    def is_const(self):
        return self.op == "const"

    def __add__(self, o): return _add(self, _wrap(o))
    def __radd__(self, o): return _add(_wrap(o), self)
    def __sub__(self, o): return _sub(self, _wrap(o))
    def __rsub__(self, o): return _sub(_wrap(o), self)
    def __mul__(self, o): return _mul(self, _wrap(o))
    def __rmul__(self, o): return _mul(_wrap(o), self)
    def __truediv__(self, o): return _div(self, _wrap(o))
    def __rtruediv__(self, o): return _div(_wrap(o), self)
    def __neg__(self): return _neg(self)
    def __pos__(self): return self

    def __pow__(self, p): return pow_(self, p)
    def __rpow__(self, o): return pow_(o, self)


def const(v):
    v = float(v)
    return Expr._get(("const", struct.pack("<d", v)), "const", None, None, v)


def V(j):
    """local variable j of the pattern's rows: x[var_index[r, j]]"""
    if not isinstance(j, (int, np.integer)) or not 0 <= j < K_MAX:
        raise ValueError(f"V({j!r}): a pattern has local variables 0 .. {K_MAX - 1}")
    return Expr._get(("var", int(j)), "var", None, None, int(j))


def P(c):
    """parameter column c of the pattern's rows: params[r, c]"""
    if not isinstance(c, (int, np.integer)) or not 0 <= c < Q_MAX:
        raise ValueError(f"P({c!r}): a pattern has parameter columns 0 .. {Q_MAX - 1}")
    return Expr._get(("par", int(c)), "par", None, None, int(c))


def _wrap(o):
    if isinstance(o, Expr):
        return o
    if isinstance(o, (int, float, np.integer, np.floating)):
        return const(o)
    raise TypeError(f"cannot use {type(o).__name__} in a tape expression")


def _node(op, a, b=None):
    return Expr._get((op, id(a), id(b)), op, a, b)


def _is(e, v):
    return e.op == "const" and e.value == v


def _add(a, b):
    if a.is_const and b.is_const:
        return const(a.value + b.value)
    if _is(a, 0.0):
        return b
    if _is(b, 0.0):
        return a
    return _node(OP_ADD, a, b)


def _sub(a, b):
    if a.is_const and b.is_const:
        return const(a.value - b.value)
    if _is(b, 0.0):
        return a
    if _is(a, 0.0):
        return _neg(b)
    return _node(OP_SUB, a, b)


def _mul(a, b):
    if a.is_const and b.is_const:
        return const(a.value * b.value)
    if _is(a, 0.0) or _is(b, 0.0):
        return const(0.0)
    if _is(a, 1.0):
        return b
    if _is(b, 1.0):
        return a
    if _is(a, -1.0):
        return _neg(b)
    if _is(b, -1.0):
        return _neg(a)
    return _node(OP_MUL, a, b)


def _div(a, b):
    if a.is_const and b.is_const and b.value != 0.0:
        return const(a.value / b.value)
    if _is(a, 0.0):
        return const(0.0)
    if _is(b, 1.0):
        return a
    return _node(OP_DIV, a, b)


def _neg(a):
    if a.is_const:
        return const(-a.value)
    if a.op == OP_NEG:
        return a.a
    return _node(OP_NEG, a, a)


def _fun(op, a):
    a = _wrap(a)
    if a.is_const:
        try:
            return const(_FOLD[op](a.value))
        except (ValueError, OverflowError):       # log / sqrt of a negative constant, exp of a huge one: left to run time
            pass
    return _node(op, a, a)


def sin(a): return _fun(OP_SIN, a)
def cos(a): return _fun(OP_COS, a)
def exp(a): return _fun(OP_EXP, a)
def log(a): return _fun(OP_LOG, a)
def sqrt(a): return _fun(OP_SQRT, a)
def tan(a): return _fun(OP_TAN, a)
def atan(a): return _fun(OP_ATAN, a)
def tanh(a): return _fun(OP_TANH, a)


def abs_(a):
    """|a|: the sign bit cleared; its derivative is sign(a), 0 at the kink"""
    return _fun(OP_ABS, a)


def sign(a):
    """(a > 0) ? 1 : (a < 0) ? -1 : 0 -- 0 for +-0 and for NaN; its derivative is the structural zero"""
    return _fun(OP_SIGN, a)


def step(a):
    """(a >= 0) ? 1 : 0 -- 1 for +-0, 0 for NaN; its derivative is the structural zero"""
    return _fun(OP_STEP, a)


def _fun2(op, a, b):
    a, b = _wrap(a), _wrap(b)
    if a.is_const and b.is_const:
        try:
            return const(_FOLD2[op](a.value, b.value))
        except (ValueError, OverflowError, ZeroDivisionError):     # a negative base with a real exponent, 0 ** -1: run time
            pass
    return _node(op, a, b)


def minimum(a, b):
    """(b < a) ? b : a -- a tie and a NaN in `b` return `a`; the derivative follows the same choice: db + step(b - a) (da - db)"""
    return _fun2(OP_MIN, a, b)


def maximum(a, b):
    """(b > a) ? b : a -- a tie and a NaN in `b` return `a`; the derivative follows the same choice: db + step(a - b) (da - db)"""
    return _fun2(OP_MAX, a, b)


def pow_(a, b):
    """a ** b.  A constant exponent with an integer value is expanded to products (a negative one to 1 / products, 0 to the
    constant 1), 0.5 is sqrt(a); every other exponent is the pow instruction.  With a constant exponent c the derivative is
    c pow(a, c - 1) da and holds wherever pow does; with an exponent that is an expression it is
    pow(a, b) (db log a + b da / a), which needs a > 0."""
    a, b = _wrap(a), _wrap(b)
    if b.is_const and abs(b.value) < 2.0 ** 31 and b.value == math.floor(b.value):     # (NaN and inf fail the bound)
        k = int(b.value)
        if k == 0:
            return const(1.0)
        e = a
        for _ in range(abs(k) - 1):
            e = _mul(e, a)
        return e if k > 0 else _div(const(1.0), e)
    if _is(b, 0.5):
        return sqrt(a)
    return _fun2(OP_POW, a, b)


def diff(e, j):
    """Symbolic derivative of `e` with respect to local variable j (folded as it is built; memoized on the node)."""
    if e._d is None:
        e._d = {}
    d = e._d.get(j)
    if d is None:
        d = e._d[j] = _diff(e, j)
    return d


def _diff(e, j):
    op = e.op
    if op in ("const", "par"):
        return const(0.0)
    if op == "var":
        return const(1.0 if e.value == j else 0.0)
    if op in (OP_SIGN, OP_STEP):              # piecewise constant: a structural zero (the jump is not differentiated)
        return const(0.0)
    da = diff(e.a, j)
    if op == OP_ADD:
        return _add(da, diff(e.b, j))
    if op == OP_SUB:
        return _sub(da, diff(e.b, j))
    if op == OP_MUL:
        return _add(_mul(da, e.b), _mul(e.a, diff(e.b, j)))
    if op == OP_DIV:
        db = diff(e.b, j)
        if _is(db, 0.0):
            return _div(da, e.b)
        return _div(_sub(_mul(da, e.b), _mul(e.a, db)), _mul(e.b, e.b))
    if op == OP_NEG:
        return _neg(da)
    if op == OP_SIN:
        return _mul(cos(e.a), da)
    if op == OP_COS:
        return _neg(_mul(sin(e.a), da))
    if op == OP_EXP:
        return _mul(e, da)
    if op == OP_LOG:
        return _div(da, e.a)
    if op == OP_SQRT:
        return _div(da, _mul(const(2.0), e))
    if op == OP_POW:
        if e.b.is_const:
            return _mul(_mul(e.b, pow_(e.a, e.b.value - 1.0)), da)
        return _mul(e, _add(_mul(diff(e.b, j), log(e.a)), _div(_mul(e.b, da), e.a)))
    if op == OP_TAN:
        return _mul(_add(const(1.0), _mul(e, e)), da)
    if op == OP_ATAN:
        return _div(da, _add(const(1.0), _mul(e.a, e.a)))
    if op == OP_TANH:
        return _mul(_sub(const(1.0), _mul(e, e)), da)
    if op == OP_ABS:
        return _mul(sign(e.a), da)
    if op in (OP_MAX, OP_MIN):                # the derivative of the operand the value rule selects (`a` at a tie)
        db = diff(e.b, j)
        pick_a = step(_sub(e.a, e.b) if op == OP_MAX else _sub(e.b, e.a))
        return _add(db, _mul(pick_a, _sub(da, db)))
    raise AssertionError(op)


def _footprint(e, seen, vars_, pars):
    if id(e) in seen:
        return
    seen.add(id(e))
    if e.op == "var":
        vars_.add(e.value)
    elif e.op == "par":
        pars.add(e.value)
    elif e.op != "const":
        _footprint(e.a, seen, vars_, pars)
        if e.b is not e.a:
            _footprint(e.b, seen, vars_, pars)


class Tape:
    """Straight-line code for a list of output expressions: `code` int32 (ninstr, 4) rows (op, dst, a, b), `consts` float64,
    `out_operand` int32 (nout) and, for derivative tapes, the local variable (pair) of every output in `out_j` (`out_l`)."""

    def __init__(self, outputs, out_j=(), out_l=()):
        order, seen = [], set()

        def visit(e):
            if id(e) in seen or e.op in ("const", "var", "par"):
                return
            seen.add(id(e))
            visit(e.a)
            if e.b is not e.a:
                visit(e.b)
            order.append(e)

        for e in outputs:
            visit(e)
        last = {}
        for i, e in enumerate(order):
            last[id(e.a)] = i
            last[id(e.b)] = i
        for e in outputs:
            last[id(e)] = len(order)          # an output stays in its slot to the end of the tape
        pool, consts, slot_of, free, nslot = {}, [], {}, [], 0

        def operand(e):
            if e.op == "const":
                key = struct.pack("<d", e.value)
                if key not in pool:
                    pool[key] = len(consts)
                    consts.append(e.value)
                return KIND_CONST << 24 | pool[key]
            if e.op == "var":
                return KIND_VAR << 24 | e.value
            if e.op == "par":
                return KIND_PAR << 24 | e.value
            return KIND_SLOT << 24 | slot_of[id(e)]

        code = []
        for i, e in enumerate(order):
            a, b = operand(e.a), operand(e.b)
            for arg in ((e.a,) if e.b is e.a else (e.a, e.b)):     # operands are read before the destination is written
                if id(arg) in slot_of and last[id(arg)] == i:
                    heapq.heappush(free, slot_of[id(arg)])
            if free:
                dst = heapq.heappop(free)
            else:
                dst, nslot = nslot, nslot + 1
            slot_of[id(e)] = dst
            code.append((e.op, dst, a, b))
        self.nslot = nslot
        self.code = np.array(code, dtype=np.int32).reshape(-1, 4)
        self.out_operand = np.array([operand(e) for e in outputs], dtype=np.int32)
        self.consts = np.array(consts, dtype=np.float64)
        self.out_j = np.array(out_j, dtype=np.int32)
        self.out_l = np.array(out_l, dtype=np.int32)

    @property
    def nout(self):
        return len(self.out_operand)

    def run(self, xv, pv, R):
        """The numpy interpreter: the instructions in order, vectorised over the R rows.  Returns one array per output."""
        slots = [None] * self.nslot
        consts = self.consts

        def get(o):
            kind, idx = o >> 24, o & 0xFFFFFF
            return slots[idx] if kind == KIND_SLOT else xv[idx] if kind == KIND_VAR else pv[idx] if kind == KIND_PAR else consts[idx]

        for op, dst, a, b in self.code.tolist():
            slots[dst] = _BINARY[op](get(a), get(b)) if op in _BINARY else _UNARY[op](get(a))
        return [np.broadcast_to(np.asarray(get(o), dtype=np.float64), (R,)) for o in self.out_operand.tolist()]


class _Pattern:
    def __init__(self, kind, expr, rows, var_index, params):
        self.kind, self.expr, self.rows, self.var_index, self.params = kind, expr, rows, var_index, params
        self.R, self.k = var_index.shape
        self.q = params.shape[1]
        self.tapes = None


class TapeModel:
    """An NLP assembled from patterns; after `finalize()` it offers the callback interface the IPM drivers use (`n, m, x0, y0,
    lvar, uvar, lcon, ucon, jac_I, jac_J, hess_I, hess_J, obj, grad, cons, jac_coord, hess_coord(x, y, w)`)."""
    is_tape_model = True      # what `DeviceMadNLPSolver` selects `DeviceTapeCallbacks` by

    def __init__(self, n, m, x0, lvar, uvar, lcon, ucon, name="tape", minimize=True):
        self.n, self.m, self.name = int(n), int(m), name
        self.minimize = bool(minimize)      # the objective sense (False: the drivers maximize)
        f = lambda a, k: np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), (k,)))  # noqa: E731
        self.x0, self.lvar, self.uvar = f(x0, self.n), f(lvar, self.n), f(uvar, self.n)
        self.lcon, self.ucon = f(lcon, self.m), f(ucon, self.m)
        self.y0 = np.zeros(self.m)
        self.patterns: list[_Pattern] = []
        self.finalized = False

    # ------------------------------------------------------------------ front end
    def _add(self, kind, expr, rows, var_index, params):
        if self.finalized:
            raise RuntimeError("TapeModel: patterns cannot be added after finalize()")
        expr = _wrap(expr)
        vi = np.asarray(var_index)
        if vi.ndim != 2 or vi.shape[0] < 1 or not 1 <= vi.shape[1] <= K_MAX or not np.issubdtype(vi.dtype, np.integer):
            raise ValueError(f"var_index must be an integer array of shape (R >= 1, 1 <= k <= {K_MAX}), got {vi.dtype} {vi.shape}")
        R, k = vi.shape
        par = np.zeros((R, 0)) if params is None else np.asarray(params, dtype=np.float64)
        if par.ndim != 2 or par.shape[0] != R or par.shape[1] > Q_MAX:
            raise ValueError(f"params must have shape (R = {R}, q <= {Q_MAX}), got {par.shape}")
        if vi.min() < 0 or vi.max() >= self.n:
            r, j = np.argwhere((vi < 0) | (vi >= self.n))[0]
            raise ValueError(f"var_index[{r}, {j}] = {vi[r, j]} is out of range: the model has {self.n} variables")
        s = np.sort(vi, axis=1)
        rep = np.nonzero((s[:, 1:] == s[:, :-1]).any(axis=1))[0]
        if len(rep):
            raise ValueError(f"row {rep[0]} of var_index names the same variable twice ({vi[rep[0]].tolist()}): the Hessian entry of "
                             "that local pair would fall on the diagonal and need doubling; write the row with distinct variables")
        vars_, pars = set(), set()
        _footprint(expr, set(), vars_, pars)
        if vars_ and max(vars_) >= k:
            raise ValueError(f"the expression uses V({max(vars_)}) but var_index has {k} columns")
        if pars and max(pars) >= par.shape[1]:
            raise ValueError(f"the expression uses P({max(pars)}) but params has {par.shape[1]} columns")
        if kind == 1:
            rows = np.asarray(rows)
            if rows.shape != (R,) or not np.issubdtype(rows.dtype, np.integer):
                raise ValueError(f"rows must be an integer array of shape ({R},), got {rows.dtype} {rows.shape}")
            if rows.min() < 0 or rows.max() >= self.m:
                r = np.nonzero((rows < 0) | (rows >= self.m))[0][0]
                raise ValueError(f"rows[{r}] = {rows[r]} is out of range: the model has {self.m} constraints")
            rows = np.ascontiguousarray(rows, dtype=np.int32)
        self.patterns.append(_Pattern(kind, expr, rows, np.ascontiguousarray(vi, dtype=np.int32), np.ascontiguousarray(par)))

    def add_objective(self, expr, var_index, params=None):
        """f += sum_r expr(x[var_index[r, :]], params[r, :])"""
        self._add(0, expr, None, var_index, params)

    def add_constraint(self, expr, rows, var_index, params=None):
        """c[rows[r]] += expr(x[var_index[r, :]], params[r, :]); rows no pattern touches evaluate to 0"""
        self._add(1, expr, rows, var_index, params)

    # ------------------------------------------------------------------ compilation
    def finalize(self):
        if self.finalized:
            return self
        jI, jJ, hI, hJ, gJ, cI = [], [], [], [], [], []
        for ip, p in enumerate(self.patterns):
            d1 = [(j, diff(p.expr, j)) for j in range(p.k)]
            d1 = [(j, e) for j, e in d1 if not _is(e, 0.0)]
            d2 = [(j, l, diff(e, l)) for j, e in d1 for l in range(j + 1)]
            d2 = [(j, l, e) for j, l, e in d2 if not _is(e, 0.0)]
            p.tapes = (Tape([p.expr]), Tape([e for _, e in d1], [j for j, _ in d1]),
                       Tape([e for _, _, e in d2], [j for j, _, _ in d2], [l for _, l, _ in d2]))
            for name, t in zip(("value", "first-derivative", "second-derivative"), p.tapes):
                if t.nslot > SLOT_MAX:
                    raise ValueError(f"pattern {ip}: its {name} tape needs {t.nslot} slots, SLOT_MAX is {SLOT_MAX}: split the "
                                     "expression into several patterns that add into the same rows")
            for j in p.tapes[1].out_j:
                if p.kind == 1:
                    jI.append(p.rows)
                    jJ.append(p.var_index[:, j])
                else:
                    gJ.append(p.var_index[:, j])
            for j, l in zip(p.tapes[2].out_j, p.tapes[2].out_l):
                a, b = p.var_index[:, j], p.var_index[:, l]
                hI.append(np.maximum(a, b))
                hJ.append(np.minimum(a, b))
            if p.kind == 1:
                cI.append(p.rows)
        cat = lambda L: np.concatenate(L).astype(np.int32) if L else np.zeros(0, dtype=np.int32)  # noqa: E731
        self.jac_I, self.jac_J, self.hess_I, self.hess_J = cat(jI), cat(jJ), cat(hI), cat(hJ)
        self._grad_J, self._cons_I = cat(gJ), cat(cI)
        self.nterms = sum(p.R for p in self.patterns if p.kind == 0)
        self.finalized = True
        return self

    # ------------------------------------------------------------------ host evaluation (numpy interpreter)
    def _eval(self, which, x, kinds):
        assert self.finalized, "TapeModel: call finalize() first"
        x = np.asarray(x, dtype=np.float64)
        for p in self.patterns:
            if p.kind in kinds:
                xv = [x[p.var_index[:, j]] for j in range(p.k)]
                pv = [p.params[:, c] for c in range(p.q)]
                yield p, p.tapes[which].run(xv, pv, p.R)

    @staticmethod
    def _cat(parts):
        return np.concatenate(parts) if parts else np.zeros(0)

    def obj_terms(self, x):
        return self._cat([o[0] for _, o in self._eval(0, x, (0,))])

    def obj(self, x):
        return float(np.sum(self.obj_terms(x)))

    def grad_terms(self, x):
        return self._cat([v for _, o in self._eval(1, x, (0,)) for v in o])

    def grad(self, x):
        g = np.zeros(self.n)
        np.add.at(g, self._grad_J, self.grad_terms(x))
        return g

    def cons_terms(self, x):
        return self._cat([o[0] for _, o in self._eval(0, x, (1,))])

    def cons(self, x):
        c = np.zeros(self.m)
        np.add.at(c, self._cons_I, self.cons_terms(x))
        return c

    def jac_coord(self, x):
        return self._cat([v for _, o in self._eval(1, x, (1,)) for v in o])

    def hess_coord(self, x, y, w=1.0):
        y = np.asarray(y, dtype=np.float64)
        out = []
        for p, o in self._eval(2, x, (0, 1)):
            wt = np.float64(w) if p.kind == 0 else y[p.rows]
            out += [wt * v for v in o]
        return self._cat(out)


# ---------------------------------------------------------------------------------------------- models written in the DSL
def acopf_tape_model(case="case118", seed=None, load=1.0):
    """The polar AC-OPF of `problems.ACOPFModel` written as patterns, from that model's own data: same n, m, variable and
    constraint order, bounds and start; the COO order is the tape model's own (and it has no explicit zeros)."""
    from .problems import ACOPFModel
    A = ACOPFModel(case, seed, load)
    S = A.S
    va, vm, pg, qg, p, q = (S[k] for k in ("va", "vm", "pg", "qg", "p", "q"))
    nbus, ngen, nbr, narc, af, at = A.nbus, A.ngen, A.nbr, A.narc, A.arc_f, A.arc_t
    M = TapeModel(A.n, A.m, A.x0, A.lvar, A.uvar, A.lcon, A.ucon, name=f"tape_{A.name}")
    col = lambda *a: np.stack(a, axis=1)  # noqa: E731
    M.add_objective(P(0) * V(0) * V(0) + P(1) * V(0) + P(2), col(pg), A.gen_cost)
    M.add_constraint(V(0), np.array([0]), np.array([[va[0]]]))
    d = V(3) - V(4)
    flow = V(0) - (P(0) * V(1) * V(1) + V(1) * V(2) * (P(1) * cos(d) + P(2) * sin(d)))
    o = 1
    for own, c0 in ((p, 0), (q, 3)):
        M.add_constraint(flow, o + np.arange(narc), col(own, vm[af], vm[at], va[af], va[at]), A.arc_coef[:, c0:c0 + 3])
        o += narc
    M.add_constraint(V(0) - V(1), o + np.arange(nbr), col(va[A.fr], va[A.to]))
    o += nbr
    M.add_constraint(V(0) * V(0) + V(1) * V(1), o + np.arange(narc), col(p, q))
    o += narc
    pd, qd, gs, bs = A.bus_data.T
    for own_arc, own_gen, bus_expr, bus_par in ((p, pg, P(0) + P(1) * V(0) * V(0), col(pd, gs)),
                                                (q, qg, P(0) - P(1) * V(0) * V(0), col(qd, bs))):
        M.add_constraint(bus_expr, o + np.arange(nbus), col(vm), bus_par)      # a balance row: bus term + arcs - generators
        M.add_constraint(V(0), o + af, col(own_arc))
        M.add_constraint(-V(0), o + A.gen_bus, col(own_gen))
        o += nbus
    assert o == A.m
    M.acopf = A
    return M.finalize()


def hs15_tape_model():
    """`problems.HS15Model` as patterns."""
    from .problems import HS15Model as H
    M = TapeModel(2, 2, H.x0, H.lvar, H.uvar, H.lcon, H.ucon, name="tape_hs15")
    xy = np.array([[0, 1]])
    M.add_objective(100.0 * (V(1) - V(0) ** 2) ** 2 + (1.0 - V(0)) ** 2, xy)
    M.add_constraint(V(0) * V(1), np.array([0]), xy)
    M.add_constraint(V(0) + V(1) ** 2, np.array([1]), xy)
    return M.finalize()


def lootsma_tape_model():
    """`problems.LootsmaModel` as patterns."""
    from .problems import LootsmaModel as Lo
    M = TapeModel(3, 2, Lo.x0, Lo.lvar, Lo.uvar, Lo.lcon, Lo.ucon, name="tape_lootsma")
    M.add_objective(V(0) ** 3 + 11.0 * V(0) - 6.0 * sqrt(V(0)) + V(1), np.array([[0, 2]]))
    xyz = np.array([[0, 1, 2]])
    M.add_constraint(-sqrt(V(0)) - sqrt(V(1)) + sqrt(V(2)), np.array([0]), xyz)
    M.add_constraint(sqrt(V(0)) + sqrt(V(1)) + sqrt(V(2)), np.array([1]), xyz)
    return M.finalize()


def lootsma_fixed_tape_model():
    """The reference's `lootsma` as it is written there (lib/MadNLPTests/src/MadNLPTests.jl:155-164): FOUR variables, the
    first one `par`, fixed at 6 by its bounds, then x1 .. x3 -- the model `fixed_variable_treatment = "make_parameter"` is
    for.  `LootsmaModel.LOOTSMA_X` is entries 1 .. 3 of its solution."""
    from .problems import LootsmaModel as Lo
    M = TapeModel(4, 2, np.concatenate(([6.0], Lo.x0)), np.concatenate(([6.0], Lo.lvar)), np.concatenate(([6.0], Lo.uvar)),
                  Lo.lcon, Lo.ucon, name="tape_lootsma_par")
    M.add_objective(V(1) ** 3 + 11.0 * V(1) - V(0) * sqrt(V(1)) + V(2), np.array([[0, 1, 3]]))
    xyz = np.array([[1, 2, 3]])
    M.add_constraint(-sqrt(V(0)) - sqrt(V(1)) + sqrt(V(2)), np.array([0]), xyz)
    M.add_constraint(sqrt(V(0)) + sqrt(V(1)) + sqrt(V(2)), np.array([1]), xyz)
    return M.finalize()


def simplex_lp_tape_model(big=1.0, minimize=True):
    """`problems.SimplexLPModel` as patterns (the LP of the reference's `test_scaling` / `test_max_problem`); it has no
    second derivatives, so its Hessian pattern is empty."""
    from .problems import SimplexLPModel
    A = SimplexLPModel(big, minimize)
    M = TapeModel(3, 1, A.x0, A.lvar, A.uvar, A.lcon, A.ucon, name="tape_simplex_lp", minimize=minimize)
    xs = np.array([[0], [1], [2]])
    M.add_objective(P(0) * V(0), xs, A.cost[:, None])
    M.add_constraint(P(0) * V(0), np.zeros(3, dtype=np.int64), xs, np.full((3, 1), A.big))
    return M.finalize()

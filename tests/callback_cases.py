"""An independent reference for the device NLP callbacks (`madnlp_jl_amd.device_callbacks`, csrc/opf_eval.hip, nlp_scale.hip,
fixed_vars.hip); a helper module, no tests in it.  tests/test_callback_cases_cpu.py, tests/test_hip_opf_reference.py and
tests/test_hip_callbacks_reference.py use it.

  model        a `ModelRef`: every objective term and every constraint row as a list of monomials, functions of the few
               variables they touch, evaluated in mpmath at PREC bits.  Values are sums of monomials; first and second partial
               derivatives are `mpmath.diff` on each monomial (no differentiation rule is shared with the code under test; a
               monomial that does not depend on a variable has the derivative 0).  `acopf_reference` writes the monomials of
               `problems.ACOPFModel` from the model's docstring, `small_tape_model` those of a `TapeModel` built from the
               trees of tests/tape_reference.py, `qp_model_reference` states the two QP models from their matrices.
  bound        `Block.bound(u)`: an output computed with r roundings from monomials t_k is within (r + 2 u) 2^-53 sum |t_k| of
               the exact value; r is counted on the expression as the docstring of the model states it (the counts are listed
               where the monomials are built), u is the error of sin / cos in ulp (1 ulp = 2 * 2^-53) and is counted only for
               entries with a transcendental factor.  The project states <= 2 ulp for ocml and <= 1 for libm (the header comment
               of csrc/opf_eval.hip, "ocml vs libm, <= 2 ulp"; tests/test_acopf.py, "<= 2 ulp each").
  solver view  `scaled_problem`: objective sense, NLP scaling, slack / rhs tail and fixed-variable reduction composed in mpmath;
               one more rounding per applied factor.

float64 forms the angle difference d = va_f - va_t before sin / cos see it.  The reference takes the exact difference, so the
points of `acopf_points` keep every angle on a grid of 2^-40: the float64 difference is then exact (|va| < 2^12) and the bound
needs no term for it."""
import functools

import numpy as np
from mpmath import mp, mpf

PREC = 400                      # bits of the derivatives (`model_reference`); values are then kept and compared at >= 200
mp.prec = max(mp.prec, 203)     # (tests/tape_reference.py sets 60 digits, the same 203 bits: whichever module comes first)
U53 = mpf(2) ** -53
NOISE = mpf(10) ** -40          # what mpmath.diff may leave of a derivative that is exactly zero: no bit of any float64 here
U_DEVICE, U_HOST = 2, 1         # ulp of sin / cos: ocml (csrc/opf_eval.hip header), libm


def exact(a):
    """the float64 entries of `a` as mpf, exactly"""
    return [mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


# ------------------------------------------------------------------------------------------------- blocks and bounds
class Block:
    """The entries of one output: value, sum |t_k| over the entry's monomials, roundings r, and whether a transcendental factor
    is in it.  An entry that was not computed (the sampled network) is None."""

    def __init__(self):
        self.val, self.mag, self.r, self.trig = [], [], [], []

    def add(self, val, mag, r, trig=False):
        self.val.append(val)
        self.mag.append(mag)
        self.r.append(r)
        self.trig.append(bool(trig))

    def skip(self):
        self.add(None, None, 0, False)

    def __len__(self):
        return len(self.val)

    def computed(self):
        return np.array([v is not None for v in self.val], dtype=bool)

    def bound(self, u):
        return [None if m is None else (r + 2 * u * t) * U53 * m for m, r, t in zip(self.mag, self.r, self.trig)]


def entry_bound(block, u):
    """Per entry (r + 2 u) 2^-53 sum |t_k| (u only where the entry has a transcendental factor); None where not computed."""
    return block.bound(u)


def ratios(got, block, u):
    """|got - ref| / bound per computed entry (0 where both vanish, inf where a zero bound is missed), and their indices."""
    got = np.asarray(got, dtype=np.float64).ravel()
    assert len(got) == len(block), (len(got), len(block))
    idx, out = [], []
    for i, (ref, b) in enumerate(zip(block.val, block.bound(u))):
        if ref is None:
            continue
        g = float(got[i])
        if not np.isfinite(g):
            idx.append(i)
            out.append(np.inf)
            continue
        err = abs(mpf(g) - ref)
        idx.append(i)
        out.append(0.0 if err <= NOISE else float(err / b) if b > 0 else np.inf)
    return np.array(idx, dtype=np.int64), np.array(out)


def worst(got, block, u):
    """The largest |got - ref| / bound of the block (0.0 for an empty one)."""
    idx, q = ratios(got, block, u)
    return float(q.max()) if len(q) else 0.0


def assert_within(got, block, u, what=""):
    idx, q = ratios(got, block, u)
    bad = idx[q > 1.0]
    assert len(bad) == 0, (what, [(int(i), float(np.asarray(got).ravel()[i]), mp.nstr(block.val[i], 20), float(q[list(idx).index(i)]))
                                  for i in bad[:5]], len(bad))
    return float(q.max()) if len(q) else 0.0


# ------------------------------------------------------------------------------------------------- monomials
class Mono:
    """One monomial of a row: `fn(*values of vars)`; `r` = roundings on its path in (value, first-derivative entry,
    second-derivative entry times its multiplier)."""

    def __init__(self, fn, vars_, r, trig=False):
        self.fn, self.vars, self.r, self.trig = fn, tuple(int(v) for v in vars_), r, trig

    def partial(self, x, wrt):
        """the partial derivative with respect to the global variables `wrt` (0, 1 or 2 of them) at x"""
        if any(v not in self.vars for v in wrt):
            return None                                   # structurally zero: the monomial does not touch the variable
        z = tuple(x[v] for v in self.vars)
        if not wrt:
            return self.fn(*z)
        orders = [0] * len(z)
        for v in wrt:
            orders[self.vars.index(v)] += 1
        return mp.diff(self.fn, z, tuple(orders))


def _entry(monos, x, wrt, order):
    """(value, sum |t_k|, r, trig) of the derivative of a row with respect to `wrt`; None when no monomial depends on it"""
    if len(monos) == 1 and isinstance(monos[0], TapeMono):
        return _tape_entry(monos[0], x, wrt)
    vals = [(m, m.partial(x, wrt)) for m in monos]
    vals = [(m, v) for m, v in vals if v is not None]
    if not vals:
        return None
    return (mp.fsum(v for _, v in vals), mp.fsum(abs(v) for _, v in vals), max(m.r[order] for m, _ in vals),
            any(m.trig for m, _ in vals))


class ModelRef:
    """A model at one point x: `terms`, `grad`, `cons`, `jac` as blocks and, per Hessian COO entry, the second partials of the
    rows that own it (`hess_parts[e]` = list of (("y", row) or ("w", term), value, sum |t_k|, r, trig); None: not computed)."""

    def __init__(self, n, m, x, jac_I, jac_J, hess_I, hess_J):
        self.n, self.m, self.x = n, m, x
        self.jac_I, self.jac_J = np.asarray(jac_I, dtype=np.int64), np.asarray(jac_J, dtype=np.int64)
        self.hess_I, self.hess_J = np.asarray(hess_I, dtype=np.int64), np.asarray(hess_J, dtype=np.int64)
        self.terms, self.grad, self.cons, self.jac = Block(), Block(), Block(), Block()
        self.hess_parts = []

    def objective(self):
        """(value, sum |t_k|, roundings) of the sum of the terms: a term's own roundings plus one per term of the reduction"""
        k = len(self.terms)
        if k == 0:
            return mpf(0), mpf(0), 0
        return mp.fsum(self.terms.val), mp.fsum(self.terms.mag), k + max(self.terms.r)

    def lagrangian(self, y, w, y_r=None, w_r=0, keep=None):
        """The block of the Lagrangian Hessian w d2f + sum_i y_i d2c_i, COO entry by COO entry (`keep`: of these entries only).
        `y`, `w`: mpf multipliers; `y_r[i]`, `w_r`: roundings that went into the multipliers themselves (the scaling layer's
        products)."""
        out = Block()
        for parts in (self.hess_parts if keep is None else [self.hess_parts[e] for e in keep]):
            if parts is None:
                out.skip()
                continue
            val = mag = mpf(0)
            r, trig = 0, False
            for (kind, i), v, g, pr, pt in parts:
                wt, extra = (y[i], y_r[i] if y_r else 0) if kind == "y" else (w, w_r)
                val += wt * v
                mag += abs(wt) * g
                r, trig = max(r, pr + extra), trig or pt
            out.add(val, mag, r + max(len(parts) - 1, 0), trig)
        return out


# ------------------------------------------------------------------------------------------------- (a) the AC-OPF model
def _flow_monos(own, vf, vt, af, at, k):
    """c = own - T(u, w, d), T = k0 u^2 + u w (k1 cos d + k2 sin d), d = va_f - va_t (the docstring of ACOPFModel) as
    monomials over (own, u, w, va_f, va_t).  Roundings, read off  own - (k0*u*u + u*w*(k1*cs + k2*sn)):
      value       k1*cs | + | u*w | * | + | own -   = 6 for the two trigonometric monomials, k0*u | *u | + | own - = 4, own 1
      first       T_u = 2 k0 u + w (k1 cs + k2 sn): 4 (k0 monomial: 2); T_w, T_d likewise at most 4; own: the constant 1
      second      at most 4 (u w (k1 cs + k2 sn)) and the multiplier: 5; 2 k0 and the multiplier: 1"""
    k0, k1, k2 = (mpf(float(v)) for v in k)
    return [Mono(lambda o: o, (own,), (1, 0, 0)),
            Mono(lambda u: -(k0 * u * u), (vf,), (4, 2, 1)),
            Mono(lambda u, w, a, b: -(k1 * u * w * mp.cos(a - b)), (vf, vt, af, at), (6, 4, 5), True),
            Mono(lambda u, w, a, b: -(k2 * u * w * mp.sin(a - b)), (vf, vt, af, at), (6, 4, 5), True)]


def acopf_rows(model):
    """(objective terms, constraint rows, rows that own each Hessian COO entry) of `problems.ACOPFModel`, from its docstring:
    c = [va_0 | p_a - P_a | q_a - Q_a | va_f - va_t per branch | p_a^2 + q_a^2 | active balance | reactive balance],
    balance_i = pd_i + gs_i vm_i^2 + sum_{a at i} p_a - sum_{g at i} pg_g  (reactive: qd_i - bs_i vm_i^2 + sum q_a - sum qg_g)."""
    nbus, ngen, nbr, narc = model.nbus, model.ngen, model.nbr, model.narc
    va, vm, pg, qg = 0, nbus, 2 * nbus, 2 * nbus + ngen
    p, q = 2 * nbus + 2 * ngen, 2 * nbus + 2 * ngen + narc
    arc_f = np.concatenate((model.fr, model.to)).astype(np.int64)
    arc_t = np.concatenate((model.to, model.fr)).astype(np.int64)
    terms = []
    for g in range(ngen):                       # c2*pg | *pg | + c1*pg | + c0 = 4; gradient 2 c2 pg + c1 = 2; Hessian w*2*c2 = 1
        c2, c1, c0 = (mpf(float(v)) for v in model.gen_cost[g])
        terms.append([Mono(lambda t, c2=c2: c2 * t * t, (pg + g,), (4, 2, 1)), Mono(lambda t, c1=c1: c1 * t, (pg + g,), (4, 2, 1)),
                      Mono(lambda c0=c0: c0, (), (4, 2, 1))])
    rows = [[Mono(lambda t: t, (va,), (0, 0, 0))]]
    for blk, own0 in enumerate((p, q)):
        for a in range(narc):
            rows.append(_flow_monos(own0 + a, vm + arc_f[a], vm + arc_t[a], va + arc_f[a], va + arc_t[a],
                                    model.arc_coef[a, 3 * blk:3 * blk + 3]))
    for l in range(nbr):                        # one subtraction
        rows.append([Mono(lambda t: t, (va + model.fr[l],), (1, 0, 0)), Mono(lambda t: -t, (va + model.to[l],), (1, 0, 0))])
    for a in range(narc):                       # p*p | q*q | + = 2; 2 p and 2 y are exact
        rows.append([Mono(lambda t: t * t, (p + a,), (2, 0, 0)), Mono(lambda t: t * t, (q + a,), (2, 0, 0))])
    for blk, (flow0, gen0) in enumerate(((p, pg), (q, qg))):
        for i in range(nbus):
            arcs, gens = np.flatnonzero(arc_f == i), np.flatnonzero(model.gen_bus == i)
            d0, sh = mpf(float(model.bus_data[i, blk])), mpf(float(model.bus_data[i, 2 + blk])) * (-1 if blk else 1)
            # value: sh*vm | *vm | d0 + | + sa | - sg = 5; an arc term of sa: deg - 1 additions and two more; a generator
            # term of sg: ng - 1 additions and one more.  first: 2 sh vm = 1.  second: 2 sh y = 1
            rc = max(5, len(arcs) + 1, len(gens))
            rows.append([Mono(lambda d0=d0: d0, (), (rc, 0, 0)), Mono(lambda t, sh=sh: sh * t * t, (vm + i,), (rc, 1, 1))]
                        + [Mono(lambda t: t, (flow0 + a,), (rc, 0, 0)) for a in arcs]
                        + [Mono(lambda t: -t, (gen0 + g,), (rc, 0, 0)) for g in gens])
    # Hessian COO layout: [10 per p row | 10 per q row | p diag | q diag | vm diag | pg diag]
    r_th, r_pb = 1 + 2 * narc + nbr, 1 + 3 * narc + nbr
    owners = [[("y", 1 + e // 10)] for e in range(20 * narc)]
    owners += [[("y", r_th + a)] for a in range(narc)] * 2
    owners += [[("y", r_pb + i), ("y", r_pb + nbus + i)] for i in range(nbus)]
    owners += [[("w", g)] for g in range(ngen)]
    assert len(rows) == model.m and len(owners) == len(model.hess_I)
    return terms, rows, owners


def flow_rows_of(model, arcs):
    """the constraint rows of the p and q flow definitions of `arcs`"""
    return sorted({1 + blk * model.narc + int(a) for a in arcs for blk in (0, 1)})


def model_reference(n, m, x, terms, rows, owners, jac_I, jac_J, hess_I, hess_J, skip_rows=()):
    """The `ModelRef` of monomial rows at x (float64 values, taken exactly).  Rows in `skip_rows` get no reference: their
    constraint, Jacobian entries and Hessian entries are None."""
    with mp.workprec(PREC):
        return _model_reference(n, m, x, terms, rows, owners, jac_I, jac_J, hess_I, hess_J, skip_rows)


def _model_reference(n, m, x, terms, rows, owners, jac_I, jac_J, hess_I, hess_J, skip_rows):
    ref = ModelRef(n, m, exact(x), jac_I, jac_J, hess_I, hess_J)
    xs, skip = ref.x, set(int(r) for r in skip_rows)
    by_var = {}
    for t, monos in enumerate(terms):
        ref.terms.add(*_entry(monos, xs, (), 0))
        for mono in monos:
            for v in mono.vars:
                by_var.setdefault(v, set()).add(t)
    for v in range(n):
        monos = [mono for t in sorted(by_var.get(v, ())) for mono in terms[t]]
        e = _entry(monos, xs, (v,), 1) if monos else None
        ref.grad.add(*(e or (mpf(0), mpf(0), 0, False)))
    for i, monos in enumerate(rows):
        if i in skip:
            ref.cons.skip()
        else:
            ref.cons.add(*_entry(monos, xs, (), 0))
    seen = set()
    for i, j in zip(ref.jac_I.tolist(), ref.jac_J.tolist()):
        assert (i, j) not in seen, "a Jacobian position is listed twice: the row's derivative cannot be split"
        seen.add((i, j))
        if i in skip:
            ref.jac.skip()
        else:
            ref.jac.add(*(_entry(rows[i], xs, (j,), 1) or (mpf(0), mpf(0), 0, False)))
    for own, i, j in zip(owners, ref.hess_I.tolist(), ref.hess_J.tolist()):
        if any(kind == "y" and r in skip for kind, r in own):
            ref.hess_parts.append(None)
            continue
        parts = []
        for kind, r in own:
            e = _entry(rows[r] if kind == "y" else terms[r], xs, (i, j), 2) or (mpf(0), mpf(0), 0, False)
            parts.append(((kind, r),) + e)
        ref.hess_parts.append(parts)
    return ref


def acopf_model_reference(model, x, arcs=None):
    """The `ModelRef` of an ACOPFModel at x; `arcs`: the arcs whose flow rows get a reference (all by default)."""
    terms, rows, owners = acopf_rows(model)
    skip = () if arcs is None else set(range(1, 1 + 2 * model.narc)) - set(flow_rows_of(model, arcs))
    return model_reference(model.n, model.m, x, terms, rows, owners, model.jac_I, model.jac_J, model.hess_I, model.hess_J, skip)


def acopf_reference(model, x, y, w, arcs=None, ref=None):
    """Objective terms, gradient, constraints, and one value per Jacobian and Hessian COO entry of `problems.ACOPFModel` at
    (x, y, w), in the model's COO order: (terms, grad, cons, jac, hess) as blocks.  `ref`: an `acopf_model_reference` of the same
    x to reuse (the partial derivatives do not depend on y and w)."""
    ref = ref or acopf_model_reference(model, x, arcs)
    return ref.terms, ref.grad, ref.cons, ref.jac, ref.lagrangian(exact(y), mpf(float(w)))


def objective_bound(ref):
    """(value, bound) of f: (nterms + r) 2^-53 sum |terms|"""
    val, mag, r = ref.objective()
    return val, r * U53 * mag


# ------------------------------------------------------------------------------------------------- networks and points
NETWORKS = ((2, 1, 1), (3, 9, 2), (70, 20, 150))
POINTS = ("x0", "random", "bounds", "reduction")
WEIGHTS = (1.0, 0.0, 0.37)
GRID = 2.0 ** -40
SAMPLED_FIXED, SAMPLED_DRAWN = (0, 255, 256), 28


def on_grid(a):
    return np.round(np.asarray(a) / GRID) * GRID


def acopf_points(model):
    """{name: x} of the four points: the start (all d = 0); a random point with |d| <= 0.5, vm in [0.94, 1.06] and flows
    ~ N(0, 1); the same with vm alternately on its bounds and the angles spread so that |d| reaches about 3; one with
    va = 100 randn for the argument reduction.  Angles lie on the 2^-40 grid."""
    rng = np.random.default_rng(model.nbus + 1000)
    S = model.S
    x = np.array(model.x0)
    raw = rng.uniform(-1.0, 1.0, model.nbus)
    spread = np.abs(raw[model.arc_f] - raw[model.arc_t]).max()
    x[S["va"]] = on_grid(raw * 0.45 / spread)          # the largest |d| is 0.45
    x[S["vm"]] = rng.uniform(0.94, 1.06, model.nbus)
    for k in ("pg", "qg", "p", "q"):
        x[S[k]] = rng.standard_normal(len(S[k]))
    xb = x.copy()
    xb[S["vm"]] = np.where(np.arange(model.nbus) % 2 == 0, 0.94, 1.06)
    xb[S["va"]] = on_grid(raw * 3.0 / spread)          # the largest |d| is 3
    xr = x.copy()
    xr[S["va"]] = on_grid(100.0 * rng.standard_normal(model.nbus))
    return {"x0": np.array(model.x0), "random": x, "bounds": xb, "reduction": xr}


def acopf_multipliers(model):
    rng = np.random.default_rng(model.nbus + 2000)
    y = rng.standard_normal(model.m)
    y[::7] = 0.0
    return y


def sampled_arcs(model):
    """None for a network whose every entry gets the reference; on the large one the arcs 0, 255, 256, narc - 1 and 28 more
    drawn with a fixed seed."""
    if model.narc <= 64:
        return None
    fixed = set(SAMPLED_FIXED) | {model.narc - 1}
    rest = [a for a in range(model.narc) if a not in fixed]
    drawn = np.random.default_rng(28).choice(rest, SAMPLED_DRAWN, replace=False)
    return sorted(fixed | set(int(a) for a in drawn))


@functools.lru_cache(maxsize=None)
def acopf_case(network, point):
    """(model, x, y, ModelRef) of one network and point, computed once per process"""
    from madnlp_jl_amd.problems import ACOPFModel
    model = ACOPFModel(network)
    x = acopf_points(model)[point]
    return model, x, acopf_multipliers(model), acopf_model_reference(model, x, sampled_arcs(model))


# ------------------------------------------------------------------------------------------------- (c) what the solver sees
class ScaledProblem:
    """See `scaled_problem`.  Every method returns a `Block` (the objective a block of one entry) over the solver's own index
    sets: free variables then slacks, constraint rows, the kept Jacobian / Hessian COO entries."""

    def __init__(self, ref, obj_sign, obj_scale, con_scale, ind_ineq, rhs, handler):
        self.ref, self.sign, self.scale = ref, mpf(float(obj_sign)), mpf(float(obj_scale))
        self.cs = exact(np.ones(ref.m) if con_scale is None else con_scale)
        self.rhs = exact(rhs)
        self.ind_ineq = np.asarray(ind_ineq, dtype=np.int64)
        self.pos = {int(i): k for k, i in enumerate(self.ind_ineq)}
        full = handler is None
        self.free = np.arange(ref.n) if full else np.asarray(handler.free)
        self.jac_keep = np.arange(len(ref.jac_I)) if full else np.asarray(handler.ind_jac_free)
        self.hess_keep = np.arange(len(ref.hess_I)) if full else np.asarray(handler.ind_hess_free)
        col = np.full(ref.n, -1, dtype=np.int64)
        col[self.free] = np.arange(len(self.free))
        self.n, self.ns = len(self.free), len(self.ind_ineq)
        self.jac_I, self.jac_J = ref.jac_I[self.jac_keep], col[ref.jac_J[self.jac_keep]]
        self.hess_I, self.hess_J = col[ref.hess_I[self.hess_keep]], col[ref.hess_J[self.hess_keep]]
        assert (self.jac_J >= 0).all() and (self.hess_I >= 0).all() and (self.hess_J >= 0).all()
        self.f_r = int(self.scale != 1)                # a product by +-1 does not round

    def objective(self):
        val, mag, r = self.ref.objective()
        out = Block()
        out.add(self.sign * (self.scale * val), abs(self.scale) * mag, r + self.f_r)
        return out

    def grad(self):
        g, out = self.ref.grad, Block()
        for v in self.free:
            out.add(self.sign * self.scale * g.val[v], abs(self.scale) * g.mag[v], g.r[v] + self.f_r, g.trig[v])
        for _ in range(self.ns):
            out.add(mpf(0), mpf(0), 0)
        return out

    def cons(self, s):
        s, c, out = exact(s), self.ref.cons, Block()
        assert len(s) == self.ns
        for i in range(self.ref.m):
            if c.val[i] is None:
                out.skip()
                continue
            sl = s[self.pos[i]] if i in self.pos else mpf(0)
            out.add(self.cs[i] * c.val[i] - sl - self.rhs[i], abs(self.cs[i]) * c.mag[i] + abs(sl) + abs(self.rhs[i]),
                    c.r[i] + int(self.cs[i] != 1) + int(sl != 0) + int(self.rhs[i] != 0), c.trig[i])
        return out

    def jac(self):
        j, out = self.ref.jac, Block()
        for e, i in zip(self.jac_keep, self.jac_I):
            if j.val[e] is None:
                out.skip()
            else:
                out.add(self.cs[i] * j.val[e], abs(self.cs[i]) * j.mag[e], j.r[e] + int(self.cs[i] != 1), j.trig[e])
        return out

    def hess(self, y, w):
        """w obj_sign obj_scale d2f + sum_i (y_i con_scale_i) d2c_i on the kept entries; the products that form the two
        multipliers round once each where the factor is not 1"""
        ys = [a * b for a, b in zip(exact(y), self.cs)]
        return self.ref.lagrangian(ys, mpf(float(w)) * self.sign * self.scale, [int(c != 1) for c in self.cs], self.f_r,
                                   self.hess_keep)

    def jtprod(self, y):
        """J' y over the free columns: per column the sum of its Jacobian entries times y: k products and k sums on top of an entry's own roundings"""
        y, j = exact(y), self.jac()
        val, mag, cnt = [mpf(0)] * self.n, [mpf(0)] * self.n, [0] * self.n
        r, trig = [0] * self.n, [False] * self.n
        for e, (i, c) in enumerate(zip(self.jac_I, self.jac_J)):
            val[c] += j.val[e] * y[i]
            mag[c] += j.mag[e] * abs(y[i])
            cnt[c] += 1
            r[c], trig[c] = max(r[c], j.r[e]), trig[c] or j.trig[e]
        out = Block()
        for c in range(self.n):
            out.add(val[c], mag[c], r[c] + cnt[c] + 1, trig[c])
        return out


def scaled_problem(model_ref, obj_sign, obj_scale, con_scale, ind_ineq, rhs, handler=None):
    """What the solver is entitled to see of the model behind `model_ref` (a `ModelRef` at x_full, the handler's expansion with
    the fixed values taken exactly):
      F = obj_sign (obj_scale f);  grad F over the free variables, then ns zeros;  C_i = con_scale_i c_i - s[pos(i)] - rhs_i
      (no slack on a row outside `ind_ineq`);  Jacobian entry e = con_scale[row(e)] dc/dx for entries with a free column;
      Hessian entry = w obj_sign obj_scale d2f + sum_i (y_i con_scale_i) d2c_i for entries with both indices free;  J' y over
      the free columns."""
    return ScaledProblem(model_ref, obj_sign, obj_scale, con_scale, ind_ineq, rhs, handler)


# ------------------------------------------------------------------------------------------------- fixed variables, independently
def reduced_rows(terms, rows, owners, handler, x_full):
    """The monomial rows of the model over its free variables: a fixed variable becomes a constant of the monomial (its value,
    taken exactly), the others are renumbered; the owners of the kept Hessian entries.  For the statement that
    `scaled_problem(..., handler)` is the reference of `handler.model`."""
    col = np.full(handler.n_full, -1, dtype=np.int64)
    col[handler.free] = np.arange(len(handler.free))
    xs = exact(x_full)

    def reduce(mono):
        keep = [k for k, v in enumerate(mono.vars) if col[v] >= 0]
        const = {k: xs[v] for k, v in enumerate(mono.vars) if col[v] < 0}

        def fn(*z, mono=mono, keep=keep, const=const):
            full = dict(const)
            full.update(zip(keep, z))
            return mono.fn(*[full[k] for k in range(len(mono.vars))])
        return Mono(fn, [col[mono.vars[k]] for k in keep], mono.r, mono.trig)      # (a tape row: its bound stays with the full model)
    red = lambda group: [[reduce(m) for m in monos] for monos in group]  # noqa: E731
    return red(terms), red(rows), [owners[e] for e in handler.ind_hess_free]


# ------------------------------------------------------------------------------------------------- a small transcendental tape model
def _tree_lib():
    v, p = (lambda j: ("var", j)), (lambda j: ("par", j))
    mul, add, sub = (lambda a, b: ("mul", a, b)), (lambda a, b: ("add", a, b)), (lambda a, b: ("sub", a, b))
    con_a = add(mul(("sin", v(0)), ("exp", mul(p(0), v(1)))), mul(v(2), v(2)))
    con_b = add(mul(("cos", sub(v(0), v(1))), v(2)), ("log", add(mul(v(1), v(1)), ("const", 1.0))))
    obj = add(mul(("sqrt", add(mul(v(0), v(0)), ("const", 0.5))), p(0)), mul(v(1), v(1)))
    return con_a, con_b, obj


class TapeMono(Mono):
    """One pattern row of a tape model as a single monomial: the tree of tests/tape_reference.py at the row's parameters.  Its
    bound is not (r, sum |t_k|) but the first-order float64 bound `tape_reference.run_tape` carries through the compiled tape
    (functions at 2 ulp); `_entry` turns it into r = 1 and sum |t_k| = |value| + bound / 2^-53 (one more rounding, for the
    product with a multiplier or the sum that follows)."""

    def __init__(self, tree, vars_, params, tapes):
        from tests import tape_reference as TR
        self.tree, self.params, self.tapes = tree, [float(t) for t in params], tapes
        super().__init__(lambda *z: TR.evaluate(tree, list(z), [mpf(t) for t in self.params]), vars_, (1, 1, 1), False)

    def partial(self, x, wrt):
        from tests import tape_reference as TR
        if any(v not in self.vars for v in wrt):
            return None
        orders = [0] * len(self.vars)
        for v in wrt:
            orders[self.vars.index(v)] += 1
        return TR.derivative(self.tree, [x[v] for v in self.vars], self.params, orders)

    def tape_bound(self, x, wrt):
        from tests import tape_reference as TR
        tape = self.tapes[len(wrt)]
        local = sorted((self.vars.index(v) for v in wrt), reverse=True)
        outs = TR.run_tape(tape, [float(x[v]) for v in self.vars], self.params)
        for o in range(tape.nout):
            key = () if not wrt else (int(tape.out_j[o]),) if len(wrt) == 1 else (int(tape.out_j[o]), int(tape.out_l[o]))
            if sorted(key, reverse=True) == local:
                return outs[o][3]
        return mpf(0)                              # structurally zero in the compiled tape


def _tape_entry(mono, x, wrt):
    val = mono.partial(x, wrt)
    if val is None:
        return None
    return val, abs(val) + mono.tape_bound(x, wrt) / U53, 1, False


def small_tape_model(rows="mixed"):
    """About 300 variables and 200 rows of two transcendental constraint patterns (rows alternate) and one objective pattern;
    every constraint row is fed by one pattern row and every variable sits in one objective term, so no output is a sum of
    contributions.  `rows`: "mixed" (every third row an equality with a non-zero right-hand side: 0 < ns < m), "ineq", "eq".
    Returns (model, monomial terms, rows, owners)."""
    from madnlp_jl_amd import tape_model as T
    from tests import tape_reference as TR
    n, m = 300, 200
    rng = np.random.default_rng(300)
    i = np.arange(m)
    eq = {"mixed": i % 3 == 0, "ineq": np.zeros(m, dtype=bool), "eq": np.ones(m, dtype=bool)}[rows]
    lcon, ucon = np.where(eq, 0.5, -1.0), np.where(eq, 0.5, 2.0)
    x0 = on_grid(rng.uniform(0.5, 1.5, n))
    M = T.TapeModel(n, m, x0, 0.0, 2.0, lcon, ucon)
    con_a, con_b, obj = _tree_lib()
    triples = lambda R: np.stack([rng.choice(n, 3, replace=False) for _ in range(R)])  # noqa: E731
    spec = [(0, obj, None, np.arange(n).reshape(n // 2, 2), rng.uniform(0.5, 1.5, (n // 2, 1))),
            (1, con_a, np.arange(0, m, 2), triples(m // 2), rng.uniform(0.5, 1.5, (m // 2, 1))),
            (1, con_b, np.arange(1, m, 2), triples(m // 2), np.zeros((m // 2, 0)))]
    for kind, tree, rws, vi, par in spec:
        if kind == 0:
            M.add_objective(TR.to_expr(tree), vi, par)
        else:
            M.add_constraint(TR.to_expr(tree), rws, vi, par)
    M.finalize()
    terms, crows, owners = [], [None] * m, []
    assert len(M.patterns) == len(spec)
    base = 0
    for (kind, tree, rws, vi, par), pat in zip(spec, M.patterns):
        assert pat.kind == kind and np.array_equal(pat.var_index, vi)
        for r in range(pat.R):
            mono = TapeMono(tree, vi[r], par[r], pat.tapes)
            if kind == 0:
                terms.append([mono])
            else:
                crows[rws[r]] = [mono]
        t2 = pat.tapes[2]
        for o in range(t2.nout):                    # the documented COO layout: entry base + o R + r
            for r in range(pat.R):
                a, b = int(vi[r, t2.out_j[o]]), int(vi[r, t2.out_l[o]])
                e = base + o * pat.R + r
                assert {int(M.hess_I[e]), int(M.hess_J[e])} == {a, b}
                owners.append([("w", len(terms) - pat.R + r) if kind == 0 else ("y", int(rws[r]))])
        base += t2.nout * pat.R
    assert base == len(M.hess_I) and all(r is not None for r in crows)
    return M, terms, crows, owners


# ------------------------------------------------------------------------------------------------- the two QP models
def qp_model_reference(n, m, hess_I, hess_J, hv, q, jac_I, jac_J, jv, x):
    """The `ModelRef` of f = 0.5 x'Hx + q'x, c = Jx with H = Symmetric(COO, :L) and J from COO values (duplicates add), in
    exact mpmath arithmetic: the matrices ARE the derivatives.  Roundings of a float64 evaluation by products and sums:
    (H x)_i: t_i products and t_i - 1 sums, + q_i: t_i + 1; c_i: t_i; f = 0.5 x'(Hx) + q'x: the longest row, two dots of n, the
    final sum: t_max + 2 n + 3.  A Hessian entry takes one rounding for an objective weight other than 0 and 1."""
    xs, qs = exact(x), exact(q)
    hI, hJ = np.asarray(hess_I, dtype=np.int64), np.asarray(hess_J, dtype=np.int64)
    jI, jJ = np.asarray(jac_I, dtype=np.int64), np.asarray(jac_J, dtype=np.int64)
    ref = ModelRef(n, m, xs, jI, jJ, hI, hJ)
    hvs, jvs = exact(hv), exact(jv)
    g, gm, gt = list(qs), [abs(t) for t in qs], [0] * n
    f = mp.fsum(a * b for a, b in zip(qs, xs))
    fm = mp.fsum(abs(a * b) for a, b in zip(qs, xs))
    for i, j, v in zip(hI.tolist(), hJ.tolist(), hvs):
        if i == j:
            f, fm = f + v * xs[i] * xs[i] / 2, fm + abs(v * xs[i] * xs[i]) / 2
            g[i], gm[i], gt[i] = g[i] + v * xs[i], gm[i] + abs(v * xs[i]), gt[i] + 1
        else:
            f, fm = f + v * xs[i] * xs[j], fm + abs(v * xs[i] * xs[j])
            g[i], gm[i], gt[i] = g[i] + v * xs[j], gm[i] + abs(v * xs[j]), gt[i] + 1
            g[j], gm[j], gt[j] = g[j] + v * xs[i], gm[j] + abs(v * xs[i]), gt[j] + 1
    ref.terms.add(f, fm, max(gt, default=0) + 2 * n + 3)
    for i in range(n):
        ref.grad.add(g[i], gm[i], gt[i] + 1)
    c, cm, ct = [mpf(0)] * m, [mpf(0)] * m, [0] * m
    for i, j, v in zip(jI.tolist(), jJ.tolist(), jvs):
        c[i], cm[i], ct[i] = c[i] + v * xs[j], cm[i] + abs(v * xs[j]), ct[i] + 1
        ref.jac.add(v, abs(v), 0)
    for i in range(m):
        ref.cons.add(c[i], cm[i], ct[i])
    ref.hess_parts = [[(("w", 0), v, abs(v), 1, False)] for v in hvs]
    return ref

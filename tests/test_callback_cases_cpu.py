"""The reference of tests/callback_cases.py itself, without a GPU: a hand-computed two-bus network pins `acopf_reference`, the
numpy model lies within the derived bound (sin / cos at 1 ulp) on every network and point of the device test, and
`scaled_problem` reduces to the plain reference (unit factors) and to the reference of the reduced model (a handler)."""
from fractions import Fraction as Fr

import numpy as np
import pytest
from mpmath import mpf

from madnlp_jl_amd import fixed_vars as FV
from madnlp_jl_amd.problems import ACOPFModel
from tests import callback_cases as CC


def _same(ref, frac):
    """an mpf against an exact rational"""
    want = mpf(frac.numerator) / mpf(frac.denominator)
    return abs(ref - want) <= mpf(10) ** -50 * max(1, abs(want))


def _close(a, b):
    """two mpf values, or lists of them, equal to 50 digits (the references are kept at 400 bits and combined at 200)"""
    if isinstance(a, list):
        return len(a) == len(b) and all(_close(u, v) for u, v in zip(a, b))
    return (a is None and b is None) or abs(a - b) <= mpf(10) ** -50 * max(1, abs(a))


def test_two_bus_network_by_hand():
    """One branch 0 -> 1, one generator; equal angles, so d = 0, cos d = 1, sin d = 0 and T = k0 u^2 + k1 u w exactly.
    x = [va0 va1 | vm0 vm1 | pg | qg | p0 p1 | q0 q1]."""
    M = ACOPFModel((2, 1, 1))
    assert (M.fr.tolist(), M.to.tolist(), M.n, M.m) == ([0], [1], 10, 12)
    gb = int(M.gen_bus[0])
    x = np.array([0.25, 0.25, 1.0, 0.5, 1.5, -0.75, 0.5, -0.25, 2.0, 0.125])
    va0, va1, vm0, vm1, pg, qg, p0, p1, q0, q1 = (Fr(float(v)) for v in x)
    k = [[Fr(float(v)) for v in row] for row in M.arc_coef]
    pd, qd, gs, bs = ([Fr(float(v)) for v in col] for col in M.bus_data.T)
    T = lambda c, u, w: c[0] * u * u + c[1] * u * w  # noqa: E731
    want = [va0,
            p0 - T(k[0][0:3], vm0, vm1), p1 - T(k[1][0:3], vm1, vm0),
            q0 - T(k[0][3:6], vm0, vm1), q1 - T(k[1][3:6], vm1, vm0),
            va0 - va1,
            p0 * p0 + q0 * q0, p1 * p1 + q1 * q1,
            pd[0] + gs[0] * vm0 * vm0 + p0 - (pg if gb == 0 else 0), pd[1] + gs[1] * vm1 * vm1 + p1 - (pg if gb == 1 else 0),
            qd[0] - bs[0] * vm0 * vm0 + q0 - (qg if gb == 0 else 0), qd[1] - bs[1] * vm1 * vm1 + q1 - (qg if gb == 1 else 0)]
    y = np.arange(1.0, 13.0)
    terms, g, c, jv, hv = CC.acopf_reference(M, x, y, 1.0)
    assert len(c) == 12 and all(_same(r, w) for r, w in zip(c.val, want))
    # the q row of arc 1 (own end bus 1): d/d(q1, vm1, vm0, va1, va0) of q1 - (k0 u^2 + u w (k1 cos d + k2 sin d)) at d = 0
    k0, k1, k2 = k[1][3:6]
    row = 4
    entries = [e for e in range(len(M.jac_I)) if M.jac_I[e] == row]
    assert [int(M.jac_J[e]) for e in entries] == [9, 3, 2, 1, 0]
    want_j = [Fr(1), -(2 * k0 * vm1 + k1 * vm0), -(k1 * vm1), -(k2 * vm1 * vm0), k2 * vm1 * vm0]
    assert all(_same(jv.val[e], w) for e, w in zip(entries, want_j))
    # its Hessian block: -y_row times the second partials; (vm1, vm1) = 2 k0, (va1, va1) = -(k1 u w) at d = 0
    base = 10 * (2 + 1)
    pairs = [(int(M.hess_I[base + t]), int(M.hess_J[base + t])) for t in range(10)]
    assert pairs[0] == (3, 3) and pairs[5] == (1, 1)
    assert _same(hv.val[base], -Fr(float(y[row])) * 2 * k0) and _same(hv.val[base + 5], Fr(float(y[row])) * k1 * vm1 * vm0)
    # objective term and gradient
    c2, c1, c0 = (Fr(float(v)) for v in M.gen_cost[0])
    assert _same(terms.val[0], c2 * pg * pg + c1 * pg + c0) and _same(g.val[4], 2 * c2 * pg + c1)
    assert all(v == 0 for i, v in enumerate(g.val) if i != 4)


@pytest.mark.parametrize("point", CC.POINTS)
@pytest.mark.parametrize("network", CC.NETWORKS, ids=lambda t: "x".join(map(str, t)))
def test_numpy_model_is_within_the_bound(network, point):
    """The bound is attainable by a correct float64 evaluation: `ACOPFModel`'s callbacks (libm: 1 ulp) stay inside it on every
    entry that has a reference."""
    model, x, y, ref = CC.acopf_case(network, point)
    va = x[model.S["va"]]
    assert np.array_equal(va[model.arc_f] - va[model.arc_t],
                          np.array([float(ref.x[f] - ref.x[t]) for f, t in zip(model.arc_f, model.arc_t)]))   # d is exact
    d = np.abs(va[model.arc_f] - va[model.arc_t]).max()
    assert {"x0": d == 0.0, "random": 0.4 < d <= 0.5, "bounds": 2.9 < d <= 3.1, "reduction": d > 50}[point], d
    fval, fbound = CC.objective_bound(ref)
    assert abs(mpf(model.obj(x)) - fval) <= fbound
    for w in CC.WEIGHTS:
        terms, g, c, jv, hv = CC.acopf_reference(model, x, y, w, ref=ref)
        for name, got, blk in (("grad", model.grad(x), g), ("cons", model.cons(x), c), ("jac", model.jac_coord(x), jv),
                               ("hess", model.hess_coord(x, y, w), hv)):
            CC.assert_within(got, blk, CC.U_HOST, name)


def test_the_bound_tells_a_wrong_entry_from_a_right_one():
    """One ulp-scale entry off by 1e-13 of the vector's largest (what the norm-wise comparison lets pass) is outside the bound."""
    model, x, y, ref = CC.acopf_case((70, 20, 150), "random")
    terms, g, c, jv, hv = CC.acopf_reference(model, x, y, 1.0, ref=ref)
    got = model.hess_coord(x, y, 1.0)
    idx = np.flatnonzero(hv.computed())
    small = idx[np.argmin([abs(got[i]) if got[i] != 0 else np.inf for i in idx])]
    assert abs(got[small]) < 1e-3 * np.abs(got).max()
    got[small] += 1e-14 * np.abs(got).max()
    assert np.abs(got - model.hess_coord(x, y, 1.0)).max() <= 1e-13 * np.abs(got).max()
    with pytest.raises(AssertionError):
        CC.assert_within(got, hv, CC.U_HOST)


def test_scaled_problem_with_unit_factors_is_the_reference():
    model, x, y, ref = CC.acopf_case((3, 9, 2), "random")
    sp = CC.scaled_problem(ref, 1.0, 1.0, np.ones(model.m), np.zeros(0, dtype=np.int64), np.zeros(model.m))
    terms, g, c, jv, hv = CC.acopf_reference(model, x, y, 0.37, ref=ref)
    fval, fbound = CC.objective_bound(ref)
    F = sp.objective()
    assert _close(F.val[0], fval) and _close(F.bound(0)[0], fbound)
    for mine, plain in ((sp.grad(), g), (sp.cons(np.zeros(0)), c), (sp.jac(), jv), (sp.hess(y, 0.37), hv)):
        assert _close(mine.val, plain.val) and _close(mine.bound(2), plain.bound(2))
    # the tail: slacks and right-hand sides enter with their own sign, the gradient ends with ns zeros
    ind = np.array([2, 5, 11])
    s, rhs = np.array([0.5, -0.25, 2.0]), np.arange(model.m) / 8.0
    sp = CC.scaled_problem(ref, -1.0, 0.5, np.full(model.m, 0.25), ind, rhs)
    C, G = sp.cons(s), sp.grad()
    for i in range(model.m):
        sl = s[list(ind).index(i)] if i in ind else 0.0
        assert _close(C.val[i], c.val[i] / 4 - mpf(float(sl)) - mpf(float(rhs[i])))
    assert len(G) == model.n + 3 and G.val[model.n:] == [0, 0, 0] and _close(G.val[:model.n], [-v / 2 for v in g.val])
    assert _close(sp.objective().val[0], -fval / 2)
    assert _close(sp.jac().val, [v / 4 for v in jv.val])
    H = sp.hess(y, 0.37)
    plain = ref.lagrangian(CC.exact(y / 4), mpf(0.37) * mpf(-0.5))
    assert _close(H.val, plain.val)


def test_scaled_problem_with_a_handler_is_the_reference_of_the_reduced_model():
    """A tape model with the first, the last and every 7th variable fixed: the view over the free variables equals the
    reference of the monomials in which the fixed variables ARE constants, and `handler.model` lies within its bound."""
    M, terms, rows, owners = CC.small_tape_model()
    x = np.array(M.x0)
    where = np.array(sorted({0, M.n - 1} | set(range(0, M.n, 7))))
    M.lvar[where] = M.uvar[where] = x[where]
    h = FV.FixedVariableHandler.create(M, True)
    assert h.fixed.tolist() == where.tolist() and 0 < len(h.ind_jac_free) < len(M.jac_I) and 0 < len(h.ind_hess_free) < len(M.hess_I)
    keep_rows = sorted(set(range(0, M.m, 9)) | {1, M.m - 1})            # (the partial derivatives are the cost: some rows)
    skip = set(range(M.m)) - set(keep_rows)
    full = CC.model_reference(M.n, M.m, x, terms, rows, owners, M.jac_I, M.jac_J, M.hess_I, M.hess_J, skip)
    rt, rr, ro = CC.reduced_rows(terms, rows, owners, h, x)
    red = CC.model_reference(len(h.free), M.m, x[h.free], rt, rr, ro, h.jac_I, h.jac_J, h.hess_I, h.hess_J, skip)
    sp = CC.scaled_problem(full, 1.0, 1.0, None, np.zeros(0, dtype=np.int64), np.zeros(M.m), h)
    y = np.linspace(-1.0, 1.0, M.m)
    assert _close(sp.objective().val[0], red.objective()[0])
    for mine, other in ((sp.grad(), red.grad), (sp.cons(np.zeros(0)), red.cons), (sp.jac(), red.jac),
                        (sp.hess(y, 0.37), red.lagrangian(CC.exact(y), mpf(0.37)))):
        assert _close(mine.val, other.val)
    assert sp.jac().computed().sum() > 20 and sp.hess(y, 0.37).computed().sum() > 100
    R = h.model
    xr = x[h.free]
    for name, got, blk in (("grad", R.grad(xr), sp.grad()), ("cons", R.cons(xr), sp.cons(np.zeros(0))),
                           ("jac", R.jac_coord(xr), sp.jac()), ("hess", R.hess_coord(xr, y, 0.37), sp.hess(y, 0.37))):
        CC.assert_within(got, blk, CC.U_DEVICE, name)


def test_qp_reference_is_the_matrix_statement():
    """`qp_model_reference` against integers: H = [[2, 1], [1, 4]], q = (1, -1), J = [[1, 2]], x = (0.5, -0.25)."""
    ref = CC.qp_model_reference(2, 1, [0, 1, 1], [0, 0, 1], [2.0, 1.0, 4.0], [1.0, -1.0], [0, 0], [0, 1], [1.0, 2.0], [0.5, -0.25])
    assert ref.objective()[0] == mpf(0.5) * (2 * 0.25 - 2 * 0.125 + 4 * 0.0625) + 0.75
    assert ref.grad.val == [mpf(0.75) + 1, mpf(-0.5) - 1] and ref.cons.val == [mpf(0)]
    assert ref.lagrangian([mpf(3)], mpf(0.5)).val == [1, 0.5, 2]

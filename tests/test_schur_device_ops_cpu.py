"""The host-only parts of the Schur handle's device-side products (no GPU): the row lists `mnk_schur_set_structure` builds for
J, J' and Symmetric(H, :L) (`mnk_schur_spmv_plan`, csrc/schur_plan.hip) against a numpy construction, and `ordered_spmv`, the
numpy mirror of the two product kernels, against integer arithmetic on dyadic data and a longdouble product on rounded data."""
import numpy as np
import pytest

from madnlp_jl_amd.schur import OP_H, OP_J, OP_JT, spmv_plan
from madnlp_jl_amd.schur_kkt import ordered_spmv
from tests.schur_ops_cases import DEFAULT_T, INT64_MAX, U, dyadic_values, dyadic_vector, exact_spmv, pattern, row_lists

OPS = (OP_J, OP_JT, OP_H)
T_VALUES = (0, 3, 64, INT64_MAX)
# local constraint rows: an empty one, rows of exactly T and T + 1 entries for T = 3 and T = 64, of 2 * 64 and 2 * 64 + 1 entries
JAC_ROWS = [0, 3, 4, 64, 65, 128, 129, 1]
CASES = {
    # duplicates (rows longer than the nv + nd columns they may touch), both Hessian triangles, design rows of H of 3 .. 129 entries
    "general": dict(ns=3, nv=5, nd=6, nc=8, nc_eq=2, jac_rows=JAC_ROWS, hess_design_rows=[0, 3, 63, 64, 127, 126]),
    "ns1": dict(ns=1, nv=4, nd=2, nc=8, nc_eq=1, jac_rows=JAC_ROWS, hess_design_rows=[63, 64]),
    "nd1": dict(ns=2, nv=3, nd=1, nc=8, nc_eq=0, jac_rows=JAC_ROWS, hess_design_rows=[128]),
}


def plan(p, T, which, **kw):
    return spmv_plan(p["n"], p["m"], p["nv"], p["nc"], p["hess_I"], p["hess_J"], p["jac_I"], p["jac_J"], p["ind_ineq"], p["ind_eq"], T,
                     which, **kw)


@pytest.fixture(scope="module", params=sorted(CASES))
def pat(request):
    return pattern(**CASES[request.param])


def test_patterns_hold_what_the_plan_must_cope_with():
    p = pattern(**CASES["general"])
    assert (p["hess_I"] < p["hess_J"]).any() and (p["hess_I"] > p["hess_J"]).any()          # both triangles
    pairs = list(zip(p["jac_I"].tolist(), p["jac_J"].tolist()))
    assert len(set(pairs)) < len(pairs)                                                       # duplicate COO entries
    hp = list(zip(np.maximum(p["hess_I"], p["hess_J"]).tolist(), np.minimum(p["hess_I"], p["hess_J"]).tolist()))
    assert len(set(hp)) < len(hp)
    for name, want in (("general", {0, 3, 4, 64, 65, 128, 129}), ("ns1", {0, 3, 4, 64, 65, 128, 129})):
        ptr, _, _ = row_lists(pattern(**CASES[name]), OP_J)
        assert want <= set(np.diff(ptr).tolist())
    ptr, _, _ = row_lists(p, OP_H)                                                            # H: rows of T, T + 1, 128, 129 entries too
    assert {3, 4, 64, 65, 128, 129} <= set(np.diff(ptr).tolist())
    ptr, _, _ = row_lists(p, OP_JT)                                                           # J': design rows collect every scenario
    assert np.diff(ptr)[p["ns"] * p["nv"]:].min() > 64


@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("which", OPS)
def test_row_lists_equal_the_numpy_construction(pat, which, T):
    ptr, idx, perm, lng, t = plan(pat, T, which)
    wptr, widx, wperm = row_lists(pat, which)
    assert t == T
    assert np.array_equal(ptr, wptr) and np.array_equal(idx, widx) and np.array_equal(perm, wperm)
    # the long-row list: exactly the rows with more than T entries, ascending
    assert np.array_equal(lng, np.nonzero(np.diff(wptr) > T)[0])
    if T == 0:
        assert len(lng) == int((np.diff(wptr) > 0).sum())
    if T == INT64_MAX:
        assert len(lng) == 0


def test_default_threshold_and_refusals(pat):
    *_, t = plan(pat, None, OP_JT)
    assert t == DEFAULT_T
    *_, t = plan(pat, -5, OP_JT)
    assert t == DEFAULT_T
    with pytest.raises(ValueError, match="single rank"):
        plan(pat, 0, OP_J, own_design=False)
    with pytest.raises(ValueError, match="single rank"):
        plan(pat, 0, OP_J, local_scen=[0])
    with pytest.raises(ValueError, match="which"):
        plan(pat, 0, 3)
    bad = dict(pat)
    bad["jac_J"] = pat["jac_J"].copy()
    bad["jac_J"][0] = pat["n"]
    with pytest.raises(ValueError, match="Jacobian index out of range"):
        plan(bad, 0, OP_J)


def _operator_inputs(p, which, seed, dyadic):
    rng = np.random.default_rng(seed)
    if dyadic:
        hess, jac = dyadic_values(p, seed)
    else:
        hess, jac = rng.standard_normal(len(p["hess_I"])), rng.standard_normal(len(p["jac_I"]))
    k = p["m"] if which == OP_JT else p["n"]
    x = dyadic_vector(rng, k) if dyadic else rng.standard_normal(k)
    return (hess if which == OP_H else jac), x


@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("which", OPS)
def test_ordered_spmv_is_exact_on_dyadic_data(pat, which, T):
    """Every product is a multiple of 2^-4 and every row stays within the bit budget (`exact_spmv` raises otherwise: no case is
    left out), so the per-lane partials, the butterfly and the sequential sum all give the integer answer."""
    ptr, idx, perm = row_lists(pat, which)
    for seed in (1, 2):
        vals, x = _operator_inputs(pat, which, seed, True)
        want = exact_spmv(ptr, idx, perm, vals, x)
        got = ordered_spmv(ptr, idx, perm, vals, x, T)
        assert np.array_equal(got, want)
        y = dyadic_vector(np.random.default_rng(seed + 10), len(want))
        got = ordered_spmv(ptr, idx, perm, vals, x, T, 0.75, -0.5, y)
        assert np.array_equal(got, 0.75 * want - 0.5 * y)


@pytest.mark.parametrize("T", T_VALUES)
@pytest.mark.parametrize("which", OPS)
def test_ordered_spmv_on_rounded_data_stays_within_the_summation_bound(pat, which, T):
    """|got_i - ref_i| <= (t_i + 6) 2^-53 S_i against a longdouble product, S_i = sum_j |v_ij| |x_j| (the bound of
    tests/kkt_exact.py: t_i + 1 for the summation of t_i rounded products in ANY order, the rest is slack here)."""
    ptr, idx, perm = row_lists(pat, which)
    vals, x = _operator_inputs(pat, which, 3, False)
    rows = len(ptr) - 1
    rid = np.repeat(np.arange(rows), np.diff(ptr))
    t = vals[perm].astype(np.longdouble) * x[idx].astype(np.longdouble)
    ref, S = np.zeros(rows, dtype=np.longdouble), np.zeros(rows, dtype=np.longdouble)
    np.add.at(ref, rid, t)
    np.add.at(S, rid, np.abs(t))
    got = ordered_spmv(ptr, idx, perm, vals, x, T)
    assert (np.abs(got - ref) <= (np.diff(ptr) + 6) * U * S).all()

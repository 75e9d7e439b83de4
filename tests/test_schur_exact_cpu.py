"""The construction of tests/schur_exact.py, pinned on the CPU for every shape tests/test_hip_schur_exact.py runs: the
builder's exactness conditions hold, the oracle's restatement of the Schur stage (LAPACK dsytrf / dsytrs per block) returns the
constructed S and the dyadic solution bit for bit, and a plain dense solve of the assembled block-arrow matrix confirms the
construction (to 1e-9 relative: the only tolerance here, and it is not about a kernel)."""
from fractions import Fraction

import numpy as np
import pytest

from oracle.schur import SchurDenseStage as OracleStage
from tests import schur_exact as se
from tests.bk_exact import layout_kinds

# (ns, blk, nd, pivoted scenarios, positive pivots): every case of the GPU file
CASES = []
for shape in se.SHAPES:
    CASES.append((*shape, (), False))
    CASES.append((*shape, se.mixed_of(shape[0]), False))
for shape in ((4, 64, 64), (5, 129, 129)):
    CASES.append((*shape, (), True))
for piv in se.PATTERNS:
    CASES.append((*se.PATTERN_SHAPE, piv, False))
CASES.append((*se.CHUNK_STATIC, (), False))
CASES.append((*se.CHUNK_MIXED, se.CHUNK_MIXED_PIVOTED, False))
CASES = sorted(set(CASES), key=CASES.index)


def _id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-piv{''.join(map(str, c[3])) or 'none'}{'-pos' if c[4] else ''}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_conditions_hold_and_the_oracle_is_exact(case):
    ns, blk, nd, piv, pos = case
    c = se.make_schur(ns, blk, nd, piv, pos)       # raises InexactCase where a condition fails
    assert c.pivoted == tuple(piv) and [s.pivoted for s in c.scen] == [k in piv for k in range(ns)]
    for k, s in enumerate(c.scen):
        assert np.array_equal(s.A, s.A.T)
        if s.pivoted:
            assert s.case.info == 0 and not np.array_equal(s.case.perm, np.arange(blk)), f"scenario {k}: no interchange"
        else:
            assert np.all(s.case.d > 0) if pos else True
            assert s.inertia()[1] == 0
    assert np.array_equal(c.S, c.S.T) and np.array_equal(c.S0, c.S0.T)
    st = OracleStage(c.A, c.C, c.S0)
    S = st.build_local()
    assert np.array_equal(S, c.S), f"oracle S differs by {np.abs(S - c.S).max():.3e}"
    assert st.factorize(S) == (nd, 0, 0)
    for k in range(ns):
        assert st.scenario_solvers[k].inertia() == c.inertia(k), k
    rk, rd = c.bk.copy(), c.bd.copy()
    rd += st.forward(rk)
    assert np.array_equal(rd, c.rd)
    st.solve_s(rd)
    st.backward(rk, rd)
    assert np.array_equal(rk, c.xk) and np.array_equal(rd, c.xd)
    # the construction itself: b = K x for the assembled matrix
    x = c.solution()
    xs = np.linalg.solve(c.assemble(), c.rhs())
    assert np.abs(xs - x).max() <= 1e-9 * np.abs(x).max(), np.abs(xs - x).max() / np.abs(x).max()
    # the shards' contributions add up exactly
    even, odd = list(range(0, ns, 2)), list(range(1, ns, 2))
    assert np.array_equal(c.contribution(even, True) + c.contribution(odd, False), c.S)


def test_pivoted_layouts_hold_every_kind():
    """From order 17 on a pivoted scenario block holds a far partner, a 1x1 pivot off the diagonal and an in-place pair; at
    order 5 (two variants) one of each pair of kinds."""
    for blk in sorted({s[1] for s in se.SHAPES} | {se.PATTERN_SHAPE[1]}):
        kinds = [layout_kinds(se.bk_layout(blk, v)) for v in (0, 1)]
        if blk >= 16:
            assert all({"far", "onexone", "pairs"} <= k for k in kinds), (blk, kinds)
        else:
            assert kinds[0] >= {"onexone", "pairs"} and kinds[1] >= {"onexone", "far"}


def test_the_builder_refuses_what_is_not_exact():
    """A coupling entry of 1/3 has no power-of-two denominator; entries of 2^20 next to 2^-20 overflow the bound of an inner
    product.  Both are refused, neither rounded."""
    with pytest.raises(se.InexactCase):
        se.Dy.of(np.array([[1.0 / 3.0]]))
    big = se.Dy.of(np.array([[2.0 ** 20, 2.0 ** -20]]))
    with pytest.raises(se.InexactCase):
        big.dot(big.T, "overflow")
    with pytest.raises(se.InexactCase):
        se.Dy.of_fractions({(0, 0): Fraction(1, 3)}, (1, 1), "third")

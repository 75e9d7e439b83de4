"""The construction of tests/bk_exact.py, pinned on the CPU: LAPACK's dsytrf takes exactly the intended Bunch-Kaufman pivots
(ipiv, info) and returns exactly the intended L and D, an exact rational replay of dsytf2 takes the same pivots, the reference's
inertia rule gives the construction's counts, and dsytrs returns the dyadic solution exactly."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack

from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver, inertia_bk
from tests.bk_exact import exact_product, fraction_dsytf2, from_dsytrf, layout, layout_kinds, make_bk
from tests.exact_factor import blocked_ldl

ALL_KINDS = {"pairs", "far", "onexone", "zeros", "ties", "thresh", "test2"}
CASES = [(5, 0), (5, 1), (5, 2), (5, 3)] + [(n, v) for n in (63, 64, 65, 128, 129, 300, 700) for v in (0, 1)]


def _case(n, v):
    return make_bk(n, 100 * n + v, **layout(n, v))


def _dsytrf(A, blocked=True):
    """dsytrf('L') with the workspace the reference queries (blocked: dlasyf panels of 64 columns and dsytf2 on the last
    one) or with too little workspace for a panel (unblocked: dsytf2 throughout)."""
    n = A.shape[0]
    lwork = int(lapack.dsytrf_lwork(n, lower=1)[0]) if blocked else n
    ldu, ipiv, info = lapack.dsytrf(np.asfortranarray(np.tril(A)), lower=1, lwork=lwork)
    return ldu, ipiv, info


def test_small_layouts_hold_every_kind_between_them():
    kinds = set().union(*(layout_kinds(layout(5, v)) for v in range(4)))
    assert kinds >= ALL_KINDS - {"ties"}
    for n in (63, 64, 65, 128, 129, 300, 700):
        assert layout_kinds(layout(n, 0)) == ALL_KINDS, n


@pytest.mark.parametrize("n,v", CASES)
@pytest.mark.parametrize("blocked", [True, False])
def test_dsytrf_takes_the_constructed_pivots_bit_for_bit(n, v, blocked):
    """ipiv, info, P, L and D of dsytrf equal the construction's.  One exception, in the blocked path only: dlasyf leaves a
    zero column as it found it (the column is not brought up to date with the panel's earlier columns, so its stored diagonal
    and L entries are stale values); dsytf2 stores the exact zeros, as the device tier does."""
    c = _case(n, v)
    ldu, ipiv, info = _dsytrf(c.A, blocked)
    assert np.array_equal(ipiv, c.ipiv), np.flatnonzero(ipiv != c.ipiv)[:8]
    assert info == c.info
    perm, L, d, doff = from_dsytrf(ldu, ipiv)
    keep = np.ones(n, dtype=bool)
    if blocked and n > 64:
        keep[(c.ptype == 1) & (c.d == 0.0)] = False
    assert np.array_equal(perm, c.perm)
    assert np.array_equal(d[keep], c.d[keep])
    assert np.array_equal(doff, c.doff)
    assert np.array_equal(L[:, keep], c.L[:, keep])
    # P A P^T == L D L^T exactly
    D = np.diag(c.d)
    k2 = np.flatnonzero(c.ptype == 2)
    D[k2 + 1, k2] = D[k2, k2 + 1] = c.doff[k2]
    assert np.array_equal(c.A[np.ix_(c.perm, c.perm)], c.L @ D @ c.L.T)
    # the interchanges are real: far partners, 1x1 pivots off the diagonal, zero columns
    if n >= 63:
        assert np.sum(c.ipiv < 0) >= 8 and np.sum((c.ipiv > 0) & (c.ipiv != np.arange(1, n + 1))) >= 1
        assert np.sum((c.ptype == 1) & (c.d == 0.0)) >= 1


@pytest.mark.parametrize("n,v", [(5, 0), (5, 1), (5, 2), (5, 3), (63, 0), (64, 1), (65, 0)])
def test_an_exact_rational_dsytf2_takes_the_same_pivots(n, v):
    """dsytf2 restated in Fractions: the partner is the first row of the largest entry, the four tests with alpha =
    (1 + sqrt(17)) / 8.  With alpha = 1/2 the 5/8 threshold pairs become 1x1 pivots: the construction tells the two apart."""
    c = _case(n, v)
    ipiv, info = fraction_dsytf2(c.A)
    assert np.array_equal(ipiv, c.ipiv) and info == c.info
    if "thresh" in layout_kinds(layout(n, v)):
        ipiv_half, _ = fraction_dsytf2(c.A, alpha=0.5)
        assert not np.array_equal(ipiv_half, c.ipiv)


def test_a_misordered_tie_is_told_apart():
    """The pair at 14 ties with row 26 for colmax.  Stored with the tie row IN FRONT of the partner (rows 15 and 26 exchanged),
    dsytrf takes the tie row as the partner: the construction's ipiv is then wrong, and the comparison says so."""
    c = _case(63, 0)
    assert (14, 26) in layout(63, 0)["ties"]
    ldu, ipiv, info = _dsytrf(c.A)
    assert np.array_equal(ipiv, c.ipiv)
    q = np.arange(63)
    q[[15, 26]] = q[[26, 15]]
    A2 = np.asfortranarray(c.A[np.ix_(q, q)])
    _, ipiv2, _ = _dsytrf(A2)
    assert not np.array_equal(ipiv2, c.ipiv)
    # the first of the tied rows wins: the tie row, now at 15, whose own diagonal passes the third test (a 1x1 pivot on it)
    assert c.ipiv[14] == -16 and ipiv2[14] == 16
    ipiv3, _ = fraction_dsytf2(A2)
    assert np.array_equal(ipiv3[:16], ipiv2[:16])   # (further on the misordered matrix is no longer exact in fp64)


@pytest.mark.parametrize("n,v", [(5, 0), (63, 1), (64, 0), (65, 1), (300, 0), (700, 1)])
def test_reference_inertia_rule_on_singular_cases(n, v):
    """info > 0: num_zero = 1 however many zero columns there are.  With the exact zero pivot dsytf2 stores, the rule gives
    num_neg = -1 (oracle.lapack_cpu.num_neg_ev stops there), so (n, 1, -1): what the reference gets for n <= 64 (dsytrf is
    unblocked there) and what the construction's rule says at every order.  Beyond one panel the reference's blocked dsytrf
    leaves a stale diagonal in the zero column, and only info and num_zero are its own."""
    c = _case(n, v)
    assert c.info > 0 and c.inertia() == (n, 1, -1)
    if n >= 300:
        assert np.sum((c.ptype == 1) & (c.d == 0.0)) >= 2
    ref = LapackCPUSolver(np.asfortranarray(np.tril(c.A)), BUNCHKAUFMAN).factorize()
    assert ref.info == c.info and ref.inertia()[1] == 1
    if n <= 64:
        assert ref.inertia() == c.inertia()
    ldu, ipiv, info = _dsytrf(c.A, blocked=False)
    assert info == c.info and inertia_bk(ldu, ipiv, info) == c.inertia()
    assert exact_product(c.A, c.x, c.b)


@pytest.mark.parametrize("n", [65, 300])
def test_nonsingular_cases_solve_exactly(n):
    """Without zero columns dsytrs returns x* exactly; the inertia is the count of negative 1x1 pivots plus one per 2x2 block."""
    spec = layout(n, 1)
    spec["zeros"] = []
    c = make_bk(n, 7 + n, **spec)
    assert c.info == 0
    for blocked in (True, False):
        ldu, ipiv, info = _dsytrf(c.A, blocked)
        assert info == 0 and np.array_equal(ipiv, c.ipiv)
        perm, L, d, doff = from_dsytrf(ldu, ipiv)
        assert np.array_equal(L, c.L) and np.array_equal(d, c.d) and np.array_equal(doff, c.doff)
        x, sinfo = lapack.dsytrs(ldu, ipiv, c.b.copy(), lower=1)
        assert sinfo == 0 and np.array_equal(x, c.x)
    assert exact_product(c.A, c.x, c.b)
    ev = np.linalg.eigvalsh(c.A)
    assert c.inertia() == (int(np.sum(ev > 0)), 0, int(np.sum(ev < 0)))
    ref = LapackCPUSolver(np.asfortranarray(np.tril(c.A)), BUNCHKAUFMAN).factorize()
    assert ref.inertia() == c.inertia()


@pytest.mark.parametrize("n", [65, 300])
def test_growth_only_case(n):
    """2x2 blocks with beta = c / 2^12 and no interchange: the static-pivot elimination in the given order meets no zero pivot,
    its pivots change sign more than once, and its growth max|d_k| / max|a_ij| is far above 64; dsytrf takes the blocks."""
    c = make_bk(n, 11 + n, pairs=[14, 31], test2=[(17, 19, 23)], growth=12)
    assert np.array_equal(c.perm, np.arange(n))
    _, d = blocked_ldl(c.A, 1)
    assert np.all(d != 0.0)
    assert np.max(np.abs(d)) / np.max(np.abs(c.A)) > 64 * 16
    assert np.sum(np.sign(d[1:]) != np.sign(d[:-1])) >= 2
    ldu, ipiv, info = _dsytrf(c.A)
    assert info == 0 and np.array_equal(ipiv, c.ipiv) and np.sum(ipiv < 0) >= 4
    perm, L, dd, doff = from_dsytrf(ldu, ipiv)
    assert np.array_equal(L, c.L) and np.array_equal(dd, c.d) and np.array_equal(doff, c.doff)

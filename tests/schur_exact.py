"""Two-stage (block-arrow) systems whose Schur-complement stage is exact in fp64 whatever the blocking, the summation order
or the use of FMA (helper module of tests/test_schur_exact_cpu.py and tests/test_hip_schur_exact.py; not collected by pytest).

    K = [[A_1, ..., 0, C_1'], ..., [0, ..., A_ns, C_ns'], [C_1, ..., C_ns, S0]],      S = S0 - sum_k C_k A_k^-1 C_k'

Scenario blocks A_k (blk x blk): `make_exact` of tests/exact_factor.py (A = (I + N) D (I + N)', N^2 = 0, d = +-4^e: the static-
pivot tier returns these factors bit for bit) or, for a scenario listed in `pivoted`, `make_bk` of tests/bk_exact.py on a layout
with far partners, 1x1 pivots off the diagonal and in-place 2x2 pivots and without zero pivots (the static tier breaks down on
them; the pivoted tier returns P, L, D bit for bit).  Coupling blocks C_k (nd x blk): about six entries per row from
{+-1, +-1/2, +-1/4}.  Design block: S = make_exact(nd, positive=True) is chosen, S0 = S + sum_k C_k A_k^-1 C_k' follows.

A_k^-1 is never computed in floating point: with M = I - N = (I + N)^-1 it is M' D^-1 M (static) or P' M' D^-1 M P with the
2x2 inverses [[0, 1/c], [1/c, -beta/c^2]] (pivoted), accumulated entry by entry in `fractions.Fraction` from the construction.
Every entry must have a power of two as its denominator; the matrix is then held as integers times 2^-q (`Dy`) and every
further quantity (S0, b = K x, A_k^-1 C_k', C_k A_k^-1 C_k', A_k^-1 b_k, C_k (A_k^-1 b_k), A_k^-1 C_k' x_d, S x_d and, for the
static blocks, the factored form V = C_k (I - N)', V D^-1 V' the device evaluates) is formed in integer arithmetic.  Each inner
product is admitted only if  sum |terms| 2^q < 2^52  with 2^-q the unit of its terms (the product of the operands' units: never
coarser than the finest term): every partial sum in any order, fused or not, is then an integer below 2^52 units, so exact.
A case that misses a condition raises `InexactCase`; nothing is rounded."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from tests.bk_exact import BKCase, layout, make_bk
from tests.exact_factor import ExactCase, make_exact

LIMIT = 2.0 ** 52
# |d| = 4^e of the static scenario blocks and of S with e in 0..3: with pivots below 1 the assembled block-arrow matrices reach
# condition numbers of 1e9 and a plain dense solve in fp64 cannot confirm the construction to 1e-9 (1.5e-7 with e in -2..3,
# 7e-11 with these); the reciprocals 1, 1/4, 1/16, 1/64 are still all in play
EXP_A, EXP_S = (0, 3), (0, 3)
_CVALS = np.array([1.0, -1.0, 0.5, -0.5, 0.25, -0.25])


class InexactCase(AssertionError):
    """The case does not meet the conditions under which every answer is exact."""


def _require(ok, what):
    if not ok:
        raise InexactCase(what)


class Dy:
    """An exact dyadic array: m 2^-q with m int64."""

    def __init__(self, m, q):
        self.m, self.q = np.asarray(m, dtype=np.int64), int(q)

    @classmethod
    def of(cls, a, what="array"):
        a = np.asarray(a, dtype=np.float64)
        for q in range(0, 61):
            w = np.ldexp(a, q)
            if np.all(w == np.round(w)):
                _require(np.abs(w).max(initial=0.0) < LIMIT, f"{what}: entries too large at unit 2^-{q}")
                return cls(w.astype(np.int64), q)
        raise InexactCase(f"{what}: not dyadic within 2^-60")

    @classmethod
    def of_fractions(cls, F, shape, what):
        """F: {(i, j): Fraction}; every denominator a power of two."""
        q = 0
        for v in F.values():
            d = v.denominator
            _require(d & (d - 1) == 0, f"{what}: the denominator {d} is not a power of two")
            q = max(q, d.bit_length() - 1)
        m = np.zeros(shape, dtype=np.int64)
        for (i, j), v in F.items():
            w = v.numerator * (1 << (q - (v.denominator.bit_length() - 1)))
            _require(abs(w) < 2 ** 52, f"{what}: entry too large at unit 2^-{q}")
            m[i, j] = w
        return cls(m, q)

    @property
    def T(self):
        return Dy(self.m.T, self.q)

    def dot(self, other, what):
        """self @ other; every inner product checked: sum |terms| < 2^52 units."""
        bound = np.abs(self.m).astype(np.float64) @ np.abs(other.m).astype(np.float64)   # (exact below 2^53: nonnegative integers)
        worst = float(np.max(bound, initial=0.0))
        _require(worst < LIMIT, f"{what}: sum |terms| = 2^{np.log2(max(worst, 1.0)):.1f} units of 2^-{self.q + other.q}")
        return Dy(self.m @ other.m, self.q + other.q)

    @staticmethod
    def total(parts, signs, what):
        """sum_i signs[i] parts[i], the sum of every entry checked like an inner product."""
        q = max(p.q for p in parts)
        ms = []
        for p in parts:
            _require(np.abs(p.m).max(initial=0) < 2 ** (62 - (q - p.q)), f"{what}: overflow when aligning units")
            ms.append(p.m * (1 << (q - p.q)))
        bound = sum(np.abs(m).astype(np.float64) for m in ms)
        _require(float(np.max(bound, initial=0.0)) < LIMIT, f"{what}: sum |terms| reaches 2^52 units of 2^-{q}")
        return Dy(sum(s * m for s, m in zip(signs, ms)), q)

    def value(self):
        assert np.abs(self.m).max(initial=0) < 2 ** 53
        return np.ldexp(self.m.astype(np.float64), -self.q)


def _rows_of_minus_n(Nsp, n):
    """Rows of M = I - N as {column: Fraction}."""
    Nc = Nsp.tocoo()
    rows = [{i: Fraction(1)} for i in range(n)]
    for i, j, v in zip(Nc.row, Nc.col, Nc.data):
        if i != j:
            rows[int(i)][int(j)] = rows[int(i)].get(int(j), Fraction(0)) - Fraction(float(v))
    return rows


def _add_outer(F, ra, rb, w, map_=None):
    for i, a in ra.items():
        for j, b in rb.items():
            key = (i, j) if map_ is None else (int(map_[i]), int(map_[j]))
            F[key] = F.get(key, Fraction(0)) + w * a * b


def inverse_static(c: ExactCase) -> Dy:
    """A^-1 = (I - N)' D^-1 (I - N) in Fractions."""
    _require(bool(np.all(c.d != 0.0)), "static block: a zero pivot")
    rows = _rows_of_minus_n(c.Nmat, c.n)
    F = {}
    for k in range(c.n):
        _add_outer(F, rows[k], rows[k], 1 / Fraction(float(c.d[k])))
    return Dy.of_fractions(F, (c.n, c.n), "inverse of a static block")


def inverse_bk(c: BKCase) -> Dy:
    """A^-1 = P' (I - N)' D^-1 (I - N) P, the 2x2 blocks [[beta, c], [c, 0]] inverted as [[0, 1/c], [1/c, -beta/c^2]]."""
    _require(c.info == 0, "pivoted block: a zero pivot")
    n = c.n
    Lc = c.Lsp.tocoo()
    rows = [{i: Fraction(1)} for i in range(n)]
    for i, j, v in zip(Lc.row, Lc.col, Lc.data):
        if i != j:
            rows[int(i)][int(j)] = -Fraction(float(v))
    # B = P A P' in pivot order: B[i, j] = A[perm[i], perm[j]], so entry (i, j) of B^-1 is entry (perm[i], perm[j]) of A^-1
    F = {}
    k = 0
    while k < n:
        if c.ptype[k] == 1:
            _add_outer(F, rows[k], rows[k], 1 / Fraction(float(c.d[k])), c.perm)
            k += 1
        else:
            beta, cc = Fraction(float(c.d[k])), Fraction(float(c.doff[k]))
            _require(c.d[k + 1] == 0.0 and cc != 0, "pivoted block: not a [[beta, c], [c, 0]] block")
            _add_outer(F, rows[k], rows[k + 1], 1 / cc, c.perm)
            _add_outer(F, rows[k + 1], rows[k], 1 / cc, c.perm)
            _add_outer(F, rows[k + 1], rows[k + 1], -beta / (cc * cc), c.perm)
            k += 2
    F = {key: v for key, v in F.items() if v != 0}
    return Dy.of_fractions(F, (n, n), "inverse of a pivoted block")


def bk_layout(blk, v):
    """The placements of a pivoted scenario block: far partners, 1x1 pivots off the diagonal, in-place pairs; no zero pivots."""
    if blk < 16:
        # (both break the static tier at column 0; the first holds an in-place pair, the second a far pair)
        assert blk >= 5
        return [dict(onexone=[(0, 2)], pairs=[3]), dict(onexone=[(0, 3)], far=[(1, 4)])][v % 2]
    spec = layout(blk, v)
    spec["zeros"] = []
    return spec


@dataclass
class Scenario:
    """One scenario block with everything that depends on it alone."""
    case: object          # ExactCase | BKCase
    pivoted: bool
    A: np.ndarray         # blk x blk
    C: np.ndarray         # nd x blk
    Ainv: Dy
    W: Dy                 # A^-1 C'      (blk x nd)
    G: Dy                 # C A^-1 C'    (nd x nd)

    def inertia(self):
        return self.case.inertia()


def coupling(nd, blk, seed, per_row=6):
    rng = np.random.default_rng(seed)
    Cm = np.zeros((nd, blk), order="F")
    for i in range(nd):
        cols = rng.choice(blk, size=min(per_row, blk), replace=False)
        Cm[i, cols] = rng.choice(_CVALS, size=len(cols))
    return Cm


@functools.lru_cache(maxsize=None)
def scenario(blk, nd, seed, pivoted, positive=False) -> Scenario:
    """Scenario block number `seed` of the (blk, nd) family: static (`positive`: d > 0 throughout, for CHOLESKY) or pivoted."""
    if pivoted:
        case = make_bk(blk, 31 * blk + seed, **bk_layout(blk, seed))
        Ainv = inverse_bk(case)
    else:
        case = make_exact(blk, 1000 + 17 * blk + seed, positive=positive, exponents=EXP_A)
        Ainv = inverse_static(case)
    A = np.asfortranarray(case.A)
    Cm = coupling(nd, blk, 7000 + 13 * blk + nd + 101 * seed)
    Ad, Cd = Dy.of(A, "A_k"), Dy.of(Cm, "C_dk")
    # the construction's inverse IS the inverse (integer arithmetic, every inner product within the bound)
    ident = Ad.dot(Ainv, "A_k A_k^-1")
    _require(np.array_equal(ident.m, np.eye(blk, dtype=np.int64) << ident.q), "A_k^-1 from the construction is not the inverse")
    W = Ainv.dot(Cd.T, "A_k^-1 C_dk'")
    G = Cd.dot(W, "C_dk A_k^-1 C_dk'")
    _require(np.array_equal(G.m, G.m.T), "C A^-1 C' is not symmetric")
    if not pivoted:
        # the factored form of the grouped build: V = C (I - N)', X = V D^-1, P = X V'
        Mi = Dy.of(np.eye(blk) - case.Nmat.toarray(), "I - N")
        V = Cd.dot(Mi.T, "V = C_dk L^-T")
        X = Dy.of(V.value() / case.d[None, :], "X = V D^-1")
        P = X.dot(V.T, "X V'")
        _require(np.array_equal(P.value(), G.value()), "V D^-1 V' differs from C A^-1 C'")
    return Scenario(case, bool(pivoted), A, Cm, Ainv, W, G)


@dataclass
class SchurCase:
    ns: int
    blk: int
    nd: int
    pivoted: tuple            # the scenarios built for the pivoted tier
    scen: list                # Scenario
    design: ExactCase         # S and its exact factor
    S: np.ndarray             # nd x nd, the Schur complement
    S0: np.ndarray            # nd x nd, the design block
    xk: np.ndarray            # (ns, blk) dyadic solution, scenario part
    xd: np.ndarray            # (nd,)     ... design part
    bk: np.ndarray            # (ns, blk) right-hand side b = K x
    bd: np.ndarray            # (nd,)
    rd: np.ndarray            # (nd,) S x_d: the reduced design right-hand side

    @property
    def A(self):
        return [s.A for s in self.scen]

    @property
    def C(self):
        return [s.C for s in self.scen]

    def inertia(self, k):
        return self.scen[k].inertia()

    def contribution(self, own, with_s0):
        """What the build of the rank that holds the scenarios `own` returns: S0 (on the rank that owns it) minus their terms."""
        parts = ([Dy.of(self.S0, "S0")] if with_s0 else []) + [self.scen[k].G for k in own]
        if not parts:
            return np.zeros((self.nd, self.nd), order="F")
        return Dy.total(parts, ([1] if with_s0 else []) + [-1] * len(own), "a rank's contribution").value()

    def assemble(self):
        N = self.ns * self.blk + self.nd
        K = np.zeros((N, N))
        n1 = self.ns * self.blk
        for k, s in enumerate(self.scen):
            sl = slice(k * self.blk, (k + 1) * self.blk)
            K[sl, sl] = s.A
            K[n1:, sl] = s.C
            K[sl, n1:] = s.C.T
        K[n1:, n1:] = self.S0
        return K

    def rhs(self):
        return np.concatenate([self.bk.ravel(), self.bd])

    def solution(self):
        return np.concatenate([self.xk.ravel(), self.xd])


@functools.lru_cache(maxsize=None)
def make_schur(ns, blk, nd, pivoted=(), positive=False, seed=0) -> SchurCase:
    """The case of `ns` scenarios of order `blk` coupled to `nd` design variables; the scenarios in `pivoted` take the pivoted
    tier.  Scenario k is the same block in every case of one (blk, nd, positive) family.  Raises InexactCase."""
    pivoted = tuple(sorted(pivoted))
    assert all(0 <= k < ns for k in pivoted) and not (positive and pivoted)
    scen = [scenario(blk, nd, k, k in pivoted, positive and k not in pivoted) for k in range(ns)]
    design = make_exact(nd, 500 + 3 * nd + seed, positive=True, exponents=EXP_S)
    Sd = Dy.of(design.A, "S")
    S0d = Dy.total([Sd] + [s.G for s in scen], [1] * (ns + 1), "S0 = S + sum_k C A^-1 C'")
    # (the device subtracts the terms from S0 one after the other: the same terms, the same bound)
    back = Dy.total([S0d] + [s.G for s in scen], [1] + [-1] * ns, "S = S0 - sum_k C A^-1 C'")
    _require(np.array_equal(back.value(), design.A), "S0 - sum_k C A^-1 C' is not S")
    rng = np.random.default_rng(900 + 7 * ns + blk + nd + seed)
    xk = rng.integers(-4, 5, size=(ns, blk)) / 4.0
    xd = rng.integers(-4, 5, size=nd) / 4.0
    xdD = Dy.of(xd[:, None], "x_d")
    bk = np.zeros((ns, blk))
    cx, cy = [], []
    for k, s in enumerate(scen):
        Ad, Cd, xkD = Dy.of(s.A), Dy.of(s.C), Dy.of(xk[k][:, None], "x_k")
        b = Dy.total([Ad.dot(xkD, "A_k x_k"), Cd.T.dot(xdD, "C_dk' x_d")], [1, 1], "b_k")
        bk[k] = b.value().ravel()
        y = s.Ainv.dot(b, "A_k^-1 b_k")                       # forward: r_k <- A_k^-1 b_k
        wx = s.W.dot(xdD, "(A_k^-1 C_dk') x_d")              # backward, as the reference applies it
        t = s.Ainv.dot(Cd.T.dot(xdD, "C_dk' x_d"), "A_k^-1 (C_dk' x_d)")   # ... and as the device does (one more solve)
        _require(np.array_equal(t.value(), wx.value()), "the two forms of the back-substitution differ")
        _require(np.array_equal(Dy.total([y, wx], [1, -1], "x_k = y_k - W x_d").value().ravel(), xk[k]), "forward / backward do not return x_k")
        cy.append(Cd.dot(y, "C_dk (A_k^-1 b_k)"))
        cx.append(Cd.dot(xkD, "C_dk x_k"))
    bdD = Dy.total(cx + [S0d.dot(xdD, "S0 x_d")], [1] * (ns + 1), "b_d")
    rdD = Dy.total([bdD] + cy, [1] + [-1] * ns, "r_d = b_d - sum_k C_dk (A_k^-1 b_k)")
    SxD = Sd.dot(xdD, "S x_d")
    _require(np.array_equal(rdD.value(), SxD.value()), "the reduced right-hand side is not S x_d")
    # S x_d = r_d through the exact factor (I + N) D (I + N)': y = (I - N) r, z = y / d, x = (I - N)' z
    Mi = Dy.of(np.eye(nd) - design.Nmat.toarray(), "I - N of S")
    yD = Mi.dot(rdD, "L^-1 r_d")
    zD = Dy.of(yD.value() / design.d[:, None], "D^-1 L^-1 r_d")
    _require(np.array_equal(Mi.T.dot(zD, "L^-T D^-1 L^-1 r_d").value().ravel(), xd), "the factor of S does not return x_d")
    return SchurCase(ns, blk, nd, pivoted, scen, design, np.asfortranarray(design.A), np.asfortranarray(S0d.value()), xk, xd, bk,
                     bdD.value().ravel(), rdD.value().ravel())


# ------------------------------------------------------------------------------------------------ the cases of both test files
SHAPES = [(1, 5, 3), (3, 17, 65), (4, 64, 64), (5, 129, 129), (5, 200, 30), (3, 384, 100)]
# which scenarios are pivoted, ns = 5: none, all, first only, last only, alternating
PATTERNS = [(), (0, 1, 2, 3, 4), (0,), (4,), (0, 2, 4)]
PATTERN_SHAPE = (5, 40, 20)        # blkp = 48 > blk, Npb = 128, ndp = 64
CHUNK_STATIC = (35, 40, 20)        # more scenarios than the default chunk holds at least (32)
CHUNK_MIXED = (7, 40, 20)          # with MNK_SCHUR_CHUNK = 3 and CHUNK_MIXED_PIVOTED: fast = [1, 2, 4, 5] in chunks of 3 + 1
CHUNK_MIXED_PIVOTED = (0, 3, 6)


def mixed_of(ns):
    """The pivoted scenarios of the mixed variant of a stage shape: the first and every third after it."""
    return tuple(range(0, ns, 3))

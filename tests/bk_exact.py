"""Matrices whose Bunch-Kaufman factorization (dsytrf, lower) is exact in fp64 and whose pivot sequence is known in advance
(helper module of tests/test_bk_exact_cpu.py and tests/test_hip_bk_exact.py; not collected by pytest).

B = L D L^T in pivot order, A = P^T B P in storage order.  D is block diagonal: 1x1 pivots +-4^e, 2x2 pivots
[[beta, c], [c, 0]] with c = +-2^e and beta in {0, +-c/4, +-c/8} (+-5c/8 or c/2^s where asked).  L = I + N: every pivot block
is a source or a target, N is nonzero only at (target row, earlier source column), so N^2 = 0; its entries are dyadic, |l| <= 1
in the columns of 1x1 sources (<= 1/2 for the sources of kind (c)) and |l| <= 1/4 in the columns of 2x2 sources.  At step k
the Schur complement's column k is then l_ik d_k (1x1) or beta l_ik + c l_i,k+1 (2x2), so dsytf2's four tests are decided by
a wide margin, every multiplier is exact and every Schur complement entry is a short dyadic sum: any blocking, summation
order or FMA gives the same bits.  P is a product of disjoint transpositions, one per interchange:

  (a) `far` (k, r): a 2x2 pivot {k, k+1} whose partner is stored at r > k + 1; the row stored at k + 1 is a target with entries
      in earlier source columns only, and ends at r.  ipiv[k] = ipiv[k+1] = -(r+1).
  (b) `pairs` k: a 2x2 pivot in place.  ipiv[k] = ipiv[k+1] = -(k+2).
  (c) `onexone` (k, r): a source p (d = 4) stored at r, its target q (l_qp = 1/2, d_q = -1, so the stored diagonal at k is 0)
      stored at k: dsytf2 takes the 1x1 pivot a_rr.  ipiv[k] = r + 1.
  `zeros` z: a target with d = 0, an all-zero Schur column: info = first such column + 1.
  (d) `thresh` k: |beta| = 5/8 |c| (just under alpha = 0.6404: alpha = 0.5 would take a 1x1 pivot with multiplier 8/5).
      `test2` (s, j, t): l_ts = 2 (|a_ss| = colmax / 2, the first test fails) and d_j l_tj = 4 d_s (rowmax = 2 colmax: the
      second test keeps the 1x1 pivot).  `ties` (k, t): l_t,k+1 = +-1, so row t ties with the partner of the pair at k for colmax;
      idamax takes the earlier one (t lies behind the partner in storage order).

The plain form of the factor is that of the device tier (mnk_ls_bk_info / get_factor): row i of P A P^T is row perm[i] of A,
L unit lower with every interchange applied to the earlier columns too, D = diag(d) plus doff[k] at (k+1, k) of a 2x2 block."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

ALPHA = (1.0 + 17.0 ** 0.5) / 8.0   # dsytf2's alpha, as LAPACK computes it
_V1 = np.array([1.0, 0.5, 0.25])      # |l| in the columns of 1x1 sources
_VC = np.array([0.5, 0.25])           # ... of the sources of kind (c)
_V2 = np.array([0.25, 0.125])         # ... of 2x2 sources


@dataclass
class BKCase:
    n: int
    A: np.ndarray        # stored symmetric matrix, column-major, both triangles
    perm: np.ndarray     # int32: row i of P A P^T = row perm[i] of A
    Lsp: sp.csc_matrix   # unit lower L of P A P^T (plain form)
    d: np.ndarray        # diagonal of D (a 2x2 block: beta, 0)
    doff: np.ndarray     # c at the first index of a 2x2 block, 0 elsewhere
    ptype: np.ndarray    # 1: 1x1 pivot, 2 / 3: first / second index of a 2x2 block
    ipiv: np.ndarray     # dsytrf's ipiv (1-based)
    x: np.ndarray        # dyadic solution
    b: np.ndarray        # A x, exact
    pattern: tuple       # (colptr, rowval) of the structural lower triangle of A, 0-based, sorted rows

    @property
    def L(self):
        return np.asfortranarray(self.Lsp.toarray())

    @property
    def info(self):
        """dsytrf's info: 1-based first zero pivot column, 0 if none."""
        z = np.flatnonzero((self.ptype == 1) & (self.d == 0.0))
        return int(z[0]) + 1 if len(z) else 0

    def inertia(self):
        """The reference's rule for a Bunch-Kaufman factor (oracle.lapack_cpu.inertia_bk): a 2x2 block counts one positive
        and one negative; any zero pivot makes num_neg = -1 and num_zero = 1 (info > 0), num_pos the rest."""
        if self.info > 0:
            return (self.n, 1, -1)
        neg = int(np.sum((self.ptype == 1) & (self.d < 0))) + int(np.sum(self.ptype == 2))
        return (self.n - neg, 0, neg)

    def lower_csc(self, base=0):
        """(colptr, rowval, nzval) of tril(A) on the structural pattern (explicit zeros kept)."""
        colptr, rowval = self.pattern
        cols = np.repeat(np.arange(self.n), np.diff(colptr))
        nz = np.ascontiguousarray(self.A[rowval, cols])
        return (colptr + base).astype(np.int32), (rowval + base).astype(np.int32), nz


def make_bk(n, seed, *, pairs=(), far=(), onexone=(), zeros=(), ties=(), thresh=(), test2=(), beta0=(), growth=None,
            p_pair=0.15, per_row=4, positive=False, zero_beta=True):
    """The case of order n with the placements given (positions in pivot order, see the module's docstring); every other
    position is a random 1x1 pivot or, with probability p_pair, a random in-place 2x2 pivot.  beta0: 2x2 blocks (of pairs or
    far) with beta = 0.  growth = s: every other 2x2 block has beta = +-c / 2^s (the static-pivot tier's second pivot is then
    -2^s c).  zero_beta: random blocks may have beta = 0."""
    rng = np.random.default_rng(seed)
    size = np.zeros(n, dtype=np.int64)    # 1 / 2 at a block start, 0 at the second index of a pair, -1 free
    size[:] = -1
    src = np.zeros(n, dtype=bool)
    vals = np.zeros(n)                    # largest |l| of a source column
    d = np.zeros(n)
    doff = np.zeros(n)
    fixed = []                            # (row, col, value)
    limit = np.arange(n)                  # random entries of target row i only in source columns < limit[i]
    exclude = {}                          # row -> source columns that get no random entry
    role = {}                             # block start -> True (source) / False (target), where prescribed
    special_d = {}                        # 1x1 position -> d
    beta_of = {}                          # pair start -> beta / c
    perm = np.arange(n)
    ipiv = np.arange(1, n + 1, dtype=np.int64)

    def take(*ps):
        for p in ps:
            assert 0 <= p < n and size[p] == -1, f"position {p} is taken or out of range (n = {n})"

    def pair(k):
        take(k, k + 1)
        size[k], size[k + 1] = 2, 0

    def one(k):
        take(k)
        size[k] = 1

    for k in pairs:
        pair(k)
        ipiv[k] = ipiv[k + 1] = -(k + 2)
    for k, r in far:
        assert r > k + 1
        pair(k)
        one(r)
        role[r] = False
        limit[r] = k
        perm[k + 1], perm[r] = r, k + 1
        ipiv[k] = ipiv[k + 1] = -(r + 1)
    for k, r in onexone:
        assert r > k
        one(k)
        one(r)
        role[k], role[r] = True, False
        special_d[k], special_d[r] = 4.0, -1.0
        vals[k] = -1.0          # marker: the value set of kind (c)
        fixed.append((r, k, 0.5))
        limit[r] = k
        perm[k], perm[r] = r, k
        ipiv[k] = r + 1
    for z in zeros:
        one(z)
        role[z] = False
        special_d[z] = 0.0
    for k, t in ties:
        assert size[k] == 2 and t > max(k + 1, abs(ipiv[k]) - 1), "a tie needs a pair and a row behind its partner"
        one(t)
        role[k], role[t] = True, False
        fixed.append((t, k + 1, rng.choice([-1.0, 1.0])))
        exclude.setdefault(t, set()).update({k, k + 1})
    for k in thresh:
        assert size[k] == 2
        beta_of[k] = rng.choice([-1.0, 1.0]) * 0.625
    for k in beta0:
        assert size[k] == 2 and k not in beta_of
        beta_of[k] = 0.0
    for s, j, t in test2:
        assert s < j < t
        one(s)
        one(j)
        one(t)
        role[s], role[j], role[t] = True, True, False
        ds = rng.choice([-1.0, 1.0])
        special_d[s], special_d[j] = ds, 4.0 * rng.choice([-1.0, 1.0])
        fixed.append((t, s, 2.0 * rng.choice([-1.0, 1.0])))
        fixed.append((t, j, rng.choice([-1.0, 1.0])))
        exclude.setdefault(t, set()).update({s, j})
    # random fill
    k = 0
    while k < n:
        if size[k] != -1:
            k += 1
            continue
        if k + 1 < n and size[k + 1] == -1 and rng.random() < p_pair:
            pair(k)
            ipiv[k] = ipiv[k + 1] = -(k + 2)
            k += 2
        else:
            one(k)
            k += 1
    # roles, pivots
    starts = [k for k in range(n) if size[k] > 0]
    for k in starts:
        is_src = role.get(k, bool(k == 0 or rng.random() < 0.5))
        if size[k] == 1:
            src[k] = is_src
            if is_src:
                vals[k] = 0.5 if vals[k] == -1.0 else 1.0
            if k in special_d:
                d[k] = special_d[k]
            else:
                d[k] = 4.0 ** rng.integers(-1, 2) * (1.0 if positive else rng.choice([-1.0, 1.0]))
        else:
            src[k] = src[k + 1] = is_src
            vals[k] = vals[k + 1] = 0.25
            c = 2.0 ** rng.integers(-1, 3) * rng.choice([-1.0, 1.0])
            if k in beta_of:
                rb = beta_of[k]
            elif growth is not None:
                rb = rng.choice([-1.0, 1.0]) * 2.0 ** -growth
            else:
                rb = rng.choice([0.0, 0.25, -0.25, 0.125, -0.125] if zero_beta else [0.25, -0.25, 0.125, -0.125])
            d[k], d[k + 1], doff[k] = rb * c, 0.0, c
    for (r, col, v) in fixed:
        assert src[col] and not src[r], (r, col)
    # L: the fixed entries, then up to per_row random ones per target row
    rows, cols, lv = [], [], []
    for (r, col, v) in fixed:
        rows.append(r); cols.append(col); lv.append(v)
    fixed_at = {(r, col) for (r, col, _) in fixed}
    srcs = np.flatnonzero(src)
    for i in range(n):
        if src[i]:
            continue
        blk0 = i if size[i] != 0 else i - 1
        cand = srcs[srcs < min(blk0, limit[i])]
        ex = exclude.get(i, set())
        cand = np.array([j for j in cand if j not in ex and (i, j) not in fixed_at], dtype=np.int64)
        if len(cand) == 0:
            continue
        pick = rng.choice(cand, size=min(per_row, len(cand)), replace=False)
        for j in pick:
            rows.append(i); cols.append(int(j))
            lv.append(rng.choice([-1.0, 1.0]) * rng.choice(_V2 if vals[j] == 0.25 else (_VC if vals[j] == 0.5 else _V1)))
    for k, r in far:   # the displaced row must have an entry in an earlier source column
        assert any(rr == r and cc < k for rr, cc in zip(rows, cols)), f"row {r} displaced by the pair at {k} has no entry"
    Nm = sp.csc_matrix((np.array(lv, dtype=np.float64), (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64))),
                       shape=(n, n))
    Nm.sum_duplicates()
    assert (Nm @ Nm).count_nonzero() == 0
    Lsp = sp.csc_matrix(sp.identity(n, format="csc") + Nm)
    ptype = np.ones(n, dtype=np.int32)
    pk = [k for k in starts if size[k] == 2]
    ptype[pk] = 2
    ptype[np.array(pk, dtype=np.int64) + 1] = 3
    Dm = sp.diags(d, format="lil")
    for k in pk:
        Dm[k + 1, k] = Dm[k, k + 1] = doff[k]
    B = (Lsp @ sp.csc_matrix(Dm) @ Lsp.T).toarray()
    iperm = np.argsort(perm)
    A = np.asfortranarray(B[np.ix_(iperm, iperm)])
    # the structural pattern (no cancellation: |L| |D|_pattern |L|^T, zero pivots included)
    Dp = sp.identity(n, format="lil")
    for k in pk:
        Dp[k + 1, k] = Dp[k, k + 1] = 1.0
    Pat = abs(Lsp) @ sp.csc_matrix(Dp) @ abs(Lsp).T
    Pat = sp.csc_matrix(sp.tril(sp.csc_matrix(Pat)[iperm][:, iperm]))
    Pat.sort_indices()
    pattern = (Pat.indptr.astype(np.int32), Pat.indices.astype(np.int32))
    x = rng.choice([-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0], size=n)
    b = A @ x
    return BKCase(n, A, perm.astype(np.int32), Lsp, d, doff, ptype, ipiv, x, b, pattern)


def layout(n, variant=0):
    """The placements of the tests at order n: every kind of the module's docstring where it fits, 2x2 pivots on the columns
    where a panel of 63 or 64 columns ends (variant 0: 62/63 and 125/126, variant 1: 63/64 and 126/127), far partners in
    later panels and across the 256-row workgroups of the multi-workgroup panel."""
    if n < 16:
        # (each holds a kind (c) pivot or a zero column: the static-pivot tier breaks down on every one of them)
        return [dict(far=[(1, 4)], zeros=[3]),
                dict(onexone=[(0, 2)], pairs=[3]),
                dict(test2=[(0, 1, 2)], zeros=[3]),
                dict(pairs=[1], thresh=[1], onexone=[(3, 4)])][variant % 4]
    spec = dict(pairs=[], far=[], onexone=[], zeros=[], ties=[], thresh=[], test2=[])
    used = set()

    def fits(*ps):
        return all(p < n and p not in used for p in ps)

    def add(key, item, *ps):
        if fits(*ps):
            used.update(ps)
            spec[key].append(item)
            return True
        return False

    add("far", (3, 5), 3, 4, 5)
    add("onexone", (8, 11), 8, 11)
    if add("pairs", 14, 14, 15):
        add("ties", (14, 26), 26)
    add("test2", (17, 19, 23), 17, 19, 23)
    add("zeros", 29, 29)
    if add("pairs", 31, 31, 32):
        spec["thresh"].append(31)
    if add("far", (34, 40), 34, 35, 40):
        add("ties", (34, 44), 44)
    for k in ((62, 125) if variant % 2 == 0 else (63, 126)):
        add("pairs", k, k, k + 1)
    if add("far", (50, 120), 50, 51, 120):      # partner in the next panel
        spec["thresh"].append(50)
    add("onexone", (70, 140), 70, 140)
    add("far", (100, 400), 100, 101, 400)       # ... across a 256-row workgroup
    add("onexone", (150, 480), 150, 480)
    add("pairs", 255, 255, 256)
    add("far", (260, 600), 260, 261, 600)
    add("zeros", 300, 300)
    # colmax ties with the tie row in a later panel, ~100 rows behind the partner (another wave of the same workgroup in both
    # panel kernels) and ~300 rows behind it (another 256-row workgroup of the multi-workgroup panel)
    for k, t in ((130, 233), (190, 292), (205, 517)):
        if fits(k, k + 1, t):
            add("pairs", k, k, k + 1)
            add("ties", (k, t), t)
    for k, r in ((700, 1900), (1500, 3900), (n // 2, n - 2)):
        add("far", (k, r), k, k + 1, r)
    for k, r in ((800, 2200), (2000, 3990), (n // 2 + 3, n - 1)):
        add("onexone", (k, r), k, r)
    for z in (1200, n - 4):
        add("zeros", z, z)
    add("far", (n - 8, n - 6), n - 8, n - 7, n - 6)
    return spec


def layout_kinds(spec):
    """Which kinds a layout holds (for the tests' own checks)."""
    return {k for k, v in spec.items() if v}


def from_dsytrf(ldu, ipiv):
    """dsytrf's output (lower; ipiv 1-based, L with the interchanges not applied to the earlier columns) -> the plain form
    (perm, L unit lower, d, doff)."""
    n = len(ipiv)
    Lm = np.tril(np.array(ldu, dtype=np.float64), -1)
    d = np.diag(ldu).copy()
    doff = np.zeros(n)
    perm = np.arange(n)
    k = 0
    while k < n:
        if ipiv[k] > 0:
            kk, kp, step = k, ipiv[k] - 1, 1
        else:
            assert ipiv[k + 1] == ipiv[k]
            kk, kp, step = k + 1, -ipiv[k] - 1, 2
            doff[k] = Lm[k + 1, k]
            Lm[k + 1, k] = 0.0
        if kp != kk:
            Lm[[kk, kp], :k] = Lm[[kp, kk], :k]
            perm[[kk, kp]] = perm[[kp, kk]]
        k += step
    return perm.astype(np.int32), np.asfortranarray(Lm + np.eye(n)), d, doff


def fraction_dsytf2(A, alpha=ALPHA):
    """dsytf2 ('L') in exact rational arithmetic: (ipiv 1-based, info).  The four tests with `alpha` (its float value, as
    LAPACK has it), the partner = the first row of the largest |entry| (idamax), rowmax over the partner's row and column."""
    n = A.shape[0]
    al = Fraction(alpha)
    M = [[Fraction(float(A[i, j])) for j in range(n)] for i in range(n)]
    ipiv = np.zeros(n, dtype=np.int64)
    info = 0
    k = 0

    def swap(a, b):
        M[a], M[b] = M[b], M[a]
        for row in M:
            row[a], row[b] = row[b], row[a]

    while k < n:
        absakk = abs(M[k][k])
        if k + 1 < n:
            imax = max(range(k + 1, n), key=lambda i: (abs(M[i][k]), -i))
            colmax = abs(M[imax][k])
        else:
            imax, colmax = k, Fraction(0)
        kstep, kp = 1, k
        if max(absakk, colmax) == 0:
            info = info or k + 1
            ipiv[k] = k + 1
            k += 1
            continue
        if absakk < al * colmax:
            rowmax = max(abs(M[imax][j]) for j in range(k, n) if j != imax)
            if absakk >= al * colmax * (colmax / rowmax):
                kp = k
            elif abs(M[imax][imax]) >= al * rowmax:
                kp = imax
            else:
                kp, kstep = imax, 2
        kk = k + kstep - 1
        if kp != kk:
            swap(kk, kp)   # (the earlier columns too: only the trailing part is read below)
        if kstep == 1:
            p = M[k][k]
            w = [M[i][k] for i in range(n)]
            nz = [i for i in range(k + 1, n) if w[i] != 0]
            for i in nz:
                li = w[i] / p
                for j in nz:
                    M[i][j] -= li * w[j]
                M[i][k] = M[k][i] = li
            ipiv[k] = kp + 1
        else:
            p11, p21, p22 = M[k][k], M[k + 1][k], M[k + 1][k + 1]
            det = p11 * p22 - p21 * p21
            w1 = [M[i][k] for i in range(n)]
            w2 = [M[i][k + 1] for i in range(n)]
            nz = [i for i in range(k + 2, n) if w1[i] != 0 or w2[i] != 0]
            for i in nz:
                l1 = (w1[i] * p22 - w2[i] * p21) / det
                l2 = (w2[i] * p11 - w1[i] * p21) / det
                for j in nz:
                    M[i][j] -= l1 * w1[j] + l2 * w2[j]
                M[i][k], M[i][k + 1] = l1, l2
            ipiv[k] = ipiv[k + 1] = -(kp + 1)
        k += kstep
    return ipiv, info


def exact_product(A, x, b):
    """True iff b == A x exactly: A and x scaled by powers of two to integers, the product in int64."""
    def scale(v):
        for s in range(64):
            w = v * 2.0 ** s
            if np.all(w == np.round(w)):
                return s, w
        raise ValueError("not dyadic")
    sa, Ai = scale(np.asarray(A))
    sx, xi = scale(np.asarray(x))
    assert np.abs(Ai).max() * A.shape[1] * np.abs(xi).max() < 2.0 ** 62
    bi = np.asarray(b) * 2.0 ** (sa + sx)
    if not np.all(bi == np.round(bi)) or np.abs(bi).max() >= 2.0 ** 62:
        return False
    return bool(np.array_equal(Ai.astype(np.int64) @ xi.astype(np.int64), bi.astype(np.int64)))

"""Patterns, data and references for the tests of the Schur handle's device-side products (`mnk_schur_mul`, `mnk_schur_jtprod`,
`mnk_schur_mul_hess_blk`, `mnk_schur_solve_kkt`; helper module of tests/test_schur_device_ops_cpu.py and
tests/test_hip_schur_device_ops.py, not collected by pytest).

`pattern(ns, nv, nd, nc, nc_eq, jac_rows, hess_design_rows, ...)` is a two-stage layout whose row lengths are chosen entry by
entry: local constraint row i of every scenario holds `jac_rows[i]` COO entries that cycle over the scenario's own variables and
the design variables (more entries than columns: duplicates, which stay separate terms), and design variable j couples to
scenario variables through `hess_design_rows[j]` Hessian entries.  The Hessian is given with entries in BOTH triangles and with
duplicates; one local pattern serves all scenarios, as the Schur system requires.

Dyadic data (`dyadic_values`): entries of J from {+-1, +-1/2, +-2}, H small multiples of 1/4, vectors integers in [-8, 8] times
{1, 1/2, 1/4}, diagonals and bound terms powers of two -- every product chain of the four operations is a multiple of a power of two
and `exact_*` computes the answer in int64 after checking that the sum of the absolute values of the terms of every row stays
below 2^52 granules (`bit_budget`; it raises, it never rounds)."""
from __future__ import annotations

import numpy as np

INT64_MAX = 2 ** 63 - 1
DEFAULT_T = 64
THRESHOLDS = (None, 0, INT64_MAX)        # of the GPU tests: the default, every row on the wavefront path, none
_JVALS = np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])
_XMULT = np.array([1.0, 0.5, 0.25])
U = 2.0 ** -53


def pattern(ns, nv, nd, nc, nc_eq, jac_rows, hess_design_rows=None, offdiag=((1, 0), (2, 0)), dup_hess=2):
    """-> dict(n, m, ns, nv, nd, nc, hess_I, hess_J, jac_I, jac_J, ind_eq, ind_ineq), 0-based."""
    assert len(jac_rows) == nc
    n, m, off = ns * nv + nd, ns * nc, ns * nv
    jI, jJ = [], []
    for k in range(ns):
        cols = np.concatenate((np.arange(k * nv, (k + 1) * nv), np.arange(off, n)))
        for i, ln in enumerate(jac_rows):
            start = (2 * i) % len(cols)
            jI += [k * nc + i] * ln
            jJ += [int(cols[(start + q) % len(cols)]) for q in range(ln)]
    hI, hJ = list(range(n)), list(range(n))
    for k in range(ns):                                            # the same local off-diagonal pattern, some entries above the diagonal
        for t, (i, j) in enumerate(offdiag):
            if i < nv and j < nv and i != j:
                a, b = k * nv + i, k * nv + j
                hI.append(b if t % 2 else a)
                hJ.append(a if t % 2 else b)
    for j, ln in enumerate(hess_design_rows or []):               # design variable j x scenario variables, cycling (duplicates)
        for q in range(ln):
            v = (q + j) % off
            if q % 3 == 0:
                hI.append(v); hJ.append(off + j)                   # above the diagonal
            else:
                hI.append(off + j); hJ.append(v)
    if nd > 1:
        hI.append(off + nd - 1); hJ.append(off)                    # design x design
        hI.append(off); hJ.append(off + nd - 1)                    # ... and the same entry from the other triangle
    for t in range(dup_hess):                                      # duplicates at the end of the COO list: scenario 1's first
        e = n if t % 2 == 0 and len(hI) > n else 0                 # off-diagonal entry, the diagonal entry of variable 0
        hI.append(hI[e]); hJ.append(hJ[e])
    rows = np.arange(m)
    is_eq = (rows % nc) < nc_eq
    return dict(n=n, m=m, ns=ns, nv=nv, nd=nd, nc=nc, hess_I=np.array(hI, dtype=np.int64), hess_J=np.array(hJ, dtype=np.int64),
                jac_I=np.array(jI, dtype=np.int64), jac_J=np.array(jJ, dtype=np.int64), ind_eq=rows[is_eq], ind_ineq=rows[~is_eq])


def model_pattern(nlp):
    """The pattern of a `TwoStageQPModel` (diagonal Hessian)."""
    eq = np.nonzero(nlp.lcon == nlp.ucon)[0].astype(np.int64)
    ineq = np.nonzero(nlp.lcon != nlp.ucon)[0].astype(np.int64)
    return dict(n=nlp.n, m=nlp.m, ns=nlp.ns, nv=nlp.nv, nd=nlp.nd, nc=nlp.nc, hess_I=np.asarray(nlp.hess_I), hess_J=np.asarray(nlp.hess_J),
                jac_I=np.asarray(nlp.jac_I), jac_J=np.asarray(nlp.jac_J), ind_eq=eq, ind_ineq=ineq)


def row_lists(p, which):
    """The numpy construction of an operator's row list: (row, column, COO position) triples in COO order, stably sorted by row.
    which: 0 J, 1 J', 2 Symmetric(H, :L) -- every Hessian entry forced to the lower triangle and mirrored, a diagonal entry once."""
    if which in (0, 1):
        r, c = (p["jac_I"], p["jac_J"]) if which == 0 else (p["jac_J"], p["jac_I"])
        e = np.arange(len(r))
        rows = p["m"] if which == 0 else p["n"]
    else:
        i, j = np.maximum(p["hess_I"], p["hess_J"]), np.minimum(p["hess_I"], p["hess_J"])
        r, c, e = [], [], []
        for q in range(len(i)):
            r.append(i[q]); c.append(j[q]); e.append(q)
            if i[q] != j[q]:
                r.append(j[q]); c.append(i[q]); e.append(q)
        r, c, e = np.array(r, dtype=np.int64), np.array(c, dtype=np.int64), np.array(e, dtype=np.int64)
        rows = p["n"]
    o = np.argsort(r, kind="stable")
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.add.at(ptr, np.asarray(r, dtype=np.int64) + 1, 1)
    return np.cumsum(ptr), np.asarray(c)[o], np.asarray(e)[o]


def dyadic_values(p, seed):
    """(hess, jac) COO values: J from {+-1, +-1/2, +-2}, H multiples of 1/4 in [-2, 2]."""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, len(p["hess_I"])) / 4.0, rng.choice(_JVALS, len(p["jac_I"]))


def dyadic_vector(rng, k):
    """Integers in [-8, 8] times {1, 1/2, 1/4}."""
    return rng.integers(-8, 9, k) * rng.choice(_XMULT, k)


def bit_budget(terms_abs_sum, gbits):
    """Raises unless every row's sum of |terms|, in granules of 2^-gbits, stays below 2^52: then no partial sum of any order rounds."""
    worst = float(np.max(terms_abs_sum, initial=0.0)) * 2.0 ** gbits
    if not worst < 2.0 ** 52:
        raise AssertionError(f"bit budget exceeded: {worst:.3g} granules of 2^-{gbits}")


def exact_spmv(ptr, idx, perm, vals, x, vbits=2, xbits=2):
    """The row sums in integer arithmetic: vals are multiples of 2^-vbits, x of 2^-xbits."""
    vi, xi = np.rint(vals * 2 ** vbits).astype(np.int64), np.rint(x * 2 ** xbits).astype(np.int64)
    assert np.array_equal(vi / 2 ** vbits, vals) and np.array_equal(xi / 2 ** xbits, x)
    t = vi[perm] * xi[idx]
    rows = len(ptr) - 1
    rid = np.repeat(np.arange(rows), np.diff(ptr))
    out, mag = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    np.add.at(out, rid, t)
    np.add.at(mag, rid, np.abs(t))
    bit_budget(mag / 2.0 ** (vbits + xbits), vbits + xbits)
    return out / 2.0 ** (vbits + xbits)


def unreduced_matrix(p, hess, jac, reg, du_diag, ind_lb, ind_ub, l_diag, u_diag, l_lower, u_lower):
    """The matrix of `mul!` over (x, s, y, z_l, z_u) (reference src/KKT/Schur/schur.jl:1112-1139, src/IPM/kernels.jl:161-180),
    dense, entry by entry."""
    n, m, ni = p["n"], p["m"], len(p["ind_ineq"])
    nlb, nub = len(ind_lb), len(ind_ub)
    npr = n + ni
    N = npr + m + nlb + nub
    K = np.zeros((N, N))
    hi, hj = np.maximum(p["hess_I"], p["hess_J"]), np.minimum(p["hess_I"], p["hess_J"])
    for e in range(len(hi)):
        K[hi[e], hj[e]] += hess[e]
        if hi[e] != hj[e]:
            K[hj[e], hi[e]] += hess[e]
    for e in range(len(jac)):
        K[npr + p["jac_I"][e], p["jac_J"][e]] += jac[e]
        K[p["jac_J"][e], npr + p["jac_I"][e]] += jac[e]
    for q, r in enumerate(p["ind_ineq"]):
        K[n + q, npr + r] -= 1.0
        K[npr + r, n + q] -= 1.0
    K[np.arange(npr), np.arange(npr)] += reg
    K[npr + np.arange(m), npr + np.arange(m)] += du_diag
    ol, ou = npr + m, npr + m + nlb
    for i, q in enumerate(ind_lb):
        K[q, ol + i] -= 1.0
        K[ol + i, q] += l_lower[i]
        K[ol + i, ol + i] -= l_diag[i]
    for i, q in enumerate(ind_ub):
        K[q, ou + i] += 1.0
        K[ou + i, q] += u_lower[i]
        K[ou + i, ou + i] += u_diag[i]
    return K


def exact_axpby(K, x, w, alpha, beta, kbits=4, xbits=2):
    """alpha K x + beta w in int64: K a multiple of 2^-kbits, x, w of 2^-xbits, alpha, beta of 1/4."""
    Ki, xi, wi = (np.rint(a * 2 ** b).astype(np.int64) for a, b in ((K, kbits), (x, xbits), (w, xbits)))
    ai, bi = int(round(alpha * 4)), int(round(beta * 4))
    assert np.array_equal(Ki / 2 ** kbits, K) and np.array_equal(xi / 2 ** xbits, x) and np.array_equal(wi / 2 ** xbits, w)
    assert ai / 4 == alpha and bi / 4 == beta
    g = kbits + xbits + 2
    mag = abs(ai) * (np.abs(Ki) @ np.abs(xi)) + abs(bi) * np.abs(wi) * 2 ** kbits
    bit_budget(mag / 2.0 ** g, g)
    return (ai * (Ki @ xi) + bi * wi * 2 ** kbits) / 2.0 ** g

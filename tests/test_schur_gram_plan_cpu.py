"""The planner of the Schur stage's device-side assembly (csrc/schur_plan.hip), host only through mnk_debug_schur_assembly_plan:
which inequality rows keep their pair lists and which are long (more COO entries than the Gram row threshold T, duplicates
counted), how many terms the lists then hold and how much the staging operands of the long rows take.

The reference of the comparisons is the rule written out below (`expected`), not the planner.  A short inequality row with lv
recourse and ld design entries adds lv^2 terms to A_k, ld * lv to C_dk and ld^2 to S0 (the products of a recourse entry with a
design entry land in C_dk once: it is stored as nd x blk only) -- len^2 - lv * ld in all; a long row adds none."""
import ctypes as C

import numpy as np
import pytest

from madnlp_jl_amd import _lib as L
from madnlp_jl_amd.problems import random_twostage_qp

INT64_MAX = 2 ** 63 - 1
DEFAULT_T = 64
SIZES = dict(ns=3, nv=70, nd=37, nc=23, nc_eq=4)


def up(x, q):
    return -(-x // q) * q


def pattern(nlp):
    eq = np.nonzero(nlp.lcon == nlp.ucon)[0].astype(np.int64)
    ineq = np.nonzero(nlp.lcon != nlp.ucon)[0].astype(np.int64)
    return dict(n=nlp.n, m=nlp.m, ns=nlp.ns, nv=nlp.nv, nd=nlp.nd, nc=nlp.nc, hI=np.asarray(nlp.hess_I), hJ=np.asarray(nlp.hess_J),
                jI=np.asarray(nlp.jac_I), jJ=np.asarray(nlp.jac_J), ind_ineq=ineq, ind_eq=eq)


def plan(p, T, local=None, own_design=True, blk=None):
    """-> (rc, the five numbers, the error string)."""
    hI, hJ, jI, jJ = (np.ascontiguousarray(p[k], dtype=np.int32) for k in ("hI", "hJ", "jI", "jJ"))
    ii, ie = (np.ascontiguousarray(p[k], dtype=np.int64) for k in ("ind_ineq", "ind_eq"))
    ls = None if local is None else np.ascontiguousarray(local, dtype=np.int64)
    ns_local = p["ns"] if local is None else len(local)
    nc_eq = len(ie) // max(p["ns"], 1)
    out = (C.c_int64 * 5)(-1, -1, -1, -1, -1)
    rc = L.lib().mnk_debug_schur_assembly_plan(p["n"], p["m"], p["nv"], p["nc"], len(hI), hI.ctypes.data, hJ.ctypes.data, len(jI),
                                               jI.ctypes.data, jJ.ctypes.data, len(ii), ii.ctypes.data, len(ie), ie.ctypes.data, 0, p["ns"],
                                               None if ls is None else ls.ctypes.data, 1 if own_design else 0, ns_local,
                                               p["nv"] + nc_eq if blk is None else blk, p["nd"], T, out, 5)
    return rc, tuple(int(v) for v in out), L.lib().mnk_last_error_string().decode()


def row_lengths(p, local=None):
    """(lv, ld) of every inequality row of the local scenarios, COO entries counted as they come."""
    local = range(p["ns"]) if local is None else local
    off = p["ns"] * p["nv"]
    lv, ld = np.zeros(p["m"], dtype=np.int64), np.zeros(p["m"], dtype=np.int64)
    np.add.at(lv, p["jI"][p["jJ"] < off], 1)
    np.add.at(ld, p["jI"][p["jJ"] >= off], 1)
    rows = [r for r in p["ind_ineq"] if r // p["nc"] in local]
    return lv[rows], ld[rows]


def expected(p, T, local=None, own_design=True):
    """The rule.  -> (pair-list terms, long rows, staged doubles, T in force, terms the inequality rows contribute)."""
    ns, nv, nd, nc = p["ns"], p["nv"], p["nd"], p["nc"]
    local = list(range(ns)) if local is None else list(local)
    T = DEFAULT_T if T < 0 else T
    off = ns * nv
    terms = 0
    hi, hj = np.maximum(p["hI"], p["hJ"]), np.minimum(p["hI"], p["hJ"])
    for i, j in zip(hi, hj):                                   # Hessian entries: both triangles of A_k / S0, C_dk once
        if i < off and j < off:
            terms += (2 if i != j else 1) if i // nv in local else 0
        elif i >= off and j >= off:
            terms += (2 if i != j else 1) if own_design else 0
        else:
            terms += 1 if j // nv in local else 0
    eq_local = [r for r in p["ind_eq"] if r // nc in local]
    terms += len(local) * nv + len(eq_local) + (nd if own_design else 0)      # diagonal terms
    is_eq = np.zeros(p["m"], dtype=bool)
    is_eq[eq_local] = True
    sel = is_eq[p["jI"]]
    terms += 2 * int((p["jJ"][sel] < off).sum()) + int((p["jJ"][sel] >= off).sum())   # equality rows: J_E and J_E' in A_k, J_E,d' in C_dk
    lv, ld = row_lengths(p, local)
    ln = lv + ld
    short = ln <= T
    ineq_terms = int((ln[short] ** 2 - lv[short] * ld[short]).sum())
    nlong = int((~short).sum())
    assert nlong % max(len(local), 1) == 0                     # (one local pattern: the same long rows in every scenario)
    R = nlong // max(len(local), 1)
    staged = 2 * len(local) * up(R, 16) * (up(nv, 64) + up(nd, 64))
    return terms + ineq_terms, nlong, staged, T, ineq_terms


def check(p, T, **kw):
    rc, got, err = plan(p, T, **kw)
    assert rc == 0, err
    want = expected(p, T, **kw)
    assert (got[0], got[2], got[3], got[4]) == want[:4], (got, want)
    assert 0 < got[1] <= got[0]
    return got, want


@pytest.fixture(scope="module")
def dense():
    return pattern(random_twostage_qp(seed=5, **SIZES))


@pytest.fixture(scope="module")
def sparse():
    return pattern(random_twostage_qp(seed=5, density_v=0.3, density_d=0.5, **SIZES))


def with_duplicates(p, i):
    """Two COO entries of inequality row i of every scenario (one pattern for all) once more, at the end of the COO lists."""
    e = np.concatenate([np.nonzero(p["jI"] == k * p["nc"] + i)[0][[0, -1]] for k in range(p["ns"])])   # a recourse and a design entry
    q = dict(p)
    q["jI"], q["jJ"] = np.concatenate((p["jI"], p["jI"][e])), np.concatenate((p["jJ"], p["jJ"][e]))
    return q


def test_dense_rows_of_107_entries_at_the_default_never_and_zero(dense):
    lv, ld = row_lengths(dense)
    assert set(lv + ld) == {107} and len(lv) == 3 * 19
    got, want = check(dense, -1)
    assert got[2] == 57 and got[4] == DEFAULT_T and want[4] == 0            # the default takes every row to the Gram path
    assert got[3] == 2 * 3 * 32 * (128 + 64)
    got0, _ = check(dense, 0)
    assert got0[:4] == got[:4] and got0[4] == 0
    gotn, wantn = check(dense, INT64_MAX)
    assert gotn[2] == 0 and gotn[3] == 0 and gotn[4] == INT64_MAX
    assert gotn[0] - got[0] == wantn[4] == 57 * (107 ** 2 - 70 * 37)         # what the pair lists of these rows hold
    assert got[1] < gotn[1]


def test_shared_sparse_mask_at_the_median_row_length(sparse):
    lv, ld = row_lengths(sparse)
    T = int(np.median(lv + ld))
    got, want = check(sparse, T)
    assert 0 < got[2] < len(lv) and want[4] > 0                # both kinds of rows
    # a row of exactly T entries is short, one of T + 1 long
    assert got[2] == int((lv + ld > T).sum())
    check(sparse, T - 1)
    check(sparse, INT64_MAX)
    check(sparse, 0)


def test_duplicated_entries_count_towards_the_length(sparse):
    lv, ld = row_lengths(sparse)
    ln = (lv + ld)[:SIZES["nc"] - SIZES["nc_eq"]]              # scenario 1's rows (the same in every scenario)
    T = int(np.median(ln))
    base, _ = check(sparse, T)
    i_long = SIZES["nc_eq"] + int(np.nonzero(ln > T)[0][0])
    got, _ = check(with_duplicates(sparse, i_long), T)
    assert got == base                                          # the row was long already: no pairs, the same staging slots
    i_edge = SIZES["nc_eq"] + int(np.nonzero(ln == T)[0][0])    # a row of exactly T entries is short ...
    got, want = check(with_duplicates(sparse, i_edge), T)
    assert got[2] == base[2] + SIZES["ns"]                      # ... and long with two duplicates: entries are counted as they come
    assert got[0] == base[0] - SIZES["ns"] * int(T * T - lv[i_edge - SIZES["nc_eq"]] * ld[i_edge - SIZES["nc_eq"]])


def test_two_of_three_scenarios_are_local(dense, sparse):
    lv, ld = row_lengths(sparse)
    T = int(np.median(lv + ld))
    for p, t in ((dense, -1), (sparse, T), (sparse, INT64_MAX)):
        for own in (True, False):
            got, _ = check(p, t, local=[0, 2], own_design=own)
            one, _ = check(p, t, local=[1], own_design=not own)
            full, _ = check(p, t)
            assert got[2] + one[2] == full[2] and got[0] + one[0] == full[0]
            assert got[3] + one[3] == full[3]


def test_doubling_nd_grows_the_staging_linearly_and_adds_no_pairs():
    T = 64
    small = pattern(random_twostage_qp(seed=5, **SIZES))
    big = pattern(random_twostage_qp(seed=5, **dict(SIZES, nd=2 * SIZES["nd"])))
    gs, ws = check(small, T)
    gb, wb = check(big, T)
    assert ws[4] == wb[4] == 0 and gs[2] == gb[2] == 57
    assert gs[3] == 2 * 3 * 32 * (128 + 64) and gb[3] == 2 * 3 * 32 * (128 + 128)      # by the padded factor, not by its square
    # the terms that remain are the Hessian's, the diagonals' and the equality rows': linear in nd
    assert gb[0] - gs[0] == SIZES["nd"] * (1 + 1 + 3 * SIZES["nc_eq"])


def test_layout_errors_carry_the_messages_of_set_structure(dense):
    bad = dict(dense)
    e = np.nonzero((dense["jI"] == 0) & (dense["jJ"] < dense["nv"]))[0][0]
    bad["jJ"] = dense["jJ"].copy()
    bad["jJ"][e] = dense["nv"] + 1                              # c_1 reaches a variable of scenario 2
    rc, out, err = plan(bad, 0)
    assert rc < 0 and "mnk_schur_set_structure: a constraint reaches the variables of another scenario" in err
    bad = dict(dense)
    bad["ind_eq"] = dense["ind_eq"][:-1]                        # the last scenario has one equality row less ...
    bad["ind_ineq"] = np.sort(np.concatenate((dense["ind_ineq"], dense["ind_eq"][-1:])))
    rc, out, err = plan(bad, 0, blk=dense["nv"] + 4)
    assert rc < 0 and "the scenarios have different numbers of equality / inequality constraints" in err
    bad["ind_eq"] = np.concatenate((dense["ind_eq"][:-1], [dense["ind_eq"][0] + 5]))   # ... or the same number, unevenly spread
    bad["ind_ineq"] = np.setdiff1d(np.arange(dense["m"]), bad["ind_eq"])
    rc, out, err = plan(bad, 0, blk=dense["nv"] + 4)
    assert rc < 0 and "the scenarios have different numbers of equality / inequality constraints" in err
    rc, out, err = plan(dense, 0)
    assert rc == 0
    rc = L.lib().mnk_debug_schur_assembly_plan(*([0] * 5), None, None, 0, None, None, 0, None, 0, None, 0, 0, None, 1, 0, 1, 1, 0, None, 5)
    assert rc < 0

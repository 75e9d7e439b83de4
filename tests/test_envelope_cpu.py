"""The envelope of the sparse-condensed KKT matrix per 128-row tile row (csrc/ls.h: mnk_tile_envelope), which the task-DAG
bulk kernel uses to skip structurally zero tiles of L.  Host only: the symbolic analysis of a KKT handle without a device,
checked against a numpy computation from the COO patterns."""

import ctypes as C

import numpy as np
import pytest

from madnlp_jl_amd import _lib as L
from madnlp_jl_amd.problems import _opf_structure


def _numpy_first_nonzero(S):
    """First nonzero column of every row of K = H + J' Sigma J + diag (lower triangle), from the COO patterns."""
    n = S["n"]
    fnz = np.arange(n)
    hi, hj = S["hess_I"].astype(np.int64), S["hess_J"].astype(np.int64)
    r, c = np.maximum(hi, hj), np.minimum(hi, hj)
    np.minimum.at(fnz, r, c)
    con, var = S["jac_I"].astype(np.int64), S["jac_J"].astype(np.int64)
    minvar = np.full(S["m"], n)
    np.minimum.at(minvar, con, var)
    np.minimum.at(fnz, var, minvar[con])   # every pair of variables of a constraint row is an entry of J' Sigma J
    return fnz


def _numpy_tile_env(fnz, order):
    """env[I] = min over the rows of tile I of the first nonzero, / 128; rows >= order are padding (their own first nonzero)."""
    ntile = (order + 127) // 128
    f = np.arange(ntile * 128)
    f[:order] = fnz[:order]
    return f.reshape(ntile, 128).min(axis=1) // 128


def _sc_host(S):
    lib = L.lib()
    jI, jJ = S["jac_I"].astype(np.int32), S["jac_J"].astype(np.int32)
    hI, hJ = S["hess_I"].astype(np.int32), S["hess_J"].astype(np.int32)
    h = C.c_void_p()
    L.check(lib.mnk_sc_create(None, S["n"], S["m"], len(jI), jI.ctypes.data, jJ.ctypes.data, len(hI), hI.ctypes.data,
                              hJ.ctypes.data, 0, C.byref(h)), "mnk_sc_create")
    return h


def _sc_env(h, order):
    lib = L.lib()
    nt = lib.mnk_sc_debug_tile_env(h, order, None, 0)
    assert nt == (order + 127) // 128
    out = np.full(nt, -1, dtype=np.int32)
    assert lib.mnk_sc_debug_tile_env(h, order, out.ctypes.data, nt) == nt
    return out


@pytest.mark.parametrize("case", ["case30", "case118", "case1354pegase"])
def test_tile_envelope_of_a_kkt_handle(case):
    S, _ = _opf_structure(case)
    h = _sc_host(S)
    try:
        n = S["n"]
        fnz = _numpy_first_nonzero(S)
        env = _sc_env(h, n)
        np.testing.assert_array_equal(env, _numpy_tile_env(fnz, n))
        assert (env <= np.arange(len(env))).all()
        # a leading principal block (the probe's child solver): the leading part of the envelope, exactly
        for order in sorted({min(n, 256), min(n, 300), n // 2 // 256 * 256 or n, n - 1}):
            if order <= 0:
                continue
            np.testing.assert_array_equal(_sc_env(h, order), _numpy_tile_env(fnz, order))
        # bad arguments
        lib = L.lib()
        assert lib.mnk_sc_debug_tile_env(h, n + 1, None, 0) < 0
        assert lib.mnk_sc_debug_tile_env(h, 0, None, 0) < 0
    finally:
        L.lib().mnk_sc_destroy(h)


def test_case1354_envelope_has_skippable_tiles():
    """The C3 matrix: its flow rows form a staircase, so a real share of the tiles left of the diagonal is structurally zero."""
    S, _ = _opf_structure("case1354pegase")
    h = _sc_host(S)
    try:
        env = _sc_env(h, S["n"]).astype(np.int64)
        nt = len(env)
        zero_tiles = int(env.sum())          # tiles (I, J), J < env[I]
        lower = nt * (nt - 1) // 2
        assert 0.03 * lower < zero_tiles < lower
    finally:
        L.lib().mnk_sc_destroy(h)


@pytest.mark.parametrize("n,seed", [(5, 0), (300, 1), (1000, 2)])
def test_tile_envelope_of_a_lower_csc(n, seed):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for c in range(n):
        r = np.unique(np.concatenate(([c], rng.integers(c, min(n, c + 200), 3))))
        rows.append(r)
        cols.append(np.full(len(r), c))
    row, col = np.concatenate(rows), np.concatenate(cols)
    # a row without any entry left of its diagonal, a column without its diagonal
    keep = ~((col == 0) & (row == 0))
    row, col = row[keep], col[keep]
    colptr = np.zeros(n + 1, dtype=np.int32)
    np.add.at(colptr, col + 1, 1)
    colptr = np.cumsum(colptr).astype(np.int32)
    rowval = row.astype(np.int32)
    fnz = np.arange(n)
    np.minimum.at(fnz, row, col)
    nt = (n + 127) // 128
    out = np.full(nt, -1, dtype=np.int32)
    for base in (0, 1):
        cp, rv = colptr + base, rowval + base
        assert L.lib().mnk_debug_tile_env_csc(n, cp.ctypes.data, rv.ctypes.data, base, out.ctypes.data, nt) == nt
        np.testing.assert_array_equal(out, _numpy_tile_env(fnz, n))

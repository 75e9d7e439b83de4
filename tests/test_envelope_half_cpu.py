"""The half-tile envelope of a sparse source (csrc/ls.h: mnk_tile_envelope_half): the first nonzero column
per 64-row half of a tile row, in 64-column units, by which the waves of the task-DAG bulk kernel skip the k-tiles whose operand
rows are structurally zero.  Host only: the envelope against numpy (KKT handles, leading blocks, lower CSC), its relation to the
tile envelope, and the statistics envh_ksteps / envh_ksteps_skipped against a count made here from the pattern."""
import ctypes as C

import numpy as np
import pytest

from madnlp_jl_amd import _lib as L
from madnlp_jl_amd.problems import _opf_structure

BAND, FINAL, FIRST, FILL = 1, 2, 4, 8
CHUNK, BAND_TILES, TAPER0 = 64, 8, 2   # the shipped settings (dag_chunk, dag_band / 2, dag_taper0)
DEEP_TILES = 42


def _js2(ntile):
    return 0 if ntile <= DEEP_TILES else (ntile + 1) // 2


def _numpy_first_nonzero(S):
    """First nonzero column of every row of K = H + J' Sigma J + diag (lower triangle), from the COO patterns."""
    n = S["n"]
    fnz = np.arange(n)
    hi, hj = S["hess_I"].astype(np.int64), S["hess_J"].astype(np.int64)
    np.minimum.at(fnz, np.maximum(hi, hj), np.minimum(hi, hj))
    con, var = S["jac_I"].astype(np.int64), S["jac_J"].astype(np.int64)
    minvar = np.full(S["m"], n)
    np.minimum.at(minvar, con, var)
    np.minimum.at(fnz, var, minvar[con])
    return fnz


def _numpy_env(fnz, order, rows):
    """min over every `rows`-row group of the first nonzero, / rows; rows >= order are padding (their own first nonzero).  Always
    over whole 128-row tiles: rows = 64 gives two entries per tile."""
    ntile = (order + 127) // 128
    f = np.arange(ntile * 128)
    f[:order] = fnz[:order]
    return f.reshape(-1, rows).min(axis=1) // rows


def _sc_host(S):
    lib = L.lib()
    jI, jJ = S["jac_I"].astype(np.int32), S["jac_J"].astype(np.int32)
    hI, hJ = S["hess_I"].astype(np.int32), S["hess_J"].astype(np.int32)
    h = C.c_void_p()
    L.check(lib.mnk_sc_create(None, S["n"], S["m"], len(jI), jI.ctypes.data, jJ.ctypes.data, len(hI), hI.ctypes.data,
                              hJ.ctypes.data, 0, C.byref(h)), "mnk_sc_create")
    return h


def _sc_env(h, order, half):
    lib = L.lib()
    fn = lib.mnk_sc_debug_tile_envh if half else lib.mnk_sc_debug_tile_env
    nt = fn(h, order, None, 0)
    assert nt == (2 if half else 1) * ((order + 127) // 128)
    out = np.full(nt, -1, dtype=np.int32)
    assert fn(h, order, out.ctypes.data, nt) == nt
    return out.astype(np.int64)


_CACHE = {}


def _case(case):
    """(structure, first nonzeros, envh, env) of a case; computed once, never changed."""
    if case not in _CACHE:
        S, _ = _opf_structure(case)
        h = _sc_host(S)
        try:
            _CACHE[case] = (S, _numpy_first_nonzero(S), _sc_env(h, S["n"], True), _sc_env(h, S["n"], False))
        finally:
            L.lib().mnk_sc_destroy(h)
    return _CACHE[case]


@pytest.mark.parametrize("case", ["case30", "case118", "case1354pegase"])
def test_half_envelope_of_a_kkt_handle(case):
    S, fnz, envh, env = _case(case)
    n = S["n"]
    np.testing.assert_array_equal(envh, _numpy_env(fnz, n, 64))
    np.testing.assert_array_equal(env, _numpy_env(fnz, n, 128))
    np.testing.assert_array_equal(np.minimum(envh[0::2], envh[1::2]) // 2, env)
    assert (envh <= np.arange(len(envh))).all()
    # halves of padding rows only point at their own diagonal
    for hh in range(len(envh)):
        if 64 * hh >= n:
            assert envh[hh] == hh
    # a leading principal block (the probe's child solver) uses the leading part: exact where the block ends on a half's boundary,
    # never right of the block's own envelope otherwise (the parent's rows can only lower a minimum)
    h = _sc_host(S)
    try:
        for order in sorted({min(n, 256), min(n, 320), min(n, 300), n // 2 // 256 * 256 or n, n - 1}):
            if order <= 0:
                continue
            got, want = _sc_env(h, order, True), _numpy_env(fnz, order, 64)
            np.testing.assert_array_equal(got, envh[: len(got)])
            full = order // 64                      # halves without padding rows
            np.testing.assert_array_equal(got[:full], want[:full])
            assert (got <= want).all()
        lib = L.lib()
        assert lib.mnk_sc_debug_tile_envh(h, n + 1, None, 0) < 0
        assert lib.mnk_sc_debug_tile_envh(h, 0, None, 0) < 0
    finally:
        L.lib().mnk_sc_destroy(h)


def test_case1354_last_tile_row():
    """N = 11 192 = 87 * 128 + 56: the lower half of the last tile row is padding only."""
    S, fnz, envh, env = _case("case1354pegase")
    assert S["n"] == 11192 and len(envh) == 176
    assert envh[175] == 175 and envh[174] < 174


@pytest.mark.parametrize("case", ["case30", "case118", "case1354pegase"])
def test_half_envelope_of_the_csc_path(case):
    """The condensed pattern of the case as a lower CSC matrix (what mnk_ls_factorize_csc walks): the same envelope."""
    S, fnz, envh, env = _case(case)
    n = S["n"]
    h = _sc_host(S)
    try:
        lib = L.lib()
        nnz = C.c_int64(0)
        L.check(lib.mnk_sc_sizes(h, None, None, C.byref(nnz), None), "mnk_sc_sizes")
        colptr = np.zeros(n + 1, dtype=np.int32)
        rowval = np.zeros(nnz.value, dtype=np.int32)
        L.check(lib.mnk_sc_get_structure(h, 2, colptr.ctypes.data, rowval.ctypes.data), "mnk_sc_get_structure")
    finally:
        L.lib().mnk_sc_destroy(h)
    base0 = int(colptr[0])
    out = np.full(len(envh), -1, dtype=np.int32)
    out1 = np.full(len(env), -1, dtype=np.int32)
    for base in (0, 1):
        cp, rv = colptr - base0 + base, rowval - base0 + base
        assert lib.mnk_debug_tile_envh_csc(n, cp.ctypes.data, rv.ctypes.data, base, out.ctypes.data, len(out)) == len(out)
        np.testing.assert_array_equal(out, envh)
        assert lib.mnk_debug_tile_env_csc(n, cp.ctypes.data, rv.ctypes.data, base, out1.ctypes.data, len(out1)) == len(out1)
        np.testing.assert_array_equal(np.minimum(out[0::2], out[1::2]) // 2, out1)


@pytest.mark.parametrize("n,seed", [(5, 0), (300, 1), (1000, 2)])
def test_half_envelope_of_a_random_lower_csc(n, seed):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for c in range(n):
        r = np.unique(np.concatenate(([c], rng.integers(c, min(n, c + 200), 3))))
        rows.append(r)
        cols.append(np.full(len(r), c))
    row, col = np.concatenate(rows), np.concatenate(cols)
    keep = ~((col == 0) & (row == 0))
    row, col = row[keep], col[keep]
    colptr = np.zeros(n + 1, dtype=np.int32)
    np.add.at(colptr, col + 1, 1)
    colptr = np.cumsum(colptr).astype(np.int32)
    rowval = row.astype(np.int32)
    fnz = np.arange(n)
    np.minimum.at(fnz, row, col)
    nh = 2 * ((n + 127) // 128)
    out = np.full(nh, -1, dtype=np.int32)
    for base in (0, 1):
        cp, rv = colptr + base, rowval + base
        assert L.lib().mnk_debug_tile_envh_csc(n, cp.ctypes.data, rv.ctypes.data, base, out.ctypes.data, nh) == nh
        np.testing.assert_array_equal(out, _numpy_env(fnz, n, 64))


def _task_list(ntile):
    cap = 400000
    tasks = np.zeros(4 * cap, dtype=np.int32)
    n1 = C.c_int(0)
    n = L.lib().mnk_debug_dag_tasks(ntile, CHUNK, BAND_TILES, _js2(ntile), TAPER0, tasks.ctypes.data, cap, C.byref(n1))
    assert 0 < n <= cap
    return tasks[: 4 * n].reshape(n, 4).astype(np.int64)


def test_c3_skipped_half_ksteps_against_numpy():
    """C3 (case1354pegase, 88 tiles): the statistics against a count made here, half-column by half-column, from the pattern's
    envelope and the task list.  A quadrant (r, c) of a chunk of tile (I, J) meets a structural zero in every product of the
    64-column half-steps left of max(envh[2I + r], envh[2J + c]); the upper quadrant of a diagonal tile is never needed."""
    S, fnz, envh_lib, env_lib = _case("case1354pegase")
    n = S["n"]
    envh, env = _numpy_env(fnz, n, 64), _numpy_env(fnz, n, 128)
    ntile = len(env)
    t = _task_list(ntile)
    total = skipped = 0
    for flags, I, J, kk in zip(t[:, 0] & 255, t[:, 1], t[:, 2], t[:, 3]):
        kb, ke = int(kk) & 0xffff, int(kk) >> 16
        closing = bool(flags & FINAL) and not (flags & BAND)
        if closing and J < env[I]:
            continue                                    # a structurally zero tile is closed without its K-step
        halfsteps = np.arange(2 * kb, 2 * ke)           # the 64-column half-steps of the task
        run = halfsteps[halfsteps // 2 >= max(env[I], env[J])]   # ... that the tile envelope leaves
        total += 4 * len(run)
        if closing:
            continue
        for r in (0, 1):
            for c in (0, 1):
                if I == J and (r, c) == (0, 1):
                    skipped += len(run)
                else:
                    skipped += int((run < max(envh[2 * I + r], envh[2 * J + c])).sum())
    cnt = np.zeros(2, dtype=np.int64)
    env32, envh32 = env_lib.astype(np.int32), envh_lib.astype(np.int32)
    assert L.lib().mnk_debug_envh_ksteps(ntile, CHUNK, BAND_TILES, _js2(ntile), TAPER0, env32.ctypes.data, envh32.ctypes.data,
                                         cnt.ctypes.data) == len(t)
    print(f"C3: {cnt[0]} half-tile k-steps behind the tile envelope, {cnt[1]} of them skipped ({100.0 * cnt[1] / cnt[0]:.2f} %)")
    assert (int(cnt[0]), int(cnt[1])) == (total, skipped)
    assert 0.02 * total < skipped < 0.2 * total
    # without the half-tile envelope nothing is skipped; without any envelope the total is the nominal one
    assert L.lib().mnk_debug_envh_ksteps(ntile, CHUNK, BAND_TILES, _js2(ntile), TAPER0, env32.ctypes.data, None, cnt.ctypes.data) == len(t)
    assert (int(cnt[0]), int(cnt[1])) == (total, 0)
    assert L.lib().mnk_debug_envh_ksteps(ntile, CHUNK, BAND_TILES, _js2(ntile), TAPER0, None, None, cnt.ctypes.data) == len(t)
    assert int(cnt[0]) == 8 * int(((t[:, 3] >> 16) - (t[:, 3] & 0xffff))[(t[:, 0] & FILL) == 0].sum()) and cnt[1] == 0

"""The pivoted Bunch-Kaufman tier (csrc/bk.hip) against matrices whose dsytrf factorization is known exactly (-m gpu).

tests/bk_exact.py builds A = P^T L D L^T P with 1x1 and 2x2 pivots, far partners, 1x1 pivots off the diagonal, zero columns,
threshold and tie cases, all exact in fp64 whatever the blocking; tests/test_bk_exact_cpu.py pins it against LAPACK's dsytrf
and an exact dsytf2.  Here the device tier must return those bits: perm, doff, D and L equal, info and the inertia of the
reference's rule, and the dyadic solution x* of A x* = b, through every panel kind, matrix source, solve and batch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import madnlp_jl_amd as mj
from tests.bk_exact import layout, make_bk
from tests.exact_factor import make_exact, scalar_ldl

pytestmark = pytest.mark.gpu

SIZES = [5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 1000, 2100, 4000]
# (bk_panel_wgs, bk_max_wgs): a workgroup per 256 rows, one workgroup per panel, multi-workgroup panels capped at 2
PANELS = [(0, 0), (1, 0), (0, 2)]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=8)
def _case(n, v):
    return make_bk(n, 100 * n + v, **layout(n, v))


def _variants(n):
    return (0, 1, 2, 3) if n < 16 else (n % 2,)


def _solver(ctx, A, wgs=0, cap=0):
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    M.set_option("bk_panel_wgs", wgs)
    M.set_option("bk_max_wgs", cap)
    return M


def _check_factor(M, c, tag, count=None):
    """perm, doff, D, L of the device factor equal the construction's; info and inertia too."""
    active, cnt, perm, doff = M.bk_info()
    assert active, tag + ": the pivoted tier was not taken"
    if count is not None:
        assert cnt == count, tag + f": bk count {cnt}"
    bad = np.flatnonzero(perm != c.perm)
    assert len(bad) == 0, tag + f": perm differs at {bad[:6]}: {perm[bad[:6]]} != {c.perm[bad[:6]]}"
    bad = np.flatnonzero(doff != c.doff)
    assert len(bad) == 0, tag + f": doff differs at {bad[:6]}"
    if c.n <= 1000:
        Lg, D = M.get_factor()
        bad = np.flatnonzero(D != c.d)
        assert len(bad) == 0, tag + f": D differs at {bad[:6]}: {D[bad[:6]]} != {c.d[bad[:6]]}"
        err = np.tril(Lg, -1) != np.tril(c.L, -1)
        assert not err.any(), tag + f": L differs at {np.argwhere(err)[:4].tolist()}"
    else:
        Lt, D = M.get_factor_device()
        Dx = torch.from_numpy(c.d).to(D.device)
        assert torch.equal(D, Dx), tag + f": D differs at {torch.nonzero(D != Dx)[:6].flatten().tolist()}"
        Lx = torch.from_numpy(np.tril(c.L, -1)).to(D.device)
        err = torch.tril(Lt, -1) != Lx
        assert not bool(err.any()), tag + f": L differs at {torch.nonzero(err)[:4].tolist()}"
        del Lt, Lx, err
    assert M.inertia() == c.inertia(), tag + f": inertia {M.inertia()} != {c.inertia()}"
    assert M.info == c.info, tag + f": info {M.info} != {c.info}"


def _check_solve(M, c, tag):
    if c.info:
        return
    x = M.solve_linear_system(c.b.copy())
    bad = np.flatnonzero(x != c.x)
    assert len(bad) == 0, tag + f": x differs at {bad[:6]}"


def _nonsingular(n, v, **kw):
    """The layout without its zero columns (at n < 16 the one whose kind (c) pivot still breaks the static-pivot tier)."""
    spec = layout(n, 1 if n < 16 else v)
    spec["zeros"] = []
    return make_bk(n, 31 * n + v, **spec, **kw)


# ------------------------------------------------------------------------------------------------ factor, every panel kind
@pytest.mark.parametrize("n", SIZES)
def test_pivoted_tier_returns_the_constructed_factor(ctx, n):
    """Dense host input; the one-workgroup panels, the multi-workgroup panels, and a cap of two workgroups per panel (one-
    workgroup panels first, multi-workgroup ones from 512 trailing rows on).  The layouts put 2x2 blocks where a 63- or
    64-column panel ends, far partners in later panels and 256-row workgroups, and colmax ties across waves and workgroups.
    (bk_panel_multi reports the kernel kind the factorization was allowed, not which panels ran it.)"""
    for v in _variants(n):
        c = _case(n, v)
        for wgs, cap in PANELS:
            tag = f"N={n} layout={v} bk_panel_wgs={wgs} bk_max_wgs={cap}"
            M = _solver(ctx, c.A, wgs, cap)
            try:
                M.factorize()
                _check_factor(M, c, tag, count=1)
                assert M.get_stat("bk_panel_multi") == (1.0 if wgs == 0 else 0.0), tag
                assert M.get_stat("bk_mw_fallbacks") == 0, tag
            finally:
                M.close()
    # nonsingular: the solve returns x* bit for bit on both panel kinds
    c = _nonsingular(n, _variants(n)[0])
    for wgs, cap in PANELS[:2]:
        tag = f"N={n} nonsingular bk_panel_wgs={wgs}"
        M = _solver(ctx, c.A, wgs, cap)
        try:
            M.factorize()
            _check_factor(M, c, tag, count=1)
            _check_solve(M, c, tag)
        finally:
            M.close()


@pytest.mark.parametrize("n", [700, 2100])
def test_growth_guard_alone_leads_into_the_tier(ctx, n):
    """No exact zero anywhere in the given order: 2x2 blocks with beta = c / 2^12, so the static tier's second pivot of a block
    is -2^12 c (growth far above bk_growth_tol = 64, pivots of both signs throughout).  The tier must be taken, and exact."""
    c = make_bk(n, 5 + n, pairs=[14, 31, 62, 125], test2=[(17, 19, 23)], growth=12)
    assert np.array_equal(c.perm, np.arange(n)) and c.info == 0
    for wgs in (0, 1):
        tag = f"N={n} growth bk_panel_wgs={wgs}"
        M = _solver(ctx, c.A, wgs)
        try:
            M.factorize()
            _check_factor(M, c, tag, count=1)
            assert M.get_stat("growth") > 64.0, tag
            _check_solve(M, c, tag)
        finally:
            M.close()


# ------------------------------------------------------------------------------------------------ matrix sources
@pytest.mark.parametrize("n", [129, 700])
def test_every_matrix_source(ctx, n):
    """Dense device input with lda > N, lower CSC 0- and 1-based, and a KKT handle with m = 0 whose aug_com is A."""
    from madnlp_jl_amd import _lib as L
    dev = torch.device("cuda", 0)
    for c, kind in ((_case(n, n % 2), "singular"), (_nonsingular(n, 1 - n % 2), "nonsingular")):
        # dense device, lda = N + 5 (the padding is NaN: it must not be read)
        buf = torch.full((n, n + 5), float("nan"), dtype=torch.float64, device=dev)
        buf[:, :n] = torch.from_numpy(np.ascontiguousarray(c.A))
        Ad = buf[:, :n]
        M = _solver(ctx, Ad)
        try:
            M.factorize()
            _check_factor(M, c, f"N={n} {kind} dense device lda={n + 5}", count=1)
            _check_solve(M, c, f"N={n} {kind} dense device")
            # lower CSC, 0-based (the Python path) then 1-based (the C ABI as the Julia glue calls it)
            M.A = c.lower_csc()
            M.factorize()
            _check_factor(M, c, f"N={n} {kind} csc0", count=2)
            colptr, rowval, nz = c.lower_csc(base=1)
            info = C.c_int(0)
            L.check(L.lib().mnk_ls_factorize_csc(M._h, colptr.ctypes.data, rowval.ctypes.data, nz.ctypes.data, 1,
                                                 C.byref(info)), "mnk_ls_factorize_csc")
            M.info = info.value
            _check_factor(M, c, f"N={n} {kind} csc1", count=3)
            _check_solve(M, c, f"N={n} {kind} csc1")
        finally:
            M.close()
        # KKT handle, m = 0, Hessian COO = tril(A) on the pattern, pr_diag = 0
        pc, pr = c.pattern
        rows, cols = pr.astype(np.int64), np.repeat(np.arange(n), np.diff(pc)).astype(np.int64)
        e = np.zeros(0, dtype=np.int64)
        k = mj.SparseCondensedKKTSystem(n, 0, e, e, rows, cols, e, e, e, ctx=ctx,
                                        opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), early_reject=False)
        try:
            k.linear_solver.set_option("accept_only_pd", 0)   # (the inertia of this test is the whole one, not "PD or not")
            k.hess[:] = c.A[rows, cols]
            k.compress_hessian()
            k.build_kkt()
            assert np.array_equal(k.aug_com.to_dense(), np.tril(c.A)), f"N={n} {kind} kkt: aug_com is not A"
            k.linear_solver.factorize()
            _check_factor(k.linear_solver, c, f"N={n} {kind} kkt", count=1)
            _check_solve(k.linear_solver, c, f"N={n} {kind} kkt")
        finally:
            k.close()


# ------------------------------------------------------------------------------------------------ solves
@pytest.mark.parametrize("n", [257, 2100])
def test_solves_return_the_dyadic_solution(ctx, n):
    """Host and device vectors, three right-hand sides in a strided device view (ldx > N), and a solve issued inside
    mnk_solve_batch_begin / _end: x* comes back bit for bit."""
    dev = torch.device("cuda", 0)
    c = _nonsingular(n, 0)
    M = _solver(ctx, c.A)
    try:
        M.factorize()
        _check_factor(M, c, f"N={n} solves", count=1)
        _check_solve(M, c, f"N={n} host")
        xd = torch.from_numpy(c.b.copy()).to(dev)
        M.solve_linear_system(xd)
        M.check_solve()
        assert torch.equal(xd.cpu(), torch.from_numpy(c.x)), f"N={n} device vector"
        ldx = n + 7
        buf = torch.full((3, ldx), float("nan"), dtype=torch.float64, device=dev)
        X = buf.T[:n]                                          # (n, 3), column stride ldx
        scale = torch.tensor([1.0, -0.5, 4.0], dtype=torch.float64, device=dev)
        X[:] = torch.from_numpy(c.b).to(dev)[:, None] * scale
        M.solve_linear_system(X)
        M.check_solve()
        want = torch.from_numpy(c.x).to(dev)[:, None] * scale
        assert torch.equal(X, want), f"N={n} strided right-hand sides"
        assert bool(torch.isnan(buf.T[n:]).all()), f"N={n} the padding rows were written"
        xb = torch.from_numpy(c.b.copy()).to(dev)
        with mj.solve_batch():
            M.solve_linear_system(xb)
        M.check_solve()
        try:   # a pivoted factor is solved stepwise, inside a batch too (None: a build of the library without the statistic)
            path = M.get_stat("solve_path")
        except mj.HipError:
            path = None
        assert path in (1, None), path
        assert torch.equal(xb.cpu(), torch.from_numpy(c.x)), f"N={n} solve inside a solve batch"
    finally:
        M.close()


# ------------------------------------------------------------------------------------------------ batches and repeats
def _first_static_zero(c):
    """The first column at which the static-pivot LDL^T of the stored matrix meets an exact zero pivot (its leading block of
    order 320 decides it), None if none there."""
    m = min(c.n, 320)
    _, d = scalar_ldl(c.A[:m, :m])
    z = np.flatnonzero(d == 0.0)
    return int(z[0]) if len(z) else None


def _batch_pivoted_members():
    """Three members that leave the static-pivot tier at different columns: a 2x2 block with beta = 0 at column 1, the far 2x2
    block of the standard layout at column 3 (beta = 0 in this one), and a zero column at 200, in the fourth 64-column block
    (every 2x2 block before it has beta != 0)."""
    return [make_bk(257, 9257, pairs=[1, 130], beta0=[1], far=[(40, 200)], onexone=[(60, 250)], ties=[(130, 233)]),
            _case(700, 0),
            make_bk(1000, 9100, zero_beta=False, zeros=[200], far=[(300, 700)], onexone=[(400, 900)], pairs=[205],
                    ties=[(205, 517)])]


def test_a_batch_of_pivoted_and_static_members(ctx):
    """One factorize_batch of 6 members of mixed orders: three whose static tier breaks down at different columns (they take the
    pivoted tier) and three that stay static (tests/exact_factor.py).  Each member's factor equals its construction, and the
    inertia batch agrees with each one's inertia."""
    from madnlp_jl_amd import _lib as L
    bk = _batch_pivoted_members()
    assert [_first_static_zero(m) for m in bk] == [1, 3, 200]
    st = [make_exact(257, 43, positive=False), make_exact(700, 41, positive=False), make_exact(1000, 47)]
    members = [bk[0], st[0], bk[1], st[1], bk[2], st[2]]
    Ms = [_solver(ctx, m.A) for m in members]
    try:
        with mj.factorize_batch():
            for M in Ms:
                M.factorize()
        hs = (C.c_void_p * 6)(*[M._h.value for M in Ms])
        p, z, ng = (C.c_int64 * 6)(), (C.c_int64 * 6)(), (C.c_int64 * 6)()
        L.check(L.lib().mnk_ls_inertia_batch(6, hs, p, z, ng), "mnk_ls_inertia_batch")
        for i, (M, m) in enumerate(zip(Ms, members)):
            tag = f"batch member {i} N={m.n}"
            assert (p[i], z[i], ng[i]) == m.inertia(), tag + f": inertia batch {(p[i], z[i], ng[i])} != {m.inertia()}"
            if i % 2 == 0:
                _check_factor(M, m, tag, count=1)
                _check_solve(M, m, tag)
            else:
                assert M.bk_info()[:2] == (False, 0), tag + ": a static member took the pivoted tier"
                _, D = M.get_factor()
                assert np.array_equal(D, m.d), tag + ": static D"
    finally:
        for M in Ms:
            M.close()


def test_repeats_on_one_solver_are_bit_identical(ctx):
    """A second factorization on the same solver gives the same bits; so does static -> pivoted -> static -> pivoted."""
    n = 700
    c = _case(n, 1)
    s = make_exact(n, 53, positive=False)
    M = _solver(ctx, c.A)
    try:
        M.factorize()
        _check_factor(M, c, "repeat 1", count=1)
        L1, D1 = M.get_factor()
        M.factorize()
        _check_factor(M, c, "repeat 2", count=2)
        L2, D2 = M.get_factor()
        assert np.array_equal(np.tril(L1), np.tril(L2)) and np.array_equal(D1, D2)
        count = 2
        for step in range(2):
            M.A = s.A
            M.factorize()
            assert M.bk_info()[:2] == (False, count), f"static step {step}"
            assert M.inertia() == s.inertia() and np.array_equal(M.get_factor()[1], s.d), f"static step {step}"
            M.A = c.A
            M.factorize()
            count += 1
            _check_factor(M, c, f"pivoted step {step}", count=count)
    finally:
        M.close()

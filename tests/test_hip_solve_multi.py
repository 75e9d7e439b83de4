"""The blocked solve for several right-hand sides (SOLVE_BLOCKED = 5, csrc/solve_multi.hip) on the device (-m gpu).

The systems of tests/solve_multi_cases.py have one right answer in fp64 whatever the grouping of the sums, so the blocked path
must return X* with array_equal -- for CHOLESKY and LDL, over the orders at which the step structure changes and the widths at
the MFMA tile edge and the chunk edge, with X on the host or the device, contiguous or strided.  Every solve asserts the path
(option multi_rhs_min = 2 forces it) and the chunk count first.  On real data: the same bits from two calls, a column's bits
independent of its neighbours and of its position, a power-of-two scaling commuting with the whole solver, and the componentwise
backward error per column against the oracle's dpotrs / dsytrs (MNK_SOLVE_MULTI_ACCURACY_OUT names a file: the figures of
profiles/solve_multi_accuracy.json)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import madnlp_jl_amd as mj
from madnlp_jl_amd import _lib as L
from oracle.lapack_cpu import BUNCHKAUFMAN, CHOLESKY, LapackCPUSolver
from tests.bk_exact import layout, make_bk
from tests.exact_factor import ExactCase
from tests.solve_exact import device_system
from tests.solve_multi_cases import DEVICE_CASE, GPU_CASES, W, multi_case
from tests.test_hip_pivot_ladder import _KKT

pytestmark = pytest.mark.gpu

ALGS = [mj.CHOLESKY, mj.LDL]
NAN = float("nan")
BLOCKED = 5
# device <= ACCURACY_MARGIN * oracle per column, componentwise backward error: the next power of two above twice the largest
# ratio measured on an MI355X for the cases of test_componentwise_backward_error_per_column (profiles/solve_multi_accuracy.json: 2.62,
# CHOLESKY at N = 257), capped at 64
ACCURACY_MARGIN = 8.0
_measured = {}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()
    out = os.environ.get("MNK_SOLVE_MULTI_ACCURACY_OUT")
    if out and _measured:
        with open(out, "w") as f:
            json.dump({"bound": f"device <= {ACCURACY_MARGIN:g} * oracle, per column", "cases": _measured,
                       "note": "tests/test_hip_solve_multi.py on one MI355X: componentwise backward error max_i |A x - b|_i / "
                               "(|A| |x| + |b|)_i in longdouble, per column, of the blocked solve (solve_path 5) and of the oracle's "
                               "dpotrs (CHOLESKY) / dsytrs (LDL) on the same graded matrix S B S; ratio = the largest device / oracle "
                               "ratio over the columns"}, f, indent=1, sort_keys=True)


def _dev():
    return torch.device("cuda", 0)


def _solver(ctx, A, alg, multi_rhs_min=2, **opts):
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg, pivot_tol=0.0, multi_rhs_min=multi_rhs_min))
    for key, v in opts.items():
        M.set_option(key, v)
    return M


def _chunks(R):
    out = (C.c_int * 5)()
    assert L.lib().mnk_debug_solve_plan_multi(64, 256, 0, 1, 0, 0, 0, 0, 0, 0, 0, R, 2, out) == 0
    assert out[0] == BLOCKED and out[1] == W
    return out[2]


def _assert_blocked(M, R, tag):
    assert M.get_stat("solve_path") == BLOCKED, tag + f": solve_path {M.get_stat('solve_path')}, expected {BLOCKED}"
    assert M.get_stat("solve_rhs_chunks") == _chunks(R), tag + f": {M.get_stat('solve_rhs_chunks')} chunks for {R} columns"


def _assert_exact(X, want, tag):
    X, want = (torch.as_tensor(X), torch.as_tensor(want))
    bad = torch.nonzero(X != want)
    if len(bad):
        i = bad[0].tolist()
        raise AssertionError(tag + f": {len(bad)} entries differ from X*, first at {i}: {X[tuple(i)].item()!r} != {want[tuple(i)].item()!r}")


def _colmajor(n, R, ld=None, extra=0):
    """(buffer, view): an n x R column-major device view with column stride `ld` inside a NaN-filled buffer of R + extra columns."""
    ld = ld or n
    buf = torch.full((R + extra, ld), NAN, dtype=torch.float64, device=_dev())
    return buf, buf.T[:n, :R]


def _four_forms(M, B, X, tag):
    """B (numpy, n x R column-major) through the solver in the four forms; X* bit for bit, path, chunks, padding untouched."""
    n, R = B.shape
    Bd, Xd = torch.from_numpy(B).to(_dev()), torch.from_numpy(X).to(_dev())
    xh = np.asfortranarray(B.copy())
    M.solve_linear_system(xh)
    _assert_blocked(M, R, tag + " host")
    _assert_exact(xh, X, tag + " host")
    buf, V = _colmajor(n, R)
    V[:] = Bd
    torch.cuda.synchronize()
    M.solve_linear_system(V)
    M.check_solve()
    _assert_blocked(M, R, tag + " device")
    _assert_exact(V, Xd, tag + " device")
    buf, V = _colmajor(n, R, ld=n + 7, extra=1)
    V[:] = Bd
    torch.cuda.synchronize()
    M.solve_linear_system(V)
    M.check_solve()
    _assert_blocked(M, R, tag + " strided")
    _assert_exact(V, Xd, tag + " strided")
    assert bool(torch.isnan(buf.T[n:]).all()), tag + ": rows >= N of the strided view were written"
    assert bool(torch.isnan(buf[R:]).all()), tag + ": a column >= nrhs of the device buffer was written"
    wide = np.full((n, R + 1), NAN, order="F")
    wide[:, :R] = B
    M.solve_linear_system(wide[:, :R])
    _assert_blocked(M, R, tag + " host, NaN column behind")
    _assert_exact(wide[:, :R], X, tag + " host, NaN column behind")
    assert np.isnan(wide[:, R]).all(), tag + ": the column behind nrhs was written"


def _factorize(M, c, tag):
    torch.cuda.synchronize()
    M.factorize()
    assert M.inertia() == c.inertia(), tag + f": inertia {M.inertia()} != {c.inertia()}"


# ------------------------------------------------------------------------------- exact answers
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n,R,scale_bits", GPU_CASES)
def test_blocked_solves_return_the_dyadic_solutions(ctx, n, R, scale_bits, alg):
    mc = multi_case(n, alg == mj.CHOLESKY, scale_bits, R)
    tag = f"N={n} R={R} {alg} scale_bits={scale_bits}"
    M = _solver(ctx, torch.from_numpy(np.ascontiguousarray(mc.base.A)).to(_dev()), alg)
    try:
        _factorize(M, mc.base, tag)
        _four_forms(M, mc.B, mc.X, tag)
    finally:
        M.close()


def test_seventeen_steps_built_on_the_device(ctx):
    """N = 4100 (17 steps, a last step of 64 padded rows), LDL, from the sparse factors on the device."""
    n, R, sb = DEVICE_CASE
    mc = multi_case(n, False, sb, R)
    A, _ = device_system(mc.base, _dev())
    M = _solver(ctx, A, mj.LDL)
    try:
        _factorize(M, mc.base, f"N={n}")
        buf, V = _colmajor(n, R, ld=n + 7)
        V[:] = torch.from_numpy(mc.B).to(_dev())
        torch.cuda.synchronize()
        M.solve_linear_system(V)
        M.check_solve()
        _assert_blocked(M, R, f"N={n}")
        _assert_exact(V, torch.from_numpy(mc.X).to(_dev()), f"N={n} R={R}")
        assert bool(torch.isnan(buf.T[n:]).all())
    finally:
        M.close()


@pytest.mark.parametrize("alg", ALGS)
def test_a_nan_column_stays_alone(ctx, alg):
    n, R, bad = 700, 17, 5
    mc = multi_case(n, alg == mj.CHOLESKY, 0, R)
    M = _solver(ctx, torch.from_numpy(np.ascontiguousarray(mc.base.A)).to(_dev()), alg)
    try:
        _factorize(M, mc.base, f"N={n} {alg}")
        for host in (True, False):
            B = mc.B.copy(order="F")
            B[:, bad] = NAN
            if host:
                got = M.solve_linear_system(B)
            else:
                _, V = _colmajor(n, R)
                V[:] = torch.from_numpy(B).to(_dev())
                torch.cuda.synchronize()
                M.solve_linear_system(V)
                M.check_solve()
                got = V.cpu().numpy()
            _assert_blocked(M, R, f"N={n} {alg}")
            keep = [r for r in range(R) if r != bad]
            _assert_exact(got[:, keep], mc.X[:, keep], f"N={n} {alg} host={host}: the columns beside the NaN column")
            assert np.isnan(got[:, bad]).all(), "the NaN column is NaN in every row"
    finally:
        M.close()


# ------------------------------------------------------------------------------- real data
REAL_SIZES = [257, 1300]


@functools.lru_cache(maxsize=None)
def _real(n, alg):
    """(B, S B S, s, rhs) as tests/test_hip_solve_exact.py::_real builds them: B = R R^T / 64 + I with R n x 64 standard normal, for
    LDL its trailing third negated (quasi-definite, condition number at most 1e3); S = diag(2^k), k uniform in [0, 40]; rhs: n x
    (W + 1) standard normal."""
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(1000 + n)
    R = torch.randn(n, 64, dtype=torch.float64, device=dev, generator=g)
    B = R @ R.T / 64.0
    B.diagonal().add_(1.0)
    B = (B + B.T) / 2.0
    if alg == mj.LDL:
        h = n // 3
        B[n - h:, n - h:].neg_()
    assert torch.linalg.matrix_norm(B, ord=float("inf")).item() <= 1e3
    s = torch.from_numpy(np.ldexp(1.0, np.random.default_rng(1000 + n).integers(0, 41, size=n))).to(dev)
    assert bool((torch.frexp(s)[0] == 0.5).all())
    rhs = torch.randn(W + 1, n, dtype=torch.float64, device=dev, generator=g).T   # (column-major)
    return B, s[:, None] * B * s[None, :], s, rhs


def _real_solver(ctx, A, alg, n):
    M = _solver(ctx, A, alg)
    torch.cuda.synchronize()
    M.factorize()
    n_pos = n if alg == mj.CHOLESKY else n - n // 3
    assert M.inertia() == (n_pos, 0, n - n_pos)
    return M


def _solve_columns(M, rhs, cols):
    """The columns `cols` of rhs, solved together in a fresh column-major buffer."""
    n = rhs.shape[0]
    _, V = _colmajor(n, len(cols))
    V[:] = rhs[:, cols]
    torch.cuda.synchronize()
    M.solve_linear_system(V)
    M.check_solve()
    _assert_blocked(M, len(cols), f"N={n} columns {cols[:4]}..")
    return V.clone()


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n", REAL_SIZES)
def test_repeatable_and_independent_of_the_neighbours(ctx, n, alg):
    """Two calls give the same bits; column r has the same bits among 4 columns, among W + 1 columns and at another position."""
    B, _, _, rhs = _real(n, alg)
    M = _real_solver(ctx, B, alg, n)
    try:
        everything = list(range(W + 1))
        X1 = _solve_columns(M, rhs, everything)
        X2 = _solve_columns(M, rhs, everything)
        assert torch.equal(X1, X2), "two calls differ"
        four = [7, 20, 3, W]
        X4 = _solve_columns(M, rhs, four)
        _assert_exact(X4, X1[:, four], f"N={n} {alg}: among 4 columns, at other positions")
        rev = everything[::-1]
        Xr = _solve_columns(M, rhs, rev)
        _assert_exact(Xr, X1[:, rev], f"N={n} {alg}: reversed positions")
    finally:
        M.close()


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n", REAL_SIZES)
def test_a_power_of_two_scaling_commutes_with_the_blocked_solve(ctx, n, alg):
    """solve(S B S, S rhs) == S^-1 solve(B, rhs) bit for bit."""
    B, SBS, s, rhs = _real(n, alg)
    cols = list(range(17))
    M0, M1 = _real_solver(ctx, B, alg, n), _real_solver(ctx, SBS, alg, n)
    try:
        X0 = _solve_columns(M0, rhs, cols)
        X1 = _solve_columns(M1, s[:, None] * rhs, cols)
        _assert_exact(X1, X0 / s[:, None], f"N={n} {alg}")
    finally:
        M0.close()
        M1.close()


def _componentwise_backward_errors(A, X, Bm):
    A, X, Bm = A.astype(np.longdouble), X.astype(np.longdouble), Bm.astype(np.longdouble)
    return np.max(np.abs(A @ X - Bm) / (np.abs(A) @ np.abs(X) + np.abs(Bm)), axis=0).astype(np.float64)


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n", REAL_SIZES)
def test_componentwise_backward_error_per_column(ctx, n, alg):
    """The graded S B S with 17 random right-hand sides: max_i |A x - b|_i / (|A| |x| + |b|)_i in longdouble of every column of the
    blocked solve is at most ACCURACY_MARGIN times that of the oracle's dpotrs / dsytrs for the same column."""
    _, SBS, _, rhs = _real(n, alg)
    cols = list(range(17))
    Ah, Bh = SBS.cpu().numpy(), np.asfortranarray(rhs[:, cols].cpu().numpy())
    ref = LapackCPUSolver(np.asfortranarray(np.tril(Ah)), CHOLESKY if alg == mj.CHOLESKY else BUNCHKAUFMAN).factorize()
    assert ref.info == 0
    Xref = np.stack([ref.solve_linear_system(Bh[:, r].copy()) for r in cols], axis=1)
    e_ref = _componentwise_backward_errors(Ah, Xref, Bh)
    assert (e_ref > 0.0).all()
    M = _real_solver(ctx, SBS, alg, n)
    try:
        X = _solve_columns(M, rhs, cols).cpu().numpy()
    finally:
        M.close()
    e = _componentwise_backward_errors(Ah, X, Bh)
    ratio = float(np.max(e / e_ref))
    print(f"N={n} {alg} blocked: device max {e.max():.3e}, oracle max {e_ref.max():.3e}, largest ratio {ratio:.2f}")
    _measured[f"{alg}-{n}"] = {"device_max": float(e.max()), "oracle_max": float(e_ref.max()), "ratio": ratio}
    assert (e <= ACCURACY_MARGIN * e_ref).all(), (n, alg, ratio)


# ------------------------------------------------------------------------------- mixing with the other paths
@pytest.mark.parametrize("alg", ALGS)
def test_blocked_and_single_solves_take_turns_and_a_second_matrix(ctx, alg):
    n, R = 700, 17
    mc, mc2 = multi_case(n, alg == mj.CHOLESKY, 0, R), multi_case(n, alg == mj.CHOLESKY, 0, R, 1)
    dev = _dev()
    M = _solver(ctx, torch.from_numpy(np.ascontiguousarray(mc.base.A)).to(dev), alg)
    try:
        _factorize(M, mc.base, f"N={n} {alg}")
        B, X = torch.from_numpy(mc.B).to(dev), torch.from_numpy(mc.X).to(dev)

        def blocked(tag):
            _, V = _colmajor(n, R)
            V[:] = B
            torch.cuda.synchronize()
            M.solve_linear_system(V)
            M.check_solve()
            _assert_blocked(M, R, tag)
            _assert_exact(V, X, tag)

        blocked("first blocked solve")
        for rep in range(2):   # (both publication buffers of the one-launch solve)
            v = B[:, 2].clone()
            torch.cuda.synchronize()
            M.solve_linear_system(v)
            M.check_solve()
            assert M.get_stat("solve_path") == 2
            _assert_exact(v, X[:, 2], f"single device vector {rep} after a blocked solve")
        blocked("blocked solve after single solves")
        M.A = torch.from_numpy(np.ascontiguousarray(mc2.base.A)).to(dev)
        _factorize(M, mc2.base, "second matrix")
        _four_forms(M, mc2.B, mc2.X, f"N={n} {alg} second matrix")
    finally:
        M.close()


@pytest.mark.parametrize("alg", ALGS)
def test_blocked_solve_through_a_sparse_condensed_kkt_handle(ctx, alg):
    """N = 1300, scale_bits = 40, K = A fed as the Hessian's lower triangle on its structural pattern, as
    test_solves_through_a_sparse_condensed_kkt_handle does."""
    n, R = 1300, 4
    mc = multi_case(n, alg == mj.CHOLESKY, 40, R)
    c = mc.base
    pat = ExactCase(n, c.Nmat, c.d, c.A).lower_pattern()
    K = _KKT(ctx, n, alg, pat) if alg == mj.CHOLESKY else _KKT(ctx, n, alg, pat, early_reject=False, accept_only_pd=0)
    try:
        K.M.set_option("pivot_tol", 0.0)
        K.M.set_option("multi_rhs_min", 2)
        K.factorize(c)
        assert K.M.inertia() == c.inertia()
        _, V = _colmajor(n, R, ld=n + 7)
        V[:] = torch.from_numpy(mc.B).to(_dev())
        torch.cuda.synchronize()
        K.M.solve_linear_system(V)
        K.M.check_solve()
        _assert_blocked(K.M, R, f"N={n} {alg} kkt")
        _assert_exact(V, torch.from_numpy(mc.X).to(_dev()), f"N={n} {alg} kkt")
    finally:
        K.close()


# ------------------------------------------------------------------------------- what keeps the column loop
def test_a_pivoted_factor_keeps_the_column_loop(ctx):
    """A matrix of tests/bk_exact.py that takes the pivoted tier, four right-hand sides with multi_rhs_min = 2: stepwise, right."""
    n = 257
    spec = layout(n, 0)
    spec["zeros"] = []
    c = make_bk(n, 31 * n, **spec)
    M = mj.HipLinearSolver(c.A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN, multi_rhs_min=2))
    try:
        M.factorize()
        assert M.bk_info()[0], "the pivoted tier was not taken"
        scale = np.array([1.0, -0.5, 4.0, 0.25])
        X = np.asfortranarray(c.b[:, None] * scale)
        M.solve_linear_system(X)
        assert M.get_stat("solve_path") == 1
        _assert_exact(X, c.x[:, None] * scale, "pivoted tier, four columns")
    finally:
        M.close()


@pytest.mark.parametrize("alg", ALGS)
def test_multi_rhs_min_zero_and_the_threshold(ctx, alg):
    n, R = 257, 17
    mc = multi_case(n, alg == mj.CHOLESKY, 0, R)
    dev = _dev()
    M = _solver(ctx, torch.from_numpy(np.ascontiguousarray(mc.base.A)).to(dev), alg, multi_rhs_min=0)
    try:
        _factorize(M, mc.base, f"N={n} {alg}")
        for mn, want in ((0, 2), (R + 1, 2), (R, BLOCKED)):
            M.set_option("multi_rhs_min", mn)
            _, V = _colmajor(n, R)
            V[:] = torch.from_numpy(mc.B).to(dev)
            torch.cuda.synchronize()
            M.solve_linear_system(V)
            M.check_solve()
            assert M.get_stat("solve_path") == want, (mn, M.get_stat("solve_path"))
            _assert_exact(V, torch.from_numpy(mc.X).to(dev), f"N={n} {alg} multi_rhs_min={mn}")
    finally:
        M.close()

"""Exact-answer tests of the KKT handles' device `mul!`, `build_kkt!` and `solve_kkt!` (`mnk_dc_*`, `mnk_sc_*`: csrc/dense_kkt.hip,
csrc/sparse_kkt.hip, csrc/kkt_vec.h) on the cases of tests/kkt_exact.py: systems of general structure (interleaved equality and
inequality rows, primal entries with both bounds, one or none, dense inequality rows, COO patterns with duplicates and
upper-triangular entries) on which no operation rounds, so that the one right answer is known to the bit whatever the kernels'
summation order, tiling or fusing, and a wrong index shows as a wrong bit.  tests/test_kkt_exact_cpu.py checks the cases themselves.

The shapes (n, m, n_eq) are the smallest that cross each threshold of the kernels: 64 (the lane stride of gemv_t_kernel /
symv_l_kernel and the row block of gemv_n_kernel), 4 columns per workgroup with n no multiple of it, the 32 x 32 transpose tiles,
the npad = 64 k / kpad = 16 k padding, order 258 > 256 (a second row block of init_condensed_kernel) and order 310 > 256 of
dense_aug_kernel.

The augmented system (`dense`) has no exact factorization; its `solve_kkt!` -- and, once more, everybody's -- runs on the rounded
twins `random_kkt_case` with bounds derived from the number format: per entry for `mul!` and `build_kkt!`, and for `solve_kkt!`
the residual acceptance of tests/test_hip_parity.py::test_device_solve_kkt_and_mul_match_oracle (100 x the oracle's, floor 1e-10)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from tests import kkt_exact as ke  # noqa: E402

CASES = [(k, s) for k in ke.KINDS for s in ke.SHAPES[k]]
CONDENSED = [p for p in CASES if p[0] != "dense"]
CALLERS = [(k, s) for k, s in CASES if s[:2] in ((65, 70), (130, 97))]
ROUNDED = [(k, s) for k in ke.KINDS for s in ke.ROUNDED_SHAPES]


def _id(p):
    return f"{p[0]}-" + "-".join(map(str, p[1]))


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


_CASES = {}


def _case(param, rounded=False):
    key = (param, rounded)
    if key not in _CASES:
        _CASES[key] = (ke.random_kkt_case if rounded else ke.exact_kkt_case)(param[0], *param[1])
    return _CASES[key]


def _handle(ctx, c, exact=True):
    """The HIP system of the case's kind, fed through its host fields and built (`build_kkt` uploads hess / jac, the diagonals
    and, with `device_kkt_ops`, the barrier terms).  Exact cases: the static-pivot tier alone factors A (LDL, or CHOLESKY where
    there is no equality row), which returns I + N and d exactly; rounded cases: the handle's defaults."""
    opt = None
    if exact:
        opt = mj.HipSolverOptions(lapack_algorithm=mj.LDL if c.n_eq else mj.CHOLESKY, pivot_tol=0.0)
    if c.kind == "sparse_condensed":
        q = c.coo
        kh = mj.SparseCondensedKKTSystem(c.n, c.m, q["jac_I"], q["jac_J"], q["hess_I"], q["hess_J"], c.ind_ineq, c.ind_lb, c.ind_ub,
                                         ctx=ctx, opt_linear_solver=opt or mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY),
                                         device_kkt_ops=True)
        kh.jac[:] = q["jac"]
        kh.hess[:] = q["hess"]
    else:
        if c.kind == "dense_condensed":
            kh = mj.DenseCondensedKKTSystem(c.n, c.m, c.ind_ineq, c.ind_eq, c.ind_lb, c.ind_ub, ctx=ctx, opt_linear_solver=opt,
                                            device_kkt_ops=True)
        else:
            kh = mj.DenseKKTSystem(c.n, c.m, c.ind_ineq, c.ind_lb, c.ind_ub, ctx=ctx, device_kkt_ops=True)
        kh.hess[...] = c.hess
        kh.jac[...] = c.jac
    for name in ("reg", "pr_diag", "du_diag", "l_diag", "u_diag", "l_lower", "u_lower"):
        getattr(kh, name)[:] = getattr(c, name)
    kh.compress_jacobian()
    kh.compress_hessian()
    kh.build_kkt()
    return kh


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _mismatch(c, got, want):
    """Per block (x, s, y, z_l, z_u): the number of entries that differ and the first of them."""
    out = []
    for name, sl in c.blocks().items():
        bad = np.flatnonzero(got[sl] != want[sl])
        if len(bad):
            i = int(bad[0])
            out.append(f"{name}: {len(bad)} of {sl.stop - sl.start} differ, first at {i}: {got[sl][i]!r} != {want[sl][i]!r}")
        else:
            out.append(f"{name}: 0")
    return "; ".join(out)


def _built_matrix(c, kh):
    """(what the handle built, the same entries of the reference matrix `want`-> callable)."""
    if c.kind == "sparse_condensed":
        cols = np.repeat(np.arange(c.n), np.diff(kh.aug_com.colptr))
        rows = np.asarray(kh.aug_com.rowval)
        return kh.aug_com.nzval, lambda M: M[rows, cols]
    K = kh.aug_com.to_host()
    if c.kind == "dense":
        return np.tril(K), np.tril
    return K, lambda M: M


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("param", CASES, ids=_id)
def test_mul_gives_the_exact_product(ctx, param):
    """alpha K_u x + beta w for four (alpha, beta), x and w drawn like x*: the bits of the integer evaluation."""
    c = _case(param)
    kh = _handle(ctx, c)
    try:
        for k, (alpha, beta) in enumerate(ke.ALPHA_BETA):
            x, w = ke.draw_vector(c, 2 * k), ke.draw_vector(c, 2 * k + 1)
            want = ke.exact_mul(c, x, w, alpha, beta)
            got = kh.mul_device(w.copy(), x.copy(), alpha, beta)
            assert np.array_equal(got, want), f"alpha={alpha} beta={beta}: " + _mismatch(c, got, want)
    finally:
        kh.close()


@pytest.mark.parametrize("param", CASES, ids=_id)
def test_build_kkt_gives_the_exact_matrix(ctx, param):
    """Condensed kinds: aug_com (dense: both triangles; sparse: the CSC values, whose pattern holds every nonzero of A) is
    A = (I + N) diag(d) (I + N)'; augmented: the lower triangle is that of the reduced matrix."""
    c = _case(param)
    kh = _handle(ctx, c)
    try:
        got, pick = _built_matrix(c, kh)
        want = pick(ke.reduced_matrix(c) if c.kind == "dense" else c.A)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{len(bad)} entries differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
        if c.kind == "sparse_condensed":
            assert np.array_equal(kh.aug_com.to_dense(), np.tril(c.A)), "the pattern of aug_com misses a nonzero of A"
    finally:
        kh.close()


def _solve_exact(ctx, c):
    kh = _handle(ctx, c)
    try:
        kh.linear_solver.factorize()
        assert kh.linear_solver.inertia() == (c.n, 0, c.n_eq), kh.linear_solver.inertia()
        b = c.b
        got = kh.solve_kkt_device(b.copy())
        assert np.array_equal(got, c.xstar), _mismatch(c, got, c.xstar)
        return kh, got
    except BaseException:
        kh.close()
        raise


@pytest.mark.parametrize("param", CONDENSED, ids=_id)
def test_solve_kkt_returns_the_dyadic_solution(ctx, param):
    """The inertia is (n, 0, n_eq) and `solve_kkt_device(K_u x*)` is x* bit for bit."""
    kh, _ = _solve_exact(ctx, _case(param))
    kh.close()


@pytest.mark.parametrize("param", CALLERS, ids=_id)
def test_host_vectors_and_device_tensors_give_the_same_bits(ctx, param):
    """`mul_device` and `solve_kkt_device` on host vectors (staged through the handle's buffers) and on device tensors (in place).
    The augmented system is factored by the handle's default algorithm: its solution is compared between the callers only."""
    c = _case(param)
    exact = c.kind != "dense"
    kh = _handle(ctx, c, exact=exact)
    try:
        x, w = ke.draw_vector(c, 40), ke.draw_vector(c, 41)
        for alpha, beta in ke.ALPHA_BETA:
            wh = kh.mul_device(w.copy(), x.copy(), alpha, beta)
            wd = kh.mul_device(_dev(w), _dev(x), alpha, beta)
            ctx.synchronize()
            assert np.array_equal(wd.cpu().numpy(), wh), f"mul alpha={alpha} beta={beta}: " + _mismatch(c, wd.cpu().numpy(), wh)
        kh.linear_solver.factorize()
        sh = kh.solve_kkt_device(c.b)
        sd = kh.solve_kkt_device(_dev(c.b))
        ctx.synchronize()
        assert np.array_equal(sd.cpu().numpy(), sh), "solve_kkt: " + _mismatch(c, sd.cpu().numpy(), sh)
        if exact:
            assert np.array_equal(sh, c.xstar), _mismatch(c, sh, c.xstar)
    finally:
        kh.close()


def test_blocks_forty_binary_orders_apart_still_match_bit_for_bit(ctx):
    """(130, 97, 14) in the units x 2^20, s 2^0, y 2^40: the blocks of the solution and of the right-hand side span 2^0 ... 2^40,
    every sum of the chain is scaled row by row by one power of two, and the small blocks -- which no norm-wise check sees --
    still come back bit for bit."""
    c = ke.scaled_case(_case(("dense_condensed", (130, 97, 14))), 20, 0, 40)
    units = ke.solution_units(c)
    assert units.min() == 0 and units.max() == 40
    kh, got = _solve_exact(ctx, c)
    try:
        A = kh.aug_com.to_host()
        assert np.array_equal(A, c.A)
        x = np.ldexp(ke.draw_vector(c, 50), units)
        got = kh.mul_device(np.zeros(c.lw), x.copy(), 1.0, 0.0)
        want = np.ldexp(ke.exact_mul(c.base, np.ldexp(x, -units), np.zeros(c.lw), 1.0, 0.0), ke.rhs_units(c))
        assert np.array_equal(got, want), _mismatch(c, got, want)
    finally:
        kh.close()


# ------------------------------------------------------------------------------------------------ rounded data, general structure
@pytest.mark.parametrize("param", ROUNDED, ids=_id)
def test_rounded_data_within_the_bounds_of_the_number_format(ctx, param):
    """`mul_device` per entry within (t_i + 6) 2^-53 S_i of longdouble K_u, `build_kkt` (dense condensed) per entry within
    (ns + 8) 2^-53 of the sum of the magnitudes of its terms, `solve_kkt_device` with a residual within 100 x the oracle's
    (floor 1e-10); both residuals are printed."""
    c = _case(param, rounded=True)
    kh = _handle(ctx, c, exact=False)
    try:
        rng = np.random.default_rng(3)
        for alpha, beta in ke.ALPHA_BETA:
            x, w = rng.standard_normal(c.lw), rng.standard_normal(c.lw)
            got = kh.mul_device(w.copy(), x.copy(), alpha, beta)
            ref, bound = ke.mul_bound(c, x, w, alpha, beta)
            err = np.abs(got - ref)
            print(f"{_id(param)} mul alpha={alpha} beta={beta}: largest error / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (alpha, beta, int(np.argmax(err / bound)), float((err / bound).max()))
        if c.kind == "dense_condensed":
            ref, bound = ke.build_bound(c)
            i, j = np.tril_indices(c.order)
            err, bd = np.abs(kh.aug_com.to_host() - ref)[i, j], bound[i, j]
            print(f"{_id(param)} build_kkt: largest error / bound {float((err[bd > 0] / bd[bd > 0]).max()):.3f}")
            assert (err <= bd).all(), (int(i[np.argmax(err - bd)]), int(j[np.argmax(err - bd)]))
        kh.linear_solver.factorize()
        b = rng.standard_normal(c.lw)
        got = kh.solve_kkt_device(b.copy())
        res_device = ke.residual(c, got, b)
        _, res_oracle = ke.oracle_residual(c, b)
        print(f"{_id(param)} solve_kkt residual: device {res_device:.3e}, oracle {res_oracle:.3e}")
        assert res_device <= max(1e-10, 100 * res_oracle), (res_device, res_oracle)
    finally:
        kh.close()

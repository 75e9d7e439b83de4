"""The call-order contract and the corner shapes of the KKT handles' bound / barrier state (`mnk_sc_*`, `mnk_dc_*`: one
implementation in csrc/kkt_vec.h), for the three handle kinds on a 3-variable, 2-constraint problem.

  * entry points called too early are refused with the message that names the missing call; a refused call leaves the handle
    usable: the correct sequence afterwards gives `mul_device` / `solve_kkt_device` results that match the CPU oracle classes
    (acceptance of tests/test_hip_parity.py::test_device_solve_kkt_and_mul_match_oracle: mul! 1e-12 of the largest entry,
    solve_kkt! through the KKT residual);
  * bound indices out of range are refused for either side and either `index_base`; `index_base = 1` with shifted indices
    gives the bits of `index_base = 0`;
  * host vectors and device tensors give identical bits;
  * an empty bound side and m = 0 (the launch guards), a variable with both bounds.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from oracle import dense as odense  # noqa: E402
from oracle import kernels as okern  # noqa: E402
from oracle import sparse_condensed as osc  # noqa: E402
from oracle.lapack_cpu import BUNCHKAUFMAN, CHOLESKY, LapackCPUSolver  # noqa: E402
from tests.test_hip_round2 import _iterate, _oracle_feed  # noqa: E402

KINDS = ("sparse_condensed", "dense", "dense_condensed")
N, M = 3, 2
HESS = np.array([[4.0, 0.0, 0.0], [1.0, 3.0, 0.0], [0.5, -1.0, 5.0]])      # lower triangle
JAC = np.array([[1.0, 2.0, -1.0], [0.5, -1.0, 3.0]])
DIAGS = ("pr_diag", "du_diag", "reg", "l_diag", "u_diag", "l_lower", "u_lower")
PRIMAL_REG, DUAL_REG = 0.5, 1e-8


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def _late_bounds(cls):
    """`cls` whose constructor leaves `mnk_*_set_bounds` to the test (`set_bounds_now`)."""
    class Late(cls):
        def _set_bounds(self):
            pass

        def set_bounds_now(self):
            cls._set_bounds(self)
    return Late


def _pair(kind, ctx, variant="both", late=False):
    """(oracle system, HIP system): n = 3, m = 2 (`m0`: no constraints); sparse condensed: two inequalities, dense: constraint 0
    an equality and constraint 1 an inequality.  Variable 2 carries both bounds; `nlb0` / `nub0` empty one bound side."""
    m = 0 if variant == "m0" else M
    if kind == "sparse_condensed":
        ineq, eq = np.arange(m), np.zeros(0, int)
    else:
        ineq, eq = np.arange(1, m), np.arange(min(m, 1))
    npr = N + len(ineq)
    lb = np.zeros(0, int) if variant == "nlb0" else np.array([0, 2, npr - 1])
    ub = np.zeros(0, int) if variant == "nub0" else np.array([1, 2])
    wrap = _late_bounds if late else (lambda c: c)
    if kind == "sparse_condensed":
        jI, jJ = np.divmod(np.arange(m * N), N)
        hI, hJ = np.tril_indices(N)
        ko = osc.SparseCondensedKKTSystem(N, m, jI, jJ, hI, hJ, ineq, lb, ub, lambda A: LapackCPUSolver(A, CHOLESKY))
        kh = wrap(mj.SparseCondensedKKTSystem)(N, m, jI, jJ, hI, hJ, ineq, lb, ub, ctx=ctx,
                                               opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY))
        for k in (ko, kh):
            k.jac[:] = JAC[jI, jJ]
            k.hess[:] = HESS[hI, hJ]
    else:
        fac = lambda A: LapackCPUSolver(A, BUNCHKAUFMAN)  # noqa: E731
        if kind == "dense_condensed":
            ko = odense.DenseCondensedKKTSystem(N, m, ineq, eq, lb, ub, fac)
            kh = wrap(mj.DenseCondensedKKTSystem)(N, m, ineq, eq, lb, ub, ctx=ctx)
        else:
            ko = odense.DenseKKTSystem(N, m, ineq, lb, ub, fac)
            kh = wrap(mj.DenseKKTSystem)(N, m, ineq, lb, ub, ctx=ctx)
        for k in (ko, kh):
            k.hess[...] = HESS
            k.jac[...] = JAC[:m]
    return ko, kh


def _raw(kh, name, *args):
    """The C entry point `<prefix><name>` on the handle, through `check` (HipError with the library's message)."""
    L.check(getattr(L.lib(), kh._PFX + name)(kh._h, *args), kh._PFX + name)


def _refused(kh, text, name, *args):
    with pytest.raises(L.HipError) as e:
        _raw(kh, name, *args)
    assert text.replace("PFX", kh._PFX) in str(e.value), (name, str(e.value))


def _feed(ko, kh, rng):
    """The correct sequence up to the factorization, on both systems, from one interior iterate."""
    it = _iterate(rng, len(ko.pr_diag), ko.ind_lb, ko.ind_ub)
    _oracle_feed(ko, *it, PRIMAL_REG, DUAL_REG, 0.0, 0.0)
    for k in (ko, kh):
        k.compress_jacobian()
        k.compress_hessian()
    if hasattr(kh, "_upload"):
        kh._upload()
    kh.set_aug_diagonal_device(*it, primal_reg=PRIMAL_REG, dual_reg=DUAL_REG)
    got = kh.get_diagonals_device()
    for name in DIAGS:
        np.testing.assert_array_equal(got[name], getattr(ko, name), err_msg=name)
    kh.build_kkt_device()
    ko.build_kkt()
    for k in (ko, kh):
        k.linear_solver.factorize()
    assert kh.linear_solver.inertia() == ko.linear_solver.inertia()


def _vec(ko, values):
    v = okern.UnreducedKKTVector.from_kkt(ko)
    v.values[:] = values
    return v


def _check_mul_and_solve(ko, kh, ctx, rng):
    """`mul_device` / `solve_kkt_device` against the oracle, host vectors and device tensors bit for bit the same."""
    lw = len(okern.UnreducedKKTVector.from_kkt(ko).values)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    xv, wv, bv = rng.standard_normal(lw), rng.standard_normal(lw), rng.standard_normal(lw)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.75, -0.5)):
        wo = ko.mul(_vec(ko, wv), _vec(ko, xv), alpha, beta).values
        wh = kh.mul_device(wv.copy(), xv.copy(), alpha, beta)
        assert np.abs(wh - wo).max() <= 1e-12 * np.abs(wo).max(), (alpha, beta)
        wd = kh.mul_device(dev(wv), dev(xv), alpha, beta)
        ctx.synchronize()
        np.testing.assert_array_equal(wd.cpu().numpy(), wh, err_msg=f"mul host/device {alpha} {beta}")
    bo = ko.solve_kkt(_vec(ko, bv)).values
    bh = kh.solve_kkt_device(bv.copy())
    res = lambda sol: (np.abs(ko.mul(_vec(ko, 0.0), _vec(ko, sol), 1.0, 0.0).values - bv).max()  # noqa: E731
                       / (np.abs(bv).max() + np.abs(sol).max()))
    res_h, res_o = res(bh), res(bo)
    print(f"solve_kkt residual: device {res_h:.3e}, oracle {res_o:.3e}")
    assert res_h <= max(1e-10, 100 * res_o), (res_h, res_o)
    bd = kh.solve_kkt_device(dev(bv))
    ctx.synchronize()
    np.testing.assert_array_equal(bd.cpu().numpy(), bh, err_msg="solve_kkt host/device")


@pytest.mark.parametrize("kind", KINDS)
def test_calls_out_of_order_are_refused_and_the_handle_recovers(ctx, kind):
    ko, kh = _pair(kind, ctx, late=True)
    sparse = kind == "sparse_condensed"
    npr = len(ko.pr_diag)
    buf = np.zeros(64)
    v, H = buf.ctypes.data, L.MNK_HOST
    ls = kh.linear_solver._h
    # ---- before set_bounds
    first = "PFX_{}: call PFX_set_bounds first"
    _refused(kh, first.format("set_barrier_terms"), "_set_barrier_terms", v, v, v, v, v, H)
    _refused(kh, first.format("set_aug_diagonal"), "_set_aug_diagonal", v, v, v, v, v, 0.0, 0.0, H)
    _refused(kh, first.format("set_aug_RR"), "_set_aug_RR", *([v] * 10), 0.0, 0.0, 0.0)
    _refused(kh, first.format("regularize_diagonal"), "_regularize_diagonal", 0.0, 0.0)
    _refused(kh, first.format("get_diagonals"), "_get_diagonals", *([v] * 7))
    _refused(kh, "PFX_solve_kkt: call PFX_set_bounds / PFX_set_barrier_terms / PFX_build first", "_solve_kkt", ls, v, H)
    _refused(kh, "PFX_mul: call PFX_set_bounds / PFX_set_barrier_terms first", "_mul", v, v, 1.0, 0.0, H)
    kh.set_bounds_now()
    # ---- after set_bounds, before the diagonals
    _refused(kh, "PFX_regularize_diagonal: call PFX_set_aug_diagonal first", "_regularize_diagonal", 0.0, 0.0)
    if sparse:
        _refused(kh, "mnk_sc_restore_diagonals: nothing saved (mnk_sc_save_diagonals)", "_restore_diagonals")
    # ---- bad arguments: a bound index out of range, either side, either index base (the bounds set above stay)
    for base in (0, 1):
        good = np.array([base], dtype=np.int64)
        for bad in (np.array([base - 1], dtype=np.int64), np.array([npr + base], dtype=np.int64)):
            _refused(kh, "PFX_set_bounds: lower-bound index out of range", "_set_bounds", 1, bad.ctypes.data, 1,
                     good.ctypes.data, base)
            _refused(kh, "PFX_set_bounds: upper-bound index out of range", "_set_bounds", 1, good.ctypes.data, 1,
                     bad.ctypes.data, base)
    other = mj.HipLinearSolver(np.asfortranarray(np.eye(kh._order + 1)), ctx=ctx)
    _refused(kh, "PFX_solve_kkt: the solver does not belong to this system", "_solve_kkt", other._h, v, H)
    other.close()
    # ---- recovery: the correct sequence on the same handle
    rng = np.random.default_rng(5)
    _feed(ko, kh, rng)
    if sparse:   # save -> regularize -> restore returns the bits
        before = kh.get_diagonals_device()
        kh.save_diagonals_device()
        kh.regularize_diagonal_device(1e-4, 1e-8)
        assert (kh.get_diagonals_device()["reg"] != before["reg"]).all()
        kh.restore_diagonals_device()
        after = kh.get_diagonals_device()
        for name in DIAGS:
            np.testing.assert_array_equal(after[name], before[name], err_msg=name)
    _check_mul_and_solve(ko, kh, ctx, rng)
    kh.close()


@pytest.mark.parametrize("kind,variant", [(k, v) for k in KINDS for v in ("nlb0", "nub0")]
                         + [("dense", "m0"), ("dense_condensed", "m0")])
def test_empty_bound_side_and_no_constraints(ctx, kind, variant):
    """The launch guards of the shared frames: no lower bounds, no upper bounds, no constraints."""
    ko, kh = _pair(kind, ctx, variant)
    rng = np.random.default_rng(6)
    _feed(ko, kh, rng)
    _check_mul_and_solve(ko, kh, ctx, rng)
    kh.close()


@pytest.mark.parametrize("kind", KINDS)
def test_index_base_one_gives_the_bits_of_index_base_zero(ctx, kind):
    ko, kh = _pair(kind, ctx)
    it = _iterate(np.random.default_rng(7), len(ko.pr_diag), ko.ind_lb, ko.ind_ub)
    kh.set_aug_diagonal_device(*it, primal_reg=PRIMAL_REG, dual_reg=DUAL_REG)
    zero = kh.get_diagonals_device()
    lb1, ub1 = kh.ind_lb + 1, kh.ind_ub + 1
    _raw(kh, "_set_bounds", len(lb1), lb1.ctypes.data, len(ub1), ub1.ctypes.data, 1)
    kh.set_aug_diagonal_device(*it, primal_reg=PRIMAL_REG, dual_reg=DUAL_REG)
    one = kh.get_diagonals_device()
    for name in DIAGS:
        np.testing.assert_array_equal(one[name], zero[name], err_msg=name)
        assert np.isfinite(one[name]).all()
    assert (one["l_diag"] < 0).all() and (one["u_diag"] < 0).all()      # xl - x, x - xu of an interior iterate: the terms were written
    kh.close()

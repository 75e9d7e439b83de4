"""GPU tests of COO callbacks on the dense KKT handle (csrc/dense_coo.hip: mnk_dc_coo_attach, mnk_dc_compress_jacobian /
_hessian, mnk_dc_keep_jacobian, mnk_dc_coo_jtprod, mnk_dc_get_jac) and of `DeviceMadNLPSolver(..., callback="sparse",
sparse=False)`.  The scatters and the transposed product add in COO order with contraction off, so they are held to the
sequential host loops of tests/coo_dense_cases.py bit for bit."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd import tape_model as T  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel, LootsmaModel  # noqa: E402
from tests.coo_dense_cases import (HYPERBOLA_F, HYPERBOLA_X, HYPERBOLA_Y, SIZES, host_jtprod, host_scatter_hess,  # noqa: E402
                                   host_scatter_jac, hyperbola_model, random_structure, spread_values)


@pytest.fixture()
def gpu_ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    st = torch.cuda.Stream()       # NOT torch's current stream: nothing here may depend on torch's stream order
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    yield ctx
    ctx.close()


def handle(ctx, m, n, S=None):
    """A dense condensed handle with m inequality rows; `S`: the COO structure to attach."""
    e = np.zeros(0, dtype=np.int64)
    k = mj.DenseCondensedKKTSystem(n, m, np.arange(m, dtype=np.int64), e, e, e, ctx=ctx)
    if S is not None:
        k.attach_coo(S["jac_I"], S["jac_J"], S["hess_I"], S["hess_J"])
    return k


def dev(a):
    """`a` on the device.  The library's launches are asynchronous on ANOTHER stream than torch's: the caller keeps the tensor
    alive until that stream has been synchronized (a freed block is handed to the next upload at once)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    t = t if t.numel() else torch.empty(1, dtype=torch.float64, device="cuda")[:0]
    torch.cuda.synchronize()       # the upload ran on torch's stream
    return t


# ------------------------------------------------------------------------------------------ 1. the scatter kernels
@pytest.mark.parametrize("m,n", SIZES)
def test_scatter_kernels_reproduce_the_sequential_loop(gpu_ctx, m, n):
    S = random_structure(m, n)
    k = handle(gpu_ctx, m, n, S)
    rng = np.random.default_rng(7 * m + n)
    try:
        for values in (lambda c: rng.integers(-9, 10, c).astype(float), lambda c: spread_values(rng, c)):
            jv, hv = values(len(S["jac_I"])), values(len(S["hess_I"]))
            jd, hd = dev(jv), dev(hv)
            k.compress_jacobian(jd)
            k.compress_hessian(hd)
            J, H = k.get_jac(), k.get_hess()
            assert np.array_equal(J, host_scatter_jac(m, n, S["jac_I"], S["jac_J"], jv))
            assert np.array_equal(H, host_scatter_hess(n, S["hess_I"], S["hess_J"], hv))
            assert np.array_equal(H, H.T)
        # host-resident values take the same path behind a staging copy
        k.compress_jacobian(jv[::-1].copy())
        assert np.array_equal(k.get_jac(), host_scatter_jac(m, n, S["jac_I"], S["jac_J"], jv[::-1]))
    finally:
        k.close()


def test_empty_structures_leave_zero_matrices(gpu_ctx):
    z = np.zeros(0, dtype=np.int32)
    for m, n in ((0, 3), (4, 3)):
        k = handle(gpu_ctx, m, n, dict(jac_I=z, jac_J=z, hess_I=z, hess_J=z))
        try:
            lib = L.lib()
            L.check(lib.mnk_dc_set_hess(k._h, np.ones((n, n)).ctypes.data, n, L.MNK_HOST), "mnk_dc_set_hess")
            if m:
                L.check(lib.mnk_dc_set_jac(k._h, np.ones((m, n), order="F").ctypes.data, m, L.MNK_HOST), "mnk_dc_set_jac")
            L.check(lib.mnk_dc_compress_jacobian(k._h, None, L.MNK_DEVICE), "mnk_dc_compress_jacobian")
            L.check(lib.mnk_dc_compress_hessian(k._h, None, L.MNK_DEVICE), "mnk_dc_compress_hessian")
            assert not k.get_hess().any() and not k.get_jac().any()
            out, y = dev(np.full(n, np.nan)), dev(np.ones(m))
            k.jtprod_coo_device(L.MNK_DC_JAC_CURRENT, y, out)
            gpu_ctx.synchronize()
            assert np.array_equal(out.cpu().numpy(), np.zeros(n))
        finally:
            k.close()


# ------------------------------------------------------------------------------------------ 2. clear-if-dirty
@pytest.mark.parametrize("m,n", SIZES[1:3])
def test_a_dense_load_or_a_quasi_newton_write_is_cleared_before_the_scatter(gpu_ctx, m, n):
    S = random_structure(m, n)
    k = handle(gpu_ctx, m, n, S)
    lib = L.lib()
    rng = np.random.default_rng(m)
    structural_j = host_scatter_jac(m, n, S["jac_I"], S["jac_J"], np.ones(len(S["jac_I"]))) != 0
    structural_h = host_scatter_hess(n, S["hess_I"], S["hess_J"], np.ones(len(S["hess_I"]))) != 0
    try:
        L.check(lib.mnk_dc_set_jac(k._h, np.ones((m, n), order="F").ctypes.data, m, L.MNK_HOST), "mnk_dc_set_jac")
        L.check(lib.mnk_dc_set_hess(k._h, np.ones((n, n), order="F").ctypes.data, n, L.MNK_HOST), "mnk_dc_set_hess")
        jv, hv = spread_values(rng, len(S["jac_I"])), spread_values(rng, len(S["hess_I"]))
        jd, hd = dev(jv), dev(hv)
        k.compress_jacobian(jd)
        k.compress_hessian(hd)
        J, H = k.get_jac(), k.get_hess()
        assert (J[~structural_j] == 0.0).all() and (H[~structural_h] == 0.0).all()
        assert np.array_equal(J, host_scatter_jac(m, n, S["jac_I"], S["jac_J"], jv))
        assert np.array_equal(H, host_scatter_hess(n, S["hess_I"], S["hess_J"], hv))
        # a second compress holds no trace of the first
        jv2, hv2 = rng.integers(1, 5, len(jv)).astype(float), rng.integers(1, 5, len(hv)).astype(float)
        jd2, hd2 = dev(jv2), dev(hv2)
        k.compress_jacobian(jd2)
        k.compress_hessian(hd2)
        assert np.array_equal(k.get_jac(), host_scatter_jac(m, n, S["jac_I"], S["jac_J"], jv2))
        assert np.array_equal(k.get_hess(), host_scatter_hess(n, S["hess_I"], S["hess_J"], hv2))
        # the quasi-Newton init! fills the diagonal: (most of) it lies outside the structure
        k.qn_init_device("bfgs", np.ones(n), 1.0)
        assert (np.diagonal(k.get_hess()) != 0.0).all()
        k.compress_hessian(hd2)
        assert np.array_equal(k.get_hess(), host_scatter_hess(n, S["hess_I"], S["hess_J"], hv2))
    finally:
        k.close()


# ------------------------------------------------------------------------------------------ 3. the transposed product
@pytest.mark.parametrize("m,n", SIZES)
def test_transposed_product_on_current_and_kept_values(gpu_ctx, m, n):
    S = random_structure(m, n)
    k = handle(gpu_ctx, m, n, S)
    rng = np.random.default_rng(3 * m + n)
    I, J = S["jac_I"], S["jac_J"]
    try:
        v1, v2, v3 = (spread_values(rng, len(I)) for _ in range(3))
        d1, d2, d3 = dev(v1), dev(v2), dev(v3)
        y = dev(rng.standard_normal(m))
        yh = y.cpu().numpy()
        out = dev(np.full(n, np.nan))

        def product(which):
            k.jtprod_coo_device(which, y, out)
            gpu_ctx.synchronize()
            return out.cpu().numpy().copy()
        k.compress_jacobian(d1)
        assert np.array_equal(product(L.MNK_DC_JAC_CURRENT), host_jtprod(n, I, J, v1, yh))
        k.keep_jacobian_device()
        k.compress_jacobian(d2)
        assert np.array_equal(product(L.MNK_DC_JAC_CURRENT), host_jtprod(n, I, J, v2, yh))
        assert np.array_equal(product(L.MNK_DC_JAC_KEPT), host_jtprod(n, I, J, v1, yh))      # untouched by the compress
        k.compress_jacobian(d3)
        assert np.array_equal(product(L.MNK_DC_JAC_KEPT), host_jtprod(n, I, J, v1, yh))
        k.keep_jacobian_device()
        assert np.array_equal(product(L.MNK_DC_JAC_KEPT), host_jtprod(n, I, J, v3, yh))
        empty = np.setdiff1d(np.arange(n), J)
        assert (product(L.MNK_DC_JAC_CURRENT)[empty] == 0.0).all()                          # a column nothing feeds
    finally:
        k.close()


# ------------------------------------------------------------------------------------------ 4. errors without a launch
def test_errors_are_reported_without_a_launch(gpu_ctx):
    lib = L.lib()
    m, n = SIZES[1]
    S = random_structure(m, n)
    k = handle(gpu_ctx, m, n)
    v = dev(np.ones(len(S["jac_I"]) + len(S["hess_I"])))
    err = lambda: lib.mnk_last_error_string()  # noqa: E731
    p = lambda a: a.ctypes.data  # noqa: E731
    try:
        for call in (lambda: lib.mnk_dc_compress_jacobian(k._h, v.data_ptr(), L.MNK_DEVICE),
                     lambda: lib.mnk_dc_compress_hessian(k._h, v.data_ptr(), L.MNK_DEVICE),
                     lambda: lib.mnk_dc_keep_jacobian(k._h),
                     lambda: lib.mnk_dc_coo_jtprod(k._h, L.MNK_DC_JAC_CURRENT, v.data_ptr(), v.data_ptr())):
            assert call() < 0 and b"mnk_dc_coo_attach first" in err()
        with pytest.raises(mj.HipError, match="mnk_dc_coo_attach first"):
            k.compress_jacobian(v)
        jI, jJ, hI, hJ = (S[key].copy() for key in ("jac_I", "jac_J", "hess_I", "hess_J"))
        attach = lambda a, b, c, d, base=0, nj=len(jI), nh=len(hI): lib.mnk_dc_coo_attach(  # noqa: E731
            k._h, nj, p(a), p(b), nh, p(c), p(d), base)
        for key, bad in (("jI", m), ("jJ", n), ("hI", n), ("hJ", -1)):
            arrs = dict(jI=jI.copy(), jJ=jJ.copy(), hI=hI.copy(), hJ=hJ.copy())
            arrs[key][3] = bad
            assert attach(*arrs.values()) < 0 and b"out of range" in err()
        assert attach(jI, jJ, hI, hJ, base=1) < 0 and b"out of range" in err()         # index 0 with base 1
        assert lib.mnk_dc_coo_attach(k._h, 2 ** 31, None, None, 0, None, None, 0) < 0 and b"int32" in err()
        assert lib.mnk_dc_coo_attach(k._h, 3, None, None, 0, None, None, 0) < 0 and b"NULL" in err()
        assert attach(jI + 1, jJ + 1, hI + 1, hJ + 1, base=1) == 0                    # the refused calls attached nothing
        assert attach(jI, jJ, hI, hJ) < 0 and b"already" in err()
        assert lib.mnk_dc_compress_jacobian(k._h, None, L.MNK_DEVICE) < 0 and b"NULL" in err()
        assert lib.mnk_dc_compress_hessian(k._h, None, L.MNK_DEVICE) < 0 and b"NULL" in err()
        assert lib.mnk_dc_coo_jtprod(k._h, L.MNK_DC_JAC_KEPT, v.data_ptr(), v.data_ptr()) < 0 and b"mnk_dc_keep_jacobian" in err()
        assert lib.mnk_dc_coo_jtprod(k._h, 2, v.data_ptr(), v.data_ptr()) < 0
        out = np.zeros((m, n), order="F")
        assert lib.mnk_dc_get_jac(k._h, p(out), m - 1, L.MNK_HOST) < 0                  # ld < m
        assert not k.get_jac().any() and not k.get_hess().any()                       # nothing was written
    finally:
        k.close()


# ------------------------------------------------------------------------------------------ 5. tape callbacks into the handle
def test_tape_callbacks_feed_the_dense_handle(gpu_ctx):
    """tests/test_hip_tape.py's `edge_model()` and its two rules: the destinations fed by + - * / patterns alone are bit-equal
    to the host scatter of the numpy interpreter's values, all are within 1e-13 of the matrix's scale."""
    from madnlp_jl_amd.ipm_dev import DeviceTapeCallbacks
    from madnlp_jl_amd.ipm_device import IPMDeviceKernels
    from tests.test_hip_tape import edge_model, exact_masks
    M = edge_model()
    m, n = M.m, M.n
    S = dict(jac_I=M.jac_I, jac_J=M.jac_J, hess_I=M.hess_I, hess_J=M.hess_J)
    k = handle(gpu_ctx, m, n, S)
    K = IPMDeviceKernels(n, np.arange(1), np.arange(1), ctx=gpu_ctx)
    cb = DeviceTapeCallbacks(M, k, "cuda", K)
    jmask, hmask, _ = exact_masks(M)
    exact_j = host_scatter_jac(m, n, M.jac_I, M.jac_J, (~jmask).astype(float)) == 0     # no transcendental entry feeds it
    exact_h = host_scatter_hess(n, M.hess_I, M.hess_J, (~hmask).astype(float)) == 0
    assert (~exact_j).any() and (~exact_h).any()
    rng = np.random.default_rng(8)
    try:
        for sigma in (1.0, 0.0, 0.37):
            x, y = rng.uniform(0.5, 1.5, n), rng.standard_normal(m)
            y[::7] = 0.0
            xd, yd = dev(x), dev(y)
            cb.load_jac(xd)
            cb.load_hess(xd, yd, sigma)
            J, H = k.get_jac(), k.get_hess()
            rJ = host_scatter_jac(m, n, M.jac_I, M.jac_J, M.jac_coord(x))
            rH = host_scatter_hess(n, M.hess_I, M.hess_J, M.hess_coord(x, y, sigma))
            assert np.array_equal(J[exact_j], rJ[exact_j]) and np.array_equal(H[exact_h], rH[exact_h])
            assert np.abs(J - rJ).max() <= 1e-13 * np.abs(rJ).max() and np.abs(H - rH).max() <= 1e-13 * np.abs(rH).max()
            assert np.array_equal(H, H.T)
            out = dev(np.full(n, np.nan))
            cb.jtprod_x(out, yd)
            gpu_ctx.synchronize()
            ref = host_jtprod(n, M.jac_I, M.jac_J, M.jac_coord(x), y)
            assert np.abs(out.cpu().numpy() - ref).max() <= 1e-13 * np.abs(ref).max()
    finally:
        cb.close(), K.close(), k.close()


# ------------------------------------------------------------------------------------------ 6. device-resident runs
def _second_optimum(sol):
    return np.abs(sol.solution - np.array([-0.7921, -1.2624])).max() < 1e-4 and abs(sol.objective - 360.3798) < 1e-3


def _first_optimum(sol):
    return np.abs(sol.solution - np.array([0.5, 2.0])).max() < 1e-4 and abs(sol.objective - 306.49998) < 1e-3


def _lootsma(sol):
    return (np.abs(sol.solution - LootsmaModel.LOOTSMA_X).max() < 1e-4 and np.abs(sol.multipliers - LootsmaModel.LOOTSMA_Y).max() < 1e-4
            and abs(sol.objective - 3.18222774) < 1e-4)


def _hyperbola(sol):
    return (np.abs(sol.solution - HYPERBOLA_X).max() < 1e-4 and abs(sol.objective - HYPERBOLA_F) < 1e-4
            and np.abs(sol.multipliers - HYPERBOLA_Y).max() < 1e-4)


def _acopf(sol):
    A = ACOPFModel("case30")
    c = A.cons(sol.solution)           # feasibility judged by the hand-written host model
    return (c >= A.lcon - 1e-5).all() and (c <= A.ucon + 1e-5).all() and abs(sol.objective - 107.2713518) <= 1e-5 * 107.2713518


RUNS = {
    "hs15": (T.hs15_tape_model, {}, _second_optimum),
    "lootsma": (T.lootsma_tape_model, {}, _lootsma),
    "hyperbola": (hyperbola_model, {}, _hyperbola),
    "hyperbola-scaled": (hyperbola_model, dict(nlp_scaling=True), _hyperbola),
    "hs15-bfgs": (T.hs15_tape_model, dict(hessian_approximation="bfgs"), _first_optimum),
    "hs15-damped": (T.hs15_tape_model, dict(hessian_approximation="damped_bfgs"), _first_optimum),
    "hyperbola-bfgs": (hyperbola_model, dict(hessian_approximation="bfgs"), _hyperbola),
    "hyperbola-damped": (hyperbola_model, dict(hessian_approximation="damped_bfgs"), _hyperbola),
    "acopf-tape": (lambda: T.acopf_tape_model("case30"), {}, _acopf),
    "acopf": (lambda: ACOPFModel("case30"), {}, _acopf),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_device_resident_run_with_coo_callbacks(gpu_ctx, monkeypatch, name):
    """`DeviceMadNLPSolver(..., callback="sparse", sparse=False)` on `DenseCondensedKKTSystem` with the equalities enforced,
    against the host driver with the same options on the same HIP factory: the conditions of
    test_hip_quasi_newton.test_device_resident_quasi_newton_run and test_hip_tape.test_device_resident_tape_acopf_run."""
    from madnlp_jl_amd.device_callbacks import DeviceCOOCallbacks, DeviceOPFCallbacks, DeviceTapeCallbacks
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    make, kw, answer = RUNS[name]

    def factory(info):
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=gpu_ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                          device_kkt_ops=True)
    opt = lambda: IPMOptions(callback="sparse", tol=1e-8, **kw)  # noqa: E731
    sh = MadNLPSolver(make(), factory, opt(), sparse=False)
    sh.solve()
    hess_calls = [0]
    for cls in (DeviceTapeCallbacks, DeviceOPFCallbacks):
        def counted(self, *a, _real=cls.hess_coord, **k):
            hess_calls[0] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(cls, "hess_coord", counted)
    nlp = make()
    sd = DeviceMadNLPSolver(nlp, factory, opt(), sparse=False)
    try:
        sd.solve()
        monkeypatch.undo()
        x, y, zl, zu = sd.host_state()
        sol = sd.solution()
        qn = "hessian_approximation" in kw
        print(f"{name}: device {sd.status} k {sd.cnt.k} fact {sd.cnt.factorization_cnt}; host {sh.status} k {sh.cnt.k} fact "
              f"{sh.cnt.factorization_cnt}; hess_coord launches {hess_calls[0]}; x {sol.solution[:3]} f {sol.objective!r} "
              f"max|dx| {np.abs(x - sh.x).max():.3e} max|dy| {np.abs(y - sh.y).max():.3e}")
        assert isinstance(sd.cb, DeviceCOOCallbacks) and sd.kkt.coo_attached and sd.m - sd.ns == int((nlp.lcon == nlp.ucon).sum())
        assert sd.status == sh.status == "SOLVE_SUCCEEDED"
        assert (sd.cnt.k, sd.cnt.factorization_cnt) == (sh.cnt.k, sh.cnt.factorization_cnt)
        if qn:
            u, sk, _ = sd.kkt.qn_status()
            assert (u, sk) == (sh.qn.updates, sh.qn.skipped) and u + sk == sd.cnt.k - 1
            assert hess_calls[0] == 0 and sd.cnt.lag_hess_cnt == sh.cnt.lag_hess_cnt == 0
        else:
            assert hess_calls[0] >= 1 and sd.cnt.lag_hess_cnt == sh.cnt.lag_hess_cnt
        np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
        np.testing.assert_allclose(y, sh.y, rtol=0, atol=1e-6 * max(1.0, np.abs(sh.y).max()))
        assert len(sd.history) == len(sh.history)
        for a, b in zip(sd.history, sh.history):
            assert a.k == b.k
            for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
                va, vb = getattr(a, fld), getattr(b, fld)
                assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)
        assert answer(sol), (sol.solution[:4], sol.objective, sol.multipliers[:4])
    finally:
        sd.close()
        sh.kkt.close()


def test_refusals_of_the_device_driver():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import DenseQPModel
    with pytest.raises(NotImplementedError, match="sparse condensed KKT handle only"):      # "auto": as before
        DeviceMadNLPSolver(T.hs15_tape_model(), lambda info: None, IPMOptions(), sparse=False)
    with pytest.raises(NotImplementedError, match="callback = 'sparse'.*make_parameter"):
        DeviceMadNLPSolver(T.lootsma_fixed_tape_model(), lambda info: None,
                           IPMOptions(callback="sparse", fixed_variable_treatment="make_parameter"), sparse=False)
    with pytest.raises(NotImplementedError, match="callback = 'dense'.*jac_dense"):
        DeviceMadNLPSolver(T.hs15_tape_model(), lambda info: None, IPMOptions(callback="dense"), sparse=False)
    with pytest.raises(NotImplementedError, match="callback = 'sparse'.*dense QP"):
        DeviceMadNLPSolver(DenseQPModel(4, 2, 0), lambda info: None, IPMOptions(callback="sparse"), sparse=False)

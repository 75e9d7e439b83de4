"""GPU tests of the device quasi-Newton Hessians (csrc/qn.hip, through the C ABI: mnk_dc_qn_init / _update / _status,
mnk_dc_get_hess) against the host mirror (`madnlp_jl_amd.quasi_newton`) and the longdouble formula of tests/qn_cases.py.

Error rule of the random cases: the device may sum in another order than numpy, so it is held to the host mirror's own
error against the longdouble formula times a small factor, with the float64 resolution of the entries as the floor:
    err_device <= max(8 err_host, 16 eps scale),      err = max |tril(B - B'_longdouble)|,
`scale` = the sizes of the three terms of an entry (qn_cases.formula)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import DenseQPModel, HS15Model, LootsmaModel, dense_dummy_qp  # noqa: E402
from madnlp_jl_amd.quasi_newton import create_quasi_newton, rho0  # noqa: E402
from oracle import dense as odense  # noqa: E402
from oracle import kernels as okern  # noqa: E402
from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver  # noqa: E402
from qn_cases import EPS, LD, exact_case, formula, random_case, sym_lower, tril_err  # noqa: E402

APPROX = ("bfgs", "damped_bfgs")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def bare(ctx, n):
    """A dense handle with no constraints: only its Hessian buffer is used."""
    e = np.zeros(0, dtype=np.int64)
    return mj.DenseCondensedKKTSystem(n, 0, e, e, e, e, ctx=ctx)


def device_update(k, B, s, y, kind, first=False):
    """B (host, NaN in the strict upper triangle) -> the handle, one update, the result back."""
    if first:
        k.qn_init_device(kind, np.ones(len(s)), 1.0)      # not instantiated; the matrix is replaced next
        k.set_hess_device(B)
    else:
        k.set_hess_device(B)
        k.qn_init_device(kind, None)                      # adopt
    k.qn_update_device(s, y)
    return k.get_hess()


def host_update(B, s, y, kind, first=False):
    B = B.copy()
    qn = create_quasi_newton(kind, len(s))
    if not first:
        qn.adopt()
    qn.update(B, s, y)
    return B, qn


def check_random(Bd, Bh, ref, n, tag):
    err_d, err_h = tril_err(Bd, ref["B1"]), tril_err(Bh, ref["B1"])
    bound = max(8 * err_h, 16 * EPS * ref["scale"])
    print(f"{tag}: err_device {err_d:.3e} err_host {err_h:.3e} bound {bound:.3e}")
    assert err_d <= bound


# ------------------------------------------------------------------------------------------ 7. exact answers
@pytest.mark.parametrize("n", [5, 64, 65, 257, 1000])
@pytest.mark.parametrize("kind", APPROX)
@pytest.mark.parametrize("first", [False, True])
def test_exact_answer_cases(ctx, n, kind, first):
    """Integer inputs with s'y = s'Bs = a power of two (tests/test_quasi_newton_cpu.py shows host mirror == longdouble formula
    on them): the device's lower triangle equals the host mirror's bit for bit, the strict upper triangle is untouched."""
    B, s, y = exact_case(n, 11 * n + first, kind, first)
    k = bare(ctx, n)
    try:
        Bd = device_update(k, B, s, y, kind, first)
        Bh, qn = host_update(B, s, y, kind, first)
        assert np.array_equal(np.tril(Bd), np.tril(Bh))
        assert np.isnan(Bd[np.triu_indices(n, 1)]).all()
        u, sk, last = k.qn_status()
        assert (u, sk) == (1, 0) and np.array_equal(last, qn.last)
    finally:
        k.close()


# ------------------------------------------------------------------------------------------ 8. random cases
@pytest.mark.parametrize("n", [7, 130, 1023, 2048])
@pytest.mark.parametrize("mode", ["bfgs", "damped", "damped_lt1"])
def test_random_cases(ctx, n, mode):
    B, s, y, kind = random_case(n, 500 + n, mode)
    ref = formula(B, s, y, kind)
    assert (float(ref["theta"]) < 1.0) == (mode == "damped_lt1")
    k = bare(ctx, n)
    try:
        Bd = device_update(k, B, s, y, kind)
        Bh, qn = host_update(B, s, y, kind)
        check_random(Bd, Bh, ref, n, f"n={n} {mode}")
        assert np.isnan(Bd[np.triu_indices(n, 1)]).all()
        u, sk, last = k.qn_status()
        assert (u, sk) == (1, 0)
        np.testing.assert_allclose(last, qn.last, rtol=64 * n * EPS, atol=0)
    finally:
        k.close()


@pytest.mark.parametrize("n", [7, 130, 1023])
def test_bfgs_skip_leaves_the_matrix_alone(ctx, n):
    B, s, y, kind = random_case(n, 40 + n, "skip")
    k = bare(ctx, n)
    try:
        Bd = device_update(k, B, s, y, "bfgs")
        assert Bd.tobytes() == B.tobytes()
        u, sk, last = k.qn_status()
        assert (u, sk) == (0, 1)
        np.testing.assert_allclose(last[0], s @ y, rtol=64 * n * EPS)
        k.qn_update_device(s, -y)                        # the next one is performed
        assert k.qn_status()[:2] == (1, 1)
        # the damped update does not skip
        Bd = device_update(k, B, s, y, "damped_bfgs")
        Bh, _ = host_update(B, s, y, "damped_bfgs")
        ref = formula(B, s, y, "damped_bfgs")
        assert float(ref["theta"]) < 1.0
        check_random(Bd, Bh, ref, n, f"n={n} damped on the skipped pair")
        assert k.qn_status()[:2] == (1, 0)
    finally:
        k.close()


@pytest.mark.parametrize("n", [7, 130, 1023])
@pytest.mark.parametrize("kind", APPROX)
def test_first_update_after_init(ctx, n, kind):
    rng = np.random.default_rng(n)
    g0, f0 = rng.standard_normal(n), -3.5
    _, s, y, _ = random_case(n, 900 + n, "bfgs")
    k = bare(ctx, n)
    try:
        k.set_hess_device(np.full((n, n), 7.0))
        k.qn_init_device(kind, g0, f0)
        B0 = k.get_hess()
        d = 2.0 * rho0(g0, f0)
        assert np.array_equal(B0 - np.diag(np.diag(B0)), np.zeros((n, n)))          # init!: zero off the diagonal ...
        np.testing.assert_allclose(np.diag(B0), d, rtol=4 * n * EPS)                 # ... 2 rho0 on it (g0'g0: n terms, summed in another order)
        for gz, fz, want in ((g0 * 1e-9, f0, 2.0), (g0, 0.0, 2.0 / (g0 @ g0))):     # the other two branches of rho0
            k.qn_init_device(kind, gz, fz)
            np.testing.assert_allclose(np.diag(k.get_hess()), want, rtol=4 * n * EPS)
        k.qn_init_device(kind, g0, f0)
        k.qn_update_device(s, y)
        Bd = k.get_hess()
        Bh = np.zeros((n, n), order="F")
        qn = create_quasi_newton(kind, n)
        qn.init(Bh, g0, f0)
        qn.update(Bh, s, y)
        ref = formula(np.diag(np.full(n, d)), s, y, kind, first=True)
        check_random(Bd, Bh, ref, n, f"n={n} {kind} first")
        assert np.array_equal(np.triu(Bd, 1), np.zeros((n, n)))                       # the strict upper triangle stays as init! left it
    finally:
        k.close()


# ------------------------------------------------------------------------------------------ 9. a sequence
@pytest.mark.parametrize("kind", APPROX)
def test_sequence_of_updates_is_accurate_and_reproducible(ctx, kind):
    n, steps = 512, 20
    rng = np.random.default_rng(77)
    A = rng.standard_normal((n, 48))
    M = A @ A.T / 48 + np.eye(n)
    g0, f0 = rng.standard_normal(n), 2.0
    pairs = []
    for _ in range(steps):
        s = rng.standard_normal(n)
        pairs.append((s, M @ s + 0.1 * rng.standard_normal(n)))
    Bh = np.zeros((n, n), order="F")
    qn = create_quasi_newton(kind, n)
    qn.init(Bh, g0, f0)
    Bl, first = np.diag(np.full(n, 2.0 * rho0(g0, f0))).astype(LD), True
    for s, y in pairs:
        assert s @ y > 1e-8
        qn.update(Bh, s, y)
        ref = formula(Bl, s, y, kind, first)
        Bl, first = ref["B1"], False
    runs = []
    for _ in range(2):
        k = bare(ctx, n)
        try:
            k.qn_init_device(kind, g0, f0)
            for s, y in pairs:
                k.qn_update_device(s, y)
            runs.append(k.get_hess())
            u, sk, last = k.qn_status()
            assert (u, sk) == (steps, 0)
        finally:
            k.close()
    assert np.array_equal(runs[0], runs[1])                           # bitwise reproducible run to run
    check_random(runs[0], Bh, ref, n, f"{kind} after {steps} updates")


# ------------------------------------------------------------------------------------------ 10. build_kkt! reads the updated matrix
@pytest.mark.parametrize("condensed", [True, False])
def test_build_uses_the_updated_matrix(ctx, condensed):
    n, m, n_eq = 50, 10, 2 if condensed else 0
    P = dense_dummy_qp(n, m, n_eq)
    fac = lambda A: LapackCPUSolver(A, BUNCHKAUFMAN)  # noqa: E731
    opt = mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN)
    if condensed:
        ko = odense.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, fac)
        kh = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx, opt_linear_solver=opt)
    else:
        ko = odense.DenseKKTSystem(P.n, P.m, P.ind_ineq, P.ind_lb, P.ind_ub, fac)
        kh = mj.DenseKKTSystem(P.n, P.m, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx, opt_linear_solver=opt)
    try:
        for k in (ko, kh):
            for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
                getattr(k, f)[:] = getattr(P, f)
            k.jac[...] = P.jac
        okern.set_aug_diagonal(ko)
        kh.set_aug_diagonal()
        rng = np.random.default_rng(3)
        s = rng.standard_normal(n)
        y = sym_lower(P.hess) @ s + 0.5 * s
        kh.set_hess_device(P.hess)
        kh.qn_init_device("bfgs", None)
        kh.qn_update_device(s, y)
        lib = L.lib()
        L.check(lib.mnk_dc_set_jac(kh._h, kh.jac.ctypes.data, kh.jac.shape[0], L.MNK_HOST), "mnk_dc_set_jac")
        L.check(lib.mnk_dc_build(kh._h, kh.pr_diag.ctypes.data, kh.du_diag.ctypes.data, L.MNK_HOST), "mnk_dc_build")   # no upload of hess
        Hd = kh.get_hess()
        assert np.abs(np.tril(Hd) - np.tril(P.hess)).max() > 1e-3      # it was updated
        ko.hess[...] = sym_lower(Hd)
        ko.compress_hessian(); ko.compress_jacobian()
        ko.build_kkt()
        Ko, Kh = np.tril(ko.aug_com), np.tril(kh.aug_com.to_host())
        if condensed:
            assert np.abs(Kh - Ko).max() <= 1e-12 * np.abs(Ko).max()   # tests/test_hip_parity.py: the Gram product's tolerance
        else:
            np.testing.assert_array_equal(Kh, Ko)                      # pure scatter: bit-exact
    finally:
        kh.close()


@pytest.mark.parametrize("n", [1, 7, 1023])
@pytest.mark.parametrize("constrained", [True, False])
def test_secant_pair_in_one_launch(ctx, n, constrained):
    """`mnk_dc_qn_secant`: elementwise, the host mirror's operations in its order, so bit for bit its results."""
    rng = np.random.default_rng(n)
    x, g, jl, jv, lx, lg = (rng.standard_normal(n) for _ in range(6))
    dev = lambda a: torch.from_numpy(a.copy()).to("cuda")  # noqa: E731
    k = bare(ctx, n)
    try:
        dx, dg, dlx, dlg = dev(x), dev(g), dev(lx), dev(lg)
        djl, djv = (dev(jl), dev(jv)) if constrained else (None, None)
        ds, dy = torch.empty_like(dx), torch.empty_like(dx)
        k.qn_secant_device(dx, dg, djl, djv, dlx, dlg, ds, dy)
        ctx.synchronize()
        yk = g - lg
        if constrained:
            yk = yk + jl
            yk = yk - jv
        assert np.array_equal(ds.cpu().numpy(), x - lx) and np.array_equal(dy.cpu().numpy(), yk)
        assert np.array_equal(dlx.cpu().numpy(), x) and np.array_equal(dlg.cpu().numpy(), g)
        assert L.lib().mnk_dc_qn_secant(k._h, dx.data_ptr(), dg.data_ptr(), dx.data_ptr(), None, dlx.data_ptr(), dlg.data_ptr(),
                                        ds.data_ptr(), dy.data_ptr()) < 0          # jl without jv
    finally:
        k.close()


def test_calls_before_init_are_errors(ctx):
    k = bare(ctx, 8)
    try:
        lib = L.lib()
        v = torch.zeros(8, dtype=torch.float64, device="cuda")
        assert lib.mnk_dc_qn_update(k._h, v.data_ptr(), v.data_ptr()) < 0
        assert b"mnk_dc_qn_init first" in lib.mnk_last_error_string()
        assert lib.mnk_dc_qn_status(k._h, None, None, None) < 0
        assert lib.mnk_dc_qn_init(k._h, 3, None, 0.0) < 0 and b"kind" in lib.mnk_last_error_string()
        assert lib.mnk_dc_qn_update(k._h, None, v.data_ptr()) < 0
        out = np.zeros((8, 8), order="F")
        assert lib.mnk_dc_get_hess(k._h, out.ctypes.data, 4, L.MNK_HOST) < 0      # ld < n
        with pytest.raises(mj.HipError):
            k.qn_update_device(np.zeros(8), np.zeros(8))
    finally:
        k.close()


# ------------------------------------------------------------------------------------------ 11. end to end, device resident
@pytest.mark.parametrize("approx,n,m,n_eq", [("bfgs", 50, 10, 0), ("damped_bfgs", 50, 10, 0), ("bfgs", 20, 15, 2),
                                             ("damped_bfgs", 20, 15, 2), ("damped_bfgs", 200, 60, 8)])
def test_device_resident_quasi_newton_run(monkeypatch, approx, n, m, n_eq):
    """`DeviceMadNLPSolver` on `DenseCondensedKKTSystem` against the host mirror on the same HIP KKT factory: the approximation
    is updated in the handle's device buffer and never loaded (no `load_hess`, no `mnk_dc_set_hess` once the loop runs).
    Tolerances: those of tests/test_ipm_dev_driver.py::test_device_resident_ipm_on_the_dense_condensed_system."""
    from madnlp_jl_amd.ipm_dev import DeviceDenseQPCallbacks, DeviceMadNLPSolver
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    try:
        nlp = DenseQPModel(n, m, n_eq)

        def factory(info):
            return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                              ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                              device_kkt_ops=True)

        opt = lambda: IPMOptions(tol=1e-8, hessian_approximation=approx)  # noqa: E731
        sh = MadNLPSolver(nlp, factory, opt(), sparse=False)
        sh.solve()
        sd = DeviceMadNLPSolver(nlp, factory, opt(), sparse=False)
        sd.initialize()          # host, once (its least-squares multipliers factorize the host system) ...
        sd._upload()             # ... then everything lives on the device
        calls = {"load_hess": 0, "set_hess": 0}
        lib = L.lib()
        real_set, real_load = lib.mnk_dc_set_hess, DeviceDenseQPCallbacks.load_hess

        def counted_set(*a):
            calls["set_hess"] += 1
            return real_set(*a)

        def counted_load(self, *a, **kw):
            calls["load_hess"] += 1
            return real_load(self, *a, **kw)

        monkeypatch.setattr(lib, "mnk_dc_set_hess", counted_set, raising=False)
        monkeypatch.setattr(DeviceDenseQPCallbacks, "load_hess", counted_load)
        sd.solve()
        monkeypatch.undo()
        print(f"{approx} ({n},{m},{n_eq}): device {sd.status} k {sd.cnt.k} fact {sd.cnt.factorization_cnt}; host {sh.status} "
              f"k {sh.cnt.k} fact {sh.cnt.factorization_cnt}; host updates {sh.qn.updates} skipped {sh.qn.skipped}")
        assert calls == {"load_hess": 0, "set_hess": 0}
        assert sd.status == sh.status == "SOLVE_SUCCEEDED"
        assert (sd.cnt.k, sd.cnt.factorization_cnt) == (sh.cnt.k, sh.cnt.factorization_cnt)
        assert sd.cnt.lag_hess_cnt == sh.cnt.lag_hess_cnt == 0
        u, sk, _ = sd.kkt.qn_status()
        # init! is the call at k = 0 (host initialization); every later iteration but the last (which stops at its convergence
        # test) updates once, and these runs never enter a restoration phase
        assert all(r.phase == "" for r in sd.history)
        assert u + sk == sd.cnt.k - 1
        assert (u, sk) == (sh.qn.updates, sh.qn.skipped)
        x, y, zl, zu = sd.host_state()
        print(f"   max|dx| {np.abs(x - sh.x).max():.3e} max|dy| {np.abs(y - sh.y).max():.3e}")
        np.testing.assert_allclose(x, sh.x, rtol=0, atol=1e-7 * max(1.0, np.abs(sh.x).max()))
        np.testing.assert_allclose(y, sh.y, rtol=0, atol=1e-6 * max(1.0, np.abs(sh.y).max()))
        for a, b in zip(sd.history, sh.history):
            assert a.k == b.k
            for fld in ("inf_pr", "inf_du", "inf_compl", "mu"):
                va, vb = getattr(a, fld), getattr(b, fld)
                assert abs(va - vb) <= 1e-5 * abs(vb) + 1e-9, (a.k, fld, va, vb)
        sh.kkt.close(); sd.kkt.close(); sd.K.close()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        ctx.close()


def test_device_driver_refuses_sparse_quasi_newton():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    with pytest.raises(ValueError, match="dense"):
        DeviceMadNLPSolver(DenseQPModel(10, 5, 0), lambda info: None, IPMOptions(hessian_approximation="bfgs"), sparse=True)


# ------------------------------------------------------------------------------------------ 12. host mirror on the HIP KKT systems
def hip_factory(ctx, kind):
    opt = mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN)

    def make(info):
        if kind == "dense_condensed":
            return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                              info["ind_ub"], ctx=ctx, opt_linear_solver=opt)
        return mj.DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx,
                                 opt_linear_solver=opt)
    return make


@pytest.mark.parametrize("approx", APPROX)
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_lootsma_and_hs15_on_the_hip_kkt_systems(ctx, kind, approx):
    nlp = LootsmaModel()
    s = MadNLPSolver(nlp, hip_factory(ctx, kind), IPMOptions(tol=1e-8, hessian_approximation=approx), sparse=False)
    s.solve()
    assert s.status == "SOLVE_SUCCEEDED", s.status
    tol = np.sqrt(s.opt.tol)
    cmp = lambda a, b: (np.abs(a - b).max() < tol) or (np.abs(a - b).max() / np.abs(b).max() < tol)  # noqa: E731  (solcmp)
    assert cmp(s.x[:3], nlp.LOOTSMA_X), s.x[:3]
    assert cmp(s.y, nlp.LOOTSMA_Y), s.y
    assert s.cnt.lag_hess_cnt == 0
    s.kkt.close()
    s = MadNLPSolver(HS15Model(), hip_factory(ctx, kind), IPMOptions(tol=1e-8, hessian_approximation=approx), sparse=False)
    s.solve()
    assert s.status == "SOLVE_SUCCEEDED", s.status
    near = lambda p: np.abs(s.x[:2] - np.array(p)).max() < 2e-3  # noqa: E731
    assert near([0.5, 2.0]) or near([-0.7921, -1.2624]), s.x[:2]
    assert max(s.inf_pr, s.inf_du, s.inf_compl_v) <= s.opt.tol
    assert s.cnt.lag_hess_cnt == 0
    s.kkt.close()

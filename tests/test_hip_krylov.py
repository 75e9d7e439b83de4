"""The GMRES refinement on the device (`iterator = "krylov"`): the kernels of csrc/krylov.hip against the numpy mirror
(`backsolve.KrylovIterator.dots / project / axpy`) bit for bit, their argument checks, `_solve_refine_krylov` on a stale
factorization and on a dense handle against the host mirror on the same handle, and whole device runs against the Richardson
runs.  One stream, the HIP KKT back-end, as tests/test_ipm_dev_driver.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)      # torch ops and the library share ONE stream
    c = mj.HipContext(0, stream=st.cuda_stream)
    yield c
    torch.cuda.set_stream(torch.cuda.default_stream())
    c.close()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def down(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernels, bit for bit
class Basis:
    """k + 1 columns of length n in a (k + 1, ldv) buffer, NaN in the padding of every column; u and x with three NaN words
    behind their n entries."""

    def __init__(self, n, k, ldv, cols, u, x):
        self.n, self.k, self.ldv = n, k, ldv
        V = np.full((k + 1, ldv), np.nan)
        V[:, :n] = cols
        self.V0 = V.copy()
        self.u0 = np.concatenate([u, np.full(3, np.nan)])
        self.x0 = np.concatenate([x, np.full(3, np.nan)])
        self.V, self.u, self.x = up(V), up(self.u0), up(self.x0)


def integer_data(n, k, rng):
    return (rng.integers(-3, 4, (k + 1, n)).astype(float), rng.integers(-3, 4, n).astype(float),
            rng.integers(-3, 4, n).astype(float))


def normal_data(n, k, rng):
    return rng.standard_normal((k + 1, n)), rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("k", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 65537, 200003])
def test_kernels_have_the_bits_of_the_mirror(ctx, n, k):
    """One Arnoldi step (dots -> project -> dots -> project -> normalize, one batch, the coefficients passed on the device), a
    normalization with a sum of its own and the solution update, for ldv = n and n + 3, on standard-normal data against the
    numpy mirror and on small-integer data against plain integer arithmetic (every sum exact in any order).  n covers the
    first, second and fourth trip of the 256 x 256 lane grid."""
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import KrylovIterator as M
    K = mj.IPMDeviceKernels(n + 3, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), ctx=ctx)
    for ldv in (n, n + 3):
        for kind, make in (("integer", integer_data), ("normal", normal_data)):
            rng = np.random.default_rng(1000 * k + n % 997 + (ldv - n))
            cols, u, x = make(n, k, rng)
            B = Basis(n, k, ldv, cols, u, x)
            un = B.u[:n]
            with K.batch():
                b1 = K.krylov_dots(B.V, k, un)
                K.krylov_project(un, B.V, k)
                b2 = K.krylov_dots(B.V, k, un)
                K.krylov_project(un, B.V, k)
                bn = K.krylov_normalize(B.V[k], un, True, n=n)
            h1, h2, hn = list(b1), list(b2), bn[0]
            Vg, ug = down(ctx, B.V), down(ctx, B.u)
            # the mirror, step by step
            um = u.copy()
            m1 = M.dots(cols, k, um)
            M.project(um, cols, k, m1)
            m2 = M.dots(cols, k, um)
            M.project(um, cols, k, m2)
            mn = math.sqrt(M.dots(cols, 0, um)[0])
            tag = (kind, n, k, ldv)
            assert same_bits(h1, m1), tag
            assert same_bits(h2, m2), tag
            assert same_bits(hn, mn), (tag, hn, mn)
            assert same_bits(ug[:n], um) and np.isnan(ug[n:]).all(), tag
            want = B.V0.copy()
            if mn != 0:
                want[k, :n] = um / mn
                assert same_bits(Vg, want), tag                         # columns < k and every padding word untouched
            else:
                assert same_bits(Vg[:k], want[:k]) and np.isnan(Vg[k, n:]).all(), tag
            if kind == "integer":                                       # known without the mirror
                ci, ui = cols.astype(np.int64), u.astype(np.int64)
                assert h1 == [float(ci[j] @ ui) for j in range(k)] + [float(ui @ ui)], tag
            # project with coefficients of the caller, normalize with a sum of its own, axpy
            coef = rng.integers(-3, 4, k).astype(float) if kind == "integer" else rng.standard_normal(k)
            y = rng.integers(-3, 4, k).astype(float) if kind == "integer" else rng.standard_normal(k)
            B = Basis(n, k, ldv, cols, u, x)
            un, xn = B.u[:n], B.x[:n]
            K.krylov_project(un, B.V, k, coef=up(coef))
            nrm = K.krylov_normalize(B.V[k], un, False, n=n)
            K.krylov_axpy(xn, B.V, k, list(y))
            Vg, ug, xg = down(ctx, B.V), down(ctx, B.u), down(ctx, B.x)
            um, xm = u.copy(), x.copy()
            M.project(um, cols, k, coef)
            M.axpy(xm, cols, k, y)
            mn = math.sqrt(M.dots(cols, 0, um)[0])
            if kind == "integer":
                ci = cols.astype(np.int64)
                ui = u.astype(np.int64) - sum(int(coef[j]) * ci[j] for j in range(k))
                xi = x.astype(np.int64) + sum(int(y[j]) * ci[j] for j in range(k))
                assert np.array_equal(um, ui.astype(float)) and np.array_equal(xm, xi.astype(float)), tag
                assert mn == math.sqrt(float(ui @ ui)), tag
            assert same_bits(ug[:n], um) and np.isnan(ug[n:]).all(), tag
            assert same_bits(xg[:n], xm) and np.isnan(xg[n:]).all(), tag
            assert same_bits(nrm, mn), (tag, nrm, mn)
            want = B.V0.copy()
            if mn != 0:
                want[k, :n] = um / mn
                assert same_bits(Vg, want), tag
    K.close()


def test_bad_arguments_launch_nothing(ctx):
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import _lib as L
    n, k = 300, 3
    lib = L.lib()
    K = mj.IPMDeviceKernels(n, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), ctx=ctx)
    rng = np.random.default_rng(5)
    V0, u0 = rng.standard_normal((k + 1, n)), rng.standard_normal(n)
    V, u, coef = up(V0), up(u0), up(np.ones(8))
    out = (C.c_double * 9)()
    y = (C.c_double * 8)(*([1.0] * 8))
    h, pV, pu, pc = K._h, V.data_ptr(), u.data_ptr(), coef.data_ptr()
    calls = []
    for kk, ldv in ((0, n), (9, n), (-1, n), (k, n - 1)):
        calls += [("dots", lambda kk=kk, ldv=ldv: lib.mnk_ipm_krylov_dots(h, pV, ldv, kk, pu, n, out)),
                  ("project", lambda kk=kk, ldv=ldv: lib.mnk_ipm_krylov_project(h, pu, pV, ldv, kk, n, pc)),
                  ("axpy", lambda kk=kk, ldv=ldv: lib.mnk_ipm_krylov_axpy(h, pu, pV, ldv, kk, y, n))]
    calls += [("dots", lambda: lib.mnk_ipm_krylov_dots(h, None, n, k, pu, n, out)),
              ("dots", lambda: lib.mnk_ipm_krylov_dots(h, pV, n, k, None, n, out)),
              ("dots", lambda: lib.mnk_ipm_krylov_dots(h, pV, n, k, pu, n, None)),
              ("dots", lambda: lib.mnk_ipm_krylov_dots(None, pV, n, k, pu, n, out)),
              ("project", lambda: lib.mnk_ipm_krylov_project(h, None, pV, n, k, n, pc)),
              ("project", lambda: lib.mnk_ipm_krylov_project(h, pu, None, n, k, n, pc)),
              ("project", lambda: lib.mnk_ipm_krylov_project(h, pu, pV, n, k, n, None)),
              ("axpy", lambda: lib.mnk_ipm_krylov_axpy(h, None, pV, n, k, y, n)),
              ("axpy", lambda: lib.mnk_ipm_krylov_axpy(h, pu, None, n, k, y, n)),
              ("axpy", lambda: lib.mnk_ipm_krylov_axpy(h, pu, pV, n, k, None, n)),
              ("normalize", lambda: lib.mnk_ipm_krylov_normalize(h, None, pu, n, 0, out)),
              ("normalize", lambda: lib.mnk_ipm_krylov_normalize(h, pV, None, n, 0, out)),
              ("normalize", lambda: lib.mnk_ipm_krylov_normalize(h, pV, pu, n, 0, None)),
              ("normalize", lambda: lib.mnk_ipm_krylov_normalize(h, pV, pu, n, 2, out)),
              ("last_dots", lambda: lib.mnk_ipm_krylov_last_dots(h, None))]
    for name, call in calls:
        assert call() != 0, name
        assert ("mnk_ipm_krylov_" + name).encode() in lib.mnk_last_error_string(), (name, lib.mnk_last_error_string())
    assert same_bits(down(ctx, V), V0) and same_bits(down(ctx, u), u0)            # nothing ran
    p = C.c_void_p()
    assert lib.mnk_ipm_krylov_last_dots(h, C.byref(p)) != 0                       # no dots call on this handle yet
    K.close()


# --------------------------------------------------------------------------------------------------- solver fixtures
def sparse_factory(nlp, ctx):
    import madnlp_jl_amd as mj

    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                           info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    return factory


def dense_factory(ctx):
    import madnlp_jl_amd as mj

    def factory(info):
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                          device_kkt_ops=True)
    return factory


def sparse_options(**kw):
    from madnlp_jl_amd.ipm import IPMOptions
    o = IPMOptions(tol=1e-6, **kw)
    o.relax_equality, o.dual_initialization = True, "zero"       # the preset of SparseCondensedKKTSystem
    return o


def close(*solvers):
    for s in solvers:
        if hasattr(s, "cb"):
            s.cb.close()
            s.K.close()
        s.kkt.close()


def host_vectors(s, b):
    from madnlp_jl_amd.kkt import UnreducedKKTVector
    V = lambda: UnreducedKKTVector(s.nt, s.m, len(s.ind_lb), len(s.ind_ub), s.ind_lb, s.ind_ub)   # noqa: E731
    x, bb, w = V(), V(), V()
    bb.values[:] = b
    return x, bb, w


def host_ratio(s, xv, b):
    """Richardson's ratio of a downloaded x: the residual through the handle's `mul` on host vectors, the norms in numpy."""
    x, bb, w = host_vectors(s, b)
    x.values[:] = xv
    w.values[:] = b
    s.kkt.mul(w, x, -1.0, 1.0)
    nb = np.abs(b).max()
    return np.abs(w.values).max() / (min(np.abs(xv).max(), 1e6 * nb) + nb)


# ------------------------------------------------------------------------------------------ stale factor on the device
@pytest.mark.parametrize("seed", [3, 4])
def test_stale_factor_on_the_device(ctx, seed):
    """The construction of tests/test_krylov_cpu.py on the HIP `SparseCondensedKKTSystem` (case30, order 236): the state after
    8 iterations of the device driver, built and factorized on the device, then the compressed Hessian times 3 without a new
    factorization.  Both iterators at tol = 1e-8 (acceptable: 1e-5), 10 solves each."""
    from madnlp_jl_amd import KrylovIterator, RichardsonIterator
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import ACOPFModel
    nlp = ACOPFModel("case30")
    s = DeviceMadNLPSolver(nlp, sparse_factory(nlp, ctx), sparse_options(max_iter=8, iterator="krylov"))
    assert s.solve() == "MAXIMUM_ITERATIONS_EXCEEDED" and s.cnt.k == 8
    s.eval_lag_hess(s.x, s.y)
    s.set_aug_diagonal()
    s.factorize_wrapper()
    s.kkt.compress_hessian(s.cb.hv * 3.0)          # (compression is linear in the COO values)
    bh = np.random.default_rng(seed).standard_normal(s._lw)
    b, x, w = up(bh), s._new_vec(s._lw), s._new_vec(s._lw)
    s.iterator = RichardsonIterator(s.kkt, tol=1e-8)
    ok_r = s._solve_refine(x, b, w)
    print("device richardson", seed, s.iterator.ir, s.iterator.residual_ratio)
    assert not ok_r and s.iterator.ir == 10
    s.iterator = it = KrylovIterator(s.kkt, tol=1e-8)
    ok_k = s._solve_refine_krylov(x, b, w)
    xv = down(ctx, x)
    r = host_ratio(s, xv, bh)
    print("device krylov", seed, it.ir, it.steps, it.cycles, it.residual_ratio, "host ratio", r)
    assert ok_k and it.ir <= 10
    assert r < 1e-8 ** (5 / 8), r
    mirror = KrylovIterator(s.kkt, tol=1e-8)        # the host mirror through the same handle and factorization
    ok_m = mirror.solve_refine(*host_vectors(s, bh))
    print("host mirror", seed, mirror.ir, mirror.steps, mirror.cycles, mirror.residual_ratio)
    assert ok_m and abs(mirror.ir - it.ir) <= 1, (mirror.ir, it.ir)
    close(s)


# -------------------------------------------------------------------------------------------------------- a dense handle
def test_dense_condensed_handle(ctx):
    """`DenseCondensedKKTSystem`, DenseQPModel(50, 10, 2): three iterations of the device driver, then new diagonals without a
    new factorization; device GMRES and the host mirror on the same handle agree in verdict, and in `ir` within 1."""
    from madnlp_jl_amd import KrylovIterator
    from madnlp_jl_amd.ipm import IPMOptions
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import DenseQPModel
    nlp = DenseQPModel(50, 10, 2)
    s = DeviceMadNLPSolver(nlp, dense_factory(ctx), IPMOptions(tol=1e-8, max_iter=3, iterator="krylov"), sparse=False)
    assert s.solve() == "MAXIMUM_ITERATIONS_EXCEEDED"
    s.set_aug_diagonal()                            # the iterate has moved since the last factorization
    bh = np.random.default_rng(7).standard_normal(s._lw)
    b, x, w = up(bh), s._new_vec(s._lw), s._new_vec(s._lw)
    it = s.iterator
    ok = s._solve_refine_krylov(x, b, w)
    xv = down(ctx, x)
    mirror = KrylovIterator(s.kkt, tol=1e-8)
    xm, bm, wm = host_vectors(s, bh)
    ok_m = mirror.solve_refine(xm, bm, wm)
    print("dense: device", ok, it.ir, it.steps, it.residual_ratio, "mirror", ok_m, mirror.ir, mirror.steps, mirror.residual_ratio)
    assert ok == ok_m
    assert abs(it.ir - mirror.ir) <= 1, (it.ir, mirror.ir)
    if ok:
        assert host_ratio(s, xv, bh) < 1e-8 ** (5 / 8)
    close(s)


# ------------------------------------------------------------------------------------------------------------ end to end
def make_solver(system, ctx, **kw):
    from madnlp_jl_amd.ipm import IPMOptions
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import ACOPFModel, DenseQPModel
    from madnlp_jl_amd.tape_model import acopf_tape_model
    kind, _, case = system.partition("_")
    if kind == "qp":
        nlp = DenseQPModel(50, 10, 2)
        return DeviceMadNLPSolver(nlp, dense_factory(ctx), IPMOptions(tol=1e-8, **kw), sparse=False), nlp
    nlp = ACOPFModel(case) if kind == "acopf" else acopf_tape_model(case)
    return DeviceMadNLPSolver(nlp, sparse_factory(nlp, ctx), sparse_options(**kw)), ACOPFModel(case)


def counted(s):
    """Record the iterator's `ir` after every refined solve of the run."""
    total, inner = [], s.solve_refine_wrapper
    s.solve_refine_wrapper = lambda *a: (inner(*a), total.append(s.iterator.ir))[0]
    return total


@pytest.mark.parametrize("system", ["acopf_case30", "acopf_case118", "tape_case30", "tape_case118", "qp_50_10_2"])
def test_device_run_with_gmres_follows_the_richardson_run(ctx, system):
    sr, judge = make_solver(system, ctx)                        # `iterator` left at its default
    sr.solve()
    sk, _ = make_solver(system, ctx, iterator="krylov")
    irs = counted(sk)
    sk.solve()
    print(system, "richardson (k, factorizations, back-solves)", (sr.cnt.k, sr.cnt.factorization_cnt, sr.cnt.backsolve_cnt),
          "krylov", (sk.cnt.k, sk.cnt.factorization_cnt, sk.cnt.backsolve_cnt))
    assert sr.status == "SOLVE_SUCCEEDED" and sk.status == "SOLVE_SUCCEEDED", (sr.status, sk.status)
    assert abs(sk.obj_val - sr.obj_val) <= 1e-6 * abs(sr.obj_val), (sk.obj_val, sr.obj_val)
    assert abs(sk.cnt.k - sr.cnt.k) <= 2, (sk.cnt.k, sr.cnt.k)
    assert sk.cnt.backsolve_cnt == sum(irs) > 0
    x = sk.host_state()[0][:judge.n]
    c = judge.cons(x)                                           # feasibility judged by the host model
    assert (c >= judge.lcon - 1e-5).all() and (c <= judge.ucon + 1e-5).all()
    assert (x >= judge.lvar - 1e-7).all() and (x <= judge.uvar + 1e-7).all()
    assert abs(judge.obj(x) - sk.obj_val) <= 1e-9 * abs(sk.obj_val)
    close(sr, sk)


@pytest.mark.parametrize("system", ["acopf_case30", "acopf_case118", "qp_50_10_2"])
def test_default_run_is_the_run_from_before_the_option(ctx, system):
    """tests/golden/krylov_default_<system>.npz holds x, y, zl, zu and the counters of the device run made with the commit
    before the `iterator` option existed; the run with the option left at its default has the same bytes."""
    s, _ = make_solver(system, ctx)
    s.solve()
    g = np.load(os.path.join(GOLDEN, f"krylov_default_{system}.npz"))
    assert [s.cnt.k, s.cnt.factorization_cnt, s.cnt.backsolve_cnt] == g["counts"].tolist()
    for name, v in zip(("x", "y", "zl", "zu"), s.host_state()):
        assert same_bits(v, g[name]), name
    close(s)

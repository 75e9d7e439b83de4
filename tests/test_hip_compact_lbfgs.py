"""GPU tests of the compact L-BFGS path (csrc/lbfgs.hip, the additions to csrc/sparse_kkt.hip, `DeviceMadNLPSolver` with
`hessian_approximation = "compact_lbfgs"`) against the host mirror (`madnlp_jl_amd.quasi_newton`, `kkt.LowRankHessianKKT`) and
the longdouble recursion of tests/lbfgs_cases.py.

Rules: the reductions and rank-q applications equal the mirror bit for bit (the mirror sums with `ipm.ordered_sum`).  Where the
device differs from the mirror in the order of O(p) operations (U, V; solve_kkt / mul through two different linear solvers) its
error may be at most 8 x the mirror's own error on the same case, the margin of DESIGN.md section 5a-multi; both errors go to
profiles/lbfgs_accuracy.json."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from lbfgs_cases import ld_uv, random_pairs, scripted_sequence  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver, parse_indexes  # noqa: E402
from madnlp_jl_amd.kkt import DeviceCompactLBFGS, LowRankHessianKKT, UnreducedKKTVector  # noqa: E402
from madnlp_jl_amd.linear_solver import SolveException  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel, SparseQPModel  # noqa: E402
from madnlp_jl_amd.quasi_newton import CompactLBFGS, QuasiNewtonOptions, gram, lowrank_apply  # noqa: E402
from oracle.kernels import set_aug_diagonal  # noqa: E402
from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver  # noqa: E402
from oracle.sparse_condensed import SparseCondensedKKTSystem as OracleSC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "lbfgs_accuracy.json")
HOST_VS_EXACT = os.path.join(ROOT, "profiles", "lbfgs_host_vs_exact.json")      # written by tools/lbfgs_host_vs_exact.py


def record(section, key, value):
    data = json.load(open(ACCURACY)) if os.path.exists(ACCURACY) else {}
    data.setdefault(section, {})[key] = value
    with open(ACCURACY, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def cols(A):
    """n x q host matrix -> device tensor holding it column-major (shape (q, n))."""
    return dev(np.ascontiguousarray(A.T))


# ------------------------------------------------------------------------------------------ 1. kernels on their own
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 65536 + 129])
@pytest.mark.parametrize("q", [2, 4, 12, 64])
def test_reductions_and_lowrank_applications_equal_the_mirror_bit_for_bit(ctx, n, q):
    """A'B (every entry an ordered sum; the first 8 rows of A: a row only offsets a pointer) and y += alpha A (M (B'x))."""
    rng = np.random.default_rng(1000 * q + n % 997)
    scale = 10.0 ** rng.uniform(-3, 3, (n, 1))
    A, B = rng.standard_normal((n, q)) * scale, rng.standard_normal((n, q)) / scale
    M = rng.standard_normal((q, q))
    x, y0 = rng.standard_normal(n), rng.standard_normal(n)
    qd = DeviceCompactLBFGS(ctx, n, QuasiNewtonOptions(max_history=32))
    try:
        r = min(q, 8)
        G = qd.gram(cols(A[:, :r]), cols(B))
        assert G.tobytes() == np.asfortranarray(gram(A[:, :r], B)).tobytes()
        for alpha in (-1.0, 0.375):
            yd = dev(y0)
            qd.apply(yd, alpha, cols(A), cols(M), cols(B), dev(x))      # cols(M): M column-major
            want = lowrank_apply(y0.copy(), alpha, A, M, B, x)
            assert yd.cpu().numpy().tobytes() == want.tobytes()
    finally:
        qd.close()


# ------------------------------------------------------------------------------------------ 2. update!
def uv_errors(U, V, sigma, S, Y):
    Ul, Vl = ld_uv(sigma, S, Y)
    return float(np.abs(U - Ul).max()), float(np.abs(V - Vl).max())


@pytest.mark.parametrize("n", [7, 257, 1000])
def test_update_follows_the_mirror_over_the_scripted_sequence(ctx, n):
    """performed / sigma / current_mem / counters equal the mirror's after every pair of tests/lbfgs_cases.scripted_sequence
    (history 3: growth, shift, an isolated skip, two skips in a row = a reset, regrowth); S, Y are the mirror's bits; U and V
    within 8 x the mirror's error against the longdouble formulas."""
    opt = QuasiNewtonOptions(max_history=3)
    qd, qh = DeviceCompactLBFGS(ctx, n, opt), CompactLBFGS(n, opt)
    B = np.zeros(n)
    try:
        worst = {"U": (0.0, 0.0), "V": (0.0, 0.0)}
        for i, (s, y, ok) in enumerate(scripted_sequence(n)):
            done_h = qh.update(B, s, y)
            done_d, sigma_d = qd.update(dev(s), dev(y))
            st = qd.status()
            assert done_d == done_h == ok
            assert sigma_d == qh.sigma
            assert (st["current_mem"], st["updates"], st["skipped"], st["resets"], st["version"]) == \
                (qh.current_mem, qh.updates, qh.skipped, qh.resets, qh.version), i
            if qh.current_mem == 0:
                continue
            assert qd.get("S").tobytes() == np.asfortranarray(qh.S).tobytes()
            assert qd.get("Y").tobytes() == np.asfortranarray(qh.Y).tobytes()
            assert np.array_equal(qd.get("D"), qh.D) and np.array_equal(qd.get("L"), qh.L)
            if not ok:
                continue
            eu_d, ev_d = uv_errors(qd.get("U"), qd.get("V"), qh.sigma, qh.S, qh.Y)
            eu_h, ev_h = uv_errors(qh.U, qh.V, qh.sigma, qh.S, qh.Y)
            print(f"n={n} pair {i} p={qh.current_mem}: U err device {eu_d:.3e} mirror {eu_h:.3e}; V device {ev_d:.3e} mirror {ev_h:.3e}")
            if eu_d / max(eu_h, 1e-300) >= worst["U"][0] / max(worst["U"][1], 1e-300):
                worst["U"] = (eu_d, eu_h)
            if ev_d / max(ev_h, 1e-300) >= worst["V"][0] / max(worst["V"][1], 1e-300):
                worst["V"] = (ev_d, ev_h)
            assert eu_d <= 8 * eu_h and ev_d <= 8 * ev_h
        record("update_uv", f"n={n}", {"U_device": worst["U"][0], "U_mirror": worst["U"][1], "V_device": worst["V"][0],
                                      "V_mirror": worst["V"][1]})
    finally:
        qd.close()


def test_init_on_the_device_equals_the_mirror(ctx):
    rng = np.random.default_rng(5)
    for n, f0, scale in ((3, 7.0, 1e-5), (1000, 0.0, 1.0), (70000, -50.0, 1.0)):
        g = rng.standard_normal(n) * scale
        qd, qh = DeviceCompactLBFGS(ctx, n, QuasiNewtonOptions(init_value=0.25)), CompactLBFGS(n, QuasiNewtonOptions(init_value=0.25))
        B = np.zeros(n)
        qh.init(B, g, f0)
        assert qd.init(dev(g), f0) == B[0]
        qd.close()


# ------------------------------------------------------------------------------------------ 3. solve_kkt / mul with a handle attached
def barrier_point(nlp, seed):
    """`SparseQPModel`-shaped data at one barrier point: the fields both KKT systems are given."""
    idx = parse_indexes(np.asarray(nlp.lvar, float), np.asarray(nlp.uvar, float), np.asarray(nlp.lcon, float),
                        np.asarray(nlp.ucon, float), enforce_equality=False)
    rng = np.random.default_rng(seed)
    n, m = nlp.n, nlp.m
    nlb, nub = len(idx["ind_lb"]), len(idx["ind_ub"])
    return idx, dict(reg=10.0 ** rng.uniform(-2, 1, n + m), du_diag=-10.0 ** rng.uniform(-8, -4, m),
                     l_diag=-10.0 ** rng.uniform(-2, 0, nlb), u_diag=-10.0 ** rng.uniform(-2, 0, nub),
                     l_lower=10.0 ** rng.uniform(-3, 0, nlb), u_lower=10.0 ** rng.uniform(-3, 0, nub))


def fill(kkt, nlp, fields, sigma):
    kkt.initialize()
    kkt.get_jacobian()[:] = nlp.jac_coord(None)
    kkt.get_hessian()[:] = sigma
    kkt.compress_jacobian()
    kkt.compress_hessian()
    for k, v in fields.items():
        getattr(kkt, k)[:] = v


def make_pair(ctx, nlp, p, seed):
    """(HIP system with an attached handle, wrapper around the oracle with the mirror): the same p pairs, the same point."""
    n, m = nlp.n, nlp.m
    idx, fields = barrier_point(nlp, seed)
    diag = np.arange(n)
    opt = QuasiNewtonOptions(max_history=p)
    hip = mj.SparseCondensedKKTSystem(n, m, nlp.jac_I, nlp.jac_J, diag, diag, idx["ind_ineq"], idx["ind_lb"], idx["ind_ub"], ctx=ctx,
                                      opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)
    ora = OracleSC(n, m, nlp.jac_I, nlp.jac_J, diag, diag, idx["ind_ineq"], idx["ind_lb"], idx["ind_ub"],
                   lambda A: LapackCPUSolver(A, BUNCHKAUFMAN))
    qh = CompactLBFGS(n, opt)
    qd = hip.attach_quasi_newton(opt)
    S, Y = random_pairs(n, p, seed + 1)
    B = np.zeros(n)
    for i in range(p):
        assert qh.update(B, S[:, i], Y[:, i])
        done, sigma = qd.update(dev(S[:, i]), dev(Y[:, i]))
        assert done and sigma == qh.sigma
    fill(hip, nlp, fields, qh.sigma)
    fill(ora, nlp, fields, qh.sigma)
    hip.set_aug_diagonal()
    set_aug_diagonal(ora)
    wrap = LowRankHessianKKT(ora, qh)
    hip.build_kkt()
    wrap.build_kkt()
    hip.linear_solver.factorize()
    ora.linear_solver.factorize()
    return hip, wrap, qd, qh


def residual(kkt, b):
    w = UnreducedKKTVector.from_kkt(kkt)
    w.values[:] = b
    kkt.solve_kkt(w)
    y = w.copy()
    y.values[:] = 0.0
    kkt.mul(y, w)
    return float(np.abs(y.values - b).max() / np.abs(b).max()), w.values.copy(), y.values.copy()


@pytest.mark.parametrize("p", [1, 6, 32])
def test_solve_kkt_and_mul_with_an_attached_handle(ctx, p):
    """p = 1 solves H = C^-1 E by the column loop, p = 6 and p = 32 blocked."""
    nlp = SparseQPModel("case30")
    hip, wrap, qd, qh = make_pair(ctx, nlp, p, 40 + p)
    try:
        b = np.random.default_rng(p).standard_normal(len(UnreducedKKTVector.from_kkt(hip).values))
        r_dev, x_dev, y_dev = residual(hip, b)
        r_ora, x_ora, _ = residual(wrap, b)
        chunks = hip.linear_solver.get_stat("solve_rhs_chunks")      # passes of the last BLOCKED solve (0: there was none)
        print(f"p={p}: residual device {r_dev:.3e} oracle wrapper {r_ora:.3e}; |x_dev - x_ora| / |x_ora| = "
              f"{np.abs(x_dev - x_ora).max() / np.abs(x_ora).max():.3e}; builds {qd.status()['builds']}; blocked passes {chunks}")
        assert (chunks == 0) == (p == 1)
        record("solve_kkt_mul", f"p={p}", {"device": r_dev, "oracle_wrapper": r_ora})
        assert qd.status()["builds"] == 1 and qd.status()["singular"] == 0
        assert r_dev <= 8 * r_ora
        # the low-rank term is there: without it the answer is another one
        hip.attach_quasi_newton(False)
        _, x_plain, _ = residual(hip, b)
        assert np.abs(x_plain - x_dev).max() > 1e-6 * np.abs(x_dev).max()
    finally:
        hip.close()


def test_identical_calls_give_identical_bits(ctx):
    nlp = SparseQPModel("case30")
    hip, wrap, qd, qh = make_pair(ctx, nlp, 6, 77)
    try:
        b = np.random.default_rng(3).standard_normal(len(UnreducedKKTVector.from_kkt(hip).values))
        (_, x1, y1), (_, x2, y2) = residual(hip, b), residual(hip, b)
        assert x1.tobytes() == x2.tobytes() and y1.tobytes() == y2.tobytes()
        hip.build_kkt()                      # ... and so does a rebuild of H, T, W from the same factorization input
        hip.linear_solver.factorize()
        _, x3, y3 = residual(hip, b)
        assert x1.tobytes() == x3.tobytes() and y1.tobytes() == y3.tobytes()
    finally:
        hip.close()


def test_h_and_t_are_built_once_per_cause(ctx):
    nlp = SparseQPModel("case30")
    hip, wrap, qd, qh = make_pair(ctx, nlp, 3, 91)
    try:
        w = UnreducedKKTVector.from_kkt(hip)
        builds = lambda: qd.status()["builds"]  # noqa: E731

        def solve():
            w.values[:] = 1.0
            hip.solve_kkt(w)
        for _ in range(3):
            solve()
        assert builds() == 1                               # several solves on one factorization
        hip.mul(w.copy(), w)
        assert builds() == 1                               # mul! needs no H
        hip.build_kkt()
        hip.linear_solver.factorize()
        solve(); solve()
        assert builds() == 2                               # a refactorization
        S, Y = random_pairs(nlp.n, 1, 5)
        assert qd.update(dev(S[:, 0]), dev(Y[:, 0]))[0]
        solve(); solve()
        assert builds() == 3                               # a performed update
        assert not qd.update(dev(S[:, 0]), dev(-Y[:, 0]))[0]
        solve()
        assert builds() == 3                               # a skip changes nothing
        spare = hip.ensure_spare_solver()
        spare.factorize()
        hip.swap_solvers()
        solve(); solve()
        assert builds() == 4                               # the spare solver's factor
        assert not qd.update(dev(S[:, 0]), dev(-Y[:, 0]))[0] and qd.status()["current_mem"] == 0
        solve()
        assert builds() == 4                               # an empty memory: the plain solve
    finally:
        hip.close()


def test_singular_t_is_flagged_and_reported(ctx):
    """A scripted zero pivot.  (U = V cannot give one: then B = sigma I, K = C and det T = -det K / det C = -1.  K = C - U U' +
    V V' must itself be singular, which needs an entry of the diagonal below sigma.)  One pair s = (2, 0), y = (2, 4): sigma = 1,
    U = (1, 0)', V = (1, 2)'; with C = diag(0.5, 4) every number below is exact: C^-1 E = [2 2; 0 0.5], T = P + E'C^-1 E =
    [1 2; 2 4], whose second pivot is 0 after the row exchange."""
    e = np.zeros(0, dtype=np.int64)
    diag = np.arange(2)
    hip = mj.SparseCondensedKKTSystem(2, 1, [0], [0], diag, diag, [0], e, e, ctx=ctx,
                                      opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)
    try:
        qd = hip.attach_quasi_newton(QuasiNewtonOptions(max_history=1))
        done, sigma = qd.update(dev([2.0, 0.0]), dev([2.0, 4.0]))
        assert done and sigma == 1.0
        assert np.array_equal(qd.get("U"), [[1.0], [0.0]]) and np.array_equal(qd.get("V"), [[1.0], [2.0]])
        hip.initialize()
        hip.get_jacobian()[:] = 0.0
        hip.get_hessian()[:] = sigma
        hip.compress_jacobian()
        hip.compress_hessian()
        hip.pr_diag[:] = [-0.5, 3.0, 1.0]
        hip.du_diag[:] = -1.0
        hip.build_kkt()
        hip.linear_solver.factorize()
        w = UnreducedKKTVector.from_kkt(hip)
        w.values[:] = 1.0
        with pytest.raises(SolveException, match="singular"):
            hip.solve_kkt(w)
        st = qd.status()
        assert (st["singular"], st["builds"]) == (1, 1)
        assert np.all(np.isfinite(w.values))               # the correction was not applied: w holds the condensed solve
    finally:
        hip.close()


def test_batch_entry_points_refuse_an_attached_handle(ctx):
    nlp = SparseQPModel("case30")
    hip, wrap, qd, qh = make_pair(ctx, nlp, 1, 13)
    try:
        batch = mj.ScenarioBatch([hip])
        x = dev(np.ones(nlp.n))
        with pytest.raises(mj.HipError, match="L-BFGS"):
            batch.solve([x])
        t = [dev(hip.jac), dev(hip.hess), dev(hip.pr_diag), dev(hip.du_diag)]
        batch.bind([t[0]], [t[1]], [t[2]], [t[3]])
        with pytest.raises(mj.HipError, match="L-BFGS"):
            batch.step()
    finally:
        hip.close()


# ------------------------------------------------------------------------------------------ 4. device-resident runs
def hip_factory(ctx, nlp):
    def make(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, info.get("hess_I", nlp.hess_I),
                                           info.get("hess_J", nlp.hess_J), info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                           device_kkt_ops=True)
    return make


def options(approx):
    o = IPMOptions(tol=1e-6, hessian_approximation=approx)
    o.relax_equality, o.dual_initialization = True, "zero"
    return o


CASES = {"acopf_case30": lambda: ACOPFModel("case30"), "acopf_case118": lambda: ACOPFModel("case118"),
         "sparse_qp_case30": lambda: SparseQPModel("case30")}


@pytest.mark.parametrize("case", list(CASES))
def test_device_resident_run(monkeypatch, case):
    """`DeviceMadNLPSolver` with the device callbacks: no Hessian callback is ever launched, the run is reproducible to the bit,
    and its objective is within 10 x the host mirror's distance from the exact-Hessian run (profiles/lbfgs_host_vs_exact.json;
    the convention and the reason for the decade of tests/test_quasi_newton_cpu.py::test_dense_qp_against_the_exact_hessian_run).
    Iteration counts of the host mirror and of the device run are printed and recorded, not compared.

    Measured on the MI355X: acopf_case30 16 iterations (host mirror 16), |obj - obj_exact| 5.18e-6 (host mirror 5.16e-6);
    acopf_case118 82 (81), 1.733e-5 (1.733e-5); sparse_qp_case30 139 (134), 6.7e-10 (6.8e-10).  The QP run is the one that
    needs the reference's "second chance" of the regular line search (line_search.jl:79-96, `MadNLPSolver.filter_line_search`):
    at iteration 88 the filter, fed rounding-noise theta by the linear constraints, rejects an accurate descent step at every
    length, and the regular phase starts again there with an empty filter."""
    from madnlp_jl_amd import ipm_dev
    rec = json.load(open(HOST_VS_EXACT))["cases"][case]
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    try:
        nlp = CASES[case]()
        calls = {"hessian": 0}
        for cls in (ipm_dev.DeviceQPCallbacks, ipm_dev.DeviceOPFCallbacks, ipm_dev.DeviceTapeCallbacks):
            for name in ("load_hess", "hess_coord", "zero_hess"):
                if hasattr(cls, name):
                    def counted(self, *a, _real=getattr(cls, name), **kw):
                        calls["hessian"] += 1
                        return _real(self, *a, **kw)
                    monkeypatch.setattr(cls, name, counted)
        runs = []
        for _ in range(2):
            sd = ipm_dev.DeviceMadNLPSolver(nlp, hip_factory(ctx, nlp), options("compact_lbfgs"))
            sd.solve()
            runs.append((sd.status, sd.cnt.k, sd.obj_val, sd.host_state()[0].copy(), sd.kkt.qn_status(),
                         max(sd.inf_pr, sd.inf_du, sd.inf_compl_v), sd.cnt.lag_hess_cnt, sd.cnt.factorization_cnt, sd.cnt.backsolve_cnt))
            assert not isinstance(sd.kkt, LowRankHessianKKT)          # the wrapper came off at the upload
            sd.kkt.close(); sd.K.close(); sd.cb.close()
        hessian_calls = calls["hessian"]
        monkeypatch.undo()
        ex = ipm_dev.DeviceMadNLPSolver(nlp, hip_factory(ctx, nlp), options("exact"))
        ex.solve()
        status, k, obj, x, qst, inf_total, lag_hess, nfact, nsolve = runs[0]
        dobj = abs(obj - ex.obj_val)
        print(f"{case}: device {status} k {k} fact {nfact} backsolves {nsolve} updates {qst['updates']} skipped {qst['skipped']} "
              f"resets {qst['resets']} builds {qst['builds']}; host mirror k {rec['k']} ({rec['status']}); exact device k {ex.cnt.k}; "
              f"|obj - obj_exact| {dobj:.3e} (host mirror {rec['dobj']:.3e})")
        record("device_runs", case, {"status": status, "k": k, "host_mirror_k": rec["k"], "exact_k": ex.cnt.k, "dobj": dobj,
                                     "host_mirror_dobj": rec["dobj"], "factorizations": nfact, "backsolves": nsolve,
                                     "updates": qst["updates"], "skipped": qst["skipped"], "resets": qst["resets"],
                                     "builds": qst["builds"]})
        ex.kkt.close(); ex.K.close(); ex.cb.close()
        assert status == "SOLVE_SUCCEEDED" and ex.status == "SOLVE_SUCCEEDED"
        assert inf_total <= 1e-6
        assert lag_hess == 0 and hessian_calls == 0
        assert qst["singular"] == 0
        assert runs[1][0] == status and runs[1][1] == k and runs[1][3].tobytes() == x.tobytes()
        assert dobj <= 10 * rec["dobj"]
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        ctx.close()


def test_host_driver_on_the_hip_handle_goes_through_the_wrapper(ctx):
    """`MadNLPSolver` (host vectors, `device_kkt_ops=False`) on the HIP KKT handle: the mirror's wrapper applies the low-rank
    term around the handle's condensed solve."""
    nlp = ACOPFModel("case30")

    def make(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, info["hess_I"], info["hess_J"], info["ind_ineq"],
                                           info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN))
    s = MadNLPSolver(nlp, make, options("compact_lbfgs"), sparse=True)
    s.solve()
    rec = json.load(open(HOST_VS_EXACT))["cases"]["acopf_case30"]
    print(f"host driver on the HIP handle: {s.status} k {s.cnt.k} (CPU oracle: {rec['k']}) builds {s.kkt.builds}")
    assert isinstance(s.kkt, LowRankHessianKKT) and s.kkt.builds > 0
    assert s.status == "SOLVE_SUCCEEDED" and s.cnt.lag_hess_cnt == 0
    assert abs(s.obj_val - rec["exact"]["obj"]) <= 10 * rec["dobj"]
    s.kkt.close()


def test_device_driver_checks_the_options():
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    with pytest.raises(ValueError, match="sparse=True"):
        DeviceMadNLPSolver(SparseQPModel("case30"), lambda info: None, IPMOptions(hessian_approximation="compact_lbfgs"), sparse=False)
    assert L.MNK_SC_JT_KEPT == 4

"""Bit-exact record of IPM runs, for A/B comparisons of two versions of the driver (`madnlp.jl_amd/ipm.py`, `ipm_dev.py`,
`device_callbacks.py`).

  python tools/ipm_trajectory_dump.py --out A.json                       host driver (MadNLPSolver) on the CPU oracle back-end
  python tools/ipm_trajectory_dump.py --device --out A.json              DeviceMadNLPSolver on the HIP KKT systems (needs a GPU)
  python tools/ipm_trajectory_dump.py --device --time 3 --out T.json     wall clock of the two runs bench.py's `ipm_loop` times
  python tools/ipm_trajectory_dump.py --device --handles --out H.json    the KKT handles' own entry points, host and device vectors
  python tools/ipm_trajectory_dump.py --compare A.json B.json            identical, or per field the largest relative difference
  ... --package DIR                                                      take the package from DIR (a copy of another commit's
                                                                         `madnlp.jl_amd/`; with MNK_LIBPATH the same built library)

Per run: status, counters, every `IterRecord` field and the final x, y, zl, zu, floats as `float.hex()`; a SHA-256 over all runs.
Two versions that perform the same IEEE operations in the same order write identical files.

By wrapping (nothing in the product counts), per run: which branches of the line search and of the inertia correction were
reached; in --device mode also the result-returning `mnk_ipm_*` calls made outside a batch (one host synchronization each),
the `mnk_ipm_batch_end` calls (one synchronization per batch), the `vec_*` launches and the `scale_grad`, `scale_cons` and `gemv`
launches of the callbacks' scaling layer -- integers fixed by the control flow.
The host mode refuses to write unless its runs reach every branch a driver refactor moves (`REQUIRED`)."""
import argparse
import hashlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

KINDS = ("dense", "dense_condensed", "sparse_condensed")
# branch counters the host list must reach at least this often (a refactor of the driver moves every one of them)
REQUIRED = {"soc_accepted": 1, "soc_rejected": 1, "ls_backtracked": 1, "ls_restore": 1, "ic_3_trials_inertia_based": 1,
            "ic_3_trials_inertia_free": 1, "ic_overflow": 1}


def load_package(pkg_dir):
    """`madnlp_jl_amd` from the repository, or from `pkg_dir` (loaded the way the repository's import shim loads its own)."""
    sys.path.insert(0, ROOT)
    if pkg_dir:
        pkg_dir = os.path.abspath(pkg_dir)
        spec = importlib.util.spec_from_file_location("madnlp_jl_amd", os.path.join(pkg_dir, "__init__.py"),
                                                      submodule_search_locations=[pkg_dir])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["madnlp_jl_amd"] = mod
        spec.loader.exec_module(mod)
    import madnlp_jl_amd
    return madnlp_jl_amd


class DuplicateRowQP:
    """min 0.5 |x|^2 s.t. x1 + x2 = 1, twice: a rank-deficient Jacobian, so the unperturbed KKT matrix is singular and a solve
    on its LU factor fails -- the one thing that makes the `ignore` corrector perturb."""
    n, m = 2, 2
    x0, y0 = np.zeros(2), np.zeros(2)
    lvar, uvar = np.full(2, -np.inf), np.full(2, np.inf)
    lcon = ucon = np.ones(2)
    jac_I, jac_J = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    hess_I, hess_J = np.array([0, 1]), np.array([0, 1])

    def obj(self, x): return 0.5 * float(x @ x)
    def grad(self, x): return np.array(x, dtype=float)
    def cons(self, x): return np.array([x[0] + x[1], x[0] + x[1]])
    def jac_coord(self, x): return np.ones(4)
    def jac_dense(self, x): return np.ones((2, 2), order="F")
    def hess_coord(self, x, y, w=1.0): return np.array([w, w])
    def hess_dense(self, x, y, w=1.0): return np.array([[w, 0.0], [0.0, w]], order="F")


def counted(cls, counts):
    """`cls` with the line search and the inertia correction wrapped: counts the branches they take into `counts`."""
    def bump(key):
        counts[key] = counts.get(key, 0) + 1

    class Counted(cls):
        def _second_order_correction(self, *a):
            ok = super()._second_order_correction(*a)
            bump("soc_accepted" if ok else "soc_rejected")
            return ok

        def filter_line_search(self):
            st = super().filter_line_search()
            if self.cnt.l > 1:
                bump("ls_backtracked")
            if st == "RESTORE":
                bump("ls_restore")
            return st

        def inertia_correction(self):
            f0 = self.cnt.factorization_cnt
            ok = super().inertia_correction()
            if not ok:
                bump("ic_overflow")
            if self.cnt.factorization_cnt - f0 >= 3:
                bump("ic_3_trials_" + self.inertia_correction_method)
            if self.cnt.factorization_cnt - f0 >= 2 and self.inertia_correction_method == "ignore":
                bump("ic_ignore_perturbed")
            return ok
    return Counted


class Forced:
    """The regular phase reports a line-search failure at iteration 2 (-> restore!) and an inertia-correction failure at
    iteration 5 (-> robust!), once each: a convex QP walks through both restoration phases (as tests/test_ipm_restoration_driver.py)."""
    _f1 = _f2 = False

    def filter_line_search(self):
        st = super().filter_line_search()
        if self.cnt.k == 2 and not self._f1 and st == "LINESEARCH_SUCCEEDED":
            self._f1 = True
            self.cnt.k += 1
            return "RESTORE"
        return st

    def inertia_correction(self):
        ok = super().inertia_correction()
        if self.status == "REGULAR" and self.cnt.k >= 5 and not self._f2:
            self._f2 = True
            return False
        return ok


def hexes(v):
    return [float(a).hex() for a in np.asarray(v, dtype=float).ravel()]


def record(s, state, counts):
    x, y, zl, zu = state
    return {"status": s.status, "k": s.cnt.k, "factorizations": s.cnt.factorization_cnt, "backsolves": s.cnt.backsolve_cnt,
            "history": [[r.k, r.phase, r.ls] + hexes([r.obj, r.inf_pr, r.inf_du, r.inf_compl, r.mu, r.del_w, r.alpha])
                        for r in s.history],
            "x": hexes(x), "y": hexes(y), "zl": hexes(zl), "zu": hexes(zu), "branches": dict(sorted(counts.items()))}


def finish(out, path, extra=None):
    blob = json.dumps(out, sort_keys=True)
    doc = {"sha256": hashlib.sha256(blob.encode()).hexdigest(), "runs": out}
    doc.update(extra or {})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, sort_keys=True, indent=0)
    return doc["sha256"]


# ------------------------------------------------------------------------------------------------ host: CPU oracle back-end
def host_cases():
    from madnlp_jl_amd.problems import (CubicDiskModel, DenseQPModel, HS15Model, InfeasibleModel, LootsmaModel, SparseQPModel,
                                        WachterBieglerModel)
    from oracle.lapack_cpu import BUNCHKAUFMAN, LU
    cubic = lambda: CubicDiskModel(2.636, [-4.9627, -2.877])  # noqa: E731
    cases = []
    for kind in KINDS:
        for alg in (BUNCHKAUFMAN, LU):       # auto: inertia_based with BUNCHKAUFMAN, inertia_free with LU
            for name, mk in (("hs15", HS15Model), ("lootsma", LootsmaModel), ("infeasible", InfeasibleModel), ("cubic2.636", cubic)):
                cases.append((f"{name}-{kind}-{alg}", kind, mk, alg, {}))
    dqp = lambda: DenseQPModel(20, 15, 2)  # noqa: E731
    cases += [("hs15-dense-ignore", "dense", HS15Model, LU, {"inertia_correction_method": "ignore"}),
              ("duplicate-row-dense-ignore", "dense", DuplicateRowQP, LU, {"inertia_correction_method": "ignore"}),
              ("wachter-biegler-dense", "dense", WachterBieglerModel, BUNCHKAUFMAN, {}),
              ("cubic1.0178-dense", "dense", lambda: CubicDiskModel(1.0178, [-1.7068, 1.069]), BUNCHKAUFMAN, {}),
              ("sparse-qp-case30", "sparse_condensed", lambda: SparseQPModel("case30"), BUNCHKAUFMAN, {}),
              ("dense-qp-bfgs", "dense_condensed", dqp, BUNCHKAUFMAN, {"hessian_approximation": "bfgs"}),
              ("dense-qp-damped-bfgs", "dense_condensed", dqp, BUNCHKAUFMAN, {"hessian_approximation": "damped_bfgs"}),
              ("cubic2.636-dense-max-perturbation-1", "dense", cubic, BUNCHKAUFMAN, {"max_hessian_perturbation": 1.0})]
    return cases


def oracle_factory(kind, nlp, alg):
    from oracle.dense import DenseCondensedKKTSystem, DenseKKTSystem
    from oracle.lapack_cpu import LapackCPUSolver
    from oracle.sparse_condensed import SparseCondensedKKTSystem
    fac = lambda A: LapackCPUSolver(A, alg)  # noqa: E731

    def make(info):
        if kind == "sparse_condensed":
            return SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J,
                                            info["ind_ineq"], info["ind_lb"], info["ind_ub"], fac)
        if kind == "dense_condensed":
            return DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"],
                                           info["ind_ub"], fac)
        return DenseKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_lb"], info["ind_ub"], fac)
    return make


def options(IPMOptions, sparse, **kw):
    o = IPMOptions(tol=1e-6 if sparse else 1e-8, **kw)
    if sparse:  # preset of SparseCondensedKKTSystem (reference src/IPM/options.jl:146-147,160,226)
        o.relax_equality, o.dual_initialization = True, "zero"
    return o


def run_host(args):
    from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
    out, total = {}, {}
    for name, kind, mk, alg, kw in host_cases():
        nlp, sparse, counts = mk(), kind == "sparse_condensed", {}
        s = counted(MadNLPSolver, counts)(nlp, oracle_factory(kind, nlp, alg), options(IPMOptions, sparse, max_iter=300, **kw),
                                          sparse=sparse)
        with np.errstate(all="ignore"):
            s.solve()
        out[name] = record(s, (s.x, s.y, s.zl, s.zu), counts)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
        print(f"{name}: {s.status}, {s.cnt.k} iterations, {s.cnt.factorization_cnt} factorizations {counts}", flush=True)
    missing = {k: (total.get(k, 0), v) for k, v in REQUIRED.items() if total.get(k, 0) < v}
    if missing:
        sys.exit(f"refusing to write: branches not reached often enough (reached, required): {missing}")
    total.setdefault("ic_ignore_perturbed", 0)     # 0: a perturbation inside the `ignore` loop is not exercised
    digest = finish(out, args.out, {"branches": dict(sorted(total.items())), "cases": sorted(out),
                                    "iteration_records": sum(len(r["history"]) for r in out.values())})
    print(f"sha256 {digest}  {len(out)} runs  branches {dict(sorted(total.items()))}")


# ------------------------------------------------------------------------------------------------ device: HIP KKT systems
LAUNCH_KEYS = ("unbatched_results", "batch_ends", "vec_launches", "scale_grad", "scale_cons", "gemv")


def count_launches(mj_ipm_device, counts):
    """Wrap `IPMDeviceKernels` so that `counts` holds: unbatched result calls, batch ends, vec_* launches, and the `scale_grad`,
    `scale_cons` and `gemv` launches under their own names."""
    K, B = mj_ipm_device.IPMDeviceKernels, mj_ipm_device._Batch
    call, leave = K._call, B.__exit__

    def _call(self, name, *a, **k):
        if not self._batching:
            counts["unbatched_results"] += 1
        return call(self, name, *a, **k)

    def __exit__(self, *exc):
        counts["batch_ends"] += 1
        return leave(self, *exc)
    K._call, B.__exit__ = _call, __exit__
    for name in [n for n in vars(K) if n.startswith("vec_")] + list(LAUNCH_KEYS[3:]):
        def wrap(f, key):
            def g(self, *a, **k):
                counts[key] += 1
                return f(self, *a, **k)
            return g
        setattr(K, name, wrap(getattr(K, name), "vec_launches" if name.startswith("vec_") else name))


def acopf_case30_fixed():
    """tests/test_hip_fixed_variables.py's model: the tape AC-OPF with variables fixed at the (CPU oracle's) unfixed optimum."""
    from madnlp_jl_amd.ipm import MadNLPSolver
    from madnlp_jl_amd.tape_model import acopf_tape_model
    from tests.test_fixed_variables_cpu import acopf_fixed, factory, sparse_options
    M0 = acopf_tape_model("case30")
    s0 = MadNLPSolver(M0, factory("sparse_condensed", M0), sparse_options(), sparse=True)
    assert s0.solve() == "SOLVE_SUCCEEDED"
    return acopf_fixed("case30", s0.solution().solution)[0]


def device_cases(mj):
    """(name, model, sparse, forced, options, solver attributes).  Between them the runs reach every way the callbacks are
    evaluated: raw values (hand-written and tape), prescaled data (sparse and dense QP) and the fixed-variable wrapper, each
    scaled and unscaled; equalities beside inequalities; exact, BFGS and compact L-BFGS Hessians; a maximization."""
    from madnlp_jl_amd import tape_model as T
    from madnlp_jl_amd.problems import ACOPFModel, DenseQPModel, InfeasibleModel, SparseQPModel
    from tests.nlp_scaling_cases import rescaled_dense_qp
    from tests.test_fixed_variables_cpu import qp_fixed
    acopf = lambda: ACOPFModel("case1354pegase")  # noqa: E731
    dqp = lambda: DenseQPModel(20, 15, 2)  # noqa: E731
    rqp = lambda: rescaled_dense_qp(20, 15, 2)  # noqa: E731
    scaled, mp = {"nlp_scaling": True}, {"fixed_variable_treatment": "make_parameter"}
    scaled10 = {"nlp_scaling": True, "nlp_scaling_max_gradient": 10.0}
    fixed30 = acopf_case30_fixed()
    small = [("hs15-tape-scaled", T.hs15_tape_model, True, False, scaled, {}),
             ("hs15-tape-unscaled", T.hs15_tape_model, True, False, {"nlp_scaling": False}, {}),
             ("acopf-case30-scaled", lambda: ACOPFModel("case30"), True, False, scaled10, {}),
             ("acopf-case30-tape-scaled", lambda: T.acopf_tape_model("case30"), True, False, scaled10, {}),
             ("acopf-case30-tape-fixed-scaled", lambda: fixed30, True, False, {**mp, **scaled10}, {}),
             ("acopf-case30-tape-fixed-unscaled", lambda: fixed30, True, False, mp, {}),
             ("lootsma-tape-fixed-scaled", T.lootsma_fixed_tape_model, True, False, {**mp, **scaled}, {}),
             ("lootsma-tape-fixed-unscaled", T.lootsma_fixed_tape_model, True, False, mp, {}),
             ("simplex-lp-tape-max-scaled", lambda: T.simplex_lp_tape_model(1.0, minimize=False), True, False, scaled, {}),
             ("simplex-lp-tape-max-unscaled", lambda: T.simplex_lp_tape_model(1.0, minimize=False), True, False, {}, {}),
             ("rescaled-dense-qp-scaled-exact", rqp, False, False, scaled, {}),
             ("rescaled-dense-qp-scaled-bfgs", rqp, False, False, {**scaled, "hessian_approximation": "bfgs"}, {}),
             ("dense-qp-frozen", lambda: qp_fixed(2), False, False, mp, {}),
             ("dense-qp-frozen-scaled", lambda: qp_fixed(2), False, False, {**mp, **scaled}, {}),
             ("sparse-qp-case30-lbfgs-scaled", lambda: SparseQPModel("case30"), True, False,
              {**scaled, "hessian_approximation": "compact_lbfgs"}, {})]
    return small + [("acopf-case1354pegase", acopf, True, False, {}, {}),
            ("acopf-case1354pegase-speculate", acopf, True, False, {}, {"speculate": True}),
            ("sparse-qp-case30-forced", lambda: SparseQPModel("case30"), True, True, {}, {}),
            ("sparse-qp-case118-forced", lambda: SparseQPModel("case118"), True, True, {}, {}),
            ("infeasible", InfeasibleModel, True, False, {}, {}),
            ("dense-qp-exact", dqp, False, False, {}, {}),
            ("dense-qp-bfgs", dqp, False, False, {"hessian_approximation": "bfgs"}, {})]


def hip_factory(mj, nlp, ctx, sparse):
    from madnlp_jl_amd.fixed_vars import structure
    opt = lambda: mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN)  # noqa: E731

    def make(info):
        if sparse:       # (`structure`: the reduced problem's under make_parameter, the diagonal Hessian's under compact L-BFGS)
            return mj.SparseCondensedKKTSystem(info["n"], info["m"], *structure(nlp, info), info["ind_ineq"],
                                               info["ind_lb"], info["ind_ub"], ctx=ctx, opt_linear_solver=opt(), device_kkt_ops=True)
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=ctx, opt_linear_solver=opt(), device_kkt_ops=True)
    return make


def close(s):
    if hasattr(s, "close"):
        return s.close()
    s.cb.close()          # (--package: a driver from before `DeviceMadNLPSolver.close`)
    s.K.close()
    s.kkt.close()


def run_device(args, mj):
    import torch
    from madnlp_jl_amd import ipm_device
    from madnlp_jl_amd.ipm import IPMOptions
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    assert torch.cuda.is_available(), "--device needs a GPU"
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)       # torch and the library share one stream
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    launches = {}
    count_launches(ipm_device, launches)
    out = {}
    for name, mk, sparse, forced, kw, attrs in device_cases(mj):
        nlp, counts = mk(), {}
        cls = counted(DeviceMadNLPSolver, counts)
        if forced:
            cls = type("ForcedDevice", (Forced, cls), {})
        launches.update(dict.fromkeys(LAUNCH_KEYS, 0))
        s = cls(nlp, hip_factory(mj, nlp, ctx, sparse), options(IPMOptions, sparse, **kw), sparse=sparse)
        for k, v in attrs.items():
            setattr(s, k, v)
        s.solve()
        rec = record(s, s.host_state(), counts)
        rec.update(launches=dict(launches), probe_hits=int(s.probe_hits), probe_misses=int(s.probe_misses),
                   speculative_factorizations=int(s.speculative_factorizations), speculative_wasted=int(s.speculative_wasted))
        out[name] = rec
        print(f"{name}: {s.status}, {s.cnt.k} iterations, {s.cnt.factorization_cnt} factorizations, {s.cnt.backsolve_cnt} "
              f"back-solves, {launches}, {counts}", flush=True)
        close(s)
    print(f"sha256 {finish(out, args.out, {'cases': sorted(out)})}  {len(out)} runs")
    ctx.close()


def time_device(args, mj):
    """it/s as bench.py's `ipm_loop` measures it (initialize, upload, synchronize, host clock around solve + synchronize): one
    warm-up run, then `args.time` timed runs, for the AC-OPF NLP and for the QP with its sparsity."""
    import torch
    from madnlp_jl_amd.ipm import IPMOptions
    from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver
    from madnlp_jl_amd.problems import ACOPFModel, SparseQPModel
    ctx = mj.HipContext(0)
    out = {}
    for key, nlp in (("end_to_end_ipm", ACOPFModel("case1354pegase")), ("end_to_end_ipm_qp", SparseQPModel("case1354pegase"))):
        samples = []
        for i in range(1 + args.time):
            s = DeviceMadNLPSolver(nlp, hip_factory(mj, nlp, ctx, True), options(IPMOptions, True))
            s.initialize()
            s._upload()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.solve()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if i:
                samples.append(s.cnt.k / wall)
            status, k = s.status, s.cnt.k
            close(s)
        out[key] = {"status": status, "iterations": k, "it_per_s": samples}
        print(f"{key}: {status}, {k} iterations, it/s {['%.2f' % v for v in samples]}, median {statistics.median(samples):.2f}", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ device: the KKT handles alone
def handle_cases(mj, ctx):
    """(name, system) on a 3-variable, 2-constraint problem: sparse condensed (two inequalities), dense augmented and dense
    condensed (one equality, one inequality); variable 2 carries both bounds; one bound side empty; dense without constraints."""
    n, hess, jac = 3, np.array([[4.0, 0, 0], [1.0, 3.0, 0], [0.5, -1.0, 5.0]]), np.array([[1.0, 2.0, -1.0], [0.5, -1.0, 3.0]])
    for kind in ("sparse_condensed", "dense", "dense_condensed"):
        for variant in ("both", "nlb0", "nub0") + (() if kind == "sparse_condensed" else ("m0",)):
            m = 0 if variant == "m0" else 2
            ineq, eq = (np.arange(m), []) if kind == "sparse_condensed" else (np.arange(1, m), np.arange(min(m, 1)))
            npr = n + len(ineq)
            lb = [] if variant == "nlb0" else [0, 2, npr - 1]
            ub = [] if variant == "nub0" else [1, 2]
            if kind == "sparse_condensed":
                jI, jJ = np.divmod(np.arange(m * n), n)
                hI, hJ = np.tril_indices(n)
                k = mj.SparseCondensedKKTSystem(n, m, jI, jJ, hI, hJ, ineq, lb, ub, ctx=ctx,
                                                opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY))
                k.jac[:], k.hess[:] = jac[jI, jJ], hess[hI, hJ]
                k.compress_jacobian()
                k.compress_hessian()
            else:
                k = (mj.DenseCondensedKKTSystem(n, m, ineq, eq, lb, ub, ctx=ctx) if kind == "dense_condensed" else
                     mj.DenseKKTSystem(n, m, ineq, lb, ub, ctx=ctx))
                k.hess[...], k.jac[...] = hess, jac[:m]
                k._upload()
            yield f"{kind}-{variant}", k


def run_handles(args, mj):
    """The handles' entry points on their own, which the IPM runs reach with device vectors only: the diagonals after
    set_aug_diagonal, after regularize_diagonal and (sparse) after save -> regularize -> restore; mul! for three (alpha, beta);
    solve_kkt! -- each vector once as a host array and once as a device tensor."""
    import torch
    assert torch.cuda.is_available(), "--device needs a GPU"
    ctx = mj.HipContext(0)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    out = {}
    for name, k in handle_cases(mj, ctx):
        rng = np.random.default_rng(3)
        npr, nlb, nub = len(k.pr_diag), len(k.ind_lb), len(k.ind_ub)
        lw = npr + len(k.du_diag) + nlb + nub
        x, xl, xu, zl, zu = rng.uniform(-0.4, 0.4, npr), np.full(npr, -1e300), np.full(npr, 1e300), np.zeros(npr), np.zeros(npr)
        xl[k.ind_lb], xu[k.ind_ub] = -rng.uniform(0.5, 2.0, nlb), rng.uniform(0.5, 2.0, nub)
        zl[k.ind_lb], zu[k.ind_ub] = 10.0 ** rng.uniform(-8, 2, nlb), 10.0 ** rng.uniform(-8, 2, nub)
        rec = {}

        def diagonals(key):
            rec[key] = {f: hexes(v) for f, v in sorted(k.get_diagonals_device().items())}
        for where, put in (("host", np.array), ("device", dev)):
            k.set_aug_diagonal_device(*[put(v) for v in (x, xl, xu, zl, zu)], primal_reg=0.5, dual_reg=1e-8)
            diagonals(f"set_aug_diagonal-{where}")
        if hasattr(k, "save_diagonals_device"):
            k.save_diagonals_device()
        k.regularize_diagonal_device(1e-4, 1e-8)
        diagonals("regularize_diagonal")
        if hasattr(k, "save_diagonals_device"):
            k.restore_diagonals_device()
            diagonals("save-regularize-restore")
        k.build_kkt_device()
        k.linear_solver.factorize()
        rec["inertia"] = list(k.linear_solver.inertia())
        xv, wv, bv = rng.standard_normal(lw), rng.standard_normal(lw), rng.standard_normal(lw)
        for where, put in (("host", np.array), ("device", dev)):
            for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.75, -0.5)):
                w = k.mul_device(put(wv), put(xv), alpha, beta)
                ctx.synchronize()
                rec[f"mul-{alpha}-{beta}-{where}"] = hexes(w if where == "host" else w.cpu().numpy())
            w = k.solve_kkt_device(put(bv))
            ctx.synchronize()
            rec[f"solve_kkt-{where}"] = hexes(w if where == "host" else w.cpu().numpy())
        out[name] = rec
        print(f"{name}: inertia {rec['inertia']}, host == device: "
              f"{all(rec[f] == rec[f[:-4] + 'device'] for f in rec if f.endswith('-host'))}", flush=True)
        k.close()
    print(f"sha256 {finish(out, args.out, {'cases': sorted(out)})}  {len(out)} handles")
    ctx.close()


# ------------------------------------------------------------------------------------------------ compare two dumps
def compare(a_path, b_path):
    """Exit status 0: every integer, status, phase and branch / launch count equal.  Prints `identical` when the floats are too,
    else per field the largest relative difference."""
    A, B = json.load(open(a_path)), json.load(open(b_path))
    if A["sha256"] == B["sha256"]:
        print(f"identical: sha256 {A['sha256']} ({len(A['runs'])} runs)")
        return 0
    bad, worst = [], {}

    def rel(field, xa, xb):
        if len(xa) != len(xb):
            bad.append(f"{field}: lengths {len(xa)} != {len(xb)}")
            return
        for u, v in zip(xa, xb):
            u, v = float.fromhex(u), float.fromhex(v)
            if u != v:
                d = abs(u - v) / max(abs(u), abs(v)) if np.isfinite(u) and np.isfinite(v) else float("inf")
                worst[field] = max(worst.get(field, 0.0), d)
    if sorted(A["runs"]) != sorted(B["runs"]):
        bad.append("different case lists")
    for name in sorted(set(A["runs"]) & set(B["runs"])):
        ra, rb = A["runs"][name], B["runs"][name]
        for key in sorted(set(ra) | set(rb)):
            if key in ("x", "y", "zl", "zu"):
                rel(f"{name}.{key}", ra[key], rb[key])
            elif key == "history":
                if [h[:3] for h in ra[key]] != [h[:3] for h in rb[key]]:
                    bad.append(f"{name}: iteration numbers / phases / line-search counts differ")
                else:
                    for i, fld in enumerate(("obj", "inf_pr", "inf_du", "inf_compl", "mu", "del_w", "alpha")):
                        rel(f"{name}.{fld}", [h[3 + i] for h in ra[key]], [h[3 + i] for h in rb[key]])
            elif ra.get(key) != rb.get(key):
                bad.append(f"{name}.{key}: {ra.get(key)} != {rb.get(key)}")
    for f, d in sorted(worst.items()):
        print(f"float field differs: {f}: largest relative difference {d:.3e}")
    for msg in bad:
        print("DIFFERENT:", msg)
    print(json.dumps({"identical": False, "integers_equal": not bad, "largest_relative_difference": max(worst.values(), default=0.0)}))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--package", help="directory to load as madnlp_jl_amd instead of the repository's madnlp.jl_amd/")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--handles", action="store_true", help="with --device: the KKT handles' entry points instead of IPM runs")
    ap.add_argument("--time", type=int, default=0, help="with --device: timed runs per problem (after one warm-up run)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("--out is required")
    mj = load_package(args.package)
    if args.device and args.time:
        time_device(args, mj)
    elif args.device and args.handles:
        run_handles(args, mj)
    elif args.device:
        run_device(args, mj)
    else:
        run_host(args)


if __name__ == "__main__":
    main()

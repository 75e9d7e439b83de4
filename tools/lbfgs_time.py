"""What compact L-BFGS Hessians cost on the device at case1354pegase (history 6): writes profiles/lbfgs_case1354.json (or the
file given as the first argument).

End to end: `DeviceMadNLPSolver` on the polar AC-OPF with `hessian_approximation = "exact"` and `"compact_lbfgs"`, alternating,
a cold and a warm run each (wall time of solve() after initialize() and the upload; iterations, factorizations, back-solves).
A run that does not end in SOLVE_SUCCEEDED within MAX_ITER iterations is recorded as it ended.

Pieces, on the state the warm L-BFGS run leaves (full memory, a factorization in place), each as a host clock around CALLS calls
that end in a stream synchronization, REPEATS times, alternating with its exact-Hessian twin in the same process (the same handle
with the L-BFGS handle detached):
  solve_kkt          device vectors, H / T / W cached              vs  the plain solve_kkt
  mul                                                              vs  the plain mul
  factorize + solve  the first solve_kkt of a factorization (build) vs  factorize + plain solve_kkt
  update             mnk_lbfgs_update on fresh pairs (it synchronizes once by itself)
`added_*` are differences of the medians; min / max of the repeats are kept as the spread."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel  # noqa: E402

CASE = sys.argv[2] if len(sys.argv) > 2 else "case1354pegase"
MAX_ITER, CALLS, REPEATS = 600, 40, 7
st = torch.cuda.Stream()
torch.cuda.set_stream(st)
ctx = mj.HipContext(0, stream=st.cuda_stream)
A = ACOPFModel(CASE)


def factory(info):
    return mj.SparseCondensedKKTSystem(info["n"], info["m"], A.jac_I, A.jac_J, info.get("hess_I", A.hess_I), info.get("hess_J", A.hess_J),
                                       info["ind_ineq"], info["ind_lb"], info["ind_ub"], ctx=ctx,
                                       opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)


def run(approx, keep=False):
    o = IPMOptions(tol=1e-6, hessian_approximation=approx, max_iter=MAX_ITER)
    o.relax_equality, o.dual_initialization = True, "zero"
    s = DeviceMadNLPSolver(A, factory, o)
    s.initialize()
    s._upload()
    ctx.synchronize()
    t0 = time.perf_counter()
    s.solve()
    ctx.synchronize()
    rec = dict(status=s.status, objective=float(s.obj_val), iterations=s.cnt.k, factorizations=s.cnt.factorization_cnt,
               backsolves=s.cnt.backsolve_cnt, lag_hess_cnt=s.cnt.lag_hess_cnt, wall_s=time.perf_counter() - t0)
    if approx == "compact_lbfgs":
        rec["lbfgs"] = s.kkt.qn_status()
    if keep:
        return rec, s
    s.close()
    return rec, None


def clock(fn):
    """seconds per call of `fn` over CALLS calls, each ending in a synchronization"""
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
        ctx.synchronize()
    return (time.perf_counter() - t0) / CALLS


def ab(with_lbfgs, plain, attach):
    """REPEATS alternating windows of the two variants: medians, spreads and the difference of the medians"""
    a, b = [], []
    for _ in range(REPEATS):
        attach(True)
        a.append(clock(with_lbfgs))
        attach(False)
        b.append(clock(plain))
    attach(True)
    f = lambda v: dict(median_s=statistics.median(v), min_s=min(v), max_s=max(v))  # noqa: E731
    return dict(lbfgs=f(a), exact_twin=f(b), added_s=statistics.median(a) - statistics.median(b))


def pieces(s):
    kkt, qd, lib = s.kkt, s.kkt.qn_dev, L.lib()
    attach = lambda on: L.check(lib.mnk_sc_attach_lbfgs(kkt._h, qd._h if on else None), "mnk_sc_attach_lbfgs")  # noqa: E731
    w0, w, x = s.p.clone(), s.p.clone(), s.d.clone()

    def solve():
        w.copy_(w0)
        kkt.solve_kkt_device(w)

    def fact_solve():
        kkt.linear_solver.factorize_async()
        w.copy_(w0)
        kkt.solve_kkt_device(w)

    for _ in range(5):          # warm-up of both variants
        fact_solve(); solve(); kkt.mul_device(w, x)
        attach(False); fact_solve(); solve(); kkt.mul_device(w, x); attach(True)
    ctx.synchronize()
    out = {"solve_kkt": ab(solve, solve, attach), "mul": ab(lambda: kkt.mul_device(w, x), lambda: kkt.mul_device(w, x), attach),
           "factorize_and_first_solve_kkt": ab(fact_solve, fact_solve, attach)}
    out["build_s"] = out["factorize_and_first_solve_kkt"]["added_s"] - out["solve_kkt"]["added_s"]
    rng = np.random.default_rng(0)
    pairs = []
    for _ in range(16):
        sv = rng.standard_normal(A.n)
        pairs.append((torch.from_numpy(sv).cuda(), torch.from_numpy(2.0 * sv + 0.1 * rng.standard_normal(A.n)).cuda()))
    ctx.synchronize()
    ups, k = [], 0
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            done, _ = qd.update(*pairs[k % 16])
            assert done
            k += 1
        ctx.synchronize()
        ups.append((time.perf_counter() - t0) / CALLS)
    out["update"] = dict(median_s=statistics.median(ups), min_s=min(ups), max_s=max(ups))
    return out


out = {"case": CASE, "n": A.n, "m": A.m, "max_history": 6, "max_iter": MAX_ITER,
       "method": f"host clock; pieces: {REPEATS} alternating windows of {CALLS} synchronizing calls after a warm-up; end to end: "
                 "solve() after initialize() and the upload, exact and compact_lbfgs alternating, cold then warm",
       "end_to_end": {}}
for phase in ("cold", "warm"):
    for approx in ("exact", "compact_lbfgs"):
        rec, s = run(approx, keep=(phase == "warm" and approx == "compact_lbfgs"))
        out["end_to_end"].setdefault(approx, {})[phase] = rec
        print(phase, approx, rec, flush=True)
if s.kkt.qn_status()["current_mem"] > 0:
    out["pieces"] = pieces(s)
    print(json.dumps(out["pieces"], indent=1), flush=True)
s.close()
ctx.close()
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "lbfgs_case1354.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
print("written", dest)

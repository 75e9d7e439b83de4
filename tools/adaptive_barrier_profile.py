"""The barrier rules on the device AC-OPF solve at case1354pegase: one cold and one warm end-to-end run of `DeviceMadNLPSolver` per
rule (`barrier = "monotone" / "loqo" / "quality_function"`), and the mean time of one `mnk_ipm_quality_function` call on that
solve's vectors (a host clock around calls that each end in the stream synchronization, after a warm-up: 200 calls of 1 sigma,
200 of 4).  Writes profiles/adaptive_barrier_case1354.json (or the file given as the first argument).  A rule that does not end
in SOLVE_SUCCEEDED within `MAX_ITER` iterations is recorded as it ended: the record is a finding about the rule, not a test."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd.ipm import BARRIER_UPDATES, IPMOptions  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel  # noqa: E402

CASE = "case1354pegase"
MAX_ITER = 500
CALLS = 200
st = torch.cuda.Stream()
ctx = mj.HipContext(0, stream=st.cuda_stream)
A = ACOPFModel(CASE)


def factory(info):
    return mj.SparseCondensedKKTSystem(info["n"], info["m"], A.jac_I, A.jac_J, A.hess_I, A.hess_J, info["ind_ineq"],
                                       info["ind_lb"], info["ind_ub"], ctx=ctx,
                                       opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)


def time_quality_function(s):
    """Mean seconds of one call on the solver's final iterate, the two last directions standing in for the probe steps."""
    K, a, c = s.K, s.d, s._w1
    out = {}
    for sigmas in ([0.5], [0.1, 0.5, 1.0, 2.0]):
        call = lambda: K.quality_function(sigmas, s.x, s.xl, s.xu, s.zl, s.zu, s._primal(a), s._dual_lb(a), s._dual_ub(a),  # noqa: E731
                                          s._primal(c), s._dual_lb(c), s._dual_ub(c), s.tau)
        for _ in range(20):
            call()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        out[f"{len(sigmas)}_sigma_mean_s"] = (time.perf_counter() - t0) / CALLS
    return out


def run(barrier, timing=False):
    o = IPMOptions(tol=1e-6, barrier=barrier, max_iter=MAX_ITER)
    o.relax_equality, o.dual_initialization = True, "zero"
    s = DeviceMadNLPSolver(A, factory, o)
    s.initialize()
    s._upload()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rec = dict(status=s.status, objective=float(s.obj_val), iterations=s.cnt.k, factorizations=s.cnt.factorization_cnt,
               backsolves=s.cnt.backsolve_cnt, barrier_updates=s.cnt.barrier_update_cnt, probe_solve_cnt=s.cnt.probe_solve_cnt,
               quality_evaluations=s.cnt.quality_eval_cnt, mu_increases=sum(b.mu > a.mu for a, b in zip(s.history, s.history[1:])),
               wall_s=wall)
    if timing:
        rec["quality_function_call"] = time_quality_function(s)
    s.close()
    return rec


out = {"case": CASE, "n": A.n, "m": A.m, "max_iter": MAX_ITER,
       "method": "wall time of solve() after initialize() and the upload, a cold then a warm run per rule in one process; "
                 f"quality_function_call: host clock over {CALLS} synchronizing calls after 20 warm-up calls",
       "rules": {}}
for barrier in BARRIER_UPDATES:
    cold = run(barrier)
    warm = run(barrier, timing=barrier == "quality_function")
    out["rules"][barrier] = dict(cold=cold, warm=warm)
    print(barrier, warm, flush=True)
ctx.close()
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "adaptive_barrier_case1354.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
print("written", dest)

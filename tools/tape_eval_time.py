"""Callback timing (HIP events, 100 calls after 10 warm-up calls, evaluators alternated) and end-to-end device runs of the
tape AC-OPF beside the hand-written one at case1354pegase; writes profiles/tape_eval_case1354.json
(or the file given as the first argument)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import tape_model as T  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver, DeviceOPFCallbacks, DeviceTapeCallbacks, _up  # noqa: E402
from madnlp_jl_amd.ipm_device import IPMDeviceKernels  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel  # noqa: E402

CASE = "case1354pegase"
out = {"case": CASE, "method": "HIP events around 100 calls after 10 warm-up calls, per round; 7 rounds, the two evaluators "
       "alternated inside every round, one process; microseconds per call"}
st = torch.cuda.Stream()
ctx = mj.HipContext(0, stream=st.cuda_stream)
A = ACOPFModel(CASE)
t0 = time.perf_counter()
M = T.acopf_tape_model(CASE)
out["host_compile_s"] = time.perf_counter() - t0
out["sizes"] = dict(n=M.n, m=M.m, nnzj_tape=len(M.jac_I), nnzj_hand=len(A.jac_I), nnzh_tape=len(M.hess_I), nnzh_hand=len(A.hess_I))
K = IPMDeviceKernels(A.n, np.arange(1), np.arange(1), ctx=ctx)
cbs = {"tape": DeviceTapeCallbacks(M, None, "cuda", K), "hand": DeviceOPFCallbacks(A, None, "cuda", K)}
rng = np.random.default_rng(5)
x, y = A.x0 + 0.1 * rng.standard_normal(A.n), rng.standard_normal(A.m)
xd, yd = _up(x, "cuda"), _up(y, "cuda")
g = torch.empty(A.n, dtype=torch.float64, device="cuda")
c = torch.empty(A.m, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
calls = {"cons": lambda cb: cb.cons(c, xd), "jac_coord": lambda cb: cb.jac_coord(xd), "hess_coord": lambda cb: cb.hess_coord(xd, yd, 1.0),
         "grad": lambda cb: cb.grad(g, xd)}
times = {k: {w: [] for w in cbs} for k in calls}
with torch.cuda.stream(st):
    for rnd in range(7):
        for name, fn in calls.items():
            for w, cb in cbs.items():
                for _ in range(10):
                    fn(cb)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(100):
                    fn(cb)
                e1.record(st)
                e1.synchronize()
                times[name][w].append(e0.elapsed_time(e1) * 10.0)      # ms / 100 calls -> us per call
out["callback_us"] = {k: {w: dict(median=statistics.median(v), min=min(v), max=max(v)) for w, v in d.items()} for k, d in times.items()}
for k, d in out["callback_us"].items():
    d["ratio_median"] = d["tape"]["median"] / d["hand"]["median"]
print(json.dumps(out["callback_us"], indent=1), flush=True)

# accuracy at this size (summed matrices, 1e-13 scale rule) and the sqrt observation
ctx.synchronize()
jt, jo = cbs["tape"].jac_coord(xd), cbs["hand"].jac_coord(xd)
cbs["tape"].cons(c, xd)
ctx.synchronize()
ct = c.cpu().numpy().copy()
out["cons_maxdiff_vs_host_hand"] = float(np.abs(ct - A.cons(x)).max())
out["cons_tape_device_vs_tape_host_maxdiff"] = float(np.abs(ct - M.cons(x)).max())
for cb in cbs.values():
    cb.close()

S = T.TapeModel(4096, 4096, np.ones(4096), 0.0, 10.0, 0.0, 0.0)
S.add_constraint(T.sqrt(T.V(0)), np.arange(4096), np.arange(4096)[:, None])
S.finalize()
cbq = DeviceTapeCallbacks(S, None, "cuda", K)
xs = np.random.default_rng(1).uniform(1e-3, 10.0, 4096)
cs = torch.empty(4096, dtype=torch.float64, device="cuda")
xsd = _up(xs, "cuda")
torch.cuda.synchronize()
cbq.cons(cs, xsd)
jq = cbq.jac_coord(xsd)
ctx.synchronize()
out["sqrt_bit_identical"] = bool(np.array_equal(cs.cpu().numpy(), np.sqrt(xs)))
out["sqrt_derivative_bit_identical"] = bool(np.array_equal(jq.cpu().numpy(), S.jac_coord(xs)))
cbq.close()
K.close()
print("sqrt bit-identical:", out["sqrt_bit_identical"], out["sqrt_derivative_bit_identical"], flush=True)


def run(nlp):
    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                           info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)
    o = IPMOptions(tol=1e-6)
    o.relax_equality, o.dual_initialization = True, "zero"
    s = DeviceMadNLPSolver(nlp, factory, o)
    s.initialize()
    s._upload()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rec = dict(status=s.status, objective=s.obj_val, iterations=s.cnt.k, factorizations=s.cnt.factorization_cnt,
               backsolves=s.cnt.backsolve_cnt, wall_s=wall)
    s.cb.close(); s.K.close(); s.kkt.close()
    return rec


runs = {"tape": [], "hand": []}
for rnd in range(4):                     # (the first round is the cold one)
    for w, nlp in (("hand", A), ("tape", M)):
        runs[w].append(run(nlp))
        print(w, runs[w][-1], flush=True)
out["end_to_end"] = {w: dict(runs=v, warm_wall_s_median=statistics.median(r["wall_s"] for r in v[1:]),
                             warm_wall_s_min=min(r["wall_s"] for r in v[1:])) for w, v in runs.items()}
ctx.close()
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "tape_eval_case1354.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
print("written", dest)

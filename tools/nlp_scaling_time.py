"""What the scaled launches cost when the factors are one: end-to-end device AC-OPF runs at case1354pegase with `nlp_scaling` off
and on (per iteration +2 `mnk_ipm_vec_mul`, and `mnk_ipm_scale_cons` / `mnk_ipm_scale_grad` in place of two / one launches), one
cold round, then three warm rounds alternated in one process, timed as tools/tape_eval_time.py times its end-to-end runs (DESIGN.md
section 15); writes profiles/nlp_scaling_case1354.json (or the file given as the first argument)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel  # noqa: E402

CASE = "case1354pegase"
st = torch.cuda.Stream()
ctx = mj.HipContext(0, stream=st.cuda_stream)
A = ACOPFModel(CASE)


def run(scaling):
    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], A.jac_I, A.jac_J, A.hess_I, A.hess_J, info["ind_ineq"],
                                           info["ind_lb"], info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)
    o = IPMOptions(tol=1e-6, nlp_scaling=scaling)
    o.relax_equality, o.dual_initialization = True, "zero"
    s = DeviceMadNLPSolver(A, factory, o)
    s.initialize()
    s._upload()
    assert s._scaled == scaling and s.obj_scale == 1.0 and (s.con_scale == 1.0).all()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rec = dict(status=s.status, objective=s.obj_val, iterations=s.cnt.k, factorizations=s.cnt.factorization_cnt,
               backsolves=s.cnt.backsolve_cnt, wall_s=wall)
    s.close()
    return rec


runs = {"off": [], "on": []}
for rnd in range(4):                     # (the first round is the cold one)
    for w in ("off", "on"):
        runs[w].append(run(w == "on"))
        print(w, runs[w][-1], flush=True)
ctx.close()
counts = lambda r: (r["status"], r["objective"], r["iterations"], r["factorizations"], r["backsolves"])  # noqa: E731
out = {"case": CASE, "method": "wall time of solve() after initialize() and the upload, one cold round then three warm rounds, "
       "nlp_scaling off / on alternated inside every round, one process; all factors are 1",
       "counts_identical": len({counts(r) for v in runs.values() for r in v}) == 1,
       "end_to_end": {w: dict(runs=v, warm_wall_s_median=statistics.median(r["wall_s"] for r in v[1:]),
                              warm_wall_s_min=min(r["wall_s"] for r in v[1:]), warm_wall_s_max=max(r["wall_s"] for r in v[1:]))
                      for w, v in runs.items()}}
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "nlp_scaling_case1354.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
print("written", dest)

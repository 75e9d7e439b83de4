"""What `fixed_variable_treatment = "make_parameter"` costs on the device, at case1354pegase as tapes with
every 29th variable (from 5) and the last one fixed at their values in the unfixed optimum: per callback, the plain
`DeviceTapeCallbacks` on the full model (what a `"relax_bound"` run launches) beside `DeviceFixedVariableCallbacks` around them
(one expand, one gather more), HIP events around 100 calls after 10 warm-up calls, the two alternated inside every round; and
end to end, `DeviceMadNLPSolver` with either option value on the same model, alternated.  The parent commit's record of the same
tape callbacks (profiles/tape_eval_case1354.json) is copied beside the numbers.  Writes profiles/fixed_variables_case1354.json
(or the file given as the first argument)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import fixed_vars as FV  # noqa: E402
from madnlp_jl_amd import tape_model as T  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions  # noqa: E402
from madnlp_jl_amd.device_callbacks import DeviceFixedVariableCallbacks, DeviceTapeCallbacks, _up  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.ipm_device import IPMDeviceKernels  # noqa: E402

CASE = sys.argv[2] if len(sys.argv) > 2 else "case1354pegase"
ROUNDS, WARM, CALLS = 7, 10, 100

st = torch.cuda.Stream()
ctx = mj.HipContext(0, stream=st.cuda_stream)


def solve(nlp, treatment, tol=1e-6):
    def factory(info):
        return mj.SparseCondensedKKTSystem(info["n"], info["m"], *FV.structure(nlp, info), info["ind_ineq"], info["ind_lb"],
                                           info["ind_ub"], ctx=ctx,
                                           opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)
    o = IPMOptions(tol=tol, fixed_variable_treatment=treatment)
    o.relax_equality, o.dual_initialization = True, "zero"
    s = DeviceMadNLPSolver(nlp, factory, o)
    s.initialize()
    s._upload()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    r = s.solution()
    rec = dict(status=s.status, objective=r.objective, n=s.n, iterations=s.cnt.k, factorizations=s.cnt.factorization_cnt,
               backsolves=s.cnt.backsolve_cnt, obj_grad_evals=s.cnt.obj_grad_cnt, wall_s=wall)
    s.close()
    return rec, r


M = T.acopf_tape_model(CASE)
rec0, r0 = solve(M, "relax_bound")
print("unfixed", rec0, flush=True)
where = np.array(sorted(set(range(5, M.n, 29)) | {M.n - 1}))
M.lvar, M.uvar = M.lvar.copy(), M.uvar.copy()
lvar0, uvar0 = M.lvar.copy(), M.uvar.copy()
M.lvar[where] = M.uvar[where] = r0.solution[where]
h = FV.FixedVariableHandler.create(M, True)
out = {"case": CASE,
       "method": f"HIP events around {CALLS} calls after {WARM} warm-up calls, per round; {ROUNDS} rounds, plain and wrapped callbacks "
                 "alternated inside every round (the first one changing from round to round), one process; microseconds per call",
       "sizes": dict(n=M.n, m=M.m, nfixed=len(h.fixed), nfree=len(h.free), nnzj=len(M.jac_I), nnzj_free=len(h.ind_jac_free),
                     nnzh=len(M.hess_I), nnzh_free=len(h.ind_hess_free)),
       "unfixed_run": rec0}

K = IPMDeviceKernels(M.n, np.arange(1), np.arange(1), ctx=ctx)
plain = DeviceTapeCallbacks(M, None, "cuda", K)
wrapped = DeviceFixedVariableCallbacks(DeviceTapeCallbacks(M, None, "cuda", K), h, None, "cuda", K)
rng = np.random.default_rng(5)
x, y = M.x0 + 0.1 * rng.standard_normal(M.n), rng.standard_normal(M.m)
xs = {"plain": _up(x, "cuda"), "wrapped": _up(x[h.free], "cuda")}
gs = {"plain": torch.empty(M.n, dtype=torch.float64, device="cuda"), "wrapped": torch.empty(len(h.free), dtype=torch.float64, device="cuda")}
yd, c = _up(y, "cuda"), torch.empty(M.m, dtype=torch.float64, device="cuda")
jscale, jscale_full = _up(rng.uniform(0.5, 2.0, len(h.ind_jac_free)), "cuda"), _up(rng.uniform(0.5, 2.0, len(M.jac_I)), "cuda")
torch.cuda.synchronize()
cbs = {"plain": plain, "wrapped": wrapped}
calls = {"cons": lambda w: cbs[w].cons(c, xs[w]), "jac_coord": lambda w: cbs[w].jac_coord(xs[w]),
         "hess_coord": lambda w: cbs[w].hess_coord(xs[w], yd, 1.0), "grad": lambda w: cbs[w].grad(gs[w], xs[w]),
         # the scaled path: the plain callbacks are followed by the solver's separate launch, the wrapped ones fuse it
         "jac_coord_scaled": lambda w: (K.vec_mul(plain.jv, plain.jac_coord(xs[w]), jscale_full) if w == "plain"
                                        else wrapped.jac_coord(xs[w], jscale))}
times = {k: {w: [] for w in cbs} for k in calls}
with torch.cuda.stream(st):
    for rnd in range(ROUNDS):
        for name, fn in calls.items():
            for w in list(cbs)[::-1 if rnd % 2 else 1]:
                for _ in range(WARM):
                    fn(w)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(CALLS):
                    fn(w)
                e1.record(st)
                e1.synchronize()
                times[name][w].append(e0.elapsed_time(e1) * 1000.0 / CALLS)
out["callback_us"] = {k: {w: dict(median=statistics.median(v), min=min(v), max=max(v)) for w, v in d.items()} for k, d in times.items()}
for d in out["callback_us"].values():
    d["layer_us_median"] = d["wrapped"]["median"] - d["plain"]["median"]
print(json.dumps(out["callback_us"], indent=1), flush=True)
ctx.synchronize()
plain.close(); wrapped.close(); K.close()



def emptied_rows(nlp, hd):
    """Rows whose Jacobian entries all belong to fixed variables: constants of the reduced problem.  (count, their worst
    violation of lcon / ucon at x_full): a violation above the 1e-8 equality relaxation makes the reduced problem infeasible."""
    rows = np.setdiff1d(np.unique(nlp.jac_I), np.unique(hd.jac_I))
    cv = nlp.cons(hd.x_full)[rows]
    viol = np.maximum(np.maximum(nlp.lcon[rows] - cv, cv - nlp.ucon[rows]), 0.0)
    return int(len(rows)), float(viol.max(initial=0.0))


# end to end, twice: the fixed values taken from the unfixed optimum at the runs' own tolerance (1e-6, the instance above), and
# from an unfixed optimum computed at tol 1e-8, i.e. accurate to the width of the relaxed equality rows
out["end_to_end"] = {}
for label, x_src in (("fixed_at_tol_1e-6_optimum", r0.solution), ("fixed_at_tol_1e-8_optimum", None)):
    if x_src is None:
        M.lvar[where], M.uvar[where] = lvar0[where], uvar0[where]
        rec8, r8 = solve(M, "relax_bound", tol=1e-8)
        print("unfixed at tol 1e-8", rec8, flush=True)
        x_src = r8.solution
    M.lvar[where] = M.uvar[where] = x_src[where]
    hd = FV.FixedVariableHandler.create(M, True)
    hd.x_full[hd.free] = x_src[hd.free]
    nrows, viol = emptied_rows(M, hd)
    runs = {"relax_bound": [], "make_parameter": []}
    for rnd in range(3):                     # (the first round is the cold one)
        for w in list(runs)[::-1 if rnd % 2 else 1]:
            runs[w].append(solve(M, w)[0])
            print(label, w, runs[w][-1], flush=True)
    out["end_to_end"][label] = dict(rows_without_a_free_variable=nrows, their_worst_violation_at_the_fixed_values=viol,
                                    **{w: dict(runs=v, warm_wall_s_median=statistics.median(r["wall_s"] for r in v[1:]),
                                               warm_wall_s_min=min(r["wall_s"] for r in v[1:])) for w, v in runs.items()})
    print(label, "rows without a free variable", nrows, "worst violation", viol, flush=True)
try:
    parent = json.load(open(os.path.join(ROOT, "profiles", "tape_eval_case1354.json")))
    out["parent_record_tape_eval_case1354"] = dict(
        callback_us={k: d["tape"] for k, d in parent["callback_us"].items()},
        end_to_end_unfixed_warm_wall_s_median=parent["end_to_end"]["tape"]["warm_wall_s_median"],
        end_to_end_unfixed_iterations=parent["end_to_end"]["tape"]["runs"][0]["iterations"])
except (OSError, KeyError):
    pass
ctx.close()
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fixed_variables_case1354.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
print("written", dest)

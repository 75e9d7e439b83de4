"""The two refinement iterators on the device AC-OPF solve at case1354pegase: one cold and one warm end-to-end run of
`DeviceMadNLPSolver` per iterator (`iterator = "richardson" / "krylov"`) with iterations, factorizations, back-solves, Arnoldi
steps, GMRES cycles and wall time; next to them the mean time of the vector launches of one Arnoldi step (dots -> project ->
dots -> project -> normalize in one batch, k = 1 and k = 5 columns) and of one `solve_kkt!` on that solve's vectors (a host
clock around calls that each end in the stream synchronization, after a warm-up).  Writes
profiles/krylov_iterator_case1354.json (or the file given as the first argument).  A run that does not end in SOLVE_SUCCEEDED is
recorded as it ended: the record is a finding, not a test."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd.backsolve import ITERATORS  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel  # noqa: E402

CASE = "case1354pegase"
MAX_ITER = 500
CALLS = 200
st = torch.cuda.Stream()
torch.cuda.set_stream(st)
ctx = mj.HipContext(0, stream=st.cuda_stream)
A = ACOPFModel(CASE)


def factory(info):
    return mj.SparseCondensedKKTSystem(info["n"], info["m"], A.jac_I, A.jac_J, A.hess_I, A.hess_J, info["ind_ineq"],
                                       info["ind_lb"], info["ind_ub"], ctx=ctx,
                                       opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN), device_kkt_ops=True)


def mean_time(call):
    for _ in range(20):
        call()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        call()
    return (time.perf_counter() - t0) / CALLS


def time_step_pieces(s):
    """Mean seconds of the vector part of one Arnoldi step and of one solve_kkt! on the solver's final vectors."""
    K, n = s.K, s._lw
    V = torch.randn((6, n), dtype=torch.float64, device=s.dev)
    u = s._new_vec(n)
    out = {"kkt_vector_length": n}
    for k in (1, 5):
        def step():
            K.vec_copy(u, s.d)
            with K.batch():
                K.krylov_dots(V, k, u)
                K.krylov_project(u, V, k)
                K.krylov_dots(V, k, u)
                K.krylov_project(u, V, k)
                K.krylov_normalize(V[k], u, True)
        out[f"arnoldi_vector_part_k{k}_mean_s"] = mean_time(step)

    def solve():
        K.vec_copy(u, s.p)
        s.kkt.solve_kkt_device(u)
        s._sync()
    out["solve_kkt_mean_s"] = mean_time(solve)

    def norms():
        with K.batch():
            K.get_norms(u)
            K.get_norms(s.d)
    out["two_norms_batch_mean_s"] = mean_time(norms)
    return out


def run(iterator, timing=False):
    o = IPMOptions(tol=1e-6, iterator=iterator, max_iter=MAX_ITER)
    o.relax_equality, o.dual_initialization = True, "zero"
    s = DeviceMadNLPSolver(A, factory, o)
    s.initialize()
    s._upload()
    tally = dict(refined_solves=0, arnoldi_steps=0, gmres_cycles=0, refinements_given_up=0)
    inner = s.solve_refine_wrapper

    def counted(*a):
        ok = inner(*a)
        tally["refined_solves"] += 1
        tally["arnoldi_steps"] += getattr(s.iterator, "steps", 0)
        tally["gmres_cycles"] += getattr(s.iterator, "cycles", 0)
        tally["refinements_given_up"] += not ok
        return ok
    s.solve_refine_wrapper = counted
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rec = dict(status=s.status, objective=float(s.obj_val), iterations=s.cnt.k, factorizations=s.cnt.factorization_cnt,
               backsolves=s.cnt.backsolve_cnt, **tally, wall_s=wall)
    if timing:
        rec["step_pieces"] = time_step_pieces(s)
    s.close()
    return rec


out = {"case": CASE, "n": A.n, "m": A.m, "max_iter": MAX_ITER,
       "method": "wall time of solve() after initialize() and the upload, a cold then a warm run per iterator in one process; "
                 f"step_pieces: host clock over {CALLS} synchronizing calls after 20 warm-up calls",
       "iterators": {}}
for iterator in ITERATORS:
    cold = run(iterator)
    warm = run(iterator, timing=iterator == "krylov")
    out["iterators"][iterator] = dict(cold=cold, warm=warm)
    print(iterator, warm, flush=True)
ctx.close()
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "krylov_iterator_case1354.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
print("written", dest)

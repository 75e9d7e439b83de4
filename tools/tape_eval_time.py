"""Callback timing (HIP events, 100 calls after 10 warm-up calls, evaluators alternated) and end-to-end device runs of the
tape AC-OPF beside the hand-written one at case1354pegase; writes profiles/tape_eval_case1354.json
(or the file given as the first argument).

`tape_eval_time.py --against PARENT_LIB [DEST]` instead times the tape callbacks of THIS tree's library against a second
libmadnlp_hip.so built from another commit (its parent: `git worktree add DIR HEAD~1`, build there, pass DIR's library), both
loaded into one process and alternated inside every round, and the callbacks of the three closed-form problems with the new
operations (tests/tape_ops_cases.py) at 11 192 rows; writes profiles/tape_ops_case1354.json.  Acceptance per callback: this
tree's median <= the other library's median + its own (max - min) across the rounds."""
import ctypes as C
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
from madnlp_jl_amd.device_callbacks import DeviceOPFCallbacks, DeviceTapeCallbacks, _up  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.ipm_device import IPMDeviceKernels  # noqa: E402
from madnlp_jl_amd.problems import ACOPFModel  # noqa: E402

CASE = "case1354pegase"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, WARM, CALLS = 8, 10, 100


class RawTape:
    """`mnk_tape_*` of ONE loaded library on a model: what `DeviceTapeCallbacks` does, without the package's library singleton."""

    def __init__(self, lib, stream, nlp):
        from madnlp_jl_amd import _lib as L
        for name in ("mnk_ctx_create", "mnk_ctx_destroy", "mnk_ctx_synchronize", "mnk_last_error_string", "mnk_tape_create", "mnk_tape_destroy",
                     "mnk_tape_add_pattern", "mnk_tape_finalize", "mnk_tape_grad", "mnk_tape_cons", "mnk_tape_jac_coord", "mnk_tape_hess_coord"):
            f = getattr(lib, name)
            f.restype, f.argtypes = L.SIGNATURES[name]
        self.lib, self.ctx, self.h = lib, C.c_void_p(), C.c_void_p()
        self.ok(lib.mnk_ctx_create(0, C.c_void_p(stream), C.byref(self.ctx)))
        self.ok(lib.mnk_tape_create(self.ctx, nlp.n, nlp.m, C.byref(self.h)))
        for p in nlp.patterns:
            args = []
            for t in p.tapes:
                args += [len(t.code), t.code.ctypes.data, len(t.consts), t.consts.ctypes.data, t.nout, t.out_operand.ctypes.data,
                         t.out_j.ctypes.data, t.out_l.ctypes.data, t.nslot]
            self.ok(lib.mnk_tape_add_pattern(self.h, p.kind, p.R, p.k, p.q, p.var_index.ctypes.data, p.params.ctypes.data,
                                             p.rows.ctypes.data if p.kind == 1 else None, *args))
        self.ok(lib.mnk_tape_finalize(self.h))
        self.jv = torch.empty(max(len(nlp.jac_I), 1), dtype=torch.float64, device="cuda")
        self.hv = torch.empty(max(len(nlp.hess_I), 1), dtype=torch.float64, device="cuda")

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.lib.mnk_last_error_string().decode())

    def cons(self, c, x): self.ok(self.lib.mnk_tape_cons(self.h, x.data_ptr(), c.data_ptr()))
    def grad(self, g, x): self.ok(self.lib.mnk_tape_grad(self.h, x.data_ptr(), g.data_ptr()))
    def jac_coord(self, x): self.ok(self.lib.mnk_tape_jac_coord(self.h, x.data_ptr(), self.jv.data_ptr()))
    def hess_coord(self, x, y, w): self.ok(self.lib.mnk_tape_hess_coord(self.h, x.data_ptr(), y.data_ptr(), w, self.hv.data_ptr()))

    def close(self):
        self.lib.mnk_ctx_synchronize(self.ctx)
        self.lib.mnk_tape_destroy(self.h)
        self.lib.mnk_ctx_destroy(self.ctx)


def time_callbacks(st, cbs, n, m, x, y):
    """median / min / max microseconds per call over ROUNDS rounds, the evaluators of `cbs` alternated inside every round (and
    which of them goes first alternated from round to round)"""
    xd, yd = _up(x, "cuda"), _up(y, "cuda")
    g = torch.empty(n, dtype=torch.float64, device="cuda")
    c = torch.empty(max(m, 1), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    calls = {"cons": lambda cb: cb.cons(c, xd), "jac_coord": lambda cb: cb.jac_coord(xd), "hess_coord": lambda cb: cb.hess_coord(xd, yd, 1.0),
             "grad": lambda cb: cb.grad(g, xd)}
    times = {k: {w: [] for w in cbs} for k in calls}
    with torch.cuda.stream(st):
        for rnd in range(ROUNDS):
            for name, fn in calls.items():
                for w, cb in list(cbs.items())[::-1 if rnd % 2 else 1]:
                    for _ in range(WARM):
                        fn(cb)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(CALLS):
                        fn(cb)
                    e1.record(st)
                    e1.synchronize()
                    times[name][w].append(e0.elapsed_time(e1) * 1000.0 / CALLS)      # ms / CALLS calls -> us per call
    return {k: {w: dict(median=statistics.median(v), min=min(v), max=max(v)) for w, v in d.items()} for k, d in times.items()}


def against(parent_path, dest):
    sys.path.insert(0, ROOT)
    from tests import tape_ops_cases as cases
    res = {"case": CASE, "method": f"HIP events around {CALLS} calls after {WARM} warm-up calls, per round; {ROUNDS} rounds, the two libraries "
           "alternated inside every round (the first one changing from round to round), one process, raw mnk_tape_* calls on both; "
           "microseconds per call",
           "acceptance": "this tree's median <= the parent's median + the parent's (max - min)"}
    st = torch.cuda.Stream()
    libs = {"parent": C.CDLL(os.path.abspath(parent_path)), "tree": mj.lib()}
    M = T.acopf_tape_model(CASE)
    rng = np.random.default_rng(5)
    x, y = M.x0 + 0.1 * rng.standard_normal(M.n), rng.standard_normal(M.m)
    cbs = {w: RawTape(lib, st.cuda_stream, M) for w, lib in libs.items()}
    res["callback_us"] = time_callbacks(st, cbs, M.n, M.m, x, y)
    for k, d in res["callback_us"].items():
        d["accepted"] = d["tree"]["median"] <= d["parent"]["median"] + (d["parent"]["max"] - d["parent"]["min"])
    # same inputs, same answers: the AC-OPF tapes have no new instruction
    torch.cuda.synchronize()
    xd = _up(x, "cuda")
    torch.cuda.synchronize()
    for cb in cbs.values():
        cb.jac_coord(xd)
    torch.cuda.synchronize()
    res["jac_bit_identical_to_parent"] = bool(torch.equal(cbs["tree"].jv, cbs["parent"].jv))
    for cb in cbs.values():
        cb.close()
    print(json.dumps(res["callback_us"], indent=1), flush=True)
    # the closed-form problems with the new operations at the AC-OPF's variable count
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    K = IPMDeviceKernels(M.n, np.arange(1), np.arange(1), ctx=ctx)
    res["new_operations_us"] = {}
    for name, make in cases.NLPS.items():
        N, _ = make(M.n)
        cb = DeviceTapeCallbacks(N, None, "cuda", K)
        xs = np.random.default_rng(6).uniform(0.5, 1.5, N.n)
        t = time_callbacks(st, {"tree": cb}, N.n, N.m, xs, np.ones(N.m))
        res["new_operations_us"][name] = dict(rows=N.n, extended_launches=cb.extended(), **{k: d["tree"] for k, d in t.items()})
        print(name, json.dumps(res["new_operations_us"][name]), flush=True)
        cb.close()
    K.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    json.dump(res, open(dest, "w"), indent=1)
    print("written", dest)


if len(sys.argv) > 1 and sys.argv[1] == "--against":
    against(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "tape_ops_case1354.json"))
    sys.exit(0)

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
    s.close()
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

"""Writes profiles/qn_bfgs_update.json (run once on the MI355X, from the repository root):

1. device-event time of one `mnk_dc_qn_update` (damped BFGS: the longer of the two kinds) at n = 512, 2048, 8192: median of
   20 after 3 warm-ups, with the algorithmic bytes 1.5 x 8 n^2 and the resulting TB/s;
2. the same update written with torch on the same card and stream (`torch.mv` on the full symmetric matrix, two `addr_`
   rank-1 updates: vendor BLAS, at least 5 x 8 n^2 bytes) as the comparator -- tools only, never in the library;
3. the C2-sized end-to-end pair of the device-resident driver on DenseQPModel(2048, 512, 0): ms per iteration with
   `hessian_approximation = "exact"` (one device-to-device copy of P per iteration), with "damped_bfgs", and with the exact
   run that also updates a quasi-Newton matrix in a second handle (same trajectory, plus the quasi-Newton step), five
   repetitions each, alternated, with iteration counts, back-solves and line-search trials per iteration and the exact run's
   spread (max - min); and, from one more pair of runs, the Hessian step alone between two synchronizations (the copy of P
   against forming s, y and updating).

    python tools/qn_update_bench.py [--sizes 512,2048,8192] [--e2e 2048,512,0] [--out profiles/qn_bfgs_update.json]
"""
import argparse
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
from madnlp_jl_amd.ipm import IPMOptions  # noqa: E402
from madnlp_jl_amd.ipm_dev import DeviceMadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import DenseQPModel  # noqa: E402

COPY_TBS = 6.29      # the device-to-device copy rate DESIGN.md quotes for this card
WARMUP, REPS = 3, 20


def event_times(fn, stream):
    """ms of each of REPS calls of fn (enqueue only), after WARMUP calls."""
    for _ in range(WARMUP):
        fn()
    stream.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def update_case(ctx, stream, n):
    rng = np.random.default_rng(n)
    dev = torch.device("cuda")
    e = np.zeros(0, dtype=np.int64)
    k = mj.DenseCondensedKKTSystem(n, 0, e, e, e, e, ctx=ctx)
    s = torch.from_numpy(rng.standard_normal(n)).to(dev)
    y = (2.0 * s + 0.1 * torch.from_numpy(rng.standard_normal(n)).to(dev)).contiguous()
    g0 = torch.from_numpy(rng.standard_normal(n)).to(dev)
    k.qn_init_device("damped_bfgs", g0, 1.0)          # B = 2 rho0 I; every update keeps it positive definite (s'y > 0)
    hip = event_times(lambda: k.qn_update_device(s, y), stream)
    updates = k.qn_status()[0]
    k.close()
    B = (2.0 * torch.eye(n, dtype=torch.float64, device=dev)).contiguous()

    def torch_update():
        bs = torch.mv(B, s)
        sbs = torch.dot(s, bs)
        sy = torch.dot(s, y)
        B.addr_(bs * (-1.0 / sbs), bs)
        B.addr_(y * (1.0 / sy), y)
    ref = event_times(torch_update, stream)
    del B
    bytes_ = 1.5 * 8 * n * n
    med, rmed = statistics.median(hip), statistics.median(ref)
    return {"n": n, "hip_update_ms_median": med, "hip_update_ms_min": min(hip), "hip_update_ms_max": max(hip),
            "algorithmic_bytes": bytes_, "hip_TBps": bytes_ / (med * 1e-3) / 1e12, "copy_TBps_quoted": COPY_TBS,
            "torch_update_ms_median": rmed, "torch_update_ms_min": min(ref), "torch_update_ms_max": max(ref),
            "torch_bytes_at_least": 5 * 8 * n * n, "hip_not_slower_than_torch": bool(med <= rmed), "updates_run": int(updates)}


class ExactWithShadowUpdate(DeviceMadNLPSolver):
    """The exact-Hessian run -- its trajectory, its work per iteration -- that ALSO forms the secant pair and updates a
    quasi-Newton matrix of the same order in a second handle every iteration: what the quasi-Newton step costs inside the loop
    with everything else equal (the quasi-Newton run itself follows another trajectory, with other numbers of back-solves and
    line-search trials per iteration)."""

    def _upload(self):
        super()._upload()
        n, e = self.n, np.zeros(0, dtype=np.int64)
        self.shadow = mj.DenseCondensedKKTSystem(n, 0, e, e, e, e, ctx=self.kkt.ctx)
        self.shadow.qn_init_device("damped_bfgs", self.f[:n], self.obj_val)
        self.sv = {k: self._new_vec(n) for k in ("sk", "yk", "last_x", "last_g", "last_jv")}
        self.K.vec_copy(self.sv["last_x"], self.x[:n])
        self.K.vec_copy(self.sv["last_g"], self.f[:n])

    def eval_lag_hess(self, x, y, is_resto=False):
        super().eval_lag_hess(x, y, is_resto)
        if getattr(self, "shadow", None) is None:
            return
        n, v = self.n, self.sv
        self.cb.jtprod_at(v["last_x"], y, v["last_jv"])
        self.shadow.qn_secant_device(x[:n], self.f[:n], self.jacl[:n], v["last_jv"], v["last_x"], v["last_g"], v["sk"], v["yk"])
        self.shadow.qn_update_device(v["sk"], v["yk"])


def e2e_run(ctx, nlp, approx, max_iter, time_hess=False):
    def factory(info):
        return mj.DenseCondensedKKTSystem(info["n"], info["m"], info["ind_ineq"], info["ind_eq"], info["ind_lb"], info["ind_ub"],
                                          ctx=ctx, opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=mj.BUNCHKAUFMAN),
                                          device_kkt_ops=True)
    shadow = approx == "exact+shadow"
    cls = ExactWithShadowUpdate if shadow else DeviceMadNLPSolver
    s = cls(nlp, factory, IPMOptions(tol=1e-8, hessian_approximation="exact" if shadow else approx, max_iter=max_iter), sparse=False)
    s.initialize()
    s._upload()
    ctx.synchronize()
    hess = {"s": 0.0, "calls": 0}
    if time_hess:      # the Hessian step alone, between two synchronizations (perturbs the loop: never in the timed pairs)
        inner = s.eval_lag_hess

        def timed(x, y, is_resto=False):
            ctx.synchronize()
            t = time.perf_counter()
            inner(x, y, is_resto)
            ctx.synchronize()
            hess["s"] += time.perf_counter() - t
            hess["calls"] += 1
        s.eval_lag_hess = timed
    t0 = time.perf_counter()
    s.solve()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    k = max(1, s.cnt.k)
    rec = {"hessian_approximation": approx, "status": s.status, "k": s.cnt.k, "factorizations": s.cnt.factorization_cnt,
           "loop_ms": ms, "ms_per_iteration": ms / k, "lag_hess_cnt": s.cnt.lag_hess_cnt,
           "backsolves_per_iteration": s.cnt.backsolve_cnt / k, "line_search_trials_per_iteration": sum(r.ls for r in s.history) / k}
    if time_hess:
        rec = {"hessian_approximation": approx, "k": s.cnt.k, "hessian_step_us_synchronized": 1e6 * hess["s"] / max(1, hess["calls"])}
    elif approx != "exact":
        u, sk, _ = (s.shadow if shadow else s.kkt).qn_status()
        rec.update(updates=u, skipped=sk)
    if shadow:
        s.shadow.close()
    s.kkt.close()
    s.K.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048,8192")
    ap.add_argument("--e2e", default="2048,512,0")
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qn_bfgs_update.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "update": [], "end_to_end": None}
    for n in [int(v) for v in a.sizes.split(",") if v]:
        rec = update_case(ctx, st, n)
        print(json.dumps(rec), flush=True)
        out["update"].append(rec)
    if a.e2e:
        n, m, n_eq = (int(v) for v in a.e2e.split(","))
        nlp = DenseQPModel(n, m, n_eq)
        e2e_run(ctx, nlp, "exact", a.max_iter)            # warm-up of every kernel and buffer of the loop
        runs = []
        for _ in range(5):
            for approx in ("exact", "exact+shadow", "damped_bfgs"):
                r = e2e_run(ctx, nlp, approx, a.max_iter)
                print(json.dumps(r), flush=True)
                runs.append(r)
        ex = [r["ms_per_iteration"] for r in runs if r["hessian_approximation"] == "exact"]
        sh = [r["ms_per_iteration"] for r in runs if r["hessian_approximation"] == "exact+shadow"]
        qn = [r["ms_per_iteration"] for r in runs if r["hessian_approximation"] == "damped_bfgs"]
        upd = next((u["hip_update_ms_median"] for u in out["update"] if u["n"] == n), None)
        spread = max(ex) - min(ex)
        e = {"size": [n, m, n_eq], "runs": runs, "exact_ms_per_iteration_median": statistics.median(ex),
             "exact_spread_ms": spread, "damped_bfgs_ms_per_iteration_median": statistics.median(qn),
             "exact_with_shadow_update_ms_per_iteration_median": statistics.median(sh), "update_ms_at_n": upd}
        if upd is not None:     # the requirement, on the quasi-Newton run itself and with the trajectory held equal
            e["within_update_plus_spread"] = bool(statistics.median(qn) <= statistics.median(ex) + upd + spread)
            e["shadow_within_update_plus_spread"] = bool(statistics.median(sh) <= statistics.median(ex) + upd + spread)
        e["hessian_step"] = [e2e_run(ctx, nlp, approx, a.max_iter, time_hess=True) for approx in ("exact", "damped_bfgs")]
        out["end_to_end"] = e
        print(json.dumps({k: v for k, v in e.items() if k != "runs"}), flush=True)
    torch.cuda.set_stream(torch.cuda.default_stream())
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Writes profiles/lbfgs_host_vs_exact.json: the host mirror's compact L-BFGS runs (`hessian_approximation = "compact_lbfgs"`,
`kkt.LowRankHessianKKT` around the CPU oracle's SparseCondensedKKTSystem, sparse-condensed preset, tol = 1e-6) against the
exact-Hessian run of the same system, on the cases of tests/test_hip_compact_lbfgs.py::test_device_resident_run, which
asserts ten times the `dobj` recorded here for the device run.  `SparseQPModel("case118")` is recorded as the known limit
(DESIGN.md section 18), with both history lengths.  No GPU needed:  python tools/lbfgs_host_vs_exact.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from madnlp_jl_amd.problems import ACOPFModel, SparseQPModel  # noqa: E402
from test_compact_lbfgs_cpu import run  # noqa: E402

CASES = [("acopf_case30", lambda: ACOPFModel("case30"), {}), ("acopf_case118", lambda: ACOPFModel("case118"), {}),
         ("sparse_qp_case30", lambda: SparseQPModel("case30"), {}),
         ("sparse_qp_case118", lambda: SparseQPModel("case118"), {}),
         ("sparse_qp_case118_history20", lambda: SparseQPModel("case118"), {"qn_max_history": 20})]

out = {"what": "host mirror, compact L-BFGS run against the exact-Hessian run, CPU oracle SparseCondensedKKTSystem, "
               "sparse-condensed preset, tol = 1e-6", "cases": {}}
for name, make, kw in CASES:
    nlp = make()
    ex = run(nlp, "exact")
    s = run(nlp, "compact_lbfgs", **kw)
    rec = {"n": nlp.n, "m": nlp.m, "options": kw, "exact": {"status": ex.status, "k": ex.cnt.k, "obj": ex.obj_val},
           "status": s.status, "k": s.cnt.k, "obj": s.obj_val, "updates": s.qn.updates, "skipped": s.qn.skipped,
           "resets": s.qn.resets, "lag_hess_cnt": s.cnt.lag_hess_cnt, "factorizations": s.cnt.factorization_cnt,
           "backsolves": s.cnt.backsolve_cnt, "dobj": float(abs(s.obj_val - ex.obj_val)),
           "dx": float(np.abs(s.x[:nlp.n] - ex.x[:nlp.n]).max())}
    out["cases"][name] = rec
    print(name, rec["status"], rec["k"], "exact", ex.status, ex.cnt.k, "dobj", rec["dobj"], "dx", rec["dx"], flush=True)
with open(os.path.join(ROOT, "profiles", "lbfgs_host_vs_exact.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")

"""Writes profiles/qn_host_vs_exact.json: the host mirror's quasi-Newton runs (`hessian_approximation = "bfgs" /
"damped_bfgs"`, both dense KKT systems of the CPU oracle) against the exact-Hessian run on `DenseKKTSystem`, on the
`DenseQPModel` sizes of tests/test_quasi_newton_cpu.py::test_dense_qp_against_the_exact_hessian_run, which asserts ten
times the `max_dx` / `max_dy` recorded here.  No GPU needed:  python tools/qn_host_vs_exact.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from madnlp_jl_amd.problems import DenseQPModel  # noqa: E402
from test_quasi_newton_cpu import APPROX, KINDS, run  # noqa: E402

SIZES = [(10, 5, 0), (50, 10, 0), (20, 15, 2), (200, 60, 8)]

out = {"what": "host mirror, quasi-Newton run against the exact-Hessian run on DenseKKTSystem, tol = 1e-8 (CPU oracle KKT systems)",
       "sizes": []}
for size in SIZES:
    nlp = DenseQPModel(*size)
    ex = run("dense", nlp, "exact")
    rec = {"size": list(size), "exact": {"status": ex.status, "k": ex.cnt.k}, "runs": []}
    for kind in KINDS:
        for approx in APPROX:
            s = run(kind, nlp, approx)
            rec["runs"].append({"kkt": kind, "hessian_approximation": approx, "status": s.status, "k": s.cnt.k,
                                "updates": s.qn.updates, "skipped": s.qn.skipped, "lag_hess_cnt": s.cnt.lag_hess_cnt,
                                "dobj": float(abs(s.obj_val - ex.obj_val)),
                                "dx": float(np.abs(s.x[:size[0]] - ex.x[:size[0]]).max()),
                                "dy": float(np.abs(s.y - ex.y).max())})
    ok = [r for r in rec["runs"] if r["status"] == "SOLVE_SUCCEEDED"]
    rec["max_dx"] = max(r["dx"] for r in ok)
    rec["max_dy"] = max(r["dy"] for r in ok)
    rec["max_dobj"] = max(r["dobj"] for r in ok)
    out["sizes"].append(rec)
    print(size, rec["max_dx"], rec["max_dy"], rec["max_dobj"], [(r["hessian_approximation"], r["status"], r["k"]) for r in rec["runs"]])
with open(os.path.join(ROOT, "profiles", "qn_host_vs_exact.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")

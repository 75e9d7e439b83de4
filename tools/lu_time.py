"""Times the LU solver (lapack_algorithm = LU, csrc/lu.hip) against the QR solver (csrc/qr.hip) in the same run: factorize!
and solve! at the C2 order (N = 2048, dense condensed) and the C3 order (N = 11 192, sparse condensed) on the bench's matrix
generators, HIP events on the launch stream, one warm-up and `--trials` timed calls each, LU and QR alternating per size.
TFLOP/s against 2N^3/3 (LU) and 4N^3/3 (QR).

  python tools/lu_time.py [--sizes 2048,11192] [--trials 10] [--json profiles/lu_time.json]
  python tools/lu_time.py --split results.db           # rocprofv3 --kernel-trace --stats: per-phase breakdown
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import qr_time  # noqa: E402  (the QR tool: event timing, dense image, rocprofv3 split)

PEAK_TFLOPS = qr_time.PEAK_TFLOPS

# kernel name fragment -> phase of the LU schedule (the QR phases are kept: a trace of this tool holds both)
PHASES = [("lu_panel_kernel", "LU panel"), ("lu_laswp_kernel", "LU interchanges"), ("lu_trsm_kernel", "LU U12 = L11^-1 A12"),
          ("lu_init_kernel", "LU panel"), ("lu_gather_kernel", "LU solve: P b"), ("lu_lsolve_kernel", "LU solve: L^-1"),
          ("lu_pivots_out_kernel", "other")] + qr_time.PHASES


def system(N, ctx, mj, algo):
    """The KKT system of order N from the bench's generators, built, with a solver of the given algorithm."""
    from madnlp_jl_amd.problems import dense_dummy_qp, opf_shaped
    opt = mj.HipSolverOptions(lapack_algorithm=algo)
    cls = mj.HipLUSolver if algo == mj.LU else mj.HipLinearSolver
    if N == 11192:
        P = opf_shaped("case1354pegase", du=1e-8)
        k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                        linear_solver=cls, opt_linear_solver=opt)
        k.jac[:] = P.jac
        k.hess[:] = P.hess
        src = f"opf_shaped(case1354pegase), sparse condensed, N = {P.n}"
    else:
        P = dense_dummy_qp(N, N // 4)
        k = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx, linear_solver=cls,
                                       opt_linear_solver=opt)
        k.jac[...] = P.jac
        k.hess[...] = P.hess
        src = f"dense_dummy_qp({N}, {N // 4}), dense condensed, N = {N}"
    for f in ("reg", "l_diag", "u_diag", "l_lower", "u_lower", "du_diag"):
        getattr(k, f)[:] = getattr(P, f)
    k.compress_jacobian()
    k.compress_hessian()
    k.set_aug_diagonal()
    k.build_kkt()
    return k, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,11192")
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--split", default=None, help="rocpd .db or kernel_stats.csv of a rocprofv3 --kernel-trace run: per-phase breakdown")
    a = ap.parse_args()
    if a.split:
        qr_time.PHASES = PHASES
        qr_time.split(a.split)
        return
    import torch

    import madnlp_jl_amd as mj
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    out = []
    for N in [int(v) for v in a.sizes.split(",")]:
        rec = {"N": N, "trials": a.trials}
        for algo, flop in ((mj.LU, 2.0 * N ** 3 / 3.0), (mj.QR, 4.0 * N ** 3 / 3.0)):
            k, src = system(N, ctx, mj, algo)
            A = qr_time.dense_of(k)
            tf, ts, x, b = qr_time.time_gpu(k, a.trials, torch)
            if algo == mj.LU:
                k.linear_solver.factorize()
                assert k.linear_solver.info == 0
            berr = float(np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))
            key = algo.lower()
            rec["source"] = src
            rec[f"{key}_factorize_ms_median"] = float(np.median(tf))
            rec[f"{key}_factorize_ms_min"] = float(np.min(tf))
            rec[f"{key}_solve_ms_median"] = float(np.median(ts))
            rec[f"{key}_solve_ms_min"] = float(np.min(ts))
            rec[f"{key}_backward_error"] = berr
            rec[f"{key}_tflops"] = flop / (rec[f"{key}_factorize_ms_median"] * 1e-3) / 1e12
            k.close()
        rec["lu_factorize_faster_than_qr"] = rec["lu_factorize_ms_median"] < rec["qr_factorize_ms_median"]
        rec["lu_over_qr_factorize"] = rec["lu_factorize_ms_median"] / rec["qr_factorize_ms_median"]
        rec["lu_over_qr_solve"] = rec["lu_solve_ms_median"] / rec["qr_solve_ms_median"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.close()
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()

"""Times the EVD solver (lapack_algorithm = EVD, csrc/evd.hip) beside QR, LU and LDL in the same run: factorize! and solve!
at the C2 order (N = 2048, dense condensed) and the C3 order (N = 11 192, sparse condensed) on the bench's matrix generators,
HIP events on the launch stream, one warm-up and `--trials` timed calls each.  EVD's TFLOP/s is counted against 12 N^3 flop per
sweep.  scipy's dsyevd runs on the same box with 1 and `--threads` BLAS threads at the sizes up to `--cpu-max`.

  python tools/evd_time.py [--sizes 2048,11192] [--trials 10] [--cpu-max 2048] [--json profiles/evd_time.json]
  python tools/evd_time.py --split results.db          # rocprofv3 --kernel-trace --stats: per-phase breakdown
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lu_time  # noqa: E402  (system(): the bench's matrices with a solver of any algorithm)
import qr_time  # noqa: E402  (event timing, dense image, rocprofv3 split)

PHASES = [("evd_pair_kernel", "EVD pair kernel (64 x 64 Jacobi in LDS)"), ("evd_update_kernel<true>", "EVD A <- Q^T A Q (MFMA)"),
          ("evd_update_kernel<false>", "EVD V <- V Q (MFMA)"), ("evd_update_kernel", "EVD updates (MFMA)"),
          ("evd_colnorm_kernel", "EVD stop test"), ("evd_norm_kernel", "EVD stop test"), ("evd_init_kernel", "EVD init"),
          ("evd_diag_kernel", "EVD sort / finish"), ("evd_rank_kernel", "EVD sort / finish"),
          ("evd_permute_kernel", "EVD sort / finish"), ("evd_inertia_kernel", "EVD sort / finish"),
          ("evd_qtx_kernel", "EVD solve"), ("evd_qt_kernel", "EVD solve"), ("evd_sum_kernel", "EVD solve")] + lu_time.PHASES


def time_dsyevd(A, threads):
    import scipy.linalg.lapack as la
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        return None
    with threadpool_limits(limits=threads):
        t0 = time.perf_counter()
        _, _, info = la.dsyevd(A, compute_v=1, lower=1)
        assert info == 0
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,11192")
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--algos", default="EVD,QR,LU,LDL")
    ap.add_argument("--cpu-max", type=int, default=2048, help="largest order at which scipy's dsyevd is timed")
    ap.add_argument("--threads", type=int, default=16)
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
        A = None
        for algo in a.algos.split(","):
            k, src = lu_time.system(N, ctx, mj, algo)
            if A is None:
                A = qr_time.dense_of(k)
            tf, ts, x, b = qr_time.time_gpu(k, a.trials, torch)
            key = algo.lower()
            rec["source"] = src
            rec[f"{key}_factorize_ms_median"] = float(np.median(tf))
            rec[f"{key}_factorize_ms_min"] = float(np.min(tf))
            rec[f"{key}_solve_ms_median"] = float(np.median(ts))
            rec[f"{key}_solve_ms_min"] = float(np.min(ts))
            rec[f"{key}_backward_error"] = float(np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))
            if algo == mj.EVD:
                sweeps = k.linear_solver.get_stat("evd_sweeps")
                rec["evd_sweeps"] = sweeps
                rec["evd_tflops"] = 12.0 * N ** 3 * sweeps / (rec["evd_factorize_ms_median"] * 1e-3) / 1e12
                rec["evd_info"] = k.linear_solver.factorize().info
            k.close()
        if N <= a.cpu_max:
            for th in (1, a.threads):
                rec[f"dsyevd_ms_{th}_threads"] = time_dsyevd(A, th)
        else:
            rec["dsyevd"] = f"not timed above N = {a.cpu_max}"
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.close()
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()

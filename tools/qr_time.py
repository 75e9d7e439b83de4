"""Times the QR solver (lapack_algorithm = QR, csrc/qr.hip): factorize! and solve! at the C2 / C3 orders on the bench's matrix
generators, HIP events on the launch stream, one warm-up and `--trials` timed calls each; TFLOP/s against 4N^3/3 and the
fraction of the 78.6 TFLOP/s fp64 MFMA peak.  The host reference (labelled) is scipy's dgeqrf + dormqr + dtrtrs on the same
matrix with the host's BLAS threads.

  python tools/qr_time.py [--sizes 2048,4096,11192] [--trials 10] [--no-cpu] [--json out.json]
  python tools/qr_time.py --split results.db           # rocprofv3 --kernel-trace --stats: panel / trailing products / solve
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 78.6

# kernel name fragment -> phase of the QR schedule
PHASES = [("qr_panel_kernel", "panel"), ("qr_extract_v_kernel", "panel"), ("qr_form_t_kernel", "panel"),
          ("qr_mirror_kernel", "transfer"), ("scatter_csc_kernel", "transfer"), ("copy_lower_kernel", "transfer"),
          ("fill_lower_kernel", "transfer"), ("qr_tn_kernel", "trailing products (MFMA)"),
          ("gemm_nt_kernel", "trailing products (MFMA)"), ("qr_wt_kernel", "trailing products (W^T T)"),
          ("qr_qt_kernel", "solve: Q^T b"), ("qr_rsolve_kernel", "solve: R^-1")]


def split(path):
    """Per-kernel and per-phase totals of a rocprofv3 --kernel-trace run: its rocpd SQLite database (.db) or --stats CSV."""
    agg = {}
    if path.endswith(".db"):
        import sqlite3
        cur = sqlite3.connect(path).cursor()
        cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
        namecol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
        for n, t0, t1 in cur.execute(f"select {namecol}, start, end from kernels"):
            a = agg.setdefault(n, [0, 0.0])
            a[0] += 1
            a[1] += (t1 - t0) / 1e6
    else:
        for r in csv.DictReader(open(path)):
            agg[r["Name"]] = [int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6]
    tot = {}
    lines = ["| phase | kernel | calls | total ms | avg us |", "|---|---|---|---|---|"]
    for name, (calls, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        ph = next((p for frag, p in PHASES if frag in name), "other")
        tot[ph] = tot.get(ph, 0.0) + ms
        short = name.split("(")[0].replace("void ", "").replace("mnk::", "")[:70]
        lines.append(f"| {ph} | {short} | {calls} | {ms:.3f} | {1e3 * ms / calls:.2f} |")
    lines += ["", "| phase | total ms |", "|---|---|"] + [f"| {p} | {v:.3f} |" for p, v in sorted(tot.items(), key=lambda kv: -kv[1])]
    print("\n".join(lines))


def system(N, ctx, mj):
    """The KKT system of order N from the bench's generators, built, with a QR solver."""
    from madnlp_jl_amd.problems import dense_dummy_qp, opf_shaped
    opt = mj.HipSolverOptions(lapack_algorithm=mj.QR)
    if N == 11192:
        P = opf_shaped("case1354pegase", du=1e-8)
        k = mj.SparseCondensedKKTSystem(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, ctx=ctx,
                                        opt_linear_solver=opt)
        k.jac[:] = P.jac
        k.hess[:] = P.hess
        src = f"opf_shaped(case1354pegase), sparse condensed, N = {P.n}"
    else:
        P = dense_dummy_qp(N, N // 4)
        k = mj.DenseCondensedKKTSystem(P.n, P.m, P.ind_ineq, P.ind_eq, P.ind_lb, P.ind_ub, ctx=ctx, opt_linear_solver=opt)
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


def dense_of(k):
    A = k.aug_com.to_dense() if hasattr(k.aug_com, "to_dense") else k.aug_com.to_host()
    return np.tril(A) + np.tril(A, -1).T


def time_gpu(k, trials, torch):
    ls = k.linear_solver
    s = torch.cuda.current_stream()
    N = ls.n
    b = torch.from_numpy(np.random.default_rng(0).standard_normal(N)).cuda()
    x = b.clone()

    def ev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ev_ms(ls.factorize_async)
    tf = [ev_ms(ls.factorize_async) for _ in range(trials)]

    def solve():
        x.copy_(b)
        ls.solve_linear_system(x)
    ev_ms(solve)
    ts = [ev_ms(solve) for _ in range(trials)]
    ls.check_solve()
    return tf, ts, x.cpu().numpy(), b.cpu().numpy()


def time_cpu(A, b):
    import scipy.linalg.lapack as la
    t0 = time.perf_counter()
    qr, tau, _, info = la.dgeqrf(A)
    t1 = time.perf_counter()
    lwork = la.dormqr("L", "T", qr, tau, b[:, None].copy(), -1)[1][0]
    y, _, _ = la.dormqr("L", "T", qr, tau, b[:, None].copy(), max(1, int(lwork)))
    x, _ = la.dtrtrs(qr, y, lower=0, trans=0, unitdiag=0)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,4096,11192")
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--split", default=None, help="rocpd .db or kernel_stats.csv of a rocprofv3 --kernel-trace run: per-phase breakdown")
    a = ap.parse_args()
    if a.split:
        split(a.split)
        return
    import torch

    import madnlp_jl_amd as mj
    # a stream of our own, shared by the library and torch: the events and the copies around the solves are ordered with the
    # library's work (the legacy default stream has no handle to share -- a context given none makes a stream of its own)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    out = []
    for N in [int(v) for v in a.sizes.split(",")]:
        k, src = system(N, ctx, mj)
        A = dense_of(k)
        tf, ts, x, b = time_gpu(k, a.trials, torch)
        berr = float(np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))
        flop = 4.0 * N ** 3 / 3.0
        rec = {"N": N, "source": src, "trials": a.trials, "factorize_ms_median": float(np.median(tf)),
               "factorize_ms_min": float(np.min(tf)), "solve_ms_median": float(np.median(ts)), "solve_ms_min": float(np.min(ts)),
               "backward_error": berr}
        rec["tflops"] = flop / (rec["factorize_ms_median"] * 1e-3) / 1e12
        rec["fraction_of_fp64_mfma_peak"] = rec["tflops"] / PEAK_TFLOPS
        if not a.no_cpu:
            from threadpoolctl import threadpool_info
            cf, cs = time_cpu(np.asfortranarray(A), b)
            rec["cpu_label"] = (f"HOST scipy dgeqrf + dormqr + dtrtrs, one call, BLAS threads "
                                f"{[p.get('num_threads') for p in threadpool_info()]}")
            rec["cpu_factorize_ms"], rec["cpu_solve_ms"] = cf, cs
        print(json.dumps(rec), flush=True)
        out.append(rec)
        k.close()
    ctx.close()
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()

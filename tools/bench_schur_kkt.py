"""One interior-point run on a two-stage QP through `SchurComplementKKTSystem`, with the scenario blocks assembled on the device
(round 6: mnk_schur_assemble) and with the host assembly of rounds 4-5 (numpy slicing + upload of every dense block): wall time of
the run, of its build_kkt! calls and of the assembly part of them.
usage: python tools/bench_schur_kkt.py [ns nv nd nc nc_eq density_v density_d] [--gram-threshold=T[,T...]] [--repeats=N]
                                       [--no-host] [--label=TEXT] [--out=FILE]
  -> one JSON line per run (appended to FILE as well)
--gram-threshold: the Gram row threshold of the device assembly (`default`, `never` or a number; inequality rows with more COO
entries are condensed as Gram products on the matrix cores instead of pair lists, which grow with the square of a row's length);
several values are run in alternation, `--repeats` times each (A/B on one box: profiles/schur_gram_assembly.jsonl).
--no-host: skip the run with the host assembly.
--kkt-ops[=FILE]: instead of the above, time `solve_kkt!` and `mul!` PER CALL at the same shape -- the host path (scipy products
around the stage), the device path (`device_kkt_ops=True`: mnk_schur_solve_kkt / mnk_schur_mul) with host vectors and with device
tensors, 10 trials each after one warm-up, in alternation on one box -- and the whole interior-point run with and without
`device_kkt_ops`; the record goes to FILE (default profiles/schur_device_kkt_ops.json)."""
import json
import os
import sys
import time
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "8")
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver  # noqa: E402
from madnlp_jl_amd.problems import random_twostage_qp  # noqa: E402
from madnlp_jl_amd import schur as _schur  # noqa: E402
from madnlp_jl_amd.schur import GRAM_NEVER  # noqa: E402
from madnlp_jl_amd.schur_kkt import SchurComplementKKTSystem  # noqa: E402

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
ns, nv, nd, nc, nc_eq = (int(a) for a in pos[:5]) if len(pos) >= 5 else (128, 384, 256, 128, 64)
dv, dd = (float(a) for a in pos[5:7]) if len(pos) >= 7 else (0.03, 0.05)
thresholds = [{"default": None, "never": GRAM_NEVER}.get(t, t) for t in flags.get("gram-threshold", "default").split(",")]
thresholds = [t if t is None or t == GRAM_NEVER else int(t) for t in thresholds]
repeats = int(flags.get("repeats", "1"))
runs = [(True, t) for _ in range(repeats) for t in thresholds] + ([] if "no-host" in flags else [(False, None)])

nlp = random_twostage_qp(ns=ns, nv=nv, nd=nd, nc=nc, nc_eq=nc_eq, seed=3, density_v=dv, density_d=dd)
row_len = np.bincount(nlp.jac_I, minlength=nlp.m)[nlp.lcon != nlp.ucon]
ctx = mj.HipContext(0)


def kkt_ops_record(trials=10):
    """Per-call times of solve_kkt! / mul! on one factorized system per path, and the two whole runs."""
    import torch

    def factory(device_ops):
        return lambda info: SchurComplementKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                                     info["ind_eq"], info["ind_lb"], info["ind_ub"], ctx=ctx, device_kkt_ops=device_ops,
                                                     **nlp.schur_opts())
    solvers = {}
    for device_ops in (False, True):
        s = MadNLPSolver(nlp, factory(device_ops), IPMOptions(), sparse=True)
        s.initialize()
        s.set_aug_diagonal()
        s.kkt.build_kkt()
        s.kkt.factorize_kkt()
        solvers[device_ops] = s
    rhs = np.random.default_rng(2).standard_normal(solvers[False].d.values.shape)
    dvc = torch.device("cuda", ctx.device)
    wh, xh = solvers[False].d.copy(), solvers[False].d.copy()
    wd, xd = solvers[True].d.copy(), solvers[True].d.copy()
    wt, xt = torch.zeros(len(rhs), dtype=torch.float64, device=dvc), torch.tensor(rhs, dtype=torch.float64, device=dvc)
    rt = xt.clone()
    xh.values[:] = rhs
    xd.values[:] = rhs

    def solve_host():
        wh.values[:] = rhs
        solvers[False].kkt.solve_kkt(wh)

    def solve_dev_host():
        wd.values[:] = rhs
        solvers[True].kkt.solve_kkt(wd)

    def solve_dev_dev():
        wt.copy_(rt)
        torch.cuda.synchronize()
        solvers[True].kkt.solve_kkt_device(wt)

    calls = {"solve_kkt": {"host_path": solve_host, "device_path_host_vectors": solve_dev_host, "device_path_device_vectors": solve_dev_dev},
             "mul": {"host_path": lambda: solvers[False].kkt.mul(wh, xh, 1.0, 0.5),
                     "device_path_host_vectors": lambda: solvers[True].kkt.mul(wd, xd, 1.0, 0.5),
                     "device_path_device_vectors": lambda: solvers[True].kkt.mul_device(wt, xt, 1.0, 0.5)}}
    out = {}
    for op, paths in calls.items():
        times = {k: [] for k in paths}
        for trial in range(trials + 1):                       # (trial 0: the warm-up)
            for k, f in paths.items():                        # in alternation
                ctx.synchronize()
                t0 = time.perf_counter()
                f()
                ctx.synchronize()
                if trial > 0:
                    times[k].append(1e3 * (time.perf_counter() - t0))
        out[op + "_ms"] = {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "trials": v} for k, v in times.items()}
    # (the device result against the host path's, for the record: another summation order)
    solve_host(); solve_dev_host()
    out["solve_kkt_max_abs_difference_device_vs_host_path"] = float(np.abs(wd.values - wh.values).max())
    for s in solvers.values():
        s.kkt.close()
    runs = {}
    for trial in range(2):                                    # (run 0 of each: the warm-up)
        for device_ops in (False, True):
            t0 = time.perf_counter()
            s = MadNLPSolver(nlp, factory(device_ops), IPMOptions(), sparse=True)
            setup = time.perf_counter() - t0
            t0 = time.perf_counter()
            s.solve()
            wall = time.perf_counter() - t0
            runs["device_kkt_ops" if device_ops else "default"] = {"status": s.status, "iterations": s.cnt.k, "objective": s.obj_val,
                                                                   "setup_s": setup, "solve_wall_s": wall}
            s.kkt.close()
    out["ipm_run"] = runs
    out["problem"] = (f"random_twostage_qp(ns={ns}, nv={nv}, nd={nd}, nc={nc}, nc_eq={nc_eq}, density_v={dv}, density_d={dd}): n={nlp.n}, "
                      f"m={nlp.m}, nnz(J)={len(nlp.jac_I)}")
    out["method"] = f"{trials} trials per path after one warm-up, the paths in alternation, wall clock around one call with the stream drained"
    return out


if "kkt-ops" in flags:
    rec = kkt_ops_record()
    if "label" in flags:
        rec["label"] = flags["label"]
    path = flags["kkt-ops"] if flags["kkt-ops"] != "1" else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                                        "schur_device_kkt_ops.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "method"}))
    ctx.close()
    sys.exit(0)
for device_assembly, threshold in runs:
    t_build, t_asm, t_struct = [], [], []

    def make(info):
        inner_set = _schur.SchurDenseStage.set_structure

        def timed_set(self, *a, **kw):
            t0 = time.perf_counter(); r = inner_set(self, *a, **kw); t_struct.append(time.perf_counter() - t0)
            return r
        _schur.SchurDenseStage.set_structure = timed_set
        try:
            k = SchurComplementKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"], info["ind_eq"],
                                         info["ind_lb"], info["ind_ub"], ctx=ctx, gram_row_threshold=threshold, **nlp.schur_opts())
        finally:
            _schur.SchurDenseStage.set_structure = inner_set
        k.device_assembly = device_assembly
        inner_build, inner_asm = k.build_kkt, (k.stage.assemble if device_assembly else k.assemble_blocks)

        def timed_build():
            ctx.synchronize(); t0 = time.perf_counter(); inner_build(); ctx.synchronize(); t_build.append(time.perf_counter() - t0)

        def timed_asm(*a):
            ctx.synchronize(); t0 = time.perf_counter(); r = inner_asm(*a); ctx.synchronize(); t_asm.append(time.perf_counter() - t0)
            return r
        k.build_kkt = timed_build
        if device_assembly:
            k.stage.assemble = timed_asm
        else:
            k.assemble_blocks = timed_asm
        return k
    t0 = time.perf_counter()
    s = MadNLPSolver(nlp, make, IPMOptions(), sparse=True)
    setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    s.solve()
    wall = time.perf_counter() - t0
    rec = {"problem": f"random_twostage_qp(ns={ns}, nv={nv}, nd={nd}, nc={nc}, nc_eq={nc_eq}, density_v={dv}, density_d={dd}): n={nlp.n}, m={nlp.m}, "
                      f"blk={s.kkt.blk}, nnz(J)={len(nlp.jac_I)}",
           "assembly": "device (mnk_schur_assemble)" if device_assembly else "host (numpy slicing + upload of the dense blocks; rounds 4-5)",
           "status": s.status, "iterations": s.cnt.k, "objective": s.obj_val, "setup_s": setup, "solve_wall_s": wall,
           "build_kkt_calls": len(t_build), "build_kkt_ms_mean": 1e3 * float(np.mean(t_build)),
           "assembly_ms_mean": 1e3 * float(np.mean(t_asm)), "assembly_ms_min": 1e3 * float(np.min(t_asm)),
           "ineq_row_entries_mean": float(row_len.mean()), "ineq_row_entries_max": int(row_len.max())}
    if device_assembly:
        rec["gram_row_threshold"] = "default" if threshold is None else "never" if threshold == GRAM_NEVER else threshold
        rec["assembly_stats"] = dict(zip(("pair_terms", "segments", "long_rows", "staged_doubles", "threshold"), s.kkt.stage.assembly_stats()))
        rec["set_structure_s"] = float(np.sum(t_struct))
    if "label" in flags:
        rec["label"] = flags["label"]
    line = json.dumps(rec)
    print(line, flush=True)
    if "out" in flags:
        with open(flags["out"], "a") as f:
            f.write(line + "\n")
    s.kkt.close()

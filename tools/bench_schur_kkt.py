"""One interior-point run on a two-stage QP through `SchurComplementKKTSystem`, with the scenario blocks assembled on the device
(round 6: mnk_schur_assemble) and with the host assembly of rounds 4-5 (numpy slicing + upload of every dense block): wall time of
the run, of its build_kkt! calls and of the assembly part of them.
usage: python tools/bench_schur_kkt.py [ns nv nd nc nc_eq density_v density_d] [--gram-threshold=T[,T...]] [--repeats=N]
                                       [--no-host] [--label=TEXT] [--out=FILE]
  -> one JSON line per run (appended to FILE as well)
--gram-threshold: the Gram row threshold of the device assembly (`default`, `never` or a number; inequality rows with more COO
entries are condensed as Gram products on the matrix cores instead of pair lists, which grow with the square of a row's length);
several values are run in alternation, `--repeats` times each (A/B on one box: profiles/schur_gram_assembly.jsonl).
--no-host: skip the run with the host assembly."""
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

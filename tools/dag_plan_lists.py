#!/usr/bin/env python3
"""sha256 of what the task-DAG planner (csrc/dag_plan.hip) produces, one line per configuration (host only, no device opened).

    python tools/dag_plan_lists.py [--lib PATH] [--quick]

Calls the host-only entries mnk_debug_dag_tasks, mnk_debug_dag_merged_tasks, mnk_debug_dag_deal (tasks, order, off, first_phase)
and mnk_debug_envh_ksteps of the library at PATH (default: this tree's build) over a grid of orders, band shapes, chunk
lengths, zero-fill, merged instances and queue deals, and prints `sha256  entry  configuration`.  Two builds that print the same
lines plan the same schedules: that is how a change of the planner's code shows that it changed no list (record:
profiles/dag_plan_lists.txt).  Not a golden file -- schedule work is meant to change these lists."""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import sys

import numpy as np

NTILES = (2, 3, 10, 11, 12, 43, 44, 88, 154, 240)
CAP = 1 << 22


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "madnlp.jl_amd", "lib", "libmadnlp_hip.so"))
    ap.add_argument("--quick", action="store_true", help="orders up to 44 tiles only")
    args = ap.parse_args()
    lib = C.CDLL(os.path.abspath(args.lib))
    vp, ci = C.c_void_p, C.c_int
    lib.mnk_debug_dag_tasks.argtypes = [ci] * 5 + [vp, ci, vp]
    lib.mnk_debug_dag_merged_tasks.argtypes = [ci] * 8 + [vp, ci]
    lib.mnk_debug_dag_deal.argtypes = [ci] * 10 + [vp, vp, ci, vp, vp]
    lib.mnk_debug_envh_ksteps.argtypes = [ci] * 5 + [vp, vp, vp]
    tasks = np.zeros(4 * CAP, dtype=np.int32)
    order = np.zeros(CAP, dtype=np.int32)

    def sha(*parts):
        h = hashlib.sha256()
        for p in parts:
            h.update(np.ascontiguousarray(p).tobytes())
        return h.hexdigest()

    for ntile in NTILES:
        if args.quick and ntile > 44:
            continue
        nsc = (ntile + 1) // 2
        for js2, chunk, taper0, band in itertools.product(sorted({0, (ntile + 3) // 4, nsc}), (4, 64), (1, 2), (4, 8)):
            base = f"ntile={ntile} js2={js2} chunk={chunk} taper0={taper0} band_tiles={band}"
            n1 = ci(0)
            n = lib.mnk_debug_dag_tasks(ntile, chunk, band, js2, taper0, tasks.ctypes.data, CAP, C.byref(n1))
            assert 0 <= n <= CAP
            print(sha(tasks[:4 * n], np.int64([n, n1.value])), "tasks", base, f"n={n}")
            # envelope counts: a dense envelope and a random monotone one (fixed seed), with and without the half-tile envelope
            rng = np.random.default_rng(1000 * ntile + js2)
            env_rand = np.minimum(np.sort(rng.integers(0, ntile, ntile)), np.arange(ntile)).astype(np.int32)
            for name, env in (("dense", np.zeros(ntile, dtype=np.int32)), ("random", env_rand)):
                envh = np.repeat(2 * env, 2).astype(np.int32)
                envh[1::2] = np.minimum(envh[1::2] + (rng.integers(0, 2, ntile) if name == "random" else 0), 2 * np.arange(ntile) + 1)
                cnt = np.zeros(2, dtype=np.int64)
                out = []
                for eh in (None, envh):
                    r = lib.mnk_debug_envh_ksteps(ntile, chunk, band, js2, taper0, env.ctypes.data, None if eh is None else eh.ctypes.data, cnt.ctypes.data)
                    out += [r, int(cnt[0]), int(cnt[1])]
                print(sha(np.int64(out)), "envh_ksteps", base, f"env={name}")
            for fill in (0, 1):
                for ninst, period in ((1, 0), (2, 0), (2, nsc), (5, 0), (5, nsc)):
                    cfg = f"{base} fill={fill} instances={ninst} period={period}"
                    n = lib.mnk_debug_dag_merged_tasks(ntile, chunk, band, js2, taper0, fill, ninst, period, tasks.ctypes.data, CAP)
                    assert 0 <= n <= CAP
                    print(sha(tasks[:4 * n], np.int64([n])), "merged", cfg, f"n={n}")
                    for nq, gang in itertools.product((1, 8), (-1, 1, 4)):
                        off = np.zeros(2 * (nq + 1), dtype=np.int32)
                        n = lib.mnk_debug_dag_deal(ntile, chunk, band, js2, taper0, fill, ninst, period, nq, gang, tasks.ctypes.data,
                                                   order.ctypes.data, CAP, off.ctypes.data, C.byref(n1))
                        assert 0 <= n <= CAP
                        m = n
                        print(sha(tasks[:4 * m], order[:m], off, np.int64([n, n1.value])), "deal", cfg, f"nq={nq} gang={gang} n={n}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

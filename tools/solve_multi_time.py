"""Event-timed solve_linear_system! with several right-hand sides: the blocked path (solve_path 5, option multi_rhs_min) of THIS
tree's library against the column loop of a second build of the library (the parent commit's), both loaded into one process.

usage: python tools/solve_multi_time.py --against PARENT_LIB [DEST]

Dense SPD systems (CHOLESKY) at N = 2048 and N = 11 192, device right-hand sides, nrhs in {2, 3, 4, 8, 16, 64}: HIP events
around SOLVES solves after WARM warm-up solves per round, ROUNDS rounds, the two libraries alternated inside every round (the
first one changing from round to round); raw mnk_* calls on both.  Also the host-data case at nrhs = 64 (host clock), and the
bytes per second of the blocked sweeps: 8 Np^2 bytes of factor per chunk of 64 columns and solve (both sweeps read the lower
triangle once).  The suggested default of multi_rhs_min: the smallest nrhs >= 4 from which on the blocked path's slowest round
is faster than the column loop's fastest round at both orders (0: none up to 64).  Writes DEST (default
profiles/solve_multi_ab.json)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402

ORDERS, NRHS = (2048, 11192), (2, 3, 4, 8, 16, 64)
SOLVES, WARM, ROUNDS, HOST_SOLVES = 50, 5, 5, 10
USED = ("mnk_ctx_create", "mnk_ctx_destroy", "mnk_ls_create", "mnk_ls_destroy", "mnk_ls_set_option", "mnk_ls_factorize_dense",
        "mnk_ls_solve", "mnk_ls_check_solve", "mnk_ls_get_stat", "mnk_last_error_string")


def bind(lib):
    for name in USED:
        f = getattr(lib, name)
        f.restype, f.argtypes = L.SIGNATURES[name]
    return lib


class Raw:
    """A context and a CHOLESKY solver of one library on torch stream `st`, factorized on the device matrix A."""

    def __init__(self, lib, st, A, multi_rhs_min):
        self.lib, self.ctx, self.ls = lib, C.c_void_p(), C.c_void_p()
        self.ok(lib.mnk_ctx_create(0, st.cuda_stream, C.byref(self.ctx)))
        self.ok(lib.mnk_ls_create(self.ctx, A.shape[0], L.MNK_CHOLESKY, C.byref(self.ls)))
        if multi_rhs_min is not None:
            self.ok(lib.mnk_ls_set_option(self.ls, b"multi_rhs_min", float(multi_rhs_min)))
        info = C.c_int(0)
        self.ok(lib.mnk_ls_factorize_dense(self.ls, A.data_ptr(), A.shape[0], L.MNK_DEVICE, C.byref(info)))
        assert info.value == 0

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.lib.mnk_last_error_string().decode())

    def solve(self, ptr, nrhs, ldx, loc):
        self.ok(self.lib.mnk_ls_solve(self.ls, ptr, nrhs, ldx, loc))

    def stat(self, key):
        v = C.c_double(-1.0)
        return v.value if self.lib.mnk_ls_get_stat(self.ls, key, C.byref(v)) else v.value

    def close(self):
        self.lib.mnk_ls_destroy(self.ls)
        self.lib.mnk_ctx_destroy(self.ctx)


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main(parent_path, dest):
    st = torch.cuda.Stream()
    libs = {"parent": bind(C.CDLL(os.path.abspath(parent_path))), "tree": mj.lib()}
    res = {"method": f"HIP events around {SOLVES} solves after {WARM} warm-up solves per round, {ROUNDS} rounds, the two libraries "
                     "alternated inside every round (the first one changing from round to round), one process, raw mnk_ls_solve "
                     "calls on device right-hand sides; milliseconds per solve of nrhs columns, median [min - max] over the rounds; "
                     "parent = the column loop of the parent commit's build, tree = this tree with multi_rhs_min = 2 (solve_path 5); "
                     f"host64: nrhs = 64 on pageable host memory, host clock around {HOST_SOLVES} solves",
           "orders": {}}
    with torch.cuda.stream(st):
        for N in ORDERS:
            g = torch.Generator(device="cuda").manual_seed(N)
            R = torch.randn(N, 96, dtype=torch.float64, device="cuda", generator=g)
            A = R @ R.T + torch.diag(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) * 10 + 1.0)
            B = torch.randn(max(NRHS), N, dtype=torch.float64, device="cuda", generator=g)   # (row r = column r of the right-hand sides)
            st.synchronize()
            S = {"parent": Raw(libs["parent"], st, A, None), "tree": Raw(libs["tree"], st, A, 2)}
            Np = (N + 63) // 64 * 64
            cells = {}
            for nrhs in NRHS:
                X = B[:nrhs].clone()
                t = {w: [] for w in S}
                for rnd in range(ROUNDS):
                    for w in (("parent", "tree") if rnd % 2 == 0 else ("tree", "parent")):
                        for _ in range(WARM):
                            S[w].solve(X.data_ptr(), nrhs, N, L.MNK_DEVICE)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        for _ in range(SOLVES):   # (in place, solve after solve: the values do not matter to the time; A is well conditioned)
                            S[w].solve(X.data_ptr(), nrhs, N, L.MNK_DEVICE)
                        e1.record(st)
                        st.synchronize()
                        S[w].ok(S[w].lib.mnk_ls_check_solve(S[w].ls))
                        t[w].append(e0.elapsed_time(e1) / SOLVES)
                        X.copy_(B[:nrhs])
                assert S["tree"].stat(b"solve_path") == 5.0, S["tree"].stat(b"solve_path")
                cell = {w: summary(v) for w, v in t.items()}
                cell["tree_faster_beyond_spread"] = cell["tree"]["max"] < cell["parent"]["min"]
                chunks = -(-nrhs // 64)
                cell["tree_factor_GBps"] = 8.0 * Np * Np * chunks / (cell["tree"]["median"] * 1e-3) / 1e9
                cells[str(nrhs)] = cell
                print(f"N={N} nrhs={nrhs}: " + "  ".join(f"{w} {c['median']:.4f} [{c['min']:.4f} - {c['max']:.4f}] ms"
                                                        for w, c in cell.items() if isinstance(c, dict))
                      + f"  blocked sweeps {cell['tree_factor_GBps']:.0f} GB/s", flush=True)
            # the blocked solve agrees with the column loop to rounding
            X0, X1 = B[:64].clone(), B[:64].clone()
            S["parent"].solve(X0.data_ptr(), 64, N, L.MNK_DEVICE)
            S["tree"].solve(X1.data_ptr(), 64, N, L.MNK_DEVICE)
            st.synchronize()
            rel = ((X0 - X1).abs().max() / X0.abs().max()).item()
            Xh = {w: np.asfortranarray(B[:64].T.cpu().numpy()) for w in S}
            th = {w: [] for w in S}
            for rnd in range(ROUNDS):
                for w in (("parent", "tree") if rnd % 2 == 0 else ("tree", "parent")):
                    S[w].solve(Xh[w].ctypes.data, 64, N, L.MNK_HOST)
                    t0 = time.perf_counter()
                    for _ in range(HOST_SOLVES):
                        S[w].solve(Xh[w].ctypes.data, 64, N, L.MNK_HOST)
                    th[w].append((time.perf_counter() - t0) / HOST_SOLVES * 1e3)
            res["orders"][str(N)] = {"device": cells, "host64": {w: summary(v) for w, v in th.items()},
                                     "blocked_vs_column_loop_max_rel_diff": rel}
            print(f"N={N} host nrhs=64: " + "  ".join(f"{w} {summary(v)['median']:.3f} ms" for w, v in th.items()) + f"  rel diff {rel:.1e}",
                  flush=True)
            for s in S.values():
                s.close()
    ok = {n: all(res["orders"][str(N)]["device"][str(m)]["tree_faster_beyond_spread"] for N in ORDERS for m in NRHS if m >= n)
          for n in NRHS if n >= 4}
    res["suggested_multi_rhs_min"] = min([n for n, v in ok.items() if v], default=0)
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    json.dump(res, open(dest, "w"), indent=1)
    print("suggested multi_rhs_min:", res["suggested_multi_rhs_min"], " written", dest)


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "--against":
        sys.exit(__doc__)
    main(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "solve_multi_ab.json"))

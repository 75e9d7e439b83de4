"""Microseconds per `mnk_dc_compress_jacobian`, `mnk_dc_compress_hessian` and `mnk_dc_coo_jtprod` (csrc/dense_coo.hip,
DESIGN.md section 20) beside the device-to-device `mnk_dc_set_jac` / `mnk_dc_set_hess` loads of the same matrices -- the other way
to load the dense handle on the device -- and beside the dense transposed product `mnk_ipm_gemv`.  Models: the tape AC-OPF at
case30 and a banded tape model with n = 2048, m = 512.  The method is tools/tape_eval_time.py's: HIP events around CALLS calls
after WARM warm-up calls, the alternatives alternated inside every round of one process (the first one changing from round to
round), median [min - max] over the rounds.  Within a series of calls only the first compress after a dense load clears the
buffer (a warm-up call); the measured ones never do.  Writes profiles/coo_dense_callbacks.json, or the file given as the first
argument."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402
from madnlp_jl_amd import tape_model as T  # noqa: E402
from madnlp_jl_amd.device_callbacks import _up  # noqa: E402
from madnlp_jl_amd.ipm_device import IPMDeviceKernels  # noqa: E402
from madnlp_jl_amd.ipm import hess_mirror_coo, scatter_hess_coo, scatter_jac_coo  # noqa: E402

ROUNDS, WARM, CALLS = 8, 10, 100


def banded_model(n=2048, m=512):
    """Constraint r couples five neighbours of variable 4 r; the objective couples every variable with its successor."""
    M = T.TapeModel(n, m, np.ones(n), 0.0, 2.0, -np.inf, 1.0, name=f"banded_{n}_{m}")
    i = np.arange(n - 1)
    M.add_objective((T.V(0) - T.V(1)) * (T.V(0) - T.V(1)) + T.V(0) * T.V(0) * T.V(1), np.stack([i, i + 1], axis=1))
    r = np.arange(m)
    M.add_constraint(T.V(0) * T.V(1) + T.V(2) * T.V(3) - T.V(4) * T.V(4), r, (4 * r[:, None] + np.arange(5)[None, :]) % n)
    return M.finalize()


def measure(st, ctx, M):
    m, n = M.m, M.n
    e = np.zeros(0, dtype=np.int64)
    k = mj.DenseCondensedKKTSystem(n, m, np.arange(m, dtype=np.int64), e, e, e, ctx=ctx)
    k.attach_coo(M.jac_I, M.jac_J, M.hess_I, M.hess_J)
    K = IPMDeviceKernels(n, np.arange(1), np.arange(1), ctx=ctx)
    rng = np.random.default_rng(5)
    x, y = rng.uniform(0.5, 1.5, n), rng.standard_normal(m)
    jv, hv = M.jac_coord(x), M.hess_coord(x, y, 1.0)
    J, H = np.zeros((m, n), order="F"), np.zeros((n, n), order="F")
    I64 = [np.asarray(a, dtype=np.int64) for a in (M.jac_I, M.jac_J, M.hess_I, M.hess_J)]
    scatter_jac_coo(J, I64[0], I64[1], jv)
    scatter_hess_coo(H, hess_mirror_coo(I64[2], I64[3]), hv)
    jd, hd, yd, Jd, Hd = _up(jv, "cuda"), _up(hv, "cuda"), _up(y, "cuda"), _up(J.T, "cuda"), _up(H.T, "cuda")   # (row-major of the transpose: column-major)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = L.lib()
    calls = {
        "jacobian": {"coo": lambda: k.compress_jacobian(jd),
                     "dense": lambda: L.check(lib.mnk_dc_set_jac(k._h, Jd.data_ptr(), m, L.MNK_DEVICE), "mnk_dc_set_jac")},
        "hessian": {"coo": lambda: k.compress_hessian(hd),
                    "dense": lambda: L.check(lib.mnk_dc_set_hess(k._h, Hd.data_ptr(), n, L.MNK_DEVICE), "mnk_dc_set_hess")},
        "jtprod": {"coo": lambda: k.jtprod_coo_device(L.MNK_DC_JAC_CURRENT, yd, out),
                   "dense": lambda: K.gemv(1, m, n, 1.0, Jd, m, yd, 0.0, out)},
    }
    # the two ways load the same matrices
    calls["jacobian"]["coo"](), calls["hessian"]["coo"]()
    same = bool(np.array_equal(k.get_jac(), J) and np.array_equal(k.get_hess(), H))
    times = {name: {w: [] for w in alt} for name, alt in calls.items()}
    with torch.cuda.stream(st):
        for rnd in range(ROUNDS):
            for name, alt in calls.items():
                for w, fn in list(alt.items())[::-1 if rnd % 2 else 1]:
                    for _ in range(WARM):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(CALLS):
                        fn()
                    e1.record(st)
                    e1.synchronize()
                    times[name][w].append(e0.elapsed_time(e1) * 1000.0 / CALLS)      # ms / CALLS calls -> us per call
    ctx.synchronize()
    K.close()
    k.close()
    res = {name: {w: dict(median=statistics.median(v), min=min(v), max=max(v)) for w, v in d.items()} for name, d in times.items()}
    return dict(model=M.name, n=n, m=m, nnzj=len(M.jac_I), nnzh=len(M.hess_I), scatter_equals_host_scatter=same, us_per_call=res)


def main(dest):
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    st = torch.cuda.Stream()
    ctx = mj.HipContext(0, stream=st.cuda_stream)
    out = {"method": f"HIP events around {CALLS} calls after {WARM} warm-up calls, per round; {ROUNDS} rounds, the COO entry and the dense "
           "device-to-device load (jtprod: mnk_ipm_gemv on the dense Jacobian) alternated inside every round, one process; "
           "microseconds per call, median / min / max over the rounds", "models": []}
    for M in (T.acopf_tape_model("case30"), banded_model()):
        out["models"].append(measure(st, ctx, M))
        print(json.dumps(out["models"][-1], indent=1), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    json.dump(out, open(dest, "w"), indent=1)
    print("written", dest)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "coo_dense_callbacks.json"))

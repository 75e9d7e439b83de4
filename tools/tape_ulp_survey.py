"""The two measured constants of the per-entry bound of the tape evaluator (tests/tape_reference.py);
writes profiles/tape_accuracy.json (or the file given with --out).

  functions   each library function alone in a one-instruction tape at 4096 arguments spread over the ranges the tests use, on
              the numpy interpreter and, with --device, on the GPU: the largest error against mpmath (60 digits) per function
              and side, in units of 2^-52 |value| (the bound's unit: an ulp or twice an ulp of the value).
              c_fun = twice the largest of them, rounded up (4096 points do not find the worst case); above 16 the script
              stops with an error: that is a finding, not a bound to widen.
  constants   the compiled tapes of 1000 generated patterns run in mpmath against the trees' own values and derivatives: the only
              float64 in that comparison are the constants the compiler folded.  The largest |tape - reference| in units of the
              first-order propagation of 2^-53 |c| per non-integer pool constant; c_const = twice that, rounded up.  Host only.

Every step runs in a child process under a time limit; the script reads no files."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madnlp_jl_amd import tape_model as T  # noqa: E402
from madnlp_jl_amd.tape_model import V  # noqa: E402

NPTS = 4096
STEP_LIMIT = {"host": 300, "device": 120, "const": 900}
C_FUN_MAX = 16


def _loguniform(rng, lo, hi, n, signed=False):
    v = 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), n)
    return v * rng.choice((-1.0, 1.0), n) if signed else v


def arguments():
    """name -> (expression, a, b or None): 4096 arguments per function over the ranges of the reference tests (sample points and
    what expressions make of them) and of the edge-argument rows"""
    rng = np.random.default_rng(52)
    h, qt = NPTS // 2, NPTS // 4
    trig = np.concatenate([rng.uniform(-20, 20, h), _loguniform(rng, 1e-300, 1, qt, True), _loguniform(rng, 1, 1e300, qt, True)])
    out = {"sin": (T.sin(V(0)), trig, None), "cos": (T.cos(V(0)), trig, None), "tan": (T.tan(V(0)), trig, None)}
    out["exp"] = (T.exp(V(0)), np.concatenate([rng.uniform(-20, 20, h + qt), rng.uniform(-708, 709.78, qt)]), None)
    out["log"] = (T.log(V(0)), np.concatenate([rng.uniform(0.05, 50, h), _loguniform(rng, 1e-300, 1e300, qt), 1 + rng.uniform(-1e-3, 1e-3, qt)]), None)
    out["sqrt"] = (T.sqrt(V(0)), np.concatenate([rng.uniform(0.05, 50, h), _loguniform(rng, 1e-300, 1e300, h)]), None)
    out["atan"] = (T.atan(V(0)), np.concatenate([rng.uniform(-20, 20, h), _loguniform(rng, 1e-300, 1e300, h, True)]), None)
    out["tanh"] = (T.tanh(V(0)), np.concatenate([rng.uniform(-20, 20, h), _loguniform(rng, 1e-300, 1, h, True)]), None)
    base = np.concatenate([rng.uniform(0.05, 50, h), _loguniform(rng, 1e-150, 1e150, h)])
    out["pow 1.7"] = (V(0) ** 1.7, base, None)
    out["pow -0.3"] = (V(0) ** -0.3, base, None)
    a = np.concatenate([rng.uniform(0.05, 50, h), _loguniform(rng, 1e-3, 1e3, h)])
    reach = np.concatenate([np.full(h, 20.0), np.full(h, 700.0)]) / np.maximum(np.abs(np.log(a)), 1e-3)
    out["pow"] = (T.pow_(V(0), V(1)), a, rng.uniform(-1, 1, NPTS) * np.minimum(reach, 50.0))
    return out


def model(args):
    """one constraint pattern per function, pattern i on rows i * NPTS ...; x = all first arguments, then all second ones"""
    M = T.TapeModel(2 * NPTS * len(args), NPTS * len(args), np.ones(2 * NPTS * len(args)), -np.inf, np.inf, -np.inf, np.inf)
    x = np.zeros(M.n)
    for i, (name, (expr, a, b)) in enumerate(args.items()):
        va, vb = 2 * NPTS * i + np.arange(NPTS), 2 * NPTS * i + NPTS + np.arange(NPTS)
        x[va] = a
        x[vb] = 0.0 if b is None else b
        M.add_constraint(expr, i * NPTS + np.arange(NPTS), np.stack([va, vb], axis=1))
    M.finalize()
    assert all(len(p.tapes[0].code) == 1 for p in M.patterns), "one instruction per function"
    return M, x


def exact(name, a, b):
    from mpmath import mp, mpf
    a = mpf(float(a))
    if name.startswith("pow"):
        e = mpf(float(b)) if name == "pow" else mpf(float(name.split()[1]))
        return mp.exp(e * mp.log(a))
    return mp.sin(a) / mp.cos(a) if name == "tan" else getattr(mp, name)(a)


def function_errors(values, args):
    """largest |value - exact| / (2^-52 |exact|) per function, and where"""
    from mpmath import mp, mpf
    mp.dps = 60
    table = {}
    for i, (name, (_, a, b)) in enumerate(args.items()):
        worst, at = 0.0, None
        for r in range(NPTS):
            ref = exact(name, a[r], None if b is None else b[r])
            if not 2.0 ** -1021 < abs(ref) < 2.0 ** 1023:
                continue
            err = float(abs(mpf(float(values[i * NPTS + r])) - ref) / (mpf(2) ** -52 * abs(ref)))
            if not err <= worst:                       # (a NaN counts)
                worst, at = err, [float(a[r])] + ([] if b is None else [float(b[r])])
        table[name] = {"max_error": worst, "at": at}
    return table


def step_host():
    args = arguments()
    M, x = model(args)
    return function_errors(M.cons(x), args)


def step_device():
    import torch
    import madnlp_jl_amd as mj
    from madnlp_jl_amd.device_callbacks import DeviceTapeCallbacks, _up
    from madnlp_jl_amd.ipm_device import IPMDeviceKernels
    args = arguments()
    M, x = model(args)
    ctx = mj.HipContext(0)
    K = IPMDeviceKernels(M.n, np.arange(1), np.arange(1), ctx=ctx)
    cb = DeviceTapeCallbacks(M, None, "cuda", K)
    xd = _up(x, "cuda")
    c = torch.full((M.m,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cb.cons(c, xd)
    ctx.synchronize()
    values = c.cpu().numpy()
    cb.close()
    K.close()
    ctx.close()
    return function_errors(values, args)


def step_const(npatterns):
    from mpmath import mpf
    from tests import tape_reference as R
    worst, at, done, seed = 0.0, None, 0, 1000
    while done < npatterns:
        pats, _ = R.kept_patterns(seed, count=min(25, npatterns - done), k=3, q=2, depth=4, rows=2)
        seed += 1
        done += len(pats)
        for pat in pats:
            pairs = [[[0] * pat.k], [R.orders_of(pat.k, j) for j in pat.tapes[1].out_j.tolist()],
                     [R.orders_of(pat.k, j, l) for j, l in zip(pat.tapes[2].out_j.tolist(), pat.tapes[2].out_l.tolist())]]
            for x, p in pat.points:
                for tape, orders in zip(pat.tapes, pairs):
                    for (v, _, e_const, _), o in zip(R.run_tape(tape, x, p), orders):
                        diff = abs(v - R.derivative(pat.tree, x, p, o))
                        if e_const > 0 and diff > max(abs(v), 1) * mpf(10) ** -40:       # (below: mpmath.diff's own noise)
                            ratio = float(diff / (e_const / R.C_CONST))
                            if ratio > worst:
                                worst, at = ratio, repr(pat.tree)
    return {"patterns": done, "max_ratio": worst, "at": at}


def run_step(name, extra=()):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, *extra], capture_output=True, text=True,
                       timeout=STEP_LIMIT[name], cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true", help="measure the GPU interpreter too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tape_accuracy.json"))
    ap.add_argument("--const-patterns", type=int, default=1000)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        res = step_host() if a.step == "host" else step_device() if a.step == "device" else step_const(a.const_patterns)
        print(json.dumps(res))
        return
    out = {"unit": "2^-52 |exact value| (functions), first-order propagation of 2^-53 |c| per folded constant (constants)",
           "points_per_function": NPTS, "functions": {"host": run_step("host")}}
    if a.device:
        out["functions"]["device"] = run_step("device")
    largest = max(e["max_error"] for side in out["functions"].values() for e in side.values())
    out["largest_function_error"] = largest
    out["c_fun"] = math.ceil(2 * largest)
    out["constants"] = run_step("const", ["--const-patterns", str(a.const_patterns)])
    out["c_const"] = math.ceil(2 * out["constants"]["max_ratio"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("largest_function_error", "c_fun", "c_const")}))
    if not out["c_fun"] <= C_FUN_MAX:
        raise SystemExit(f"c_fun = {out['c_fun']} exceeds {C_FUN_MAX}: a finding about the library, not a bound to widen")


if __name__ == "__main__":
    main()

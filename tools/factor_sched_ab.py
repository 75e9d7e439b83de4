"""A/B of two builds of the library on the launch-per-panel factorization schedules (panel_algo 1 and 4; csrc/factor_plan.hip,
the executor in csrc/factor.hip): one sha256 of the factor's bits (tril(L) and D) per configuration.  These schedules are
deterministic (tests/test_hip_parity.py::test_repeated_factorizations_are_deterministic), so a change of the host driver that
keeps the launches must keep every hash.  Run it once as it is (this tree's library) and once with MNK_LIBPATH=<libmadnlp_hip.so
built from the parent commit, same ABI> -- or from a checkout of the parent, if this tree binds entries the parent's library
lacks -- and compare the listings (record: profiles/factor_plan_ab.txt).
usage: [MNK_LIBPATH=...] python tools/factor_sched_ab.py [--quick]"""
import hashlib
import itertools
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj  # noqa: E402

quick = "--quick" in sys.argv[1:]
s = torch.cuda.Stream()


def matrix(N, alg):
    g = torch.Generator(device="cuda").manual_seed(N)
    R = torch.randn(N, 96, dtype=torch.float64, device="cuda", generator=g)
    A = R @ R.T + torch.diag(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) * 10 + 1.0)
    if alg == "LDL":
        n1 = 2 * N // 3
        A[n1:, n1:].neg_()
    s.synchronize()
    return A


def factor_sha(ctx, A, what, alg, options, **opt):
    ls = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg, **opt))
    for key, val in options:
        ls.set_option(key, val)
    ls.factorize()
    inertia = ls.inertia()
    Lf, D = ls.get_factor_device()
    s.synchronize()
    h = hashlib.sha256(torch.tril(Lf).contiguous().cpu().numpy().tobytes() + D.cpu().numpy().tobytes()).hexdigest()[:16]
    print(f"{what:74s} algo {ls.get_stat('panel_algo'):.0f} fallbacks {ls.get_stat('pp_fallbacks'):.0f} inertia {inertia} factor sha {h}", flush=True)
    ls.close()


with torch.cuda.stream(s):
    ctx = mj.HipContext(0, stream=s.cuda_stream)
    for N in (1100,) if quick else (1100, 4672):
        for alg in ("CHOLESKY", "LDL"):
            A = matrix(N, alg)
            for algo, la, nbo, share, fuse in itertools.product((1, 4), (0, 1), (192, 256, 512), (0, 2), (0, 4096)):
                factor_sha(ctx, A, f"N={N} {alg} panel_algo={algo} lookahead={la} outer_block={nbo} share={share} pp_fuse_rows={fuse}", alg,
                           [("pp_fuse_rows", fuse)], panel_algo=algo, lookahead=bool(la), outer_block=nbo, share=share, single_rows=0)
    for N in (1024, 2048) if quick else (1024, 2048, 11192):
        for alg in ("CHOLESKY", "LDL"):
            factor_sha(ctx, matrix(N, alg), f"N={N} {alg} defaults", alg, [])
    ctx.close()

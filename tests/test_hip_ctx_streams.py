"""Every CU-masked stream pair of a process in ONE process and on ONE context (csrc/ctx.hip owns them per device; which CUs each
stream gets: csrc/stream_plan.hip): the task-DAG pair made with the context, the deep-band pair, the look-ahead pair of the
launch-per-panel schedules, the second chain partition of a large batch and the chains' partition of a round of small systems.
Each is made by the first factorization that needs it, destroyed by `release_idle_streams` and by the device's last context, and
made again on demand -- in another order, too -- and none of that may change a bit of a factor or the schedule that produced it:

  (a) deep band: N = 1280 (the smallest order of the task-DAG schedule), every row in the chain's band (`dag_js2` 0);
  (b) band + bulk kernel: N = 5504, the smallest multiple of 128 above `dag_deep_rows` (`dag_js2` = ceil(Np / 256); the bulk grid
      beside the 16-CU chain of a 256-CU device is 672 workgroups);
  (c) look-ahead: panel_algo 4 at the smallest order for which the planner (`mnk_debug_factor_plan`) lists a look-ahead plan;
  (d) large batch: `factorize_batch` of two solvers of N = 5504;
  (e) small batch: `factorize_batch` of four solvers of N = 512.

The members of a batch are the solvers of dense-condensed KKT systems: only a device-resident matrix can be queued
(`factorize_async`; a factorize! that returns `info` launches what is queued at once)."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from madnlp_jl_amd import _lib as L  # noqa: E402

N_DEEP, N_BULK, N_SMALL = 1280, 5504, 512
STATS = ("panel_algo", "dag_js2", "dag_bulk_wgs")


def _lookahead_order(num_cu):
    """The smallest order (a multiple of 128) whose schedule-4 plan uses the look-ahead streams on a device of `num_cu` CUs, with
    the solver's defaults: one outer panel up to single_rows = 2560 rows, 512 columns beyond; pp_fuse_rows 4096, share 1,
    small_tiles 400; the panel stream on a quarter of the CUs."""
    shape = (C.c_int * 2)(-1, -1)
    for Np in range(128, 16384, 128):
        width = Np if Np <= 2560 else 512
        n = L.lib().mnk_debug_factor_plan(Np, 0, 4, 1, width, 4096, 1, 400, num_cu, max(4, num_cu // 4), None, 0, shape)
        assert n > 0
        if shape[1] == 1:
            return Np
    raise AssertionError("no look-ahead plan below 16384 rows")


def _spd(n, dev, gen):
    G = torch.randn((n, n), dtype=torch.float64, device=dev, generator=gen)
    return (G @ G.T / n + 2.0 * torch.eye(n, dtype=torch.float64, device=dev)).contiguous()


def _kkt(ctx, n, seed, opt):
    """A dense-condensed KKT system of order n whose condensed matrix is SPD: the shape of problems.dense_dummy_qp (no equality
    constraints), with a Hessian of rank 16 + 100 I so that the generator stays cheap at n = 5504."""
    rng = np.random.default_rng(seed)
    m = 8
    k = mj.DenseCondensedKKTSystem(n, m, np.arange(m), np.arange(0), np.arange(n + m), np.arange(n + m), ctx=ctx, opt_linear_solver=opt)
    R = rng.standard_normal((n, 16))
    k.hess[...] = R @ R.T
    k.hess[np.diag_indices(n)] += 100.0
    i = np.arange(m)
    k.jac[i, i] = 1.0
    k.jac[i, i + 1] = -1.0
    k.l_diag[:] = -(10.0 ** rng.uniform(-4, 0, n + m))
    k.u_diag[:] = -(10.0 ** rng.uniform(-4, 0, n + m))
    k.l_lower[:] = 10.0 ** rng.uniform(-6, 1, n + m)
    k.u_lower[:] = 10.0 ** rng.uniform(-6, 1, n + m)
    k.set_aug_diagonal()
    k.build_kkt()
    return k


def _result(M):
    assert M.inertia() == (M.n, 0, 0)
    assert M.get_stat("pp_fallbacks") == 0.0
    # The library copies the factor on the context's own stream, which torch's stream is not ordered with: a block that torch's
    # allocator hands out again (the tril / clone temporaries of the previous member) must be at rest before the copy lands in it.
    torch.cuda.synchronize()
    Lf, D = M.get_factor_device()
    out = torch.tril(Lf).clone(), D.clone(), tuple(M.get_stat(s) for s in STATS)
    torch.cuda.synchronize()
    return out


def _same(got, ref, what):
    assert torch.equal(got[1], ref[1]), (what, "D", float((got[1] - ref[1]).abs().max()))
    assert torch.equal(got[0], ref[0]), (what, "L", float((got[0] - ref[0]).abs().max()), int((got[0] != ref[0]).sum()))
    assert got[2] == ref[2], (what, got[2], ref[2])


def test_every_stream_pair_is_made_released_and_made_again_with_the_same_bits():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda", 0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_la = _lookahead_order(num_cu)
    gen = torch.Generator(device=dev).manual_seed(5504)
    chol = mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY, panel_algo=5)
    mats = {"a": _spd(N_DEEP, dev, gen), "b": _spd(N_BULK, dev, gen), "c": _spd(n_la, dev, gen)}
    torch.cuda.synchronize()                              # (the solvers read them on the context's stream)

    def solvers_on(ctx, cases):
        return {c: [mj.HipLinearSolver(mats[c], ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.CHOLESKY, panel_algo=4) if c == "c" else chol)]
                for c in cases}

    def run(S, case):
        if case in ("d", "e"):
            with mj.factorize_batch():
                for M in S[case]:
                    M.factorize_async()
        else:
            S[case][0].factorize()
        return [_result(M) for M in S[case]]

    ctx = mj.HipContext(0)
    S = solvers_on(ctx, "abc")
    kkts = [_kkt(ctx, N_BULK, 55040 + i, chol) for i in range(2)] + [_kkt(ctx, N_SMALL, 5120 + i, chol) for i in range(4)]
    S["d"] = [k.linear_solver for k in kkts[:2]]
    S["e"] = [k.linear_solver for k in kkts[2:]]
    ref = {case: run(S, case) for case in "abcde"}
    nsc = math.ceil(N_BULK / 256)                         # (N_BULK is a multiple of 128: Np = N)
    assert ref["a"][0][2][:2] == (5.0, 0.0)               # deep band: dag_js2 == 0
    assert ref["b"][0][2][:2] == (5.0, float(nsc))        # band + bulk kernel
    if num_cu == 256:
        assert ref["b"][0][2][2] == 672.0
    assert ref["c"][0][2][0] == 4.0
    assert all(r[2][:2] == (5.0, float(nsc)) for r in ref["d"])
    assert all(r[2][:2] == (5.0, 0.0) for r in ref["e"])

    mj.release_idle_streams(0)
    for case in "ecadb":
        for i, got in enumerate(run(S, case)):
            _same(got, ref[case][i], ("after release", case, i))

    for k in kkts:
        k.close()
    for case in "abc":
        S[case][0].close()
    ctx.close()                                           # (the device's last context of this test: its pairs go with it)
    ctx = mj.HipContext(0)
    S = solvers_on(ctx, "ab")
    for case in "ab":
        _same(run(S, case)[0], ref[case][0], ("fresh context", case))
    for lst in S.values():
        for M in lst:
            M.close()
    ctx.close()

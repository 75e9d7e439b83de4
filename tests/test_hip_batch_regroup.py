"""The merged task queue of a factorization batch is kept per device from batch to batch and merged again when the next batch
is another group (csrc/dag_batch.hip: BatchBuffers::hold_merged).  Here one context re-enters it with different groups of ONE
order: dense SPD matrices of order 1536 (12 tiles; `factorize_dense`), LDL' and Cholesky, four solvers each.

  * large-batch mode, forced with dag_deep_rows = 1024 (`dag_js2` reads nsc = 6: band + bulk kernel, two alternating chains, the
    instances' lists merged with a shift): a batch of 4, a batch of 2 (other members, another instance count: merged again), a
    batch of 4 (merged again);
  * then the default dag_deep_rows (`dag_js2` = 0: every row in the chain's band, the chains side by side, the band
    accumulation of all systems in one merged queue without a shift): a batch of 3 of the same solvers.

After every batch, for every member: the task-DAG schedule ran (panel_algo 5), no fall-back, inertia (N, 0, 0), and the factor is
bit-equal to the lone factorization of the same matrix on the same solver in the same mode (the arithmetic per instance is that
of a single factorization: same task list, same order per tile)."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402

N = 1536
NSC = N // 256


def _check(M, ref, what):
    assert M.get_stat("panel_algo") == 5.0 and M.get_stat("pp_fallbacks") == 0.0, what
    assert M.inertia() == (N, 0, 0), what
    Lf, D = M.get_factor_device()
    assert torch.equal(torch.tril(Lf), ref[0]) and torch.equal(D, ref[1]), what


def _lone(M):
    M.factorize()
    assert M.inertia() == (N, 0, 0)
    Lf, D = M.get_factor_device()
    return torch.tril(Lf).clone(), D.clone()


@pytest.mark.parametrize("alg", [mj.LDL, mj.CHOLESKY])
def test_batches_of_other_groups_of_one_order(alg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda", 0)
    ctx = mj.HipContext(0)
    gen = torch.Generator(device=dev).manual_seed(1536)
    mats = []
    for _ in range(4):
        G = torch.randn((N, N), dtype=torch.float64, device=dev, generator=gen)
        mats.append((G @ G.T / N + 2.0 * torch.eye(N, dtype=torch.float64, device=dev)).contiguous())
    solvers = [mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg)) for A in mats]
    for M in solvers:
        M.set_option("dag_deep_rows", 1024)
    ref = [_lone(M) for M in solvers]
    assert all(M.get_stat("dag_js2") == NSC and M.get_stat("panel_algo") == 5.0 for M in solvers)
    for members in ((0, 1, 2, 3), (1, 3), (0, 1, 2, 3)):
        with mj.factorize_batch():
            for i in members:
                solvers[i].factorize()
        for i in members:
            _check(solvers[i], ref[i], ("large", members, i))
            assert solvers[i].get_stat("dag_js2") == NSC
    small = (0, 1, 2)
    for i in small:
        solvers[i].set_option("dag_deep_rows", 5376)
    ref_small = {i: _lone(solvers[i]) for i in small}
    assert all(solvers[i].get_stat("dag_js2") == 0 and solvers[i].get_stat("panel_algo") == 5.0 for i in small)
    with mj.factorize_batch():
        for i in small:
            solvers[i].factorize()
    for i in small:
        _check(solvers[i], ref_small[i], ("small", small, i))
        assert solvers[i].get_stat("dag_js2") == 0
    for M in solvers:
        M.close()
    ctx.close()

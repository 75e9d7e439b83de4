"""Ill-conditioned matrices of many orders through both factorizations and both schedules (round 2: a compiler problem
once made the persistent panel kernel return a non-positive pivot for ONE matrix of the whole suite -- N = 577,
condition 1e6 -- so the suite now carries a spread of such cases; `tools/stress_factor.py` is the long version)."""
import numpy as np
import pytest
import scipy.linalg as sla

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def _spd(rng, N, decades=6):
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    w = 10.0 ** rng.uniform(-decades / 2, decades / 2, N)
    A = (Q * w) @ Q.T
    return np.asfortranarray((A + A.T) / 2)


CASES = [(N, alg, la, fuse) for N in (129, 257, 577, 640, 900, 1500, 2100)
         for alg, la, fuse in ((mj.CHOLESKY, False, None), (mj.LDL, True, None), (mj.LDL, False, 0), (mj.CHOLESKY, True, 10 ** 6))]


@pytest.mark.parametrize("N,alg,lookahead_on_small,fuse", CASES)
def test_ill_conditioned_factorizations_match_lapack(ctx, N, alg, lookahead_on_small, fuse):
    _matches_lapack(ctx, N, alg, lookahead_on_small, fuse)


# From 1280 rows on the default schedule is the task-DAG one, which reads neither single_rows nor pp_fuse_rows: the look-ahead
# cases of those orders once more under the schedule they are meant for.
@pytest.mark.parametrize("N,alg,lookahead_on_small,fuse", [c for c in CASES if c[0] >= 1280 and c[2]])
def test_ill_conditioned_factorizations_match_lapack_persistent_panels(ctx, N, alg, lookahead_on_small, fuse):
    _matches_lapack(ctx, N, alg, lookahead_on_small, fuse, panel_algo=4)


def _matches_lapack(ctx, N, alg, lookahead_on_small, fuse, panel_algo=None):
    rng = np.random.default_rng(N)  # N = 577 reproduces the matrix of the round-2 incident
    A = _spd(rng, N)
    quasi = alg == mj.LDL and N % 2 == 0
    if quasi:  # quasi-definite saddle system: factorable without pivoting, inertia (n1, 0, N - n1)
        A[N // 2:, N // 2:] *= -1.0
    An = A.copy(order="F")
    An[np.triu_indices(N, 1)] = np.nan  # 'L' storage: the upper triangle must never be read
    M = mj.HipLinearSolver(An, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg, outer_block=256))
    if lookahead_on_small:
        M.set_option("single_rows", 0)  # the two-stream look-ahead schedule instead of one outer panel
    if fuse is not None:
        M.set_option("pp_fuse_rows", fuse)
    if panel_algo is not None:
        M.set_option("panel_algo", panel_algo)
    M.factorize()
    assert M.info == 0
    assert panel_algo is None or M.get_stat("panel_algo") == panel_algo
    assert M.inertia() == ((N // 2, 0, N - N // 2) if quasi else (N, 0, 0))
    b = rng.standard_normal(N)
    x = M.solve_linear_system(b.copy())
    xr = sla.solve(A, b, assume_a="sym")
    nrm = np.abs(A).max()
    res = np.abs(A @ x - b).max() / (nrm * np.abs(x).max() + np.abs(b).max())
    res_ref = np.abs(A @ xr - b).max() / (nrm * np.abs(xr).max() + np.abs(b).max())
    assert res <= 1e-12 and res <= 100 * res_ref + 1e-15, (res, res_ref)
    M.close()

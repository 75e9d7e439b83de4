"""The zero-fill of the spare factor buffer, pinned from outside (all through the C ABI).

Sparse sources are scattered into a zeroed dense buffer.  With `prefill` the zeros are written in the background into a second
buffer -- on a side stream, or (`dag_fill`, task-DAG schedule only) by DAG_FILL tasks of the factorization's own bulk queue -- and
the next transfer swaps the two.  Which buffer counts as zeroed is host bookkeeping; a mistake in it scatters a matrix over an
old factor.  The fill path does not change the arithmetic, so every comparison here is exact:

  * one solver factors SPD, SPD, a matrix that breaks Cholesky down late (LDL': one negative pivot), SPD, SPD -- same pattern,
    different values -- under prefill = 0 / prefill = 1 with the side-stream fill / prefill = 1 with DAG_FILL tasks.  After every
    successful step the factor is bit-equal across the three settings and to a fresh prefill = 0 solver that factors that matrix
    alone; the inertia is equal everywhere, the breakdown step included.  N = 1300 (11 tiles: task-DAG schedule with bulk
    tasks, the only place DAG_FILL exists) and N = 600 (schedule 4: the side stream is the only path).
  * BUNCHKAUFMAN, N = 720: two factorizations in a row take the pivoted tier (two transfers per factorize!), an SPD matrix
    follows; its factor is bit-equal to a fresh prefill = 0 solver's.
"""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import madnlp_jl_amd as mj  # noqa: E402
from tests.test_hip_round4 import _not_quasi_definite_sparse  # noqa: E402

SETTINGS = [{"prefill": 0}, {"prefill": 1, "dag_fill": 0}, {"prefill": 1, "dag_fill": 1}]
OFFSETS = (0, 1, 7, 40)      # the diagonals of the banded pattern
BREAKDOWN_STEP = 2


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def _banded_spd(rng, N):
    """Lower-triangular CSC of a strictly diagonally dominant (hence SPD) matrix with the diagonals OFFSETS."""
    rows, cols, vals = [], [], []
    for d in OFFSETS[1:]:
        j = np.arange(N - d)
        rows.append(j + d); cols.append(j); vals.append(rng.uniform(-1.0, 1.0, N - d))
    j = np.arange(N)
    rows.append(j); cols.append(j); vals.append(2.0 * (len(OFFSETS) - 1) + rng.uniform(0.5, 1.5, N))
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    A.sort_indices()
    return A


def _sequence(N):
    """The five matrices of one order (fixed seed; one pattern), and the row of the negated diagonal entry of the third."""
    rng = np.random.default_rng(1000 + N)
    mats = [_banded_spd(rng, N) for _ in range(5)]
    assert all(np.array_equal(A.indices, mats[0].indices) and np.array_equal(A.indptr, mats[0].indptr) for A in mats)
    r = N - N // 8                                 # in the last quarter
    A = mats[BREAKDOWN_STEP]
    k = A.indptr[r]
    assert A.indices[k] == r                       # first stored entry of a lower-triangular column is the diagonal
    A.data[k] = -A.data[k]
    return mats, r


def _triple(A):
    return (A.indptr.copy(), A.indices.copy(), A.data.copy())


def _solver(ctx, A, alg, settings):
    M = mj.HipLinearSolver(_triple(A), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg))
    for key, val in settings.items():
        M.set_option(key, val)
    return M


def _fresh(ctx, A, alg):
    """(info, inertia, factor or None) of a solver created for this matrix alone, prefill = 0."""
    M = _solver(ctx, A, alg, {"prefill": 0})
    M.factorize()
    out = (M.info, M.inertia(), M.get_factor() if M.info == 0 else None, M.get_stat("panel_algo"))
    M.close()
    return out


@pytest.mark.parametrize("alg", [mj.CHOLESKY, mj.LDL])
@pytest.mark.parametrize("N,schedule", [(1300, 5), (600, 4)])
def test_factor_bits_do_not_depend_on_the_fill_path(ctx, N, schedule, alg):
    mats, r = _sequence(N)
    solvers = [_solver(ctx, mats[0], alg, s) for s in SETTINGS]
    for step, A in enumerate(mats):
        info0, inertia0, factor0, algo0 = _fresh(ctx, A, alg)
        if step == BREAKDOWN_STEP and alg == mj.CHOLESKY:
            assert info0 != 0, "the negated diagonal entry should break Cholesky down"
        else:
            assert info0 == 0, (step, info0)
            assert inertia0 == ((N, 0, 0) if step != BREAKDOWN_STEP else (N - 1, 0, 1)), (step, inertia0)
            assert algo0 == schedule, (step, algo0)
        for M, s in zip(solvers, SETTINGS):
            M.A = _triple(A)
            M.factorize()
            assert M.info == info0, (step, s, M.info, info0)
            assert M.inertia() == inertia0, (step, s, M.inertia(), inertia0)
            if info0 == 0:
                assert M.get_stat("panel_algo") == schedule, (step, s)
                Lm, D = M.get_factor()
                assert np.array_equal(D, factor0[1]), (step, s)
                assert np.array_equal(Lm, factor0[0]), (step, s)
    if schedule == 5:   # the DAG_FILL path was really there: bulk tasks, and more of them with dag_fill
        assert solvers[2].get_stat("dag_ntasks") > solvers[1].get_stat("dag_ntasks") > 0
    for M in solvers:
        M.close()


@pytest.mark.parametrize("settings", SETTINGS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_pivoted_tier_twice_then_spd(ctx, settings):
    """Two transfers per factorize! (the pivoted tier fetches the matrix again), twice in a row, then an SPD matrix."""
    n1, n2 = 300, 420
    N = n1 + n2
    rng = np.random.default_rng(41)
    A = _not_quasi_definite_sparse(rng, n1, n2)
    A2 = A.copy()
    A2.data = A2.data * 1.01
    S = _banded_spd(rng, N)
    M = _solver(ctx, A, mj.BUNCHKAUFMAN, settings)
    tiers = []
    for B in (A, A2, S):
        M.A = _triple(B)
        M.factorize()
        info, inertia, factor, _ = _fresh(ctx, B, mj.BUNCHKAUFMAN)
        assert M.info == info
        assert M.inertia() == inertia
        tiers.append(bool(M.bk_info()[0]))
    assert tiers == [True, True, False], tiers
    assert info == 0 and inertia == (N, 0, 0)
    Lm, D = M.get_factor()
    assert np.array_equal(D, factor[1])
    assert np.array_equal(Lm, factor[0])
    M.close()

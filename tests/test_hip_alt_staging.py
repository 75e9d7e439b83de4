"""(-m gpu) The loop over right-hand sides that the QR, LU and EVD solvers share (csrc/ls_alt.hip: mnk_ls_alt_solve): a host
matrix of right-hand sides whose leading dimension is larger than N, and the agreement of the three routes a right-hand side
can take -- host matrix, host vector, strided device view.  All three run the same kernels on the same data, so their
solutions are equal bit for bit."""
import numpy as np
import pytest
import torch

import madnlp_jl_amd as mj
from tests.test_hip_lu import backward_error, sym_matrix

pytestmark = pytest.mark.gpu

PAD_ROWS = 24      # rows of the host matrix behind the N of the system
SENTINEL = 7.0     # what they hold, before and after


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("N", [5, 65, 200])   # below one 64-column block, one past a block, past one 128-row padding unit
@pytest.mark.parametrize("algo", [mj.QR, mj.LU, mj.EVD])
def test_host_matrix_host_vector_and_device_view_agree(ctx, algo, N):
    A = sym_matrix(N, "indefinite", 100 + N)
    B = np.random.default_rng(200 + N).standard_normal((N, 3))
    cls = mj.HipLUSolver if algo == mj.LU else mj.HipLinearSolver
    s = cls(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=algo))
    s.factorize()
    # (a) host matrix, leading dimension N + PAD_ROWS
    ld = N + PAD_ROWS
    full = np.full((ld, 3), SENTINEL, order="F")
    full[:N] = B
    s.solve_linear_system(full)
    Xa = full[:N].copy()
    for j in range(3):
        err = backward_error(A, Xa[:, j], B[:, j])
        print(f"algo {algo} N {N} column {j}: backward error {err:.3e}")
        assert err <= 1e-13
    assert np.all(full[N:] == SENTINEL)
    # (b) every column as a host vector of its own
    for j in range(3):
        x = s.solve_linear_system(B[:, j].copy())
        assert np.array_equal(x, Xa[:, j]), j
    # (c) strided device view (the layout of the three-column tests of the per-algorithm files)
    buf = torch.zeros((3, ld), dtype=torch.float64, device="cuda")
    buf[:, :N] = torch.from_numpy(B.T.copy())
    X = buf[:, :N].T          # (N, 3) view, stride(1) = ld
    assert X.stride(1) == ld
    s.solve_linear_system(X)
    s.check_solve()
    assert np.array_equal(X.cpu().numpy(), Xa)
    assert torch.all(buf[:, N:] == 0)     # nothing written between the columns
    s.close()

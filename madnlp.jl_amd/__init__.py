"""madnlp.jl_amd -- MI355X-native KKT hot path for MadNLP-style interior-point solvers.

Only what the path needs: `csrc/` (HIP kernels + the C ABI of include/madnlp_hip.h) and the
host-side mirror of the reference's KKT-system / linear-solver interfaces.  Importing the
package does not load the HIP library; the first use of a KKT system or solver does, and
fails loudly if it has not been built (no CPU fallback).
"""
from ._lib import build, lib, LIBPATH, HipError  # noqa: F401
from .linear_solver import (  # noqa: F401
    BUNCHKAUFMAN, CHOLESKY, LDL, QR, LU, EVD, HipContext, HipLinearSolver, HipLUSolver, HipSolverOptions, factorize_batch, solve_batch, release_idle_streams,
    LinearSolverException, SymbolicException, FactorizationException, SolveException, InertiaException,
)
from .kkt import (  # noqa: F401
    UnreducedKKTVector, SparseCondensedKKTSystem, DenseCondensedKKTSystem, DenseKKTSystem, ScenarioBatch, LowRankHessianKKT,
)
from .backsolve import ITERATORS, KrylovIterator, RichardsonIterator  # noqa: F401
from ._lib import MNK_QN_BFGS, MNK_QN_DAMPED_BFGS  # noqa: F401
from .quasi_newton import HESSIAN_APPROXIMATIONS, CompactLBFGS, QuasiNewtonOptions  # noqa: F401
# the values of IPMOptions.hessian_approximation
HESSIAN_EXACT, HESSIAN_BFGS, HESSIAN_DAMPED_BFGS, HESSIAN_COMPACT_LBFGS = HESSIAN_APPROXIMATIONS

__version__ = "0.1.0"
from .schur import SchurDenseStage  # noqa: F401,E402
from .ipm_device import IPMDeviceKernels  # noqa: F401,E402

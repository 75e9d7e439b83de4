"""lapack_algorithm = EVD without a device: the test matrices of tests/evd_cases.py are what the device tests assume (no
eigenvalue at rounding level, so an inertia comparison with dsyevd is meaningful; the diagonal family is reproduced exactly by
dsyevd), the bindings name EVD at every layer, and the oracle's IPM runs with LapackCPUSolver(EVD) -- the partners of the
device runs in tests/test_hip_evd.py -- are pinned."""
import os
import re

import numpy as np
import pytest

from oracle.lapack_cpu import EVD, LapackCPUSolver
from tests.evd_cases import (DIAG_SIZES, KINDS, SEPARATION, SIZES, backward_error, diag_family, dsyevd, is_permutation,
                             lower_with_garbage, ratios, sym_matrix)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_cases_have_no_eigenvalue_at_rounding_level(kind, N):
    A = sym_matrix(N, kind)
    assert np.array_equal(A, A.T)
    lam, Q = dsyevd(A)
    assert np.abs(lam).min() >= SEPARATION * np.abs(lam).max()
    # the oracle's solver reads the lower triangle only and counts the signs
    s = LapackCPUSolver(lower_with_garbage(A), EVD).factorize()
    assert np.array_equal(s.Lam, lam)
    assert s.inertia() == (int((lam > 0).sum()), 0, int((lam < 0).sum()))
    res, orth = ratios(A, lam, Q)
    assert res <= 50.0 and orth <= 50.0   # (dsyevd's own ratios, the yardstick of the device test, under LAPACK's test threshold)
    b = np.random.default_rng(N + 1).standard_normal(N)
    assert backward_error(A, s.solve_linear_system(b.copy()), b) <= 1e-13


@pytest.mark.parametrize("N", DIAG_SIZES)
def test_dsyevd_reproduces_the_diagonal_family_exactly(N):
    A, d = diag_family(N)
    lam, Q = dsyevd(lower_with_garbage(A))
    assert np.array_equal(lam, np.sort(d))
    assert is_permutation(Q)
    assert np.array_equal(A @ Q, Q * lam)
    s = LapackCPUSolver(A, EVD).factorize()
    assert s.inertia() == (int((d > 0).sum()), 1, int((d < 0).sum()))


# --------------------------------------------------------------------------- the bindings
def test_library_sources_and_python_map_evd():
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import _lib as L
    from madnlp_jl_amd.linear_solver import _ALGO
    assert "evd.hip" in L.SOURCES
    assert os.path.exists(os.path.join(L.CSRC, "evd.hip"))
    assert mj.EVD == EVD == "EVD"
    assert _ALGO[mj.EVD] == L.MNK_EVD == 6
    # HipLinearSolver, the inertia-revealing solver, serves it itself
    assert mj.EVD in mj.HipLinearSolver._algorithms
    s = mj.HipLinearSolver.__new__(mj.HipLinearSolver)
    s.opt = mj.HipSolverOptions(lapack_algorithm=mj.EVD)
    assert s.is_inertia()
    assert "EVD" in s.introduce()


def test_lu_solver_refuses_evd_before_touching_the_device():
    import madnlp_jl_amd as mj
    with pytest.raises(mj.SymbolicException, match="EVD"):
        mj.HipLUSolver(np.eye(4, order="F"), opt=mj.HipSolverOptions(lapack_algorithm=mj.EVD))


def test_header_names_evd_as_implemented():
    hdr = open(os.path.join(ROOT, "include", "madnlp_hip.h")).read()
    assert "MNK_EVD = 6" in hdr
    implemented = re.search(r"Implemented on device:(.*?)\*/", hdr, flags=re.S).group(1)
    assert "EVD" in implemented and "LU" in implemented and "QR" in implemented
    assert "MNK_EVD (solve_evd!" in hdr


def test_julia_glue_maps_evd_and_keeps_its_inertia():
    jl = open(os.path.join(ROOT, "julia", "MadNLPHIP.jl")).read()
    imported = re.search(r"import MadNLP:(.*?)\n(?:import|const)", jl, flags=re.S).group(1)
    assert "EVD" in {n.strip() for n in imported.replace("\n", " ").split(",")}
    assert re.search(r"MNK_ALGO = Dict\(.*\bEVD => Cint\(6\)", jl)
    line = re.search(r"^MadNLP\.is_inertia\(M::HipLinearSolver\{Float64\}\) = (.*)$", jl, flags=re.M).group(1)
    assert line == "!(M.opt.lapack_algorithm in (QR, LU))"


# --------------------------------------------------------------------------- the oracle's IPM runs with EVD
def _run(kind, nlp):
    from tests.test_inertia_free_cpu import run
    return run(kind, nlp, EVD)


@pytest.mark.parametrize("kind", ["dense_condensed", "sparse_condensed"])
def test_oracle_ipm_hs15_with_evd(kind):
    from madnlp_jl_amd.problems import HS15Model
    s = _run(kind, HS15Model())
    assert s.inertia_correction_method == "inertia_based"
    assert s.status == "SOLVE_SUCCEEDED", s.status


@pytest.mark.parametrize("n,m,n_eq", [(10, 5, 0), (50, 10, 0), (20, 15, 2)])
@pytest.mark.parametrize("kind", ["dense", "dense_condensed"])
def test_oracle_ipm_dense_qp_with_evd(kind, n, m, n_eq):
    from madnlp_jl_amd.problems import DenseQPModel
    from oracle.lapack_cpu import BUNCHKAUFMAN
    from tests.test_inertia_free_cpu import run
    nlp = DenseQPModel(n, m, n_eq)
    s = _run(kind, nlp)
    assert s.inertia_correction_method == "inertia_based"
    assert s.status == "SOLVE_SUCCEEDED", s.status
    assert s.cnt.k == run(kind, nlp, BUNCHKAUFMAN).cnt.k   # the exact inertia changes nothing on these


def test_oracle_ipm_sparse_qp_with_evd():
    from madnlp_jl_amd.problems import SparseQPModel
    s = _run("sparse_condensed", SparseQPModel("case30"))
    assert s.inertia_correction_method == "inertia_based"
    assert s.status == "SOLVE_SUCCEEDED", s.status

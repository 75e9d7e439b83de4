"""The LU solver (lapack_algorithm = LU) on the CPU side: the exact-answer construction of tests/lu_exact.py against LAPACK
dgetrf and a Fraction elimination, and the C ABI / Python / Julia glue that exposes the device LU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

from tests.lu_exact import exact_kkt, fraction_getrf, fractions_to_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(5))
def test_exact_construction_is_exact(seed):
    """dgetrf equals the Fraction elimination bit for bit (factors, pivots, info), with real row interchanges."""
    A, _ = exact_kkt(60, seed)
    M, ipiv, info = fraction_getrf(A)
    lu, piv, inf = sl.lapack.dgetrf(A)
    assert inf == info == 0
    assert np.array_equal(piv + 1, ipiv)
    assert np.array_equal(lu, fractions_to_float(M))
    assert (ipiv - 1 != np.arange(60)).sum() >= 10


@pytest.mark.parametrize("row", [0, 4, 11])
def test_exact_construction_singular(row):
    """A zero J entry makes a zero row and column: info is the first exactly zero pivot, dgetrf's and the Fraction one's."""
    A, _ = exact_kkt(60, 3, zero_j_row=row)
    M, ipiv, info = fraction_getrf(A)
    lu, piv, inf = sl.lapack.dgetrf(A)
    assert info > 0 and inf == info
    assert np.array_equal(piv + 1, ipiv)
    assert np.array_equal(lu, fractions_to_float(M))


@pytest.mark.parametrize("N", [300, 1000])
def test_exact_construction_swaps_cross_block_boundaries(N):
    """At the device test sizes the pivots cross 64-row panels and 256-row blocks, and the factors stay dyadic (an LU of the
    same matrix with the columns eliminated in LAPACK's blocked order and in dgetf2's order agree bit for bit)."""
    A, _ = exact_kkt(N, N)
    lu, piv, info = sl.lapack.dgetrf(A)
    assert info == 0
    rows = np.arange(N)
    assert ((piv // 64) != (rows // 64)).sum() > 0
    assert ((piv // 256) != (rows // 256)).sum() > 0
    # unblocked right-looking elimination in fp64, column by column
    F = A.copy()
    for j in range(N):
        p = j + int(np.argmax(np.abs(F[j:, j])))
        assert p == piv[j]
        F[[j, p]] = F[[p, j]]
        F[j + 1:, j] *= 1.0 / F[j, j]
        F[j + 1:, j + 1:] -= np.outer(F[j + 1:, j], F[j, j + 1:])
    assert np.array_equal(F, lu)


def test_header_declares_get_pivots_and_documents_lu():
    hdr = open(os.path.join(ROOT, "include", "madnlp_hip.h")).read()
    assert re.search(r"int\s+mnk_ls_get_pivots\s*\(\s*mnk_ls\s*\*\s*ls\s*,\s*int64_t\s*\*\s*ipiv\s*,\s*int\s+loc\s*\)\s*;", hdr)
    assert "MNK_LU = 2" in hdr
    assert "MNK_LU (solve_lu!" in hdr


def test_library_exports_get_pivots_and_python_maps_lu():
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import _lib as L
    from madnlp_jl_amd.linear_solver import _ALGO, LU
    mj.lib()
    raw = C.CDLL(L.LIBPATH)
    assert hasattr(raw, "mnk_ls_get_pivots")
    assert "mnk_ls_get_pivots" in L.SIGNATURES
    assert "lu.hip" in L.SOURCES
    assert mj.LU == LU == "LU"
    assert _ALGO[LU] == L.MNK_LU == 2
    assert issubclass(mj.HipLUSolver, mj.HipLinearSolver)
    s = mj.HipLUSolver.__new__(mj.HipLUSolver)
    s.opt = mj.HipSolverOptions(lapack_algorithm=mj.LU)
    assert not s.is_inertia()
    with pytest.raises(mj.InertiaException):
        s.inertia()


def test_python_solver_classes_split_the_algorithms():
    """HipLinearSolver keeps refusing LU (pointing at HipLUSolver); HipLUSolver serves LU only.  Both refuse before they touch
    the device."""
    import madnlp_jl_amd as mj
    A = np.eye(4, order="F")
    with pytest.raises(mj.SymbolicException, match="HipLUSolver"):
        mj.HipLinearSolver(A, opt=mj.HipSolverOptions(lapack_algorithm=mj.LU))
    for alg in (mj.QR, mj.LDL, mj.CHOLESKY, "EVD"):
        with pytest.raises(mj.SymbolicException):
            mj.HipLUSolver(A, opt=mj.HipSolverOptions(lapack_algorithm=alg))


def test_julia_glue_maps_lu():
    jl = open(os.path.join(ROOT, "julia", "MadNLPHIP.jl")).read()
    imported = re.search(r"import MadNLP:(.*?)\n(?:import|const)", jl, flags=re.S).group(1)
    assert "LU" in {n.strip() for n in imported.replace("\n", " ").split(",")}
    assert re.search(r"MNK_ALGO = Dict\(.*\bLU => Cint\(2\)", jl)
    # every solver the glue builds is a HipLinearSolver{Float64, MT}; its is_inertia method excludes both QR and LU
    assert re.search(r"^    M = HipLinearSolver\{Float64, MT\}\(", jl, flags=re.M)
    assert re.search(r"^MadNLP\.is_supported\(::Type\{<:HipLinearSolver\}, ::Type\{Float32\}\) = false$", jl, flags=re.M)
    line = re.search(r"^MadNLP\.is_inertia\(M::HipLinearSolver\{Float64\}\) = (.*)$", jl, flags=re.M).group(1)
    assert line == "!(M.opt.lapack_algorithm in (QR, LU))"

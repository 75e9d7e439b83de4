"""The blocked solve for several right-hand sides (SOLVE_BLOCKED = 5, csrc/solve_multi.hip) as far as a machine without a GPU
sees it: the planner's rule through the host-only entry mnk_debug_solve_plan_multi, the exact cases of tests/solve_multi_cases.py
(their bit budgets, and that the column-wise emulation of the library's solve returns X* bit for bit), the Julia glue's Matrix
method and option, and the new export."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from madnlp_jl_amd import _lib as L
from tests.solve_exact import emulated_solve
from tests.solve_multi_cases import BIT_CAP, DEVICE_CASE, GPU_CASES, W, WIDTHS, multi_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKED = 5
FLAGS = ("pivoted", "persistent_opt", "solve512_opt", "have_linv512", "partitioned", "abort_raised", "debug_missing", "tracing", "ldl")


def plan_multi(Np, num_cu, nrhs, multi_rhs_min, **flags):
    out = (C.c_int * 6)(*([-77] * 6))
    args = [int(flags.get(f, 1 if f == "persistent_opt" else 0)) for f in FLAGS]
    assert L.lib().mnk_debug_solve_plan_multi(Np, num_cu, *args, nrhs, multi_rhs_min, out) == 0
    assert out[5] == -77, "the entry wrote behind its five results"
    return {"path": out[0], "W": out[1], "chunks": out[2], "last_padded": out[3], "G": out[4]}


def plan_single(Np, num_cu, **flags):
    out = (C.c_int * 5)()
    args = [int(flags.get(f, 1 if f == "persistent_opt" else 0)) for f in FLAGS]
    assert L.lib().mnk_debug_solve_plan(Np, num_cu, *args, 1, out) == 0
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ the planner
def test_the_chunk_width_is_what_the_cases_assume():
    assert plan_multi(704, 256, 4, 2)["W"] == W and W % 16 == 0


@pytest.mark.parametrize("Np,cu", [(64, 256), (704, 256), (4160, 256), (11200, 256), (11200, 16), (196608, 256)])
def test_pivoted_or_switched_off_or_below_the_threshold_is_the_column_loop(Np, cu):
    single = plan_single(Np, cu)
    for nrhs in (1, 3, 4, 64, 1000):
        p = plan_multi(Np, cu, nrhs, 2, pivoted=1)
        assert (p["path"], p["G"]) == plan_single(Np, cu, pivoted=1) and p["path"] == 1, (nrhs, p)
        assert (p["W"], p["chunks"], p["last_padded"]) == (0, 0, 0)
        p = plan_multi(Np, cu, nrhs, 0)
        assert (p["path"], p["G"], p["W"], p["chunks"], p["last_padded"]) == (*single, 0, 0, 0), (nrhs, p)
    for mn in (1, 2, 4, 16, 65):   # the threshold edge
        if mn > 1:
            assert plan_multi(Np, cu, mn - 1, mn)["path"] == single[0]
        assert plan_multi(Np, cu, mn, mn)["path"] == BLOCKED and plan_multi(Np, cu, mn + 1, mn)["path"] == BLOCKED


def test_chunks_and_the_padded_last_chunk():
    for nrhs in list(WIDTHS) + [1, 2, 3, 5, 31, 32, 33, 47, 48, 49, 127, 128, 129, 1000]:
        p = plan_multi(704, 256, nrhs, 1)
        last = nrhs - (p["chunks"] - 1) * W
        assert p["path"] == BLOCKED and p["W"] == W and p["chunks"] == -(-nrhs // W) and 1 <= last <= W, (nrhs, p)
        assert p["last_padded"] == -(-last // 16) * 16 and p["G"] == 0, (nrhs, p)
    assert [plan_multi(704, 256, r, 2)["last_padded"] for r in WIDTHS] == [16, 16, 16, 32, 64, 64, 16, 16]
    assert [plan_multi(704, 256, r, 2)["chunks"] for r in WIDTHS] == [1, 1, 1, 1, 1, 1, 2, 3]


def test_the_flags_of_the_one_launch_solves_do_not_change_the_verdict():
    others = [f for f in FLAGS if f != "pivoted"]
    for bits in itertools.product((0, 1), repeat=len(others)):
        flags = dict(zip(others, bits))
        for Np, cu in ((704, 256), (11200, 256), (4160, 3)):
            p = plan_multi(Np, cu, 17, 4, **flags)
            assert (p["path"], p["W"], p["chunks"], p["last_padded"]) == (BLOCKED, W, 1, 32), (flags, p)
            q = plan_multi(Np, cu, 3, 4, **flags)
            assert (q["path"], q["G"]) == plan_single(Np, cu, **flags) and q["chunks"] == 0, (flags, q)


def test_bad_arguments():
    out = (C.c_int * 5)()
    f = L.lib().mnk_debug_solve_plan_multi
    assert f(100, 256, *([0] * 9), 4, 2, out) == -1 and f(704, 0, *([0] * 9), 4, 2, out) == -1
    assert f(704, 256, *([0] * 9), 0, 2, out) == -1 and f(704, 256, *([0] * 9), 4, 2, None) == -1


# ------------------------------------------------------------------------------------------------ the cases
def test_the_gpu_cases_cover_every_order_twice_and_every_width_at_700():
    orders = {}
    for n, r, _ in GPU_CASES:
        orders.setdefault(n, set()).add(r)
    assert set(orders) == {1, 63, 65, 256, 257, 700, 1300} and all(len(v) >= 2 for v in orders.values()), orders
    assert orders[700] == set(WIDTHS) and DEVICE_CASE[0] == 4100
    assert set(WIDTHS) == {4, 15, 16, 17, W - 1, W, W + 1, 2 * W + 2}


@pytest.mark.parametrize("positive", [True, False])
def test_every_column_of_the_gpu_cases_keeps_the_bit_budget(positive):
    for n, r, sb in GPU_CASES + [DEVICE_CASE, (1300, 4, 40)]:
        mc = multi_case(n, positive, sb, r)
        assert max(mc.budgets()) <= BIT_CAP, (n, r, sb)
        assert mc.X.shape == (n, r) and mc.B.shape == (n, r) and mc.X.flags.f_contiguous
        assert len({mc.X[:, k].tobytes() for k in range(r)}) == r or n < 3, "the columns are distinct"
    for variant in (1,):   # (the second matrix of the mixing test)
        assert max(multi_case(700, positive, 0, 17, variant).budgets()) <= BIT_CAP


@pytest.mark.parametrize("positive", [True, False])
@pytest.mark.parametrize("n,r,sb", [(1, 4, 0), (65, 16, 0), (256, 4, 0), (257, 17, 40), (700, 17, 0), (1300, 16, 0)])
def test_the_column_wise_emulation_returns_the_solutions(n, r, sb, positive):
    """The library's solve in numpy (256-column steps, explicit inverses, every sum in a shuffled order) on a few columns of a
    case, the scaled ones among them: X* bit for bit."""
    mc = multi_case(n, positive, sb, r)
    rng = np.random.default_rng(n + r)
    X = mc.X
    for k in (0, 2, 3, r - 1):
        got = emulated_solve(mc.column(k), 256, rng) * mc.colscale[k]
        assert np.array_equal(got, X[:, k]), (n, r, sb, k)
    assert np.array_equal(mc.B[:, 3], mc.column(3).b * mc.colscale[3])


# ------------------------------------------------------------------------------------------------ glue and symbol
def test_the_julia_glue_has_the_matrix_method_and_the_option():
    jl = open(os.path.join(ROOT, "julia", "MadNLPHIP.jl")).read()
    m = re.search(r"function MadNLP\.solve_linear_system!\(M::HipLinearSolver, X::Matrix\{Float64\}\)(.*?)\nend", jl, flags=re.S)
    assert m, "no Matrix method of solve_linear_system!"
    body = re.sub(r"\s+", " ", m.group(1))
    assert ":mnk_ls_solve" in body and "M.handle, X, size(X, 2), stride(X, 2), MNK_HOST" in body and "check(rc, SolveException)" in body
    opts = jl.split("struct HipSolverOptions")[1].split("\nend")[0]
    default = re.search(r"^\s+multi_rhs_min::Int = (\d+)", opts, flags=re.M)
    assert default and 'set_option!(h[], "multi_rhs_min", opt.multi_rhs_min)' in jl
    ls_h = open(os.path.join(ROOT, "madnlp.jl_amd", "csrc", "ls.h")).read()
    lib_default = int(re.search(r"int64_t multi_rhs_min = (\d+);", ls_h).group(1))
    from madnlp_jl_amd.linear_solver import HipSolverOptions
    assert int(default.group(1)) == lib_default == HipSolverOptions().multi_rhs_min
    assert lib_default == 0 or lib_default >= 4, "existing callers solve three columns on paths 1-3"


def test_the_new_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "madnlp_hip.h")).read()
    assert re.search(r"\nint mnk_debug_solve_plan_multi\(int64_t Np, int num_cu,", hdr)
    assert "mnk_debug_solve_plan_multi" in L.SIGNATURES and "solve_multi.hip" in L.SOURCES
    f = L.lib().mnk_debug_solve_plan_multi
    assert f.restype is C.c_int and len(f.argtypes) == 14
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "multi_rhs_min" in integ and "solve_rhs_chunks" in integ

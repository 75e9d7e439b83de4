"""The dense S stage of the Schur-complement KKT system (csrc/schur.hip) against two-stage systems whose every answer is known
exactly (-m gpu).

tests/schur_exact.py builds scenario blocks with exact static-pivot factors or exact Bunch-Kaufman factors, dyadic coupling
blocks and a design block such that S, every scenario term, the right-hand side b = K x and every intermediate of the solve
are short dyadic sums (tests/test_schur_exact_cpu.py pins the construction and the oracle on the CPU).  Whatever the blocking,
the summation order or FMA, the device must then return those bits: `np.array_equal` throughout, no tolerance.  The scenarios
built for the pivoted tier take the column-by-column fallback of mnk_schur_build_local (T_k = A_k^-1 C_dk', zero-padded copies,
one product) and the tier's own solve inside the stage's solve batches; every test asserts through the stage which scenarios
did, and prints it.  The all-static shapes come first: they run on paths other tests exercise too."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import madnlp_jl_amd as mj
from madnlp_jl_amd import _lib as L
from madnlp_jl_amd.schur import SchurDenseStage, shard
from tests import schur_exact as se

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    i = tuple(bad[0])
    return f"{len(bad)} entries differ, first at {i}: {got[i]!r} != {want[i]!r}"


def _tiers(st):
    return tuple(k for k in range(st.ns) if st.scenario_bk_active(k))


def check_stage(st, c, tag):
    """build_kkt = S, the tiers and inertias of the scenarios, info, inertia of S, the solve with device and with host
    vectors: all exact."""
    nd = c.nd
    S = st.build_kkt().cpu().numpy().reshape((nd, nd), order="F")
    assert np.array_equal(S, c.S), f"{tag}: S: " + _first_diff(S, c.S)
    tiers = _tiers(st)
    print(f"{tag}: scenarios on the pivoted tier (fallback build) {list(tiers)}")
    assert tiers == c.pivoted, f"{tag}: pivoted tier taken by {tiers}, meant for {c.pivoted}"
    for k in range(c.ns):
        assert st.scenario_inertia(k) == c.inertia(k), f"{tag}: inertia of scenario {k}"
    assert st.factorize_kkt() == 0, tag
    assert st.inertia() == (nd, 0, 0), tag
    rk = torch.from_numpy(c.bk.copy()).cuda()
    rd = torch.from_numpy(c.bd.copy()).cuda()
    st.solve(rk, rd)
    xk, xd = rk.cpu().numpy(), rd.cpu().numpy()
    assert np.array_equal(xd, c.xd), f"{tag}: x_d (device vectors): " + _first_diff(xd, c.xd)
    assert np.array_equal(xk, c.xk), f"{tag}: x_k (device vectors): " + _first_diff(xk, c.xk)
    hk, hd = np.ascontiguousarray(c.bk.copy()), c.bd.copy()
    st.solve_host(hk, hd)
    assert np.array_equal(hd, c.xd), f"{tag}: x_d (host vectors): " + _first_diff(hd, c.xd)
    assert np.array_equal(hk, c.xk), f"{tag}: x_k (host vectors): " + _first_diff(hk, c.xk)


def run_case(ctx, c, tag, algorithm=mj.BUNCHKAUFMAN):
    st = SchurDenseStage(c.A, c.C, c.S0, c.nd, c.blk, ctx=ctx, algorithm=algorithm)
    try:
        check_stage(st, c, tag)
    finally:
        st.close()


# ------------------------------------------------------------------------------------------------ all static: the grouped path
_SHAPE_ID = lambda s: "x".join(map(str, s))   # noqa: E731


@pytest.mark.parametrize("shape", se.SHAPES, ids=_SHAPE_ID)
def test_every_stage_shape_static(ctx, shape):
    """(1, 5, 3) the smallest system; (3, 17, 65) blkp = 32 and nd just past its pad of 64; (4, 64, 64) on the pads; (5, 129,
    129) Npb = 256, two k-steps of the grouped sweep, nd just past 128; (5, 200, 30); (3, 384, 100) Npb = 384."""
    run_case(ctx, se.make_schur(*shape), f"(ns, blk, nd) = {shape} static")


@pytest.mark.parametrize("algorithm", [mj.CHOLESKY, mj.LDL, mj.BUNCHKAUFMAN])
@pytest.mark.parametrize("shape", [(4, 64, 64), (5, 129, 129)], ids=_SHAPE_ID)
def test_every_algorithm_on_static_blocks(ctx, shape, algorithm):
    """CHOLESKY (every d > 0; V = X, no D^-1 scaling: L sqrt(D) is exact since d = 4^e), LDL (the D^-1 scaling) and
    BUNCHKAUFMAN, which must stay on its static tier."""
    c = se.make_schur(*shape, (), algorithm == mj.CHOLESKY)
    run_case(ctx, c, f"{shape} {algorithm}", algorithm)


def test_more_scenarios_than_one_default_chunk_holds_at_least(ctx, monkeypatch):
    """ns = 35, all static, MNK_SCHUR_CHUNK unset (the variable is read when the stage is created)."""
    monkeypatch.delenv("MNK_SCHUR_CHUNK", raising=False)
    c = se.make_schur(*se.CHUNK_STATIC)
    run_case(ctx, c, f"{se.CHUNK_STATIC} static")


# ------------------------------------------------------------------------------------------------ the fallback enters
@pytest.mark.parametrize("shape", se.SHAPES, ids=_SHAPE_ID)
def test_every_stage_shape_mixed(ctx, shape):
    """The same shapes with the first scenario and every third after it on the pivoted tier, the others on the grouped path."""
    run_case(ctx, se.make_schur(*shape, se.mixed_of(shape[0])), f"(ns, blk, nd) = {shape} mixed")


# ------------------------------------------------------------------------------------------------ which scenarios are pivoted
@pytest.mark.parametrize("pivoted", se.PATTERNS, ids=lambda p: "piv" + ("".join(map(str, p)) or "none"))
def test_which_scenarios_are_pivoted(ctx, pivoted):
    """ns = 5: none, all, the first only, the last only, alternating.  The grouped path's list of scenarios is compacted, so its
    i-th member is scenario i only while no pivoted scenario sits in front; the fallback reuses T, Cp, Tt from scenario to
    scenario (all: five in a row)."""
    c = se.make_schur(*se.PATTERN_SHAPE, pivoted)
    run_case(ctx, c, f"{se.PATTERN_SHAPE} pivoted {pivoted}")


def test_rebuild_on_the_same_handle(ctx):
    """set_blocks swaps a static block for a pivoted one and back, then three, then all static again: the grouped and the
    fallback buffers carry nothing over from the previous scenario or the previous build.  Exact every time."""
    ns, blk, nd = se.PATTERN_SHAPE
    c0 = se.make_schur(ns, blk, nd, ())
    st = SchurDenseStage(c0.A, c0.C, c0.S0, nd, blk, ctx=ctx)
    try:
        check_stage(st, c0, "rebuild: static")
        prev = c0
        for step, piv in enumerate([(2,), (), (0, 2, 4), (1,), ()]):
            c = se.make_schur(ns, blk, nd, piv)
            changed = [k for k in range(ns) if (k in piv) != (k in prev.pivoted)]
            st.set_blocks([c.A[k] if k in changed else None for k in range(ns)], [c.C[k] if k in changed else None for k in range(ns)], c.S0)
            check_stage(st, c, f"rebuild step {step}: pivoted {piv}")
            prev = c
    finally:
        st.close()


# ------------------------------------------------------------------------------------------------ chunks of the grouped build
_CHUNK_CHILD = r'''
import sys
sys.path.insert(0, %r)
import madnlp_jl_amd as mj
from madnlp_jl_amd.schur import SchurDenseStage
from tests import schur_exact as se
from tests.test_hip_schur_exact import check_stage
c = se.make_schur(*se.CHUNK_MIXED, se.CHUNK_MIXED_PIVOTED)
ctx = mj.HipContext(0)
st = SchurDenseStage(c.A, c.C, c.S0, c.nd, c.blk, ctx=ctx)
check_stage(st, c, "chunks of 3, mixed")
st.close()
ctx.close()
print("CHUNK_OK")
'''


def test_mixed_build_in_chunks_of_three():
    """ns = 7, scenarios 0, 3, 6 pivoted, MNK_SCHUR_CHUNK = 3: the grouped path holds scenarios [1, 2, 4] and [5], so in every
    chunk its i-th member is not scenario i.  Own process: the variable is read at creation."""
    env = dict(os.environ, MNK_SCHUR_CHUNK="3")
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD % ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "CHUNK_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-2500:]
    assert f"(fallback build) {list(se.CHUNK_MIXED_PIVOTED)}" in r.stdout


# ------------------------------------------------------------------------------------------------ two "ranks" on one GPU
@pytest.mark.parametrize("pivoted", [(), (0, 3)], ids=["static", "mixed"])
def test_two_ranks_and_a_rank_without_scenarios(ctx, pivoted):
    """The even / odd shards' contributions are the exact partial sums and add, in fp64, to S; a third handle with no scenario
    and no S0 contributes zero and, given the summed S, solves for x_d."""
    ns, blk, nd = 5, 40, 20
    c = se.make_schur(ns, blk, nd, pivoted)
    parts = []
    for rank in range(2):
        own = shard(ns, rank, 2)
        loc = SchurDenseStage([c.A[k] for k in own], [c.C[k] for k in own], c.S0 if rank == 0 else None, nd, blk, ctx=ctx)
        try:
            P = loc.build_kkt().cpu().numpy().reshape((nd, nd), order="F")
            want = c.contribution(own, rank == 0)
            assert np.array_equal(P, want), f"rank {rank}: " + _first_diff(P, want)
            assert tuple(own[i] for i in _tiers(loc)) == tuple(k for k in own if k in pivoted), rank
            parts.append(P)
        finally:
            loc.close()
    assert np.array_equal(parts[0] + parts[1], c.S)
    empty = SchurDenseStage([], [], None, nd, blk, ctx=ctx)
    try:
        Z = empty.build_kkt().cpu().numpy()
        assert Z.shape == (nd * nd,) and not Z.any(), "a rank without scenarios contributes zero"
        empty.S.copy_(torch.from_numpy((parts[0] + parts[1] + Z.reshape((nd, nd), order="F")).ravel(order="F")).cuda())
        assert empty.factorize_kkt() == 0 and empty.inertia() == (nd, 0, 0)
        rd = torch.from_numpy(c.rd.copy()).cuda()          # (the other ranks' contributions already added: S x_d)
        empty._contrib.fill_(float("nan"))
        torch.cuda.synchronize()                           # (the library works on its own stream)
        empty.solve(None, rd)
        assert not empty._contrib.cpu().numpy().any(), "forward of a rank without scenarios must zero-fill its contribution"
        assert np.array_equal(rd.cpu().numpy(), c.xd)
    finally:
        empty.close()


# ------------------------------------------------------------------------------------------------ leading dimensions
@pytest.mark.parametrize("pivoted", [(), (0, 3)], ids=["static", "mixed"])
def test_leading_dimensions_larger_than_the_orders(ctx, pivoted):
    """The raw ABI with lda = blk + 3, ldc = nd + 5 (host blocks), lds0 = nd + 2 (device S0), lds_out = nd + 7; all padding NaN:
    S is exact (no NaN was read) and the padding of S_out is untouched."""
    ns, blk, nd = 5, 40, 20
    c = se.make_schur(ns, blk, nd, pivoted)
    lib = mj.lib()
    lda, ldc, lds0, ldo = blk + 3, nd + 5, nd + 2, nd + 7
    h = C.c_void_p()
    L.check(lib.mnk_schur_create(ctx.handle, ns, blk, nd, L.MNK_BUNCHKAUFMAN, C.byref(h)), "mnk_schur_create")
    try:
        for k in range(ns):
            a = np.full((lda, blk), np.nan, order="F")
            a[:blk] = c.A[k]
            cc = np.full((ldc, blk), np.nan, order="F")
            cc[:nd] = c.C[k]
            L.check(lib.mnk_schur_set_block(h, k, a.ctypes.data, lda, cc.ctypes.data, ldc, L.MNK_HOST), "mnk_schur_set_block")
        s0 = np.full((lds0, nd), np.nan, order="F")
        s0[:nd] = c.S0
        s0_dev = torch.from_numpy(np.ascontiguousarray(s0.T)).cuda()          # (nd, lds0) row-major = column-major lds0 x nd
        out = torch.full((nd, ldo), float("nan"), dtype=torch.float64, device=s0_dev.device)
        L.check(lib.mnk_schur_build_local(h, s0_dev.data_ptr(), lds0, L.MNK_DEVICE, out.data_ptr(), ldo), "mnk_schur_build_local")
        ctx.synchronize()
        got = out.cpu().numpy().T                                              # ldo x nd
        assert np.array_equal(got[:nd], c.S), _first_diff(got[:nd], c.S)
        assert np.isnan(got[nd:]).all(), "the padding rows of S_out were written"
        act = C.c_int(0)
        tiers = []
        for k in range(ns):
            L.check(lib.mnk_schur_scenario_bk_info(h, k, C.byref(act), None), "mnk_schur_scenario_bk_info")
            tiers.append(bool(act.value))
        assert tiers == [k in pivoted for k in range(ns)]
    finally:
        lib.mnk_schur_destroy(h)

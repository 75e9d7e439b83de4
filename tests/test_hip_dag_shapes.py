"""Exact answers for factorize! and solve! under every plan shape of the task-DAG schedule (-m gpu).

A plan shape -- chunk length, band height, taper, the strip-column js2 at which every remaining row joins the pivot chain's band,
zero-fill tasks, per-XCD queues and gangs -- decides which tasks the bulk kernel runs, in which order, and which of the two
phases runs them; it cannot change the right answer.  The matrices of tests/exact_factor.py have LDL^T and Cholesky factors that
are exact in fp64 whatever the blocking and the summation order, the systems of tests/solve_exact.py solve to x* bit for bit, so
every tuple of tests/dag_shapes.py (whose task lists test_dag_shapes_cpu.py holds to the planner's invariants) is held to the
answer itself, never to another run of the library: the shape that ran is the shape that was asked for (statistics "panel_algo",
"pp_fallbacks", "dag_js2"), info and the inertia, D bit for bit and L within 4 ulp, one single-column and one 3-column solve
bit for bit -- the latter is what a wrong set of early diagonal-block inverses after a phase switch would break.

Orders: 1280 (10 tiles, the smallest of the schedule), 1300 (11 tiles: a last strip-column of one tile, padding rows), 1536 (12
tiles: with dag_band = 8 the rows below the band run out at strip-column 4), 2688 (21 tiles, 11 strip-columns: an early, a
middle and a late phase switch), and 200 / 384 / 640 (2, 3, 5 tiles) with dag_min_rows lowered to 128, where one or both
phases have no bulk task at all.  Every js2 of the grid is admissible at these orders on the default deep-band partition of
96 CUs (test_dag_shapes_cpu.py); an inadmissible one never reaches a launch (csrc/dag_plan.hip: dag_choose_js2).

NOT_SCHEDULE_5 lists the tuples the library may run as another schedule, each with the rule that excludes it; it is empty:
every tuple of the grid, at every order above, runs as schedule 5."""
import functools

import numpy as np
import pytest
import torch

import madnlp_jl_amd as mj
from tests import dag_shapes as S
from tests.exact_factor import make_exact, with_pivot
from tests.solve_exact import bit_budget, device_system, solve_case
from tests.test_hip_pivot_ladder import ULP4, _CSC, _KKT, _check_exact_ldl
from tests.test_hip_solve_exact import BIT_CAP, NAN, _assert_exact, _check_tail, _padded

pytestmark = pytest.mark.gpu

ALGS = [mj.CHOLESKY, mj.LDL]
KIND_ORDER = ("zero", "nsc", "last", "one", "half")   # closest to the shapes the sizes select first
# (n, chunk, band_tiles, taper0, js2) -> the rule of choose_schedule / mnk_ls_dag_prepare that keeps the tuple off schedule 5
NOT_SCHEDULE_5 = {}


def _params(orders):
    return [(n, kind) for n in orders for kind in KIND_ORDER if kind in S.js2_values(S.ORDERS[n])]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def _dev():
    return torch.device("cuda", 0)


class _Exact:
    """The exact-factor case of an order on the device: A, and what tril of the factor must be -- LDL^T: I + N with D = d;
    Cholesky: (I + N) sqrt(D), sqrt(4^e) = 2^e exact."""

    def __init__(self, n, positive):
        self.case = make_exact(n, 31000 + n, positive=positive)
        dev = _dev()
        self.A = torch.from_numpy(np.ascontiguousarray(self.case.A)).to(dev)
        Lx = torch.from_numpy(np.ascontiguousarray(self.case.L)).to(dev)
        self.L = Lx * torch.from_numpy(np.sqrt(self.case.d)).to(dev) if positive else Lx


class _Solve:
    """The dyadic system of an order on the device: S A S, b, the solution S^-1 x*."""

    def __init__(self, n, positive):
        self.case = solve_case(n, 100 + n, positive, scale_bits=20, dense=False)
        assert bit_budget(self.case) <= BIT_CAP, (n, positive, bit_budget(self.case))
        self.A, self.b = device_system(self.case, _dev())
        self.x = torch.from_numpy(self.case.x).to(_dev())


@functools.lru_cache(maxsize=None)
def _exact(n, positive):
    return _Exact(n, positive)


@functools.lru_cache(maxsize=None)
def _solve(n, positive):
    return _Solve(n, positive)


def _solver(ctx, A, alg, **opts):
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg, pivot_tol=0.0))
    for key, v in opts.items():
        M.set_option(key, v)
    return M


def _set_shape(M, chunk, band_tiles, taper0, js2, fill=1, queues=1, gang=4):
    for key, v in (("dag_chunk", chunk), ("dag_band", 2 * band_tiles), ("dag_taper0", taper0), ("dag_js2", js2), ("dag_fill", fill),
                   ("dag_xcd_queues", queues), ("dag_gang", gang)):
        M.set_option(key, v)


def _check_ran_as(M, js2, tag, algo=5):
    """The shape that ran is the shape that was asked for: a tuple that silently ran as another is a failure."""
    got = (M.get_stat("panel_algo"), M.get_stat("pp_fallbacks"), M.get_stat("timeout_site"))
    assert got == (algo, 0, 0), tag + f": (panel_algo, pp_fallbacks, timeout_site) = {got}, expected ({algo}, 0, 0)"
    if algo == 5:
        assert M.get_stat("dag_js2") == js2, tag + f": dag_js2 {M.get_stat('dag_js2')}, asked for {js2}"


def _check_factor(M, E, alg, tag):
    c = E.case
    assert M.info == 0, tag + f": info {M.info}"
    assert M.inertia() == c.inertia(), tag + f": inertia {M.inertia()} != {c.inertia()}"
    if alg == mj.LDL:
        _check_exact_ldl(M, c, tag, E.L)
        return
    Lt, _ = M.get_factor_device()
    L = torch.tril(Lt)
    assert torch.equal(L.diagonal(), E.L.diagonal()), tag + f": diag(L) differs at {torch.nonzero(L.diagonal() != E.L.diagonal())[:4].flatten().tolist()}"
    err = (L - E.L).abs() > ULP4 * E.L.abs()
    assert not bool(err.any()), tag + f": L off by more than 4 ulp of (I + N) sqrt(D) at {torch.nonzero(err)[:4].tolist()}"


def _check_solves(M, Sv, tag):
    n, dev = Sv.case.n, _dev()
    buf, v = _padded(Sv.b)
    torch.cuda.synchronize()
    M.solve_linear_system(v)
    M.check_solve()
    _assert_exact(v, Sv.x, tag + " one right-hand side")
    _check_tail(buf, n, tag)
    ldx = n + 7
    buf = torch.full((3, ldx), NAN, dtype=torch.float64, device=dev)
    X = buf.T[:n]
    scale = torch.tensor([1.0, -0.5, 4.0], dtype=torch.float64, device=dev)
    X[:] = Sv.b[:, None] * scale
    torch.cuda.synchronize()
    M.solve_linear_system(X)
    M.check_solve()
    _assert_exact(X, Sv.x[:, None] * scale, tag + " three right-hand sides")
    assert bool(torch.isnan(buf.T[n:]).all()), tag + ": the padding rows of the strided view were written"


def _factor_and_solve(M, E, Sv, alg, js2, tag, algo=5):
    """The exact-factor matrix, then the dyadic system, on one solver under the shape it has been given."""
    M.A = E.A
    torch.cuda.synchronize()      # (the matrices were produced on torch's stream, the solver works on its context's)
    M.factorize()
    _check_ran_as(M, js2, tag, algo)
    _check_factor(M, E, alg, tag)
    M.A = Sv.A
    M.factorize()
    _check_ran_as(M, js2, tag + " dyadic system", algo)
    assert M.info == 0 and M.inertia() == Sv.case.inertia(), tag + f" dyadic system: info {M.info}, inertia {M.inertia()}"
    _check_solves(M, Sv, tag)


def _run_grid(ctx, n, alg, kind, **opts):
    positive = alg == mj.CHOLESKY
    js2 = S.js2_values(S.ORDERS[n])[kind]
    E, Sv = _exact(n, positive), _solve(n, positive)
    M = _solver(ctx, E.A, alg, **opts)
    Mc = _CSC(ctx, n, alg, pivot_tol=0.0, **opts)
    Mc.M.A = E.case.lower_csc()
    try:
        for chunk, band_tiles, taper0 in S.shapes():
            tag = f"N={n} {alg} chunk={chunk} band={2 * band_tiles} taper0={taper0} js2={js2}"
            assert (n, chunk, band_tiles, taper0, js2) not in NOT_SCHEDULE_5
            _set_shape(M, chunk, band_tiles, taper0, js2)
            _factor_and_solve(M, E, Sv, alg, js2, tag)
        for chunk, band_tiles, taper0 in S.CORNERS:
            for fill in S.FILLS:
                for queues, gang in S.QUEUES:
                    tag = (f"N={n} {alg} chunk={chunk} band={2 * band_tiles} taper0={taper0} js2={js2} fill={fill} "
                           f"xcd_queues={queues} gang={gang}")
                    _set_shape(M, chunk, band_tiles, taper0, js2, fill, queues, gang)
                    _factor_and_solve(M, E, Sv, alg, js2, tag)
                    # a sparse source: the second factorization works in the buffer the first one's fill tasks (or, with
                    # dag_fill = 0, the side stream) have zeroed
                    _set_shape(Mc.M, chunk, band_tiles, taper0, js2, fill, queues, gang)
                    for rep in range(2):
                        Mc.M.factorize()
                        _check_ran_as(Mc.M, js2, tag + f" csc {rep}")
                        _check_factor(Mc.M, E, alg, tag + f" csc {rep}")
    finally:
        M.close()
        Mc.close()


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n,kind", _params((1280, 1300, 1536, 2688)))
def test_every_plan_shape_returns_the_exact_factor_and_solution(ctx, n, kind, alg):
    _run_grid(ctx, n, alg, kind)


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n,kind", _params(S.SMALL_ORDERS))
def test_small_orders_with_empty_phases(ctx, n, kind, alg):
    """2, 3 and 5 tiles under dag_min_rows = 128: no bulk task at all (2 and 3 tiles), or none in one of the phases -- the bulk
    launch of an empty part is skipped (dag.hip: launch_dag_bulk_single), the chain alone factors.  Never an error, an empty
    grid or a fallback; every tuple runs as schedule 5."""
    _run_grid(ctx, n, alg, kind, dag_min_rows=128)


@pytest.mark.parametrize("alg", ALGS)
def test_setting_dag_js2_alone_takes_effect_on_a_solver_that_has_factorized(ctx, alg):
    """The option rebuilds the plan: on one solver, with no other option touched in between, js2 by size (0 at this order), then
    every js2 of the grid, then by size again -- each the shape that ran, each exact."""
    n = 2688
    positive = alg == mj.CHOLESKY
    E, Sv = _exact(n, positive), _solve(n, positive)
    M = _solver(ctx, E.A, alg)
    try:
        for js2 in [-1] + list(S.js2_values(S.ORDERS[n]).values())[::-1] + [-1]:
            M.set_option("dag_js2", js2)
            _factor_and_solve(M, E, Sv, alg, max(js2, 0), f"N={n} {alg} dag_js2={js2} alone")
    finally:
        M.close()


# ------------------------------------------------------------------------------------------------ breakdowns
N_BREAK = 2688
# leaf ends (k % 64 == 63: the early rejection reports the last column of the 64-column leaf that holds the bad pivot): in
# strip-column 1, whose rows below the 4-tile band the bulk kernel closes; in strip-column 5 = nsc // 2, where the phases switch;
# the last column of the last strip-column
BREAK_COLS = (319, 1343, 2687)


@pytest.mark.parametrize("kind", ["half", "nsc"])
def test_breakdowns_under_non_default_shapes(ctx, kind):
    """A negative and a zero pivot under dag_band = 8 with the phase switch in the middle and with no second phase: CHOLESKY's
    info is k + 1, LDL^T (pivot_tol = 0) has the Sylvester inertia, D = d bit for bit and L within 4 ulp of I + N, and with
    accept_only_pd and early_reject the factorization stops in the leaf of column k."""
    n = N_BREAK
    js2 = S.js2_values(S.ORDERS[n])[kind]
    assert js2 == {"half": 5, "nsc": 11}[kind] and all(k % 64 == 63 for k in BREAK_COLS) and BREAK_COLS[1] // 256 == 5
    base, pos = _exact(n, False), _exact(n, True)
    pat = pos.case.lower_pattern()
    ldl, chol = _solver(ctx, base.A, mj.LDL), _solver(ctx, pos.A, mj.CHOLESKY)
    kh = _KKT(ctx, n, mj.BUNCHKAUFMAN, pat)
    kh.M.set_option("probe", 0)
    try:
        for M in (ldl, chol, kh.M):
            _set_shape(M, 64, 4, 2, js2)
        for k in BREAK_COLS:
            for what in ("neg", "zero"):
                tag = f"N={n} band=8 js2={js2} {what} pivot at column {k}"
                c = with_pivot(base.case, k, -abs(base.case.d[k]) if what == "neg" else 0.0)
                cp = with_pivot(pos.case, k, -pos.case.d[k] if what == "neg" else 0.0)
                ldl.A = torch.from_numpy(np.ascontiguousarray(c.A)).to(_dev())
                torch.cuda.synchronize()
                ldl.factorize()
                _check_ran_as(ldl, js2, tag + " LDL")
                assert ldl.inertia() == c.inertia(), tag + f" LDL: inertia {ldl.inertia()} != {c.inertia()}"
                _check_exact_ldl(ldl, c, tag + " LDL", base.L)
                chol.A = torch.from_numpy(np.ascontiguousarray(cp.A)).to(_dev())
                torch.cuda.synchronize()
                chol.factorize()
                _check_ran_as(chol, js2, tag + " CHOLESKY")
                assert chol.info == k + 1 == cp.dpotrf_info(), tag + f" CHOLESKY: info {chol.info}"
                assert chol.inertia() == (0, n, 0), tag + f" CHOLESKY: inertia {chol.inertia()}"
                M = kh.factorize(cp)
                want = (int(np.sum(cp.d[:k + 1] > 0)), int(np.sum(cp.d[:k + 1] == 0)))
                assert M.inertia() == (want[0], want[1], n - want[0] - want[1]), tag + f" early_reject: inertia {M.inertia()}"
                assert M.get_stat("early_reject_col") == k, tag + f": early_reject_col {M.get_stat('early_reject_col')}"
                _check_ran_as(M, js2, tag + " early_reject")
    finally:
        ldl.close(); chol.close(); kh.close()


# ------------------------------------------------------------------------------------------------ the step-down rule
@pytest.mark.parametrize("alg", ALGS)
def test_a_band_taller_than_the_chain_partition_steps_down_to_schedule_4(ctx, alg):
    """choose_schedule (factor.hip): dag_band = 20 strips on the chain's 16 CUs cannot be resident, the factorization keeps
    schedule 4 -- and is exact there."""
    n = 1300
    positive = alg == mj.CHOLESKY
    E, Sv = _exact(n, positive), _solve(n, positive)
    M = _solver(ctx, E.A, alg, dag_band=20)
    try:
        _factor_and_solve(M, E, Sv, alg, None, f"N={n} {alg} band=20", algo=4)
    finally:
        M.close()

"""The KKT-handle contract on the Schur handle (`mnk_schur_solve_kkt`, `mnk_schur_mul`, `mnk_schur_jtprod`,
`mnk_schur_mul_hess_blk`, the bound / barrier state and its feeders; csrc/schur.hip) on the device.

The comparator is the ordered host mirror of `SchurComplementKKTSystem` (`solve_kkt_ordered`, `mul_ordered`, `jtprod_ordered`,
`mul_hess_blk_ordered`): numpy code that performs the kernels' operations in the kernels' order, so the device result has to
equal it BIT FOR BIT on standard-normal data; on dyadic data (tests/schur_ops_cases.py) it has to equal the integer-arithmetic
answer.  `solve_kkt!` is also held to the oracle system's answer (1e-9 max|w|, what tests/test_schur_kkt.py gives the host path).
Every shape runs with the product row threshold at its default (64), at 0 (every nonempty row on the wavefront path) and at
INT64_MAX (one thread per row)."""
import numpy as np
import pytest

from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.problems import TwoStageQPModel, random_twostage_qp
from tests.kkt_exact import ALPHA_BETA
from tests.schur_ops_cases import (THRESHOLDS, dyadic_values, dyadic_vector, exact_axpby, exact_spmv, model_pattern,
                                   pattern, row_lists, unreduced_matrix)
from tests.test_schur_kkt import coupled_quadratic, oracle_schur, several_recourse_and_design, solve, two_by_two

pytestmark = pytest.mark.gpu


def crafted_model():
    """Design columns of exactly 64, 65, 128 and 129 Jacobian entries over two scenarios (32 + 32, 32 + 33, 64 + 64, 64 + 65 rows):
    rows of J' at, one above, at twice and one above twice the default threshold."""
    ns, nv, nd, nc, nc_eq = 2, 4, 4, 66, 1
    rng = np.random.default_rng(21)
    A_v = np.zeros((nc, nv, ns))
    for i in range(nc):
        A_v[i, i % nv, :] = 2.0 + rng.random(ns)
        A_v[i, (i + 1) % nv, :] = rng.standard_normal(ns)
    A_d = np.zeros((nc, nd, ns))
    for j, (c0, c1) in enumerate(((32, 32), (32, 33), (64, 64), (64, 65))):
        A_d[:c0, j, 0] = rng.standard_normal(c0) * 0.5
        A_d[:c1, j, 1] = rng.standard_normal(c1) * 0.5
    xs_v, xs_d = rng.uniform(-0.5, 0.5, (nv, ns)), rng.uniform(-0.5, 0.5, nd)
    c = np.einsum("ijk,jk->ik", A_v, xs_v) + np.einsum("ijk,j->ik", A_d, xs_d)
    lcon, ucon = c - rng.uniform(0.2, 1.0, (nc, ns)), c + rng.uniform(0.2, 1.0, (nc, ns))
    lcon[:nc_eq], ucon[:nc_eq] = c[:nc_eq], c[:nc_eq]
    nlp = TwoStageQPModel(ns, nv, nd, nc, rng.uniform(0.5, 4.0, (nv, ns)), rng.uniform(0.5, 4.0, nd), rng.standard_normal((nv, ns)),
                          rng.standard_normal(nd), A_v, A_d, lcon, ucon, xs_v - 2.0, xs_v + 2.0, xs_d - 2.0, xs_d + 2.0, sparse_pattern=True)
    assert np.array_equal(np.bincount(nlp.jac_J, minlength=nlp.n)[ns * nv:], [64, 65, 128, 129])
    return nlp


def empty_upper_side():
    """No upper bound anywhere: variables bounded below only, inequality rows one-sided."""
    nlp = random_twostage_qp(ns=3, nv=17, nd=4, nc=7, nc_eq=3, seed=5)
    nlp.uvar[:] = np.inf
    nlp.ucon[nlp.lcon != nlp.ucon] = np.inf
    return nlp


MODELS = {
    "ns1_nd1": lambda: random_twostage_qp(ns=1, nv=3, nd=1, nc=2, nc_eq=1, seed=3),
    "odd": lambda: random_twostage_qp(ns=3, nv=17, nd=4, nc=7, nc_eq=3, seed=5),                  # every variable has both bounds
    "dense_design": lambda: random_twostage_qp(ns=5, nv=20, nd=6, nc=30, nc_eq=4, seed=6),      # J' design rows: 150 entries, ragged last pass
    "no_inequalities": lambda: random_twostage_qp(ns=2, nv=6, nd=3, nc=3, nc_eq=3, seed=8),
    "no_equalities": lambda: random_twostage_qp(ns=2, nv=6, nd=3, nc=4, nc_eq=0, seed=9),
    "crafted_columns": crafted_model,
    "empty_upper_side": empty_upper_side,
}
# the products also run on a pattern no QP model has: both Hessian triangles, duplicates, design rows of H of 64 .. 129 entries
GENERAL = dict(ns=3, nv=5, nd=6, nc=8, nc_eq=2, jac_rows=[0, 3, 4, 64, 65, 128, 129, 1], hess_design_rows=[0, 3, 63, 64, 127, 126])
T_IDS = ["T_default", "T_0", "T_never"]


@pytest.fixture(scope="module")
def gctx():
    torch = pytest.importorskip("torch")
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models():
    return {k: f() for k, f in MODELS.items()}


def hip_schur(nlp, ctx, **kw):
    from madnlp_jl_amd.schur_kkt import SchurComplementKKTSystem

    def make(info):
        return SchurComplementKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"],
                                        info["ind_eq"], info["ind_lb"], info["ind_ub"], ctx=ctx, **nlp.schur_opts(), **kw)
    return make


def dev(ctx, a):
    import torch
    t = torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()                                       # (the library works on its own stream)
    return t


def host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


def same_bits(got, want, what=""):
    """array_equal, with the count, the size and the first places of the mismatch in the message."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want)} entries differ, first at {bad[:8].tolist()}, "
                           f"max |difference| {np.abs(got[bad] - want[bad]).max():.3e}")
    return True


def factorized(nlp, factory):
    """A solver after initialize / set_aug_diagonal / build_kkt / factorize_kkt, as tests/test_schur_kkt.py sets one up."""
    s = MadNLPSolver(nlp, factory, IPMOptions(), sparse=True)
    s.initialize()
    s.set_aug_diagonal()
    s.kkt.build_kkt()
    s.kkt.factorize_kkt()
    return s


@pytest.fixture(scope="module")
def oracle_solutions(models):
    """Per model: a right-hand side and the oracle system's solve_kkt! of it (computed once)."""
    out = {}
    for name, nlp in models.items():
        so = factorized(nlp, oracle_schur(nlp))
        w = so.d.copy()
        w.values[:] = np.random.default_rng(2).standard_normal(w.values.shape)
        rhs = w.values.copy()
        so.kkt.solve_kkt(w)
        out[name] = (rhs, w.values.copy())
    return out


# ------------------------------------------------------------------------------------------------ solve_kkt!
@pytest.mark.parametrize("T", THRESHOLDS, ids=T_IDS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_solve_kkt_device_equals_the_ordered_mirror_and_the_oracle(gctx, models, oracle_solutions, name, T):
    nlp = models[name]
    rhs, want = oracle_solutions[name]
    s = factorized(nlp, hip_schur(nlp, gctx, device_kkt_ops=True, spmv_row_threshold=T))
    k = s.kkt
    try:
        if name == "no_inequalities":
            assert k.n_ineq == 0
        if name == "no_equalities":
            assert k.nc_eq == 0 and k.blk == k.nv
        if name == "empty_upper_side":
            assert len(k.ind_ub) == 0 and len(k.ind_lb) > 0
        if name == "odd":
            assert len(np.intersect1d(k.ind_lb, k.ind_ub)) > 0
        wm, wh = s.d.copy(), s.d.copy()
        wm.values[:] = rhs
        wh.values[:] = rhs
        k.solve_kkt_ordered(wm)
        k.solve_kkt(wh)                                            # device_kkt_ops: mnk_schur_solve_kkt on a host vector
        assert same_bits(wh.values, wm.values, "solve_kkt vs mirror")
        wd = dev(gctx, rhs)
        k.solve_kkt_device(wd)                                     # ... and on a device tensor: the same bits
        assert same_bits(host(gctx, wd), wh.values, "device tensor vs host vector")
        assert np.abs(wh.values - want).max() <= 1e-9 * np.abs(want).max()
    finally:
        k.close()


# ------------------------------------------------------------------------------------------------ mul!, jtprod!, mul_hess_blk!
def product_system(p, ctx, T, ind_lb, ind_ub):
    from madnlp_jl_amd.schur_kkt import SchurComplementKKTSystem
    return SchurComplementKKTSystem(p["n"], p["m"], p["jac_I"], p["jac_J"], p["hess_I"], p["hess_J"], p["ind_ineq"], p["ind_eq"], ind_lb, ind_ub,
                                    p["ns"], p["nv"], p["nd"], p["nc"], ctx=ctx, device_kkt_ops=True, spmv_row_threshold=T)


def fill(k, p, seed, dyadic):
    """Values of every field the products read; dyadic: powers of two on the diagonals and in the bound terms."""
    rng = np.random.default_rng(seed)
    npr, nlb, nub = len(k.pr_diag), len(k.ind_lb), len(k.ind_ub)
    if dyadic:
        k.hess[:], k.jac[:] = dyadic_values(p, seed)
        pw = lambda lo, hi, cnt: 2.0 ** rng.integers(lo, hi + 1, cnt)  # noqa: E731
        k.reg[:] = pw(-4, 0, npr)
        k.pr_diag[:] = pw(-4, 2, npr)
        k.du_diag[:] = -pw(-4, -1, k.m)
        k.l_diag[:], k.u_diag[:] = -pw(-3, 0, nlb), -pw(-3, 0, nub)
        k.l_lower[:], k.u_lower[:] = pw(-2, 2, nlb), pw(-2, 2, nub)
    else:
        k.hess[:], k.jac[:] = rng.standard_normal(len(k.hess)), rng.standard_normal(len(k.jac))
        k.reg[:] = rng.uniform(1e-4, 1.0, npr)
        k.pr_diag[:] = rng.uniform(0.1, 10.0, npr)
        k.du_diag[:] = -rng.uniform(1e-8, 1e-2, k.m)
        k.l_diag[:], k.u_diag[:] = -rng.uniform(1e-2, 1.0, nlb), -rng.uniform(1e-2, 1.0, nub)
        k.l_lower[:], k.u_lower[:] = rng.uniform(1e-3, 1.0, nlb), rng.uniform(1e-3, 1.0, nub)
    k.stage.assemble(k.hess, k.jac, k.pr_diag, k.du_diag)         # the products read the values of the last assemble
    k.upload_barrier_terms()
    return rng


def vector(k, rng, dyadic):
    from madnlp_jl_amd.kkt import UnreducedKKTVector
    w = UnreducedKKTVector.from_kkt(k)
    w.values[:] = dyadic_vector(rng, len(w.values)) if dyadic else rng.standard_normal(len(w.values))
    return w


PRODUCT_PATTERNS = sorted(MODELS) + ["general"]


@pytest.mark.parametrize("T", THRESHOLDS, ids=T_IDS)
@pytest.mark.parametrize("name", PRODUCT_PATTERNS)
def test_products_equal_the_ordered_mirror_and_the_exact_answer(gctx, models, name, T):
    p = pattern(**GENERAL) if name == "general" else model_pattern(models[name])
    npr = p["n"] + len(p["ind_ineq"])
    ind_lb = np.arange(0, npr, 2)
    ind_ub = np.zeros(0, dtype=np.int64) if name == "empty_upper_side" else np.arange(0, npr, 3)   # both bounds on every sixth entry
    k = product_system(p, gctx, T, ind_lb, ind_ub)
    try:
        if name in ("dense_design", "crafted_columns", "general") and T is None:
            ptr, _, _ = row_lists(p, 1)
            assert (np.diff(ptr) > 64).any() and (np.diff(ptr) <= 64).any()            # both kernels at the default threshold
        for dyadic in (False, True):
            rng = fill(k, p, 17, dyadic)
            # ---- mul!
            if dyadic:
                K = unreduced_matrix(p, k.hess, k.jac, k.reg, k.du_diag, k.ind_lb, k.ind_ub, k.l_diag, k.u_diag, k.l_lower, k.u_lower)
            for alpha, beta in ALPHA_BETA:
                x, w0 = vector(k, rng, dyadic), vector(k, rng, dyadic)
                wm, wh = w0.copy(), w0.copy()
                k.mul_ordered(wm, x, alpha, beta)
                k.mul(wh, x, alpha, beta)                          # device_kkt_ops: mnk_schur_mul on host vectors
                assert same_bits(wh.values, wm.values, f"mul vs mirror, dyadic={dyadic}, alpha, beta = {alpha}, {beta}")
                wd = dev(gctx, w0.values)
                k.mul_device(wd, dev(gctx, x.values), alpha, beta)
                assert np.array_equal(host(gctx, wd), wh.values)
                if dyadic:
                    assert same_bits(wh.values, exact_axpby(K, x.values, w0.values, alpha, beta), f"mul vs exact, alpha, beta = {alpha}, {beta}")
            # ---- jtprod!
            xv = dyadic_vector(rng, k.m) if dyadic else rng.standard_normal(k.m)
            ym, yh = np.full(npr, np.nan), np.full(npr, np.nan)
            k.jtprod_ordered(ym, xv)
            k.jtprod(yh, xv)
            assert same_bits(yh, ym, f"jtprod vs mirror, dyadic={dyadic}")
            yd = dev(gctx, np.zeros(npr))
            k.jtprod_device(yd, dev(gctx, xv))
            assert np.array_equal(host(gctx, yd), yh)
            if dyadic:
                want = np.concatenate((exact_spmv(*row_lists(p, 1), k.jac, xv, 1, 2), -xv[k.ind_ineq]))
                assert np.array_equal(yh, want)
            # ---- mul_hess_blk!
            t = dyadic_vector(rng, npr) if dyadic else rng.standard_normal(npr)
            bm, bh = np.full(npr, np.nan), np.full(npr, np.nan)
            k.mul_hess_blk_ordered(bm, t)
            k.mul_hess_blk(bh, t)
            assert same_bits(bh, bm, f"mul_hess_blk vs mirror, dyadic={dyadic}")
            bd = dev(gctx, np.zeros(npr))
            k.mul_hess_blk_device(bd, dev(gctx, t))
            assert np.array_equal(host(gctx, bd), bh)
            if dyadic:
                want = np.concatenate((exact_spmv(*row_lists(p, 2), k.hess, t[:p["n"]]), np.zeros(npr - p["n"]))) + t * k.pr_diag
                assert np.array_equal(bh, want)
        # compress_jacobian! / compress_hessian!: fresh values reach the products without an assemble (the interior-point loop calls
        # jtprod! on the new Jacobian before it builds the next KKT system)
        k.jac[:], k.hess[:] = rng.standard_normal(len(k.jac)), rng.standard_normal(len(k.hess))
        k.compress_jacobian()
        k.compress_hessian()
        assert np.array_equal(k.jtprod(np.zeros(npr), xv), k.jtprod_ordered(np.zeros(npr), xv))
        assert np.array_equal(k.mul_hess_blk(np.zeros(npr), t), k.mul_hess_blk_ordered(np.zeros(npr), t))
    finally:
        k.close()


# ------------------------------------------------------------------------------------------------ feeders
@pytest.mark.parametrize("name", ["odd", "empty_upper_side"])
def test_device_feeders_give_the_host_diagonals_and_the_same_schur_complement(gctx, models, name):
    nlp = models[name]
    s = factorized(nlp, hip_schur(nlp, gctx, device_kkt_ops=True))
    k = s.kkt
    try:
        S_host = host(gctx, k.aug_com).copy()
        fields = ("pr_diag", "du_diag", "reg", "l_diag", "u_diag", "l_lower", "u_lower")
        for on_device in (False, True):
            vecs = [np.ascontiguousarray(v, dtype=np.float64) for v in (s.x, s.xl, s.xu, s.zl, s.zu)]
            if on_device:
                vecs = [dev(gctx, v) for v in vecs]
            k.set_aug_diagonal_device(*vecs, s.opt.default_primal_regularization, s.opt.default_dual_regularization)
            got = k.get_diagonals_device()
            for f in fields:
                assert same_bits(got[f], getattr(k, f), f)
            k.build_kkt_device()
            assert np.array_equal(host(gctx, k.aug_com), S_host)
        k.regularize_diagonal_device(1e-4, 1e-8)
        k.regularize_diagonal(1e-4, 1e-8)
        got = k.get_diagonals_device()
        for f in fields:
            assert same_bits(got[f], getattr(k, f), f)
        k.build_kkt_device()
        S_dev = host(gctx, k.aug_com).copy()
        k.build_kkt()
        assert np.array_equal(host(gctx, k.aug_com), S_dev)
    finally:
        k.close()


# ------------------------------------------------------------------------------------------------ contract
def test_calls_out_of_order_are_refused_by_name_and_the_handle_works_afterwards(gctx, models):
    from madnlp_jl_amd import _lib as L
    from madnlp_jl_amd.kkt import UnreducedKKTVector
    from madnlp_jl_amd.linear_solver import SolveException
    from madnlp_jl_amd.schur import SchurDenseStage
    nlp = models["odd"]
    p = model_pattern(nlp)
    npr = p["n"] + len(p["ind_ineq"])
    blk = p["nv"] + len(p["ind_eq"]) // p["ns"]
    stage = SchurDenseStage([np.eye(blk)] * p["ns"], [np.zeros((p["nd"], blk))] * p["ns"], np.eye(p["nd"]), p["nd"], blk, ctx=gctx)
    lib, h = L.lib(), stage._h
    err = lambda: lib.mnk_last_error_string().decode()  # noqa: E731
    N = npr + p["m"] + 2
    w, x = np.zeros(N), np.ones(N)
    lb, ub = np.array([0], dtype=np.int64), np.array([1], dtype=np.int64)
    one, neg = np.ones(npr), -np.ones(npr)
    try:
        assert lib.mnk_schur_solve_kkt(h, w.ctypes.data, L.MNK_HOST) != 0 and "call mnk_schur_set_structure first" in err()
        stage.set_structure(p["n"], p["m"], p["nv"], p["nc"], p["hess_I"], p["hess_J"], p["jac_I"], p["jac_J"], p["ind_ineq"], p["ind_eq"])
        for call in (lambda: lib.mnk_schur_solve_kkt(h, w.ctypes.data, L.MNK_HOST),
                     lambda: lib.mnk_schur_mul(h, w.ctypes.data, x.ctypes.data, 1.0, 0.0, L.MNK_HOST)):
            assert call() != 0 and "call mnk_schur_set_bounds first" in err()
        assert lib.mnk_schur_set_barrier_terms(h, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                               L.MNK_HOST) != 0
        assert "mnk_schur_set_barrier_terms: call mnk_schur_set_bounds first" in err()
        assert lib.mnk_schur_regularize_diagonal(h, 1.0, 1.0) != 0 and "call mnk_schur_set_bounds first" in err()
        assert lib.mnk_schur_set_bounds(h, 1, lb.ctypes.data, 1, ub.ctypes.data, 0) == 0
        assert lib.mnk_schur_regularize_diagonal(h, 1.0, 1.0) != 0 and "call mnk_schur_set_aug_diagonal first" in err()
        assert lib.mnk_schur_assemble(h, None, None, None, None, L.MNK_HOST) != 0
        for call in (lambda: lib.mnk_schur_solve_kkt(h, w.ctypes.data, L.MNK_HOST),
                     lambda: lib.mnk_schur_mul(h, w.ctypes.data, x.ctypes.data, 1.0, 0.0, L.MNK_HOST)):
            assert call() != 0 and "call mnk_schur_set_barrier_terms first" in err()
        assert lib.mnk_schur_set_barrier_terms(h, one.ctypes.data, neg.ctypes.data, neg.ctypes.data, one.ctypes.data, one.ctypes.data,
                                               L.MNK_HOST) == 0
        for call in (lambda: lib.mnk_schur_solve_kkt(h, w.ctypes.data, L.MNK_HOST),
                     lambda: lib.mnk_schur_mul(h, w.ctypes.data, x.ctypes.data, 1.0, 0.0, L.MNK_HOST),
                     lambda: lib.mnk_schur_jtprod(h, w.ctypes.data, x.ctypes.data, L.MNK_HOST),
                     lambda: lib.mnk_schur_mul_hess_blk(h, w.ctypes.data, x.ctypes.data, L.MNK_HOST)):
            assert call() != 0 and "call mnk_schur_assemble first" in err()
    finally:
        stage.close()
    # the same handle kind, calls in order: it works (and a refusal on the way leaves it working)
    s = factorized(nlp, hip_schur(nlp, gctx, device_kkt_ops=True))
    k = s.kkt
    try:
        assert lib.mnk_schur_mul(k._h, None, None, 1.0, 0.0, L.MNK_HOST) != 0 and "mnk_schur_mul: NULL argument" in err()
        wm, wh = s.d.copy(), s.d.copy()
        wm.values[:] = np.random.default_rng(4).standard_normal(wm.values.shape)
        wh.values[:] = wm.values
        k.solve_kkt_ordered(wm)
        k.solve_kkt(wh)
        assert np.array_equal(wh.values, wm.values)
        assert isinstance(wh, UnreducedKKTVector) and SolveException is not None
    finally:
        k.close()


def test_a_sharded_handle_is_refused(gctx, models):
    from madnlp_jl_amd import _lib as L
    from madnlp_jl_amd.schur import SchurDenseStage
    nlp = models["odd"]
    p = model_pattern(nlp)
    blk = p["nv"] + len(p["ind_eq"]) // p["ns"]
    lib = L.lib()
    w = np.zeros(p["n"] + 2 * p["m"] + 8)
    lb = np.array([0], dtype=np.int64)
    for kw in (dict(ns_global=p["ns"], local_scen=[0, 2], own_design=True), dict(own_design=False)):
        nl = len(kw.get("local_scen", range(p["ns"])))
        stage = SchurDenseStage([np.eye(blk)] * nl, [np.zeros((p["nd"], blk))] * nl, np.eye(p["nd"]), p["nd"], blk, ctx=gctx)
        try:
            stage.set_structure(p["n"], p["m"], p["nv"], p["nc"], p["hess_I"], p["hess_J"], p["jac_I"], p["jac_J"], p["ind_ineq"], p["ind_eq"],
                                **kw)
            stage.assemble(np.ones(len(p["hess_I"])), np.ones(len(p["jac_I"])), np.ones(p["n"] + len(p["ind_ineq"])), -np.ones(p["m"]))
            for rc in (lib.mnk_schur_set_bounds(stage._h, 1, lb.ctypes.data, 0, None, 0),
                       lib.mnk_schur_solve_kkt(stage._h, w.ctypes.data, L.MNK_HOST),
                       lib.mnk_schur_mul(stage._h, w.ctypes.data, w.ctypes.data, 1.0, 0.0, L.MNK_HOST),
                       lib.mnk_schur_jtprod(stage._h, w.ctypes.data, w.ctypes.data, L.MNK_HOST),
                       lib.mnk_schur_mul_hess_blk(stage._h, w.ctypes.data, w.ctypes.data, L.MNK_HOST)):
                assert rc != 0
                msg = lib.mnk_last_error_string().decode()
                assert "single rank only" in msg and "sharded" in msg
        finally:
            stage.close()


# ------------------------------------------------------------------------------------------------ IPM
IPM_MODELS = {
    "coupled": lambda: coupled_quadratic([4.0, 6.0, 8.0]), "two_by_two": two_by_two, "several": several_recourse_and_design,
    "inactive": lambda: coupled_quadratic([3.0, 7.0], d_target=5.0, lcon=-100.0, ucon=100.0),
    "random8": lambda: random_twostage_qp(ns=8, nv=40, nd=12, nc=10, nc_eq=4, seed=7),
}


@pytest.mark.parametrize("which", sorted(IPM_MODELS))
def test_ipm_with_device_kkt_ops_takes_the_iterations_of_the_default_path(gctx, which):
    nlp = IPM_MODELS[which]()
    ref = solve(nlp, hip_schur(nlp, gctx))
    got = solve(nlp, hip_schur(nlp, gctx, device_kkt_ops=True))
    try:
        assert got.kkt.device_kkt_ops and not ref.kkt.device_kkt_ops
        assert got.status == ref.status == "SOLVE_SUCCEEDED"
        assert got.cnt.k == ref.cnt.k
        assert np.abs(got.x[:nlp.n] - ref.x[:nlp.n]).max() <= 1e-6
        assert abs(got.obj_val - ref.obj_val) <= 1e-8 * max(1.0, abs(ref.obj_val))
    finally:
        got.kkt.close()
        ref.kkt.close()

"""Long inequality rows of the Schur stage's device-side assembly (csrc/schur.hip: schur_gram_stage_kernel, schur_gram_kernel):
a row with more COO entries than the Gram row threshold T adds no pairs to the source lists; J' D J of such rows is staged into
dense zero-padded operands and added to A_k, C_dk and S0 as weighted Gram products on the fp64 matrix cores.

EXACT DATA (Jacobian entries integers in -3..3, small integer Hessian and diagonals, du_diag = 0 on the inequality rows so that
D = Sigma_s drawn from {0.5, 1, 2, 4}): every product and every partial sum is a dyadic number of a few bits, so the result does
not depend on the summation order and `np.array_equal` against the numpy computation below (`dense_blocks`) is the requirement --
for both triangles of every A_k, its equality border (the guarded epilogue writes nothing outside [0:nv, 0:nv]), every C_dk and S0.
REAL DATA: the reference is exact rational arithmetic on the double inputs (`fractions.Fraction` makes the integers, the sums run
on them), the requirement the textbook bound |hip - exact| <= (L + 2) 2^-53 sum|terms| of an entry summed from L terms (source
list terms plus long rows) whose products are rounded once.  The weight D of a row is the double that
`Sigma_s / (1 - Sigma_d Sigma_s)` gives operation by operation (IEEE: the bits of schur_condense_weights_kernel), taken exactly."""
from fractions import Fraction

import numpy as np
import pytest

from madnlp_jl_amd.ipm import IPMOptions, MadNLPSolver
from madnlp_jl_amd.problems import random_twostage_qp
from oracle.schur_kkt import SchurComplementKKTSystem as OracleSchur

pytestmark = pytest.mark.gpu
NEVER = 2 ** 63 - 1


@pytest.fixture(scope="module")
def gctx():
    torch = pytest.importorskip("torch")
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


# --------------------------------------------------------------------------- structures and values
def structure(ns, nv, nd, nc, nc_eq, Mv=None, Md=None, dups=()):
    """Two-stage COO patterns (0-based): row i of every scenario touches the recourse columns of Mv[i] and the design columns of
    Md[i] (one mask for all scenarios; None: all), row-major, recourse entries first; `dups`: (row i, position in the row) of
    entries that appear once more at the end of the COO lists.  The Hessian: the diagonal, one off-diagonal entry inside every
    scenario, one coupling entry per scenario and one off-diagonal design entry (given in the upper triangle)."""
    Mv = np.ones((nc, nv), bool) if Mv is None else Mv
    Md = np.ones((nc, nd), bool) if Md is None else Md
    n, m, off = ns * nv + nd, ns * nc, ns * nv
    jI, jJ = [], []
    for k in range(ns):
        for i in range(nc):
            cols = np.concatenate((k * nv + np.nonzero(Mv[i])[0], off + np.nonzero(Md[i])[0]))
            jI.append(np.full(len(cols), k * nc + i)); jJ.append(cols)
    jI, jJ = np.concatenate(jI), np.concatenate(jJ)
    for i, pos in dups:
        for k in range(ns):
            e = np.nonzero(jI == k * nc + i)[0][pos]
            jI, jJ = np.append(jI, jI[e]), np.append(jJ, jJ[e])
    hI, hJ = list(range(n)), list(range(n))
    for k in range(ns):
        hI += [k * nv + nv - 1, off + nd - 1]; hJ += [k * nv, k * nv + 1 % nv]
    if nd > 1:
        hI.append(off); hJ.append(off + nd - 1)
    ind_eq = np.array([k * nc + i for k in range(ns) for i in range(nc_eq)], dtype=np.int64)
    ind_ineq = np.array([k * nc + i for k in range(ns) for i in range(nc_eq, nc)], dtype=np.int64)
    return dict(ns=ns, nv=nv, nd=nd, nc=nc, nc_eq=nc_eq, n=n, m=m, blk=nv + nc_eq, hI=np.array(hI), hJ=np.array(hJ), jI=jI, jJ=jJ,
                ind_eq=ind_eq, ind_ineq=ind_ineq)


def exact_values(st, seed):
    rng = np.random.default_rng(seed)
    n, m, ni = st["n"], st["m"], len(st["ind_ineq"])
    hess = rng.integers(-2, 3, len(st["hI"])).astype(float)
    hess[:n] = rng.integers(1, 5, n)
    jac = rng.integers(-3, 4, len(st["jI"])).astype(float)
    pr = np.concatenate((rng.integers(0, 4, n).astype(float), rng.choice([0.5, 1.0, 2.0, 4.0], ni)))
    du = -rng.integers(0, 3, m).astype(float)
    du[st["ind_ineq"]] = 0.0
    return hess, jac, pr, du


def real_values(st, seed):
    rng = np.random.default_rng(seed)
    n, m, ni = st["n"], st["m"], len(st["ind_ineq"])
    hess = rng.standard_normal(len(st["hI"]))
    jac = rng.standard_normal(len(st["jI"]))
    pr = np.concatenate((rng.uniform(0.1, 3.0, n), rng.uniform(0.05, 20.0, ni)))
    du = -rng.uniform(1e-3, 0.5, m)
    return hess, jac, pr, du


def weights(st, pr, du):
    """D of every inequality row, operation by operation as schur_condense_weights_kernel rounds it."""
    Ss, Sd = pr[st["n"]:], du[st["ind_ineq"]]
    return Ss / (1.0 - Sd * Ss)


def dense_blocks(st, hess, jac, pr, du, local=None, own_design=True, exact=False):
    """A_k, C_dk of the local scenarios and S0 from dense J and H.  `exact`: the values are Python integers (object arrays) and the
    weights come from st["D_exact"]."""
    ns, nv, nd, nc, n, m, blk = (st[k] for k in ("ns", "nv", "nd", "nc", "n", "m", "blk"))
    local = list(range(ns)) if local is None else local
    off = ns * nv
    zero = 0 if exact else 0.0
    J = np.full((m, n), zero, dtype=object if exact else float)
    H = np.full((n, n), zero, dtype=J.dtype)
    for e in range(len(jac)):
        J[st["jI"][e], st["jJ"][e]] = J[st["jI"][e], st["jJ"][e]] + jac[e]
    for e in range(len(hess)):
        i, j = max(st["hI"][e], st["hJ"][e]), min(st["hI"][e], st["hJ"][e])
        H[i, j] = H[i, j] + hess[e]
        if i != j:
            H[j, i] = H[j, i] + hess[e]
    D = st["D_exact"] if exact else weights(st, pr, du)
    slack_of = {int(r): p for p, r in enumerate(st["ind_ineq"])}
    S0 = np.full((nd, nd), zero, dtype=J.dtype)
    if own_design:
        S0 = S0 + H[off:, off:]
        for j in range(nd):
            S0[j, j] = S0[j, j] + pr[off + j]
    A, Cd = [], []
    for k in local:
        v = slice(k * nv, (k + 1) * nv)
        E = [r for r in st["ind_eq"] if r // nc == k]
        Ir = [r for r in st["ind_ineq"] if r // nc == k]
        Dk = np.array([D[slack_of[int(r)]] for r in Ir], dtype=J.dtype)
        JvI, JdI = J[Ir, v], J[Ir, off:]
        Ak = np.full((blk, blk), zero, dtype=J.dtype)
        Ak[:nv, :nv] = H[v, v] + JvI.T @ (Dk[:, None] * JvI)
        for j in range(nv):
            Ak[j, j] = Ak[j, j] + pr[k * nv + j]
        Ak[nv:, :nv] = J[E, v]
        Ak[:nv, nv:] = J[E, v].T
        for q, r in enumerate(E):
            Ak[nv + q, nv + q] = du[r]
        Ck = np.full((nd, blk), zero, dtype=J.dtype)
        Ck[:, :nv] = H[off:, v] + JdI.T @ (Dk[:, None] * JvI)
        Ck[:, nv:] = J[E, off:].T
        S0 = S0 + JdI.T @ (Dk[:, None] * JdI)
        A.append(Ak); Cd.append(Ck)
    return A, Cd, S0


def make_stage(ctx, st, T, local=None, own_design=True):
    from madnlp_jl_amd.schur import SchurDenseStage
    nl = st["ns"] if local is None else len(local)
    stage = SchurDenseStage([np.eye(st["blk"])] * nl, [np.zeros((st["nd"], st["blk"]))] * nl, np.eye(st["nd"]), st["nd"], st["blk"], ctx=ctx)
    stage.set_structure(st["n"], st["m"], st["nv"], st["nc"], st["hI"], st["hJ"], st["jI"], st["jJ"], st["ind_ineq"], st["ind_eq"],
                        ns_global=st["ns"], local_scen=local, own_design=own_design, gram_row_threshold=T)
    return stage


def device_blocks(stage, vals):
    stage.assemble(*vals)
    blocks = [stage.get_block(k) for k in range(stage.ns)]
    return [b[0] for b in blocks], [b[1] for b in blocks], stage.get_s0()


def assert_blocks_equal(got, want, nv):
    (A, Cd, S0), (Aw, Cw, S0w) = got, want
    assert len(A) == len(Aw)
    for k in range(len(A)):
        assert np.array_equal(A[k][:nv, :nv], Aw[k][:nv, :nv]), f"A_{k}"
        assert np.array_equal(A[k], Aw[k]), f"border of A_{k}"
        assert np.array_equal(Cd[k], Cw[k]), f"C_d{k}"
    assert np.array_equal(S0, S0w), "S0"


def row_lengths(st):
    ln = np.zeros(st["m"], dtype=np.int64)
    np.add.at(ln, st["jI"], 1)
    return ln[st["ind_ineq"]]


# --------------------------------------------------------------------------- exact data
SHAPES = {
    "k_tail_two_tiles": dict(ns=3, nv=70, nd=37, nc=23, nc_eq=4),      # R = 19; 70, 37: no multiples of 16 / 64; nv spans two tiles
    "below_one_mfma_tile": dict(ns=2, nv=5, nd=3, nc=6, nc_eq=1),
    "exact_tile_multiples": dict(ns=2, nv=64, nd=64, nc=36, nc_eq=4),  # R = 32: two k-tiles
}


def sparse_structure():
    """Shape 1 with one sparse mask for all scenarios, one inequality row with design entries only, one with recourse entries only
    and two duplicated COO entries in a long row."""
    s = SHAPES["k_tail_two_tiles"]
    rng = np.random.default_rng(3)
    Mv, Md = rng.random((s["nc"], s["nv"])) < 0.2, rng.random((s["nc"], s["nd"])) < 0.4
    Mv[:, 0] = True                       # (no empty row)
    Mv[6], Md[6] = False, True            # 37 design entries
    Mv[9], Md[9] = True, False            # 70 recourse entries
    st = structure(Mv=Mv, Md=Md, dups=((9, 3), (9, 40)), **s)
    return st, int(np.median(row_lengths(st)))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_row_long_equals_the_numpy_blocks_exactly(gctx, shape):
    st = structure(**SHAPES[shape])
    vals = exact_values(st, 1)
    stage = make_stage(gctx, st, 0)
    stats = stage.assembly_stats()
    R = st["nc"] - st["nc_eq"]
    assert stats[2] == st["ns"] * R and stats[4] == 0
    assert stats[3] == 2 * st["ns"] * (-(-R // 16) * 16) * ((-(-st["nv"] // 64) + -(-st["nd"] // 64)) * 64)
    assert_blocks_equal(device_blocks(stage, vals), dense_blocks(st, *vals), st["nv"])
    stage.close()


def test_long_and_short_rows_side_by_side(gctx):
    st, T = sparse_structure()
    ln = row_lengths(st)[:st["nc"] - st["nc_eq"]]
    assert ln[6 - st["nc_eq"]] == 37 > T and ln[9 - st["nc_eq"]] == 72 > T and (ln <= T).any() and (ln == T).any()
    vals = exact_values(st, 2)
    stage, all_long = make_stage(gctx, st, T), make_stage(gctx, st, 0)
    stats, stats0 = stage.assembly_stats(), all_long.assembly_stats()
    assert stats[2] == st["ns"] * int((ln > T).sum()) > 0 and stats[4] == T
    assert stats[0] > stats0[0]           # the short rows' pairs are in the lists (at T = 0 no inequality row has any)
    want = dense_blocks(st, *vals)
    assert_blocks_equal(device_blocks(stage, vals), want, st["nv"])
    assert_blocks_equal(device_blocks(all_long, vals), want, st["nv"])
    stage.close(); all_long.close()


def test_two_shards_add_up_to_the_single_stage(gctx):
    st = structure(**SHAPES["k_tail_two_tiles"])
    vals = exact_values(st, 3)
    one = make_stage(gctx, st, 0)
    a = make_stage(gctx, st, 0, local=[0, 2], own_design=True)
    b = make_stage(gctx, st, 0, local=[1], own_design=False)
    A, Cd, S0 = device_blocks(one, vals)
    Aa, Ca, Sa = device_blocks(a, vals)
    Ab, Cb, Sb = device_blocks(b, vals)
    assert_blocks_equal((A, Cd, S0), dense_blocks(st, *vals), st["nv"])
    for k, (Ak, Ck) in zip((0, 2, 1), list(zip(Aa, Ca)) + list(zip(Ab, Cb))):
        assert np.array_equal(Ak, A[k]) and np.array_equal(Ck, Cd[k]), k
    assert np.array_equal(Sa + Sb, S0)
    assert np.array_equal(Sb, dense_blocks(st, *vals, local=[1], own_design=False)[2])
    for s in (one, a, b):
        s.close()


def test_assembling_again_gives_the_same_bits(gctx):
    st, T = sparse_structure()
    v1, v2 = real_values(st, 4), real_values(st, 5)
    stage = make_stage(gctx, st, T)
    first = device_blocks(stage, v1)
    assert_blocks_equal(device_blocks(stage, v1), first, st["nv"])
    other = device_blocks(stage, v2)
    assert not np.array_equal(other[2], first[2])
    assert_blocks_equal(device_blocks(stage, v1), first, st["nv"])
    fresh = make_stage(gctx, st, T)       # ... and another handle of the same structure
    assert_blocks_equal(device_blocks(fresh, v1), first, st["nv"])
    stage.close(); fresh.close()


# --------------------------------------------------------------------------- real data against exact rational arithmetic
def to_int(a, S):
    """The doubles of `a` times 2^S as Python integers (exact: S covers every denominator)."""
    out = np.empty(a.size, dtype=object)
    for i, x in enumerate(np.asarray(a, dtype=float).ravel()):
        f = Fraction(float(x)) * (1 << S)
        assert f.denominator == 1
        out[i] = f.numerator
    return out.reshape(np.shape(a))


def test_real_data_within_the_summation_bound_of_the_exact_result(gctx):
    s = SHAPES["k_tail_two_tiles"]
    st = structure(**s)
    hess, jac, pr, du = real_values(st, 6)
    D = weights(st, pr, du)
    stage = make_stage(gctx, st, 0)
    A, Cd, S0 = device_blocks(stage, (hess, jac, pr, du))
    stage.close()
    # exact: J, D as integers (times 2^SJ, 2^SD), the Hessian and diagonal terms times 2^(2 SJ + SD), the blocks by integer
    # matrix products; `abs` the same sums over the absolute values of the terms
    SJ = SD = 1100
    ST = 2 * SJ + SD
    exact, absum = {}, {}
    for name, f in (("exact", lambda a: a), ("abs", np.abs)):
        sti = dict(st, D_exact=to_int(f(D), SD))
        blocks = dense_blocks(sti, to_int(f(hess), ST), to_int(f(jac), SJ), to_int(f(pr), ST), to_int(f(du), ST), exact=True)
        (exact if name == "exact" else absum).update(A=blocks[0], C=blocks[1], S0=blocks[2])
    # L of an entry: its source-list terms (Hessian entries and diagonal terms) plus the long rows summed into it
    ns, nv, nd, R = s["ns"], s["nv"], s["nd"], s["nc"] - s["nc_eq"]
    cnt = dense_blocks(st, np.ones(len(hess)), np.zeros(len(jac)), np.ones(len(pr)), np.zeros(len(du)))
    worst = 0.0
    def check(hip, ex, ab, L):
        nonlocal worst
        for idx in np.ndindex(hip.shape):
            err = abs(Fraction(float(hip[idx])) * (1 << ST) - int(ex[idx]))
            bound = Fraction(int(L[idx]) + 2, 1 << 53) * int(ab[idx])
            if bound > 0:
                worst = max(worst, float(err / bound))
            assert err <= bound, (idx, float(err) / 2.0 ** ST, float(bound) / 2.0 ** ST)
    for k in range(ns):
        check(A[k][:nv, :nv], exact["A"][k][:nv, :nv], absum["A"][k][:nv, :nv], cnt[0][k][:nv, :nv] + R)
        check(Cd[k][:, :nv], exact["C"][k][:, :nv], absum["C"][k][:, :nv], cnt[1][k][:, :nv] + R)
    check(S0, exact["S0"], absum["S0"], cnt[2] + ns * R)
    print(f"largest |hip - exact| / bound = {worst:.3f}")


# --------------------------------------------------------------------------- unchanged behaviour
def nlp_structure(nlp):
    eq = np.nonzero(nlp.lcon == nlp.ucon)[0].astype(np.int64)
    ineq = np.nonzero(nlp.lcon != nlp.ucon)[0].astype(np.int64)
    return dict(ns=nlp.ns, nv=nlp.nv, nd=nlp.nd, nc=nlp.nc, nc_eq=len(eq) // nlp.ns, n=nlp.n, m=nlp.m, blk=nlp.nv + len(eq) // nlp.ns,
                hI=np.asarray(nlp.hess_I), hJ=np.asarray(nlp.hess_J), jI=np.asarray(nlp.jac_I), jJ=np.asarray(nlp.jac_J), ind_eq=eq, ind_ineq=ineq)


def test_short_rows_keep_the_pair_path_and_its_bits_at_the_default(gctx):
    st = nlp_structure(random_twostage_qp(ns=4, nv=20, nd=6, nc=7, nc_eq=3, seed=11))
    vals = real_values(st, 7)
    dflt, never = make_stage(gctx, st, None), make_stage(gctx, st, NEVER)
    sd, sn = dflt.assembly_stats(), never.assembly_stats()
    assert sd[2] == 0 and sd[3] == 0 and sd[4] >= 64 and sn[4] == NEVER and sd[:2] == sn[:2]
    assert_blocks_equal(device_blocks(dflt, vals), device_blocks(never, vals), st["nv"])
    dflt.close(); never.close()


# --------------------------------------------------------------------------- the interior-point loop
def solve(nlp, factory):
    s = MadNLPSolver(nlp, factory, IPMOptions(), sparse=True)
    s.solve()
    return s


@pytest.mark.parametrize("case", ["dense_rows_at_the_default", "short_rows_at_zero"])
def test_ipm_on_the_gram_path_matches_the_oracle_schur_system(gctx, case):
    from madnlp_jl_amd.schur_kkt import SchurComplementKKTSystem
    if case == "dense_rows_at_the_default":
        nlp, T = random_twostage_qp(ns=3, nv=70, nd=37, nc=23, nc_eq=4, seed=5), None      # rows of 107 entries
    else:
        nlp, T = random_twostage_qp(ns=4, nv=20, nd=6, nc=24, nc_eq=3, seed=11), 0

    def hip(info):
        return SchurComplementKKTSystem(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"], info["ind_eq"],
                                        info["ind_lb"], info["ind_ub"], ctx=gctx, gram_row_threshold=T, **nlp.schur_opts())

    def oracle(info):
        return OracleSchur(info["n"], info["m"], nlp.jac_I, nlp.jac_J, nlp.hess_I, nlp.hess_J, info["ind_ineq"], info["ind_eq"],
                           info["ind_lb"], info["ind_ub"], **nlp.schur_opts())

    sch, orc = solve(nlp, hip), solve(nlp, oracle)
    assert sch.kkt.stage.assembly_stats()[2] > 0
    assert sch.status == orc.status == "SOLVE_SUCCEEDED"
    assert sch.cnt.k == orc.cnt.k
    assert np.abs(sch.x[:nlp.n] - orc.x[:nlp.n]).max() <= 1e-6
    c = nlp.cons(sch.x[:nlp.n])
    assert (c >= nlp.lcon - 1e-6).all() and (c <= nlp.ucon + 1e-6).all()
    sch.kkt.close()

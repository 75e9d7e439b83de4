"""Pivot breakdowns with exact answers (-m gpu), at every position the 64-column leaf and the schedules treat differently.

The matrices of tests/exact_factor.py have LDL^T factors that are exact in fp64 whatever the blocking and the summation order;
a breakdown at column k is an edit of d_k.  So the verdict of factorize! -- dpotrf's info, the inertia, the early rejection's
column, which pivots are recorded as zero -- has one right answer, checked exactly through the per-panel schedule
(N <= 700) and the task-DAG schedule (N >= 1280; 5400 is just above dag_deep_rows), the dense and the lower-CSC inputs,
batches and the leading-block probe.  Where exactness is lost (a pivot replaced under pivot_tol, NaN / Inf entries) the
expected answer is the plain scalar reference of the static-pivot LDL^T (exact_factor.scalar_ldl)."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import torch

import madnlp_jl_amd as mj
from oracle.lapack_cpu import BUNCHKAUFMAN, LapackCPUSolver
from tests.exact_factor import TINY, make_exact, scalar_ldl, with_pivot

pytestmark = pytest.mark.gpu

PANEL_SIZES = [5, 63, 65, 700]
DAG_SIZES = [1300, 2600, 5400]
ULP4 = 4 * np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()


def _columns(n):
    cols = [0, 1, 2, 3, 4, 15, 16, 61, 62, 63, 64, 255, 256, 511, 512, n - 65, n - 64, n - 2, n - 1]
    return sorted({k for k in cols if 0 <= k < n})


def _kinds(case, k):
    """(kind, new d_k) of a breakdown at column k: a sign flip and a zero."""
    return [("neg", -abs(case.d[k])), ("zero", 0.0)]


def _tag(n, path, alg, kind, k):
    return f"N={n} path={path} alg={alg} kind={kind} col={k}"


class _Dense:
    """A solver on host dense input (column-major)."""
    path = "dense"

    def __init__(self, ctx, n, alg, **opts):
        self.M = mj.HipLinearSolver(np.zeros((n, n), order="F"), ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg))
        for key, v in opts.items():
            self.M.set_option(key, v)

    def factorize(self, case, pattern):
        self.M.A = case.A
        self.M.factorize()
        return self.M

    def close(self):
        self.M.close()


class _CSC(_Dense):
    """A solver on a host lower-CSC triple."""
    path = "csc"

    def factorize(self, case, pattern):
        self.M.A = case.lower_csc(pattern)
        self.M.factorize()
        return self.M


class _KKT:
    """A sparse condensed KKT system with m = 0 and Hessian tril(A), pr_diag = 0: K = A exactly (the aug_com path)."""
    path = "kkt"

    def __init__(self, ctx, n, alg, pattern, early_reject=True, **opts):
        colptr, rowval = pattern
        self.rows, self.cols = rowval.astype(np.int64), np.repeat(np.arange(n), np.diff(colptr))
        e = np.zeros(0, dtype=np.int64)
        self.k = mj.SparseCondensedKKTSystem(n, 0, e, e, self.rows, self.cols, e, e, e, ctx=ctx,
                                             opt_linear_solver=mj.HipSolverOptions(lapack_algorithm=alg), early_reject=early_reject)
        self.M = self.k.linear_solver
        for key, v in opts.items():
            self.M.set_option(key, v)

    def load(self, case):
        self.k.hess[:] = case.A[self.rows, self.cols]
        self.k.compress_hessian()
        self.k.build_kkt()

    def factorize(self, case, pattern=None):
        self.load(case)
        self.M.factorize()
        return self.M

    def close(self):
        self.k.close()


def _factor(M):
    """(L unit lower, D) of the solver, as torch tensors on the device."""
    Lt, D = M.get_factor_device()
    return torch.tril(Lt, -1) + torch.eye(M.n, dtype=torch.float64, device=Lt.device), D


def _exact_L(case, Lbase):
    """I + N on the device with the columns of the zero pivots zeroed (Lbase: that of the unedited matrix)."""
    z = torch.from_numpy(np.flatnonzero(case.d == 0.0)).to(Lbase.device)
    Lx = Lbase.clone()
    Lx[:, z] = 0.0
    Lx[z, z] = 1.0
    return Lx


def _check_exact_ldl(M, case, msg, Lbase):
    L, D = _factor(M)
    Dx = torch.from_numpy(case.d).to(D.device)
    assert torch.equal(D, Dx), msg + f": D differs at {torch.nonzero(D != Dx)[:4].flatten().tolist()}"
    Lx = _exact_L(case, Lbase)
    err = (L - Lx).abs() > ULP4 * Lx.abs()
    assert not bool(err.any()), msg + f": L off by more than 4 ulp at {torch.nonzero(err)[:4].tolist()}"


def _bwd(A, x, b):
    return np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())


# --------------------------------------------------------------------------------------------------------- the ladder
@pytest.mark.parametrize("n", PANEL_SIZES + DAG_SIZES)
def test_breakdown_ladder(ctx, n):
    """At every leaf position: CHOLESKY's info is k + 1 (dpotrf's) with inertia (0, N, 0); the static-pivot LDL^T
    (pivot_tol = 0) has the Sylvester inertia, D exactly d and L within 4 ulp of I + N (column k zero at a zero pivot) and
    solves to 1e-13 where nonsingular; BUNCHKAUFMAN reports the Sylvester counts from its static tier, LAPACK's inertia on
    nonsingular matrices whatever tier ends up factoring, and never accepts a singular one -- each through the dense and the
    lower-CSC input."""
    dev = torch.device("cuda", 0)
    base = make_exact(n, 1000 + n, positive=False)        # mixed signs: the inertia is not trivial
    pos = make_exact(n, 2000 + n)                          # positive definite: CHOLESKY and the singular BUNCHKAUFMAN cases
    Lbase = torch.from_numpy(base.L).to(dev)
    pat, ppat = base.lower_pattern(), pos.lower_pattern()
    rng = np.random.default_rng(n)
    solvers = []
    try:
        for P in (_Dense, _CSC):
            chol = P(ctx, n, mj.CHOLESKY)
            ldl = P(ctx, n, mj.LDL)
            bk_static = P(ctx, n, mj.BUNCHKAUFMAN, bk_fallback=0)
            bk = P(ctx, n, mj.BUNCHKAUFMAN)
            solvers += [chol, ldl, bk_static, bk]
            for k in [None] + _columns(n):
                cases = [("none", base, pos)] if k is None else \
                        [(kind, with_pivot(base, k, v), with_pivot(pos, k, -pos.d[k] if kind == "neg" else 0.0))
                         for kind, v in _kinds(base, k)]
                for kind, c, cp in cases:
                    tag = lambda alg: _tag(n, P.path, alg, kind, k)   # noqa: E731
                    # CHOLESKY
                    M = chol.factorize(cp, ppat)
                    assert M.info == cp.dpotrf_info() == (0 if k is None else k + 1), tag("CHOLESKY") + f": info {M.info}"
                    assert M.inertia() == ((n, 0, 0) if k is None else (0, n, 0)), tag("CHOLESKY")
                    if n <= 700:
                        assert lapack.dpotrf(cp.A, lower=1)[1] == M.info, tag("CHOLESKY")
                    # LDL, pivot_tol = 0
                    M = ldl.factorize(c, pat)
                    assert M.inertia() == c.inertia(), tag("LDL") + f": {M.inertia()} != {c.inertia()}"
                    _check_exact_ldl(M, c, tag("LDL"), Lbase)
                    if kind != "zero":
                        b = rng.standard_normal(n)
                        x = M.solve_linear_system(b.copy())
                        assert _bwd(c.A, x, b) <= 1e-13, tag("LDL") + f": backward error {_bwd(c.A, x, b):.2e}"
                    # BUNCHKAUFMAN: the static tier's counts; the default tiers on nonsingular / singular matrices
                    M = bk_static.factorize(c, pat)
                    assert M.inertia() == c.inertia(), tag("BUNCHKAUFMAN static") + f": {M.inertia()}"
                    if kind != "zero":
                        M = bk.factorize(c, pat)
                        ref = c.inertia()
                        if n <= 700:
                            r = LapackCPUSolver(np.asfortranarray(np.tril(c.A)), BUNCHKAUFMAN).factorize()
                            assert tuple(int(v) for v in r.inertia()) == ref, tag("LAPACK")
                        assert M.inertia() == ref, tag("BUNCHKAUFMAN") + f": {M.inertia()} != {ref}"
                    else:
                        M = bk.factorize(cp, ppat)
                        ine = M.inertia()
                        assert sum(ine) == n and not (ine[0] == n and ine[1] == 0), tag("BUNCHKAUFMAN singular") + f": {ine}"
    finally:
        for s in solvers:
            s.close()


@pytest.mark.parametrize("n", [65, 700, 1300])
def test_breakdowns_sharing_a_pivot_group(ctx, n):
    """Two breakdowns in one 4-pivot group (zero at k, negative at k + 2) and a breakdown followed by good pivots in its group
    (k at the group's first lane): LDL^T exact, CHOLESKY info at the first one."""
    dev = torch.device("cuda", 0)
    base = make_exact(n, 3000 + n, positive=False)
    Lbase = torch.from_numpy(base.L).to(dev)
    pos = make_exact(n, 4000 + n)
    ldl = _Dense(ctx, n, mj.LDL)
    chol = _Dense(ctx, n, mj.CHOLESKY)
    try:
        for k in sorted({0, 4, 60, 64, (n - 4) // 4 * 4}):
            if k + 2 >= n:
                continue
            for kind, edits in (("zero+neg", ((k, 0.0), (k + 2, None))), ("one-then-good", ((k, None),))):
                c, cp = base, pos
                for j, v in edits:
                    c = with_pivot(c, j, -abs(c.d[j]) if v is None else v)
                    cp = with_pivot(cp, j, -cp.d[j] if v is None else v)
                M = ldl.factorize(c, None)
                assert M.inertia() == c.inertia(), _tag(n, "dense", "LDL", kind, k)
                _check_exact_ldl(M, c, _tag(n, "dense", "LDL", kind, k), Lbase)
                M = chol.factorize(cp, None)
                assert M.info == k + 1 == cp.dpotrf_info(), _tag(n, "dense", "CHOLESKY", kind, k) + f": info {M.info}"
                if n <= 700:
                    assert lapack.dpotrf(cp.A, lower=1)[1] == k + 1, _tag(n, "dense", "dpotrf", kind, k)
    finally:
        ldl.close()
        chol.close()


@pytest.mark.parametrize("n", [63, 700, 1300])
def test_pivots_below_pivot_tol_follow_the_scalar_reference(ctx, n):
    """pivot_tol = 1e-10 and d_k = 4^-20: counted as zero; D and L as the scalar reference (harmless pivot 1, the column of
    the Schur complement kept as it is) to 1e-12 max|A| (exactly where N > 700: the counts)."""
    base = make_exact(n, 5000 + n, positive=False)
    pat = base.lower_pattern()
    solvers = [P(ctx, n, mj.LDL, pivot_tol=1e-10) for P in (_Dense, _CSC)]
    try:
        for S in solvers:
            for k in _columns(n):
                c = with_pivot(base, k, TINY)
                tag = _tag(n, S.path, "LDL pivot_tol", "tiny", k)
                M = S.factorize(c, pat)
                p, z, q = c.inertia()
                assert M.inertia() == (p - 1, z + 1, q), tag + f": {M.inertia()}"
                if n <= 700:
                    Lr, dr = scalar_ldl(c.A, 1e-10)
                    Lg, D = M.get_factor()
                    Lg = np.tril(Lg, -1) + np.eye(n)
                    amax = np.abs(c.A).max()
                    assert D[k] == 0.0 and np.array_equal(D == 0.0, dr == 0.0), tag
                    assert np.abs(D - dr).max() <= 1e-12 * amax, tag + f": D {np.abs(D - dr).max():.2e}"
                    assert np.abs(Lg - Lr).max() <= 1e-12 * amax, tag + f": L {np.abs(Lg - Lr).max():.2e}"
    finally:
        for S in solvers:
            S.close()


@pytest.mark.parametrize("n", [65, 700, 1300, 2600, 5400])
def test_early_rejection_stops_at_the_leaf_of_the_first_bad_pivot(ctx, n):
    """accept_only_pd + early_reject: rejected exactly when some d_k <= 0; early_reject_col is the last column of the 64-column
    leaf holding the first bad pivot; the counts are the signs of the pivots through that leaf (everything behind counted
    negative); through the KKT path a solve after the rejection gives the bits of a solver with early_reject off, and the next
    positive definite matrix factors as on a solver that never rejected."""
    pos = make_exact(n, 6000 + n)
    pat = pos.lower_pattern()
    dn = _Dense(ctx, n, mj.LDL, accept_only_pd=1, early_reject=1)
    kh = _KKT(ctx, n, mj.BUNCHKAUFMAN, pat)
    kf = _KKT(ctx, n, mj.BUNCHKAUFMAN, pat, early_reject=False)
    kh.M.set_option("probe", 0)
    b = np.random.default_rng(n).standard_normal(n)
    try:
        for k in [None] + _columns(n):
            for kind in (("none",) if k is None else ("neg", "zero")):
                c = pos if k is None else with_pivot(pos, k, -pos.d[k] if kind == "neg" else 0.0)
                for S in (dn, kh):
                    tag = _tag(n, S.path, "LDL early_reject" if S is dn else "BUNCHKAUFMAN early_reject", kind, k)
                    M = S.factorize(c, pat)
                    ine = M.inertia()
                    if k is None:
                        assert ine == (n, 0, 0), tag + f": {ine}"
                        continue
                    if S is dn:
                        # (a host matrix does not outlive the call, so nothing could complete a stopped factorization: early
                        # rejection is not armed, and the static tier's counts are final under accept_only_pd)
                        assert ine == c.inertia(), tag + f": {ine} != {c.inertia()}"
                        continue
                    e = min(n, k // 64 * 64 + 64)
                    want = (int(np.sum(c.d[:e] > 0)), int(np.sum(c.d[:e] == 0)))
                    want = (want[0], want[1], n - want[0] - want[1])
                    assert ine == want, tag + f": {ine} != {want}"
                    assert M.get_stat("early_reject_col") == k // 64 * 64 + 63, tag + f": {M.get_stat('early_reject_col')}"
                if k is not None and kind == "neg" and k in (0, 64, n - 1):
                    tag = _tag(n, "kkt", "BUNCHKAUFMAN early_reject solve", kind, k)
                    kf.factorize(c)
                    assert kf.M.inertia() == c.inertia(), tag + f": early_reject off {kf.M.inertia()} != {c.inertia()}"
                    xh, xf = kh.M.solve_linear_system(b.copy()), kf.M.solve_linear_system(b.copy())
                    assert np.array_equal(xh, xf), tag + ": not the bits of the solver with early_reject off"
                    assert kh.M.inertia() == c.inertia(), tag + f": counts after the completed factorization {kh.M.inertia()}"
        tag = _tag(n, "kkt", "BUNCHKAUFMAN early_reject", "clean after rejections", None)
        kh.factorize(pos)
        kf.factorize(pos)
        assert kh.M.inertia() == kf.M.inertia() == (n, 0, 0), tag + f": {kh.M.inertia()} / {kf.M.inertia()}"
        assert np.array_equal(kh.M.solve_linear_system(b.copy()), kf.M.solve_linear_system(b.copy())), tag + ": solve bits"
    finally:
        dn.close(); kh.close(); kf.close()


# --------------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", [700, 1300])
def test_batched_members_breaking_at_different_columns(ctx, n):
    """One factorize_batch of 6 members that break at different columns (or not at all): each member's inertia and D are its
    exact answer, CHOLESKY members report their own info, and the members that do not break are bit-identical to lone
    factorizations."""
    dev = torch.device("cuda", 0)
    base = make_exact(n, 7000 + n, positive=False)
    Lbase = torch.from_numpy(base.L).to(dev)
    pos = make_exact(n, 8000 + n)
    breaks = [None, 0, 63, n // 2, None, n - 1]
    members = [with_pivot(base, k, 0.0 if i % 2 else -abs(base.d[k])) if k is not None else base for i, k in enumerate(breaks)]
    chol_members = [with_pivot(pos, k, -pos.d[k]) if k is not None else pos for k in breaks]
    ldl = [_Dense(ctx, n, mj.LDL) for _ in breaks]
    chol = [_Dense(ctx, n, mj.CHOLESKY) for _ in breaks]
    lone = _Dense(ctx, n, mj.LDL)
    lone_c = _Dense(ctx, n, mj.CHOLESKY)
    try:
        for S, c in zip(ldl + chol, members + chol_members):
            S.M.A = c.A
        with mj.factorize_batch():
            for S in ldl + chol:
                S.M.factorize()
        for i, (S, c, k) in enumerate(zip(ldl, members, breaks)):
            tag = _tag(n, "batch", "LDL", "member %d" % i, k)
            assert S.M.inertia() == c.inertia(), tag + f": {S.M.inertia()}"
            _check_exact_ldl(S.M, c, tag, Lbase)
            if k is None:
                L1, D1 = _factor(S.M)
                L0, D0 = _factor(lone.factorize(c, None))
                assert torch.equal(L1, L0) and torch.equal(D1, D0), tag + ": not the bits of a lone factorization"
        for i, (S, c, k) in enumerate(zip(chol, chol_members, breaks)):
            tag = _tag(n, "batch", "CHOLESKY", "member %d" % i, k)
            assert S.M.info == c.dpotrf_info(), tag + f": info {S.M.info}"
            if k is None:
                L1, _ = S.M.get_factor_device()
                L0, _ = lone_c.factorize(c, None).get_factor_device()
                assert torch.equal(torch.tril(L1), torch.tril(L0)), tag
    finally:
        for S in ldl + chol + [lone, lone_c]:
            S.close()


# --------------------------------------------------------------------------------------------------------- the probe
def _verdicts(kkt, seq):
    out = []
    for c in seq:
        M = kkt.factorize(c)
        ine = M.inertia()
        out.append((ine, kkt.k.is_inertia_correct(*ine), M.get_stat("early_reject_col")))
    return out


def test_leading_block_probe_gives_the_verdict_of_the_full_factorization_exactly(ctx):
    """N = 2600, K = A through the KKT path: after a rejection below N/2 and an acceptance, matrices that break inside the probe
    block, just past it, or nowhere -- the probe's inertia, verdict and early_reject_col are those of the full factorization,
    exactly; and the probe takes some of them."""
    n = 2600
    pos = make_exact(n, 9000 + n)
    pat = pos.lower_pattern()
    br = lambda k: with_pivot(pos, k, -pos.d[k])            # noqa: E731
    zr = lambda k: with_pivot(pos, k, 0.0)                   # noqa: E731
    # The probe block's order follows the latest early rejection below N/2 (m = (col + 256) / 256 * 256, probed if m >= 512):
    # the rejection at 700 (leaf 640..703) gives m = 768; 300 breaks inside it (col 319: m = 512); 1000 breaks past 512 (col 1023:
    # m = 1024); 1030 just past 1024 (col 1087: m = 1280); two clean matrices (no break: probes that pass); 64 inside 1280 (col 127:
    # m = 256, no probe); 1100 with no probe (col 1151: m = 1280); 5 inside 1280.  Acceptances in between re-arm the probe.
    seq = [br(700), pos, br(300), pos, zr(1000), pos, br(1030), pos, pos, br(64), pos, zr(1100), pos, br(5), pos]
    runs = {}
    for probe in (0, 1):
        K = _KKT(ctx, n, mj.BUNCHKAUFMAN, pat)
        K.M.set_option("probe", probe)
        try:
            runs[probe] = (_verdicts(K, seq), K.M.get_stat("probe_hits"))
        finally:
            K.close()
    (off, hits_off), (on, hits_on) = runs[0], runs[1]
    for i, (a, b) in enumerate(zip(off, on)):
        assert a == b, f"N={n} path=kkt alg=BUNCHKAUFMAN kind=probe step={i}: probe off {a}, on {b}"
    assert hits_off == 0 and hits_on >= 1, f"N={n} path=kkt alg=BUNCHKAUFMAN kind=probe col=-: hits off {hits_off}, on {hits_on}"
    # and the verdict is the matrix's: rejected exactly when some pivot is not positive
    for i, ((ine, ok, col), c) in enumerate(zip(off, seq)):
        assert ok == (c.dpotrf_info() == 0), f"N={n} path=kkt alg=BUNCHKAUFMAN kind=probe step={i} col={c.dpotrf_info() - 1}: {ine}"


def test_probe_follows_the_parents_pivot_tol(ctx):
    """The probe's child solver is created with the parent's pivot_tol (1e-8 here); the parent's pivot_tol then goes to 0.  A
    matrix that is positive definite with d_k = 2^-40 inside the probe block is accepted -- as with the probe off."""
    n = 2600
    pos = make_exact(n, 9100 + n)
    pat = pos.lower_pattern()
    small = with_pivot(pos, 300, 2.0 ** -40)
    seq_pre = [with_pivot(pos, 700, -pos.d[700]), pos, pos]     # reject below N/2, accept, accept (the probe's child is made)
    res = {}
    for probe in (0, 1):
        K = _KKT(ctx, n, mj.BUNCHKAUFMAN, pat)
        K.M.set_option("probe", probe)
        K.M.set_option("pivot_tol", 1e-8)
        try:
            pre = _verdicts(K, seq_pre)
            K.M.set_option("pivot_tol", 0.0)
            probes = K.M.get_stat("probe_hits") + K.M.get_stat("probe_misses")
            last = _verdicts(K, [small])
            res[probe] = (pre, last, K.M.get_stat("probe_hits") + K.M.get_stat("probe_misses") - probes)
        finally:
            K.close()
    tag = f"N={n} path=kkt alg=BUNCHKAUFMAN kind=probe pivot_tol col=300"
    assert res[0][:2] == res[1][:2], tag + f": probe off {res[0][:2]}, on {res[1][:2]}"
    assert res[1][1][0][1], tag + f": rejected {res[1][1]}"
    assert res[1][2] == 1, tag + f": the last matrix was not probed ({res[1][2]} probes)"   # (the fix was exercised)


def test_solve_after_a_probe_hit_completes_the_factorization(ctx):
    """N = 1300 (the parent on the task-DAG schedule, the child of order 512 on schedule 4): a rejection at pivot 300, an acceptance,
    the same rejection again -- the last one is the probe's alone, so the factor buffer still holds the factor of the ACCEPTED
    matrix.  A solve on it must transfer the rejected matrix and factor it to the end: the inertia after that, the count of such
    redos and the solution are the bits of a solver with the probe off, and so are the verdict and its column before the solve."""
    n = 1300
    pos = make_exact(n, 9200 + n)
    pat = pos.lower_pattern()
    bad = with_pivot(pos, 300, -pos.d[300])
    b = np.random.default_rng(n).standard_normal(n)
    res = {}
    for probe in (0, 1):
        K = _KKT(ctx, n, mj.BUNCHKAUFMAN, pat)
        K.M.set_option("probe", probe)
        try:
            before = _verdicts(K, [bad, pos])
            hits = K.M.get_stat("probe_hits")
            before += _verdicts(K, [bad])
            hit = K.M.get_stat("probe_hits") - hits
            x = K.M.solve_linear_system(b.copy())
            res[probe] = (before, hit, x, np.array(K.M.inertia()), K.M.get_stat("early_reject_redone"))
        finally:
            K.close()
    tag = f"N={n} path=kkt alg=BUNCHKAUFMAN kind=probe hit + solve col=300"
    assert (res[0][1], res[1][1]) == (0, 1), tag + f": probe hits at the last step, off {res[0][1]}, on {res[1][1]}"
    assert res[0][0] == res[1][0], tag + f": verdicts before the solve, probe off {res[0][0]}, on {res[1][0]}"
    assert res[1][0][2][2] == 300 // 64 * 64 + 63 and not res[1][0][2][1], tag + f": {res[1][0][2]}"
    assert np.array_equal(res[0][3], res[1][3]), tag + f": inertia after the redo, probe off {res[0][3]}, on {res[1][3]}"
    assert np.array_equal(res[0][3], np.array(bad.inertia())), tag + f": {res[0][3]} != {bad.inertia()}"
    assert res[0][4] == res[1][4] == 1, tag + f": early_reject_redone off {res[0][4]}, on {res[1][4]}"
    assert np.array_equal(res[0][2], res[1][2]), tag + ": the solution is not the bits of the solver with the probe off"


# --------------------------------------------------------------------------------------------------------- NaN / Inf
def _nonfinite_cases(n):
    """(where, (i, j)): a diagonal, an off-diagonal in one 4-pivot group, one in a 16-row block but another group, far below."""
    g = min(16, (n - 1) // 16 * 16) if n > 20 else 0
    out = [("diagonal", (g + 1, g + 1)), ("group", (g + 2, g)), ("far", (n - 3, 5))]
    if n >= 32:
        out.append(("block16", (g + 9, g + 2)))
    return out


@pytest.mark.parametrize("n", [63, 130, 700])
def test_non_finite_entries(ctx, n):
    """NaN or +Inf on a diagonal, on an off-diagonal in one 4-pivot group, in one 16-row block but another group, and far below
    the diagonal, through the dense and the KKT path: CHOLESKY's info is dpotrf's; LDL^T's recorded D is finite and equals the
    scalar reference (exact before the first affected pivot, 0 at every non-finite one) with its counts, and is never an
    accepted inertia; BUNCHKAUFMAN never accepts and its counts sum to N.  After each, a clean matrix on the SAME solver factors
    bit-identically to a fresh solver (no growth / amax word or spare buffer keeps state from the bad matrix)."""
    pos = make_exact(n, 9500 + n)
    # (the KKT path holds the structural pattern only: it is widened by the positions that get the non-finite entries)
    colptr, rowval = pos.lower_pattern()
    ij = np.array([p for _, p in _nonfinite_cases(n)])
    W = sp.csc_matrix((np.ones(len(rowval)), rowval, colptr), shape=(n, n)) + \
        sp.csc_matrix((np.ones(len(ij)), (ij[:, 0], ij[:, 1])), shape=(n, n))
    W.sort_indices()
    pat = (W.indptr.astype(np.int32), W.indices.astype(np.int32))
    b = np.random.default_rng(n).standard_normal(n)

    def make(P, alg):
        # (the KKT path without early rejection: the counts of every pivot, as the scalar reference has them)
        return P(ctx, n, alg, pat, early_reject=False) if P is _KKT else P(ctx, n, alg)

    def fresh_bits(P, alg):
        S = make(P, alg)
        try:
            M = S.factorize(pos, pat)
            Lf, Df = M.get_factor()
            return M.inertia(), np.tril(Lf), Df, M.solve_linear_system(b.copy())
        finally:
            S.close()

    for P in (_Dense, _KKT):
        for alg in (mj.CHOLESKY, mj.LDL, mj.BUNCHKAUFMAN):
            clean = fresh_bits(P, alg)
            S = make(P, alg)
            try:
                for where, (i, j) in _nonfinite_cases(n):
                    for val in (np.nan, np.inf):
                        tag = _tag(n, P.path, alg, f"{where} {val}", f"({i},{j})")
                        A = pos.A.copy(order="F")
                        A[i, j] = A[j, i] = val
                        c = type(pos)(n, pos.Nmat, pos.d, A)
                        M = S.factorize(c, pat)
                        ine = M.inertia()
                        _, dr = scalar_ldl(A)
                        if alg == mj.CHOLESKY:
                            # the first pivot that is not positive and finite (reference LAPACK's dpotrf stops at a NaN pivot
                            # -- `ajj <= 0 .or. disnan(ajj)`; the leaf at an infinite one as well): the scalar reference's
                            # first recorded zero, since every pivot of the clean matrix is positive
                            want = int(np.flatnonzero(dr <= 0.0)[0]) + 1
                            assert M.info == want, tag + f": info {M.info} != {want}"
                            assert ine == (0, n, 0), tag + f": {ine}"
                        elif alg == mj.LDL:
                            Lg, D = M.get_factor()
                            assert np.all(np.isfinite(D)), tag + f": D not finite at {np.flatnonzero(~np.isfinite(D))[:8]}"
                            assert np.array_equal(D == 0.0, dr == 0.0), tag + f": zero pivots {np.flatnonzero(D == 0)[:8]} != {np.flatnonzero(dr == 0)[:8]}"
                            first = max(i, j)      # (only row and column max(i, j) meet the entry before its pivot)
                            assert np.array_equal(D[:first], pos.d[:first]), tag + ": D before the first affected pivot"
                            assert np.abs(D - dr).max() <= 1e-12 * np.abs(pos.A).max(), tag + f": D {np.abs(D - dr).max():.2e}"
                            want = (int(np.sum(dr > 0)), int(np.sum(dr == 0)), int(np.sum(dr < 0)))
                            assert ine == want and ine != (n, 0, 0), tag + f": {ine} != {want}"
                        else:
                            assert sum(ine) == n and ine != (n, 0, 0), tag + f": {ine}"
                        # the same solver on a clean matrix: the bits of a fresh one
                        M = S.factorize(pos, pat)
                        Lf, Df = M.get_factor()
                        again = (M.inertia(), np.tril(Lf), Df, M.solve_linear_system(b.copy()))
                        assert again[0] == clean[0], tag + ": clean inertia after"
                        for a, z in zip(again[1:], clean[1:]):
                            assert np.array_equal(a, z), tag + ": clean factor after differs from a fresh solver's"
            finally:
                S.close()

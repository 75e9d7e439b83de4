"""Exact answers for every way solve! runs on the static-pivot tier (-m gpu).

The systems of tests/solve_exact.py have one right answer in fp64 whatever the blocking, the summation order and the fusing of
products (tests/test_solve_exact_cpu.py checks that premise, and that it leaves no slack for an error of one ulp).  So every path
of solve! -- stepwise (1), one launch over 256-column steps (2), over 512-column steps (3), a system of a merged launch (4) --
must return x* with array_equal, for CHOLESKY (positive pivots) and LDL (mixed signs, pivot_tol = 0), with the scalar and the
MFMA 256 x 256 inverses and with the 512-row stage; every case asserts the inertia first, then the path the statistic
"solve_path" reports, then the bits.  Device vectors live in a longer buffer with a NaN tail: the tail must stay NaN, and a read
of it would poison x.  With S = diag(2^k), k in [0, 40], the answer S^-1 x* spans twelve decades: no norm-wise check sees its
small entries.  On real data the power-of-two scaling must commute with the whole solver bit for bit, and the componentwise
backward error is measured against the oracle's dpotrs / dsytrs (MNK_SOLVE_ACCURACY_OUT names a file: the figures of
profiles/solve_exact_accuracy.json)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import madnlp_jl_amd as mj
from madnlp_jl_amd import _lib as L
from oracle.lapack_cpu import BUNCHKAUFMAN, CHOLESKY, LapackCPUSolver
from tests.exact_factor import ExactCase
from tests.solve_exact import bit_budget, device_system, ownership_orders, solve_case
from tests.test_hip_pivot_ladder import _KKT

pytestmark = pytest.mark.gpu

ALGS = [mj.CHOLESKY, mj.LDL]
SIZES = [1, 63, 64, 65, 255, 256, 257, 700, 1300, 2100]   # one block; a ragged last 64-block; last steps of 1, 2 and 3 blocks
NAN = float("nan")
BIT_CAP = 40
# device <= ACCURACY_MARGIN * oracle, componentwise backward error: the next power of two above twice the largest ratio measured
# on an MI355X for these cases (profiles/solve_exact_accuracy.json: 2.94, CHOLESKY at N = 4100 on path 3), capped at 64
ACCURACY_MARGIN = 8.0
_measured = {}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = mj.HipContext(0)
    yield c
    c.close()
    out = os.environ.get("MNK_SOLVE_ACCURACY_OUT")
    if out and _measured:
        with open(out, "w") as f:
            json.dump({"bound": f"device <= {ACCURACY_MARGIN:g} * oracle", "cases": _measured,
                       "note": "tests/test_hip_solve_exact.py on one MI355X: componentwise backward error max_i |A x - b|_i / "
                               "(|A| |x| + |b|)_i in longdouble of solve! on each path and of the oracle's dpotrs (CHOLESKY) / "
                               "dsytrs (LDL) on the same graded matrix S B S, and their ratio"}, f, indent=1, sort_keys=True)


def _dev():
    return torch.device("cuda", 0)


def _solve_path(M):
    """Statistic "solve_path" (csrc/solve_plan.h: 1 stepwise, 2 one launch over 256-column steps, 3 over 512-column steps, 4 a system
    of a merged launch), or None from a build of the library that does not report it (A/B runs through MNK_LIBPATH)."""
    try:
        return M.get_stat("solve_path")
    except mj.HipError:
        return None


@functools.lru_cache(maxsize=None)
def _case(n, alg, scale_bits=0, variant=0):
    """The case of the CPU test (seed 100 + n) or another exact matrix of the same order (`variant`); dense on the host below 2000
    rows, from the sparse factors on the device above."""
    c = solve_case(n, 100 + n + 7919 * variant, alg == mj.CHOLESKY, scale_bits, dense=n < 2000)
    assert bit_budget(c) <= BIT_CAP, (n, alg, scale_bits, variant, bit_budget(c))
    return c


def _system(c):
    """(A, b, x) of a case on the device."""
    dev = _dev()
    if c.A is None:
        A, b = device_system(c, dev)
    else:
        A, b = torch.from_numpy(np.ascontiguousarray(c.A)).to(dev), torch.from_numpy(c.b).to(dev)
    return A, b, torch.from_numpy(c.x).to(dev)


def _solver(ctx, A, alg, **opts):
    M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=alg, pivot_tol=0.0,
                                                               persistent_solve=bool(opts.pop("persistent_solve", True))))
    for key, v in opts.items():
        M.set_option(key, v)
    return M


def _factorize(M, c, tag):
    torch.cuda.synchronize()      # (the matrix was produced on torch's stream, the solver works on its context's)
    M.factorize()
    assert M.inertia() == c.inertia(), tag + f": inertia {M.inertia()} != {c.inertia()}"


def _assert_exact(x, want, tag):
    bad = torch.nonzero(x != want)
    if len(bad):
        i = bad[0].tolist()
        raise AssertionError(tag + f": {len(bad)} entries differ from x*, first at {i} (64-row block {i[0] // 64}): "
                                   f"{x[tuple(i)].item()!r} != {want[tuple(i)].item()!r}")


def _padded(v, tail=9):
    """(buffer, view): v at the head of a longer buffer whose tail is NaN."""
    buf = torch.full((v.shape[0] + tail,), NAN, dtype=torch.float64, device=v.device)
    buf[:v.shape[0]] = v
    return buf, buf[:v.shape[0]]


def _check_tail(buf, n, tag):
    assert bool(torch.isnan(buf[n:]).all()), tag + ": the buffer behind row N was written"


def _solve_device(M, b, x, path, tag):
    """One solve on a device vector inside a NaN-tailed buffer."""
    buf, v = _padded(b)
    torch.cuda.synchronize()
    M.solve_linear_system(v)
    M.check_solve()
    assert _solve_path(M) in (path, None), tag + f": solve_path {_solve_path(M)}, expected {path}"
    _assert_exact(v, x, tag)
    _check_tail(buf, b.shape[0], tag)


def _exercise(ctx, alg, opts, c, c2, path, tag):
    """A solver with `opts` factorizes c; a host vector, three device vectors in a row (the publication buffers of the one-launch
    solves alternate), three right-hand sides in a strided device view (ldx = n + 7) scaled by 1, -1/2 and 4; then c2 on the same
    solver and one more solve.  Every solve: the path, then x* bit for bit."""
    A, b, x = _system(c)
    M = _solver(ctx, A, alg, **opts)
    try:
        _exercise_solver(M, c, c2, A, b, x, path, tag)
    finally:
        M.close()


def _exercise_solver(M, c, c2, A, b, x, path, tag):
    n, dev = c.n, _dev()
    _factorize(M, c, tag)
    xh = M.solve_linear_system(c.b.copy())
    assert _solve_path(M) in (path, None), tag + f" host: solve_path {_solve_path(M)}, expected {path}"
    _assert_exact(torch.from_numpy(xh), torch.from_numpy(c.x), tag + " host vector")
    for rep in range(3):
        _solve_device(M, b, x, path, tag + f" device vector {rep}")
    ldx = n + 7
    buf = torch.full((3, ldx), NAN, dtype=torch.float64, device=dev)
    X = buf.T[:n]                                          # (n, 3), column stride ldx
    scale = torch.tensor([1.0, -0.5, 4.0], dtype=torch.float64, device=dev)
    X[:] = b[:, None] * scale
    torch.cuda.synchronize()
    M.solve_linear_system(X)
    M.check_solve()
    assert _solve_path(M) in (path, None), tag + f" strided: solve_path {_solve_path(M)}, expected {path}"
    _assert_exact(X, x[:, None] * scale, tag + " strided right-hand sides")
    assert bool(torch.isnan(buf.T[n:]).all()), tag + ": the padding rows of the strided view were written"
    A2, b2, x2 = _system(c2)
    M.A = A2
    _factorize(M, c2, tag + " second matrix")
    _solve_device(M, b2, x2, path, tag + " after the second factorize")


# ------------------------------------------------------------------------------- stepwise and one launch over 256 columns
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n,scale_bits", [(n, 0) for n in SIZES] + [(257, 40), (1300, 40), (4100, 40)])
def test_stepwise_and_256_column_solves_return_the_dyadic_solution(ctx, n, scale_bits, alg):
    """persistent_solve off (path 1) and on (path 2), the scalar and the MFMA 256 x 256 inverses."""
    c, c2 = _case(n, alg, scale_bits), _case(n, alg, scale_bits, 1)
    for persistent in (False, True):
        for mfma in (0, 1):
            _exercise(ctx, alg, dict(persistent_solve=persistent, linv_mfma=mfma), c, c2, 2 if persistent else 1,
                      f"N={n} {alg} scale_bits={scale_bits} persistent_solve={persistent} linv_mfma={mfma}")


# ------------------------------------------------------------------------------- 512-column steps
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n,scale_bits,path", [(3968, 0, 2), (4096, 0, 3), (4100, 0, 3), (4100, 40, 3), (4480, 0, 2), (5000, 0, 3)])
def test_512_column_solves_return_the_dyadic_solution(ctx, n, scale_bits, path, alg):
    """Option solve512: path 3 from 4096 rows on; N = 4480 (padded order 4480, a 384-row last triangle) and N = 3968 stay on
    path 2, and are exact there with the option set."""
    _exercise(ctx, alg, dict(solve512=1), _case(n, alg, scale_bits), _case(n, alg, scale_bits, 1), path,
              f"N={n} {alg} scale_bits={scale_bits} solve512")


# ------------------------------------------------------------------------------- more than one block per workgroup
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("path", [2, 3])
def test_a_workgroup_that_owns_more_than_one_block(ctx, path, alg):
    """The smallest orders at which block ownership wraps around: N = 64 (CUs + 3) + 5 on path 2 (64-row blocks), N = 32 (CUs + 5) + 3
    on path 3 (32-row blocks).  Built on the device; one solve each."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = ownership_orders(cus)[path - 2]
    Np = (n + 63) // 64 * 64
    assert Np // (64 if path == 2 else 32) > cus and (path == 2 or Np % 512 != 384)
    c = _case(n, alg)
    A, b, x = _system(c)
    M = _solver(ctx, A, alg, solve512=int(path == 3))
    try:
        _factorize(M, c, f"N={n} {alg}")
        _solve_device(M, b, x, path, f"N={n} {alg} path {path} on {cus} CUs")
    finally:
        M.close()


# ------------------------------------------------------------------------------- merged launches
def _expected_groups(Ms, alg, cus):
    """The launches mnk_debug_solve_batch_groups makes of a queue of one solve per solver, in queue order."""
    n = len(Ms)
    cols = [np.arange(n, dtype=np.int64), np.zeros(n, np.int32), np.array([(M.n + 63) // 64 * 64 for M in Ms], np.int64),
            np.full(n, int(alg == mj.LDL), np.int32), np.full(n, cus, np.int32)]
    begin, idx, G = np.zeros(n + 1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    nl = L.lib().mnk_debug_solve_batch_groups(n, *(c.ctypes.data for c in cols), begin.ctypes.data, idx.ctypes.data, G.ctypes.data)
    assert 0 < nl <= n
    return [idx[begin[l]:begin[l + 1]].tolist() for l in range(nl)]


def _batch(ctx, alg, members, rounds=1, solve512=(), min_launches=1):
    """One solver per member (n, scale_bits, variant), every one of them exact; `rounds` solve batches of one device vector each.
    The members in `solve512` have the 512-row inverses: a solve batch does not queue them, they run at once on path 3.  The others
    run as mnk_debug_solve_batch_groups groups them: path 4 in a launch of two or more, path 2 alone."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [_case(n, alg, sb, v) for (n, sb, v) in members]
    systems = {}
    Ms = []
    try:
        for i, c in enumerate(cases):
            if id(c) not in systems:
                systems[id(c)] = _system(c)
            M = _solver(ctx, systems[id(c)][0], alg, solve512=int(i in solve512))
            Ms.append(M)
            _factorize(M, c, f"batch member {i} N={c.n} {alg}")
        queued = [i for i in range(len(Ms)) if i not in solve512]
        groups = [[queued[j] for j in g] for g in _expected_groups([Ms[i] for i in queued], alg, cus)]
        want = {i: 3 for i in solve512}
        for g in groups:
            for i in g:
                want[i] = 4 if len(g) >= 2 else 2
        assert any(len(g) >= 2 for g in groups) and len(groups) >= min_launches, groups
        for rnd in range(rounds):
            bufs = [_padded(systems[id(c)][1]) for c in cases]
            torch.cuda.synchronize()
            with mj.solve_batch():
                for M, (_, v) in zip(Ms, bufs):
                    M.solve_linear_system(v)
            for M in Ms:
                M.check_solve()
            paths = [_solve_path(M) for M in Ms]
            assert paths in ([want[i] for i in range(len(Ms))], [None] * len(Ms)), (rnd, paths, groups)
            for i, (c, (buf, v)) in enumerate(zip(cases, bufs)):
                tag = f"batch member {i} N={c.n} {alg} round {rnd} groups {groups}"
                _assert_exact(v, systems[id(c)][2], tag)
                _check_tail(buf, c.n, tag)
    finally:
        for M in Ms:
            M.close()


@pytest.mark.parametrize("alg", ALGS)
def test_merged_launches_of_mixed_orders(ctx, alg):
    """(257, 257, 257, 700, 700): two orders, so at least two launches (on 256 CUs: of three and of two, all on path 4)."""
    _batch(ctx, alg, [(257, 0, 0), (257, 0, 1), (257, 0, 2), (700, 0, 0), (700, 0, 1)], min_launches=2)


@pytest.mark.parametrize("alg", ALGS)
def test_a_merged_launch_at_the_table_limit(ctx, alg):
    """Thirty-three solvers of N = 130, one more than the table of a merged launch holds (SP_BATCH_MAXQ = 32): on 256 CUs a launch
    of 32 systems and a lone solve on path 2."""
    _batch(ctx, alg, [(130, 0, i % 3) for i in range(33)], min_launches=2)


@pytest.mark.parametrize("alg", ALGS)
def test_a_merged_launch_repeated(ctx, alg):
    """Four of N = 2100, three batches in a row (the publication buffers of every member alternate)."""
    _batch(ctx, alg, [(2100, 0, i) for i in range(4)], rounds=3)


@pytest.mark.parametrize("alg", ALGS)
def test_a_member_with_the_512_row_inverses_inside_a_batch(ctx, alg):
    """N = 4100, two plain members and one with solve512: the two share a merged launch, the third runs on path 3."""
    _batch(ctx, alg, [(4100, 0, 0), (4100, 0, 1), (4100, 0, 0)], solve512=(2,))


@pytest.mark.parametrize("alg", ALGS)
def test_merged_launches_of_graded_systems(ctx, alg):
    """scale_bits = 40 at N = 257, 1300 and 4100, two of each: S^-1 x* bit for bit from merged launches."""
    _batch(ctx, alg, [(257, 40, 0), (257, 40, 1), (1300, 40, 0), (1300, 40, 1), (4100, 40, 0), (4100, 40, 1)])


# ------------------------------------------------------------------------------- through a KKT handle
@pytest.mark.parametrize("alg", ALGS)
def test_solves_through_a_sparse_condensed_kkt_handle(ctx, alg):
    """N = 1300, scale_bits = 40, K = A fed as the Hessian's lower triangle on its structural pattern (the wrappers of
    test_hip_pivot_ladder.py): a solve alone (path 2), then two handles inside one solve batch."""
    n = 1300
    cs = [_case(n, alg, 40, v) for v in (0, 1)]
    Ks = []
    try:
        for c in cs:
            pat = ExactCase(n, c.Nmat, c.d, c.A).lower_pattern()
            # (CHOLESKY: the handle's defaults, early rejection armed; LDL: the whole inertia of a mixed-sign matrix)
            K = _KKT(ctx, n, alg, pat) if alg == mj.CHOLESKY else _KKT(ctx, n, alg, pat, early_reject=False, accept_only_pd=0)
            Ks.append(K)
            K.M.set_option("pivot_tol", 0.0)
            K.factorize(c)
            assert K.M.inertia() == c.inertia(), f"N={n} {alg} kkt: inertia {K.M.inertia()} != {c.inertia()}"
        dev = _dev()
        bs = [torch.from_numpy(c.b).to(dev) for c in cs]
        xs = [torch.from_numpy(c.x).to(dev) for c in cs]
        _solve_device(Ks[0].M, bs[0], xs[0], 2, f"N={n} {alg} kkt alone")
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        groups = _expected_groups([K.M for K in Ks], alg, cus)
        want = [4 if len(groups) == 1 else 2] * 2
        bufs = [_padded(b) for b in bs]
        torch.cuda.synchronize()
        with mj.solve_batch():
            for K, (_, v) in zip(Ks, bufs):
                K.M.solve_linear_system(v)
        for K in Ks:
            K.M.check_solve()
        paths = [_solve_path(K.M) for K in Ks]
        assert paths in (want, [None, None]), (paths, groups)
        for i, (buf, v) in enumerate(bufs):
            _assert_exact(v, xs[i], f"N={n} {alg} kkt in a solve batch, member {i}")
            _check_tail(buf, n, f"N={n} {alg} kkt in a solve batch, member {i}")
    finally:
        for K in Ks:
            K.close()


# ------------------------------------------------------------------------------- real data
REAL_SIZES = [257, 1300, 4100]


@functools.lru_cache(maxsize=None)
def _real(n, alg):
    """(B, S B S, s, b): B = R R^T / 64 + I with R n x 64 standard normal (eigenvalues >= 1), for LDL its trailing third negated (a
    quasi-definite matrix: the eigenvalues stay outside (-1, 1)); |B|_inf <= 1e3 bounds its largest eigenvalue, so the condition
    number is at most 1e3.  S = diag(2^k), k uniform in [0, 40]."""
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(1000 + n)
    R = torch.randn(n, 64, dtype=torch.float64, device=dev, generator=g)
    B = R @ R.T / 64.0
    B.diagonal().add_(1.0)
    B = (B + B.T) / 2.0      # (exactly symmetric: the scaled copy below is then too)
    if alg == mj.LDL:
        h = n // 3
        B[n - h:, n - h:].neg_()
    assert torch.linalg.matrix_norm(B, ord=float("inf")).item() <= 1e3
    # (formed on the host: a device pow() need not return the exact power of two)
    s = torch.from_numpy(np.ldexp(1.0, np.random.default_rng(1000 + n).integers(0, 41, size=n))).to(dev)
    assert bool((torch.frexp(s)[0] == 0.5).all())
    b = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    return B, s[:, None] * B * s[None, :], s, b


def _real_paths(n):
    return [(1, dict(persistent_solve=False)), (2, dict())] + ([(3, dict(solve512=1))] if n >= 4096 else [])


def _real_solve(ctx, A, b, alg, path, opts, n_pos, tag):
    M = _solver(ctx, A, alg, **opts)
    try:
        torch.cuda.synchronize()
        M.factorize()
        n = A.shape[0]
        assert M.inertia() == (n_pos, 0, n - n_pos), tag + f": inertia {M.inertia()}"
        x = b.clone()
        torch.cuda.synchronize()
        M.solve_linear_system(x)
        M.check_solve()
        assert _solve_path(M) in (path, None), tag + f": solve_path {_solve_path(M)}, expected {path}"
        return x
    finally:
        M.close()


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n", REAL_SIZES)
def test_a_power_of_two_scaling_commutes_with_the_solver(ctx, n, alg):
    """solve(S B S, S b) = S^-1 solve(B, b) bit for bit on paths 1, 2 and 3 (N >= 4096): every operation of the factorization and
    of the solves commutes with a power-of-two scaling (pivot_tol = 0; nothing over- or underflows)."""
    B, SBS, s, b = _real(n, alg)
    n_pos = n if alg == mj.CHOLESKY else n - n // 3
    for path, opts in _real_paths(n):
        tag = f"N={n} {alg} path {path}"
        x0 = _real_solve(ctx, B, b, alg, path, opts, n_pos, tag + " B")
        x1 = _real_solve(ctx, SBS, s * b, alg, path, opts, n_pos, tag + " S B S")
        _assert_exact(x1, x0 / s, tag)


def _componentwise_backward_error(A, x, b):
    A, x, b = A.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    return float(np.max(np.abs(A @ x - b) / (np.abs(A) @ np.abs(x) + np.abs(b))))


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n", REAL_SIZES)
def test_componentwise_backward_error_against_the_oracle(ctx, n, alg):
    """The graded S B S with a random b: max_i |A x - b|_i / (|A| |x| + |b|)_i in longdouble of solve! on each path is at most
    ACCURACY_MARGIN times that of the oracle's dpotrs / dsytrs on the same matrix.  (The explicit block inverses and other
    groupings add a few roundings per entry, no more.)"""
    _, SBS, s, b = _real(n, alg)
    n_pos = n if alg == mj.CHOLESKY else n - n // 3
    Ah, bh = SBS.cpu().numpy(), b.cpu().numpy()
    ref = LapackCPUSolver(np.asfortranarray(np.tril(Ah)), CHOLESKY if alg == mj.CHOLESKY else BUNCHKAUFMAN).factorize()
    assert ref.info == 0
    e_ref = _componentwise_backward_error(Ah, ref.solve_linear_system(bh.copy()), bh)
    assert e_ref > 0.0
    out = {"oracle": e_ref}
    for path, opts in _real_paths(n):
        x = _real_solve(ctx, SBS, b, alg, path, opts, n_pos, f"N={n} {alg} path {path}")
        e = _componentwise_backward_error(Ah, x.cpu().numpy(), bh)
        out[f"path{path}"], out[f"path{path}_over_oracle"] = e, e / e_ref
        print(f"N={n} {alg} path {path}: device {e:.3e}, oracle {e_ref:.3e}, ratio {e / e_ref:.2f}")
    _measured[f"{alg}-{n}"] = out
    for path, _ in _real_paths(n):
        assert out[f"path{path}"] <= ACCURACY_MARGIN * e_ref, (n, alg, path, out)


# ------------------------------------------------------------------------------- the device builder
def test_the_device_builder_forms_the_host_matrix(ctx):
    """device_system gives the bits of the host's S A S and S b (N = 700, scale_bits = 40, both sign modes)."""
    for alg in ALGS:
        c = _case(700, alg, 40)
        A, b = device_system(c, _dev())
        assert np.array_equal(A.cpu().numpy(), c.A) and np.array_equal(b.cpu().numpy(), c.b), alg

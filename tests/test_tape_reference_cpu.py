"""The tape compiler and the numpy interpreter (`madnlp_jl_amd.tape_model`) against a reference that shares nothing with them:
random expression trees evaluated in mpmath at 60 digits, derivatives by `mpmath.diff`, and a per-entry float64 error bound
from a running error analysis of the compiled tape (tests/tape_reference.py).  tests/test_hip_tape_reference.py holds the device
interpreter to the same reference."""
import functools

import numpy as np
import pytest
from mpmath import mpf

from madnlp_jl_amd import tape_model as T
from tests import tape_reference as R

SEEDS = tuple(range(8))
WIDE_SEED = 100                       # the group with k = 8, q = 4: Hessians of 36 pairs
ALL_OPS = set(range(10)) | set(range(16, 25))


@functools.lru_cache(maxsize=None)
def group(seed):
    if seed == WIDE_SEED:
        return R.kept_patterns(seed, count=5, k=8, q=4, depth=3, rows=6, wide=True)
    return R.kept_patterns(seed, count=25, k=3, q=2, depth=4, rows=6)


def check_pattern(pat, worst):
    """every row of a kept pattern: the compiled tapes in mpmath and in numpy against the tree's own value and derivatives"""
    k, nrow = pat.k, len(pat.points)
    xv, pv = [pat.x[:, j] for j in range(k)], [pat.p[:, c] for c in range(pat.q)]
    host = [t.run(xv, pv, nrow) for t in pat.tapes]
    d1_kept = pat.tapes[1].out_j.tolist()
    d2_kept = list(zip(pat.tapes[2].out_j.tolist(), pat.tapes[2].out_l.tolist()))
    assert len(set(d1_kept)) == len(d1_kept) and len(set(d2_kept)) == len(d2_kept) and all(j >= l for j, l in d2_kept)
    for r, (x, p) in enumerate(pat.points):
        ref = [[R.derivative(pat.tree, x, p, [0] * k)], [R.derivative(pat.tree, x, p, R.orders_of(k, j)) for j in d1_kept],
               [R.derivative(pat.tree, x, p, R.orders_of(k, j, l)) for j, l in d2_kept]]
        # what finalize() dropped from the sparsity pattern is exactly zero
        for j in range(k):
            if j not in d1_kept:
                assert abs(R.derivative(pat.tree, x, p, R.orders_of(k, j))) <= R.DIFF_NOISE, (pat.tree, j)
            for l in range(j + 1):
                if (j, l) not in d2_kept:
                    assert abs(R.derivative(pat.tree, x, p, R.orders_of(k, j, l))) <= R.DIFF_NOISE, (pat.tree, j, l)
        for w, tape in enumerate(pat.tapes):
            outs = R.run_tape(tape, x, p)
            assert len(outs) == len(ref[w]) == len(host[w])
            for o, (v, _, e_const, e_full) in enumerate(outs):
                what = (pat.tree, x, p, ("value", "first", "second")[w], o)
                # differentiation, folding, slot allocation: no float64 noise but the folded constants'
                assert abs(v - ref[w][o]) <= e_const + abs(ref[w][o]) * mpf(10) ** -40 + R.DIFF_NOISE * mpf(10) ** -10, what
                got = host[w][o][r]
                assert R.within(got, ref[w][o], e_full), (what, got, ref[w][o], e_full)
                if e_full > abs(ref[w][o]) * mpf(2) ** -60:
                    worst[0] = max(worst[0], float(abs(mpf(float(got)) - ref[w][o]) / e_full))


@pytest.mark.parametrize("seed", SEEDS + (WIDE_SEED,))
def test_compiled_tapes_and_numpy_interpreter_match_the_independent_reference(seed):
    pats, _ = group(seed)
    if seed == WIDE_SEED:
        assert sum(pat.tapes[2].nout == 36 for pat in pats) >= 3            # Hessians of all 36 pairs go through the check
    worst = [0.0]
    for pat in pats:
        check_pattern(pat, worst)
    print(f"seed {seed}: worst |numpy - reference| / bound = {worst[0]:.3f}")


def test_generator_covers_the_vocabulary_and_keeps_half_of_its_trees():
    kept = sum(len(group(s)[0]) for s in SEEDS)
    generated = sum(group(s)[1] for s in SEEDS)
    print(f"kept {kept} of {generated} trees")
    assert 2 * kept >= generated
    derivative_ops = set().union(*(R.opcodes(t) for s in SEEDS for pat in group(s)[0] for t in pat.tapes[1:]))
    assert derivative_ops >= ALL_OPS, sorted(ALL_OPS - derivative_ops)
    assert max(t.nslot for s in SEEDS for pat in group(s)[0] for t in pat.tapes) >= 24
    assert all(t.nslot <= T.SLOT_MAX for s in SEEDS + (WIDE_SEED,) for pat in group(s)[0] for t in pat.tapes)


def test_full_footprint_pattern_gives_the_exact_integers_on_the_numpy_interpreter():
    M = R.footprint_model()
    R.assert_footprint_shape(M)
    for x, y, w in R.footprint_points(M):
        R.check_footprint_outputs(M, x, y, w, M.obj(x), M.grad(x), M.cons(x), M.jac_coord(x), M.hess_coord(x, y, w))


def test_edge_arguments_on_the_numpy_interpreter():
    """+-0, subnormals, 1 +- 2^-52, +-710, 1e300, +-Inf, NaN, pi/2 on both sides, negative bases, 0 ** b: every entry of value,
    first and second derivative has the class (NaN, +-Inf, signed zero, finite) of the 60-digit value of the same tape under
    IEEE range rules and, where finite, lies within the bound"""
    M, x, names = R.edge_model()
    with np.errstate(all="ignore"):
        c, jv, hv = M.cons(x), M.jac_coord(x), M.hess_coord(x, np.ones(M.m))
    classes, misses = R.edge_findings(M, x, c, jv, hv, names)
    assert classes == {} and misses == []

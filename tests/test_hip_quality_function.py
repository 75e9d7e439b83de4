"""`mnk_ipm_quality_function` (csrc/ipm_vec.hip: the reductions of the adaptive barrier update's quality function, reference
src/IPM/barrier.jl:157-189) against a numpy mirror of its definition: along d = aff + sigma cen (product and sum rounded on
their own) the step lengths a_pr = get_alpha_max(x, xl, xu, d_x, tau) and a_du = get_alpha_z(zl_r, zu_r, d_zl, d_zu, tau),
both starting from 1 and NaN if the step holds a NaN, and the sums S_lb, S_ub of the squared complementarity products after
that step.  The step lengths are minima of the same elementwise expressions: bit-equal.  The terms of the sums are bit-equal
too and non-negative, so only the order of summation differs from the mirror's exact `math.fsum`: the longest chain of the
device sum is 2 sequential terms per thread at the largest shape plus two 8-level trees, 18 additions, within 64 * 2^-53."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TAU = 0.99
SUM_RTOL = 64 * 2.0 ** -53
SIGMAS = [0.37, 1.0, 1e-6, 42.0]
SHAPES = [(1, 1, 0),              # smallest legal size
          (5, 0, 0),              # no bounds at all
          (257, 100, 0),          # nub = 0
          (257, 0, 31),           # nlb = 0
          (1000, 1000, 1000),     # every entry bounded on both sides
          (70001, 65537, 300)]    # one past 256 blocks x 256 threads: the grid-stride loop takes a second trip


@pytest.fixture(scope="module")
def ctx():
    import madnlp_jl_amd as mj
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = mj.HipContext(0)
    yield c
    c.close()


def make(ntot, nlb, nub, seed=0):
    rng = np.random.default_rng(1000 * seed + ntot + nlb + nub)
    lb, ub = np.sort(rng.choice(ntot, nlb, replace=False)), np.sort(rng.choice(ntot, nub, replace=False))
    xl, xu = np.full(ntot, -np.inf), np.full(ntot, np.inf)
    xl[lb], xu[ub] = -rng.uniform(0.5, 2.0, nlb), rng.uniform(0.5, 2.0, nub)
    x = rng.uniform(-0.45, 0.45, ntot)                      # xl < x < xu
    zl, zu = np.zeros(ntot), np.zeros(ntot)
    zl[lb], zu[ub] = 10.0 ** rng.uniform(-6, 2, nlb), 10.0 ** rng.uniform(-6, 2, nub)     # positive duals
    step = lambda n: rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)               # noqa: E731  (both signs)
    return dict(lb=lb, ub=ub, x=x, xl=xl, xu=xu, zl=zl, zu=zu, aff_x=step(ntot), aff_zl=step(nlb), aff_zu=step(nub),
                cen_x=step(ntot), cen_zl=step(nlb), cen_zu=step(nub))


def mirror(d, sigma, tau=TAU):
    """The definition, in numpy: the same elementwise operations in the same order; exact sums."""
    lb, ub, x, xl, xu, zl, zu = (d[k] for k in ("lb", "ub", "x", "xl", "xu", "zl", "zu"))
    nan = float("nan")
    with np.errstate(all="ignore"):
        dx = d["aff_x"] + sigma * d["cen_x"]
        dzl = d["aff_zl"] + sigma * d["cen_zl"]
        dzu = d["aff_zu"] + sigma * d["cen_zu"]
        lo = np.where(dx < 0, (-x + xl) * tau / dx, np.inf)
        up = np.where(dx > 0, (-x + xu) * tau / dx, np.inf)
        v = np.minimum(lo, up)
        a_pr = nan if np.isnan(dx).any() or np.isnan(v).any() else min(1.0, float(v.min(initial=np.inf)))
        w = np.concatenate((np.where(dzl < 0, (-zl[lb]) * tau / dzl, np.inf), np.where(dzu < 0, (-zu[ub]) * tau / dzu, np.inf)))
        a_du = nan if np.isnan(dzl).any() or np.isnan(dzu).any() or np.isnan(w).any() else min(1.0, float(w.min(initial=np.inf)))
        t = (x[lb] + a_pr * dx[lb] - xl[lb]) * (zl[lb] + a_du * dzl)
        u = (xu[ub] - x[ub] - a_pr * dx[ub]) * (zu[ub] + a_du * dzu)
        return a_pr, a_du, math.fsum(t * t), math.fsum(u * u)


class Case:
    def __init__(self, ctx, d):
        import madnlp_jl_amd as mj
        self.d = d
        self.K = mj.IPMDeviceKernels(len(d["x"]), d["lb"], d["ub"], ctx=ctx)
        self.g = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items() if k not in ("lb", "ub")}

    def call(self, sigmas, tau=TAU):
        g = self.g
        return self.K.quality_function(sigmas, g["x"], g["xl"], g["xu"], g["zl"], g["zu"], g["aff_x"], g["aff_zl"], g["aff_zu"],
                                       g["cen_x"], g["cen_zl"], g["cen_zu"], tau)


def same_bits(a, b):
    return np.array_equal(np.array(a, dtype=np.float64).view(np.int64), np.array(b, dtype=np.float64).view(np.int64))


def check(got, d, sigmas):
    assert len(got) == len(sigmas)
    for (a_pr, a_du, s_lb, s_ub), sigma in zip(got, sigmas):
        m_pr, m_du, m_lb, m_ub = mirror(d, sigma)
        print(f"sigma={sigma:g} a_pr={a_pr!r} ({m_pr!r}) a_du={a_du!r} ({m_du!r}) S_lb={s_lb!r} ({m_lb!r}) S_ub={s_ub!r} ({m_ub!r})")
        assert same_bits(a_pr, m_pr) or (math.isnan(a_pr) and math.isnan(m_pr)), (sigma, a_pr, m_pr)
        assert same_bits(a_du, m_du) or (math.isnan(a_du) and math.isnan(m_du)), (sigma, a_du, m_du)
        for s, m in ((s_lb, m_lb), (s_ub, m_ub)):
            if math.isnan(m):
                assert math.isnan(s)
            else:
                assert abs(s - m) <= SUM_RTOL * abs(m), (sigma, s, m)


@pytest.mark.parametrize("nsigma", [1, 4])
@pytest.mark.parametrize("ntot,nlb,nub", SHAPES)
def test_quality_function_matches_the_mirror(ctx, ntot, nlb, nub, nsigma):
    d = make(ntot, nlb, nub)
    c = Case(ctx, d)
    sigmas = SIGMAS[:nsigma]
    got = c.call(sigmas)
    check(got, d, sigmas)
    if nlb == 0 and nub == 0:     # the identities: full dual step, empty sums
        assert all(g[1:] == (1.0, 0.0, 0.0) for g in got)
    again = c.call(sigmas)        # fixed order of the partial results: the same bits run to run
    assert all(same_bits(a, b) for a, b in zip(got, again))
    c.K.close()


def test_zero_primal_step_gives_a_full_primal_step_length(ctx):
    d = make(1000, 1000, 1000, seed=1)
    d["aff_x"][:] = 0.0
    d["cen_x"][:] = 0.0
    c = Case(ctx, d)
    got = c.call(SIGMAS)
    assert all(g[0] == 1.0 for g in got)
    check(got, d, SIGMAS)
    c.K.close()


def test_a_nan_in_the_centering_step_reaches_the_step_length_and_the_sums(ctx):
    d = make(1000, 1000, 1000, seed=2)
    d["cen_x"][617] = float("nan")
    c = Case(ctx, d)
    got = c.call(SIGMAS)
    for a_pr, a_du, s_lb, s_ub in got:
        assert math.isnan(a_pr) and math.isnan(s_lb) and math.isnan(s_ub)
        assert not math.isnan(a_du)
    check(got, d, SIGMAS)
    c.K.close()


def test_two_calls_in_one_batch_are_filled_when_it_ends(ctx):
    d = make(70001, 65537, 300, seed=3)
    c = Case(ctx, d)
    s1, s2 = SIGMAS, [0.5, 0.25, 2.0, 1.0 - 1e-4]
    r1, r2 = c.call(s1), c.call(s2)
    with c.K.batch():
        b1 = c.call(s1)
        b2 = c.call(s2)
    assert len(b1) == len(b2) == 16      # 16 + 16 slots: the batch's 32
    flat = lambda r: [v for t in r for v in t]   # noqa: E731
    assert same_bits(list(b1), flat(r1)) and same_bits(list(b2), flat(r2))
    check([tuple(b2[4 * i:4 * i + 4]) for i in range(4)], d, s2)
    assert all(same_bits(a, b) for a, b in zip(c.call(s1), r1))      # plain calls work again after the batch
    c.K.close()


def test_a_bad_number_of_sigmas_is_an_error_and_writes_nothing(ctx):
    import madnlp_jl_amd as mj
    from madnlp_jl_amd import _lib as L
    d = make(257, 100, 0, seed=4)
    c = Case(ctx, d)
    g = c.g
    out = (C.c_double * 24)(*([-7.0] * 24))
    sig = (C.c_double * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    ptr = lambda k: g[k].data_ptr() if g[k].numel() else None   # noqa: E731
    args = [ptr(k) for k in ("x", "xl", "xu", "zl", "zu", "aff_x", "aff_zl", "aff_zu", "cen_x", "cen_zl", "cen_zu")]
    for n in (5, 0, -1):
        assert L.lib().mnk_ipm_quality_function(c.K._h, n, sig, *args, TAU, out) != 0
        assert b"nsigma" in L.lib().mnk_last_error_string()
    assert L.lib().mnk_ipm_quality_function(c.K._h, 2, sig, None, *args[1:], TAU, out) != 0     # a NULL vector
    assert L.lib().mnk_ipm_quality_function(c.K._h, 2, None, *args, TAU, out) != 0              # NULL sigmas
    assert list(out) == [-7.0] * 24
    with pytest.raises(mj.HipError):
        c.call([0.1, 0.2, 0.3, 0.4, 0.5])
    check(c.call(SIGMAS[:2]), d, SIGMAS[:2])      # the handle is usable afterwards
    c.K.close()

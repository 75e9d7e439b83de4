"""The premise of tests/test_hip_solve_exact.py, checked without a GPU: on the systems of tests/solve_exact.py the blocked solve
with explicit block inverses has one answer in fp64 whatever the order of its sums -- and no slack for an error of one ulp."""
import numpy as np
import pytest

from tests.solve_exact import MI355X_CUS, bit_budget, emulated_solve, ownership_orders, solve_case

SIZES = [1, 63, 257, 700, 1300, 4160]
BIT_CAP = 40      # of 53: a condition on the data (another seed or per_row where an order breaks it), never to be raised


@pytest.mark.parametrize("scale_bits", [0, 40])
@pytest.mark.parametrize("positive", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_the_blocked_solve_is_exact_in_every_summation_order(n, positive, scale_bits):
    """b is the longdouble product A x; the a-priori bound on the significant bits of any partial sum is <= 40; the emulation
    of the blocked solve (explicit inverses of 256- and 512-column steps, shuffled sums) returns x bit for bit."""
    c = solve_case(n, 100 + n, positive, scale_bits)
    assert sum(c.inertia()) == n and (c.inertia() == (n, 0, 0)) == (positive or n == 1 and c.d[0] > 0)
    assert np.array_equal(c.A, c.A.T)
    bl = c.A.astype(np.longdouble) @ c.x.astype(np.longdouble)
    assert np.array_equal(c.b.astype(np.longdouble), bl), "b is not the exact product"
    assert np.array_equal(np.ldexp(c.x, c.k), c.xstar) and (scale_bits == 0 or n < 63 or np.ptp(c.k) >= scale_bits - 4)
    assert bit_budget(c) <= BIT_CAP, bit_budget(c)
    rng = np.random.default_rng(n)
    for step in (256, 512):
        x = emulated_solve(c, step, rng)
        assert np.array_equal(x, c.x), (step, np.flatnonzero(x != c.x)[:8])


@pytest.mark.parametrize("positive", [True, False])
def test_the_bit_budget_of_the_device_built_orders(positive):
    """The two orders at which block ownership wraps around on the 256 CUs of an MI355X, and the other orders the GPU tests
    build on the device: the bound from the sparse factors alone is <= 40 (the GPU tests check it again for the device they run
    on)."""
    n2, n3 = ownership_orders(MI355X_CUS)
    assert (n2, n3) == (16581, 8355)
    for n in (2100, 3968, 4096, 4100, 4480, 5000, n3, n2):
        for scale_bits in (0, 40):
            c = solve_case(n, 100 + n, positive, scale_bits, dense=False)
            assert c.A is None and bit_budget(c) <= BIT_CAP, (n, bit_budget(c))


@pytest.mark.parametrize("step", [256, 512])
def test_one_ulp_in_one_product_is_not_absorbed(step):
    """The emulation with ONE product multiplied by 1 + 2^-52 does not return x: the diagonal term of the last row in the
    backward product with the inverse (that product is the row's solution), and its D^-1 scaling.  The answer moves by one ulp
    in that entry and nowhere else."""
    n = 700
    c = solve_case(n, 100 + n, False, 40)
    last = n - 1
    assert c.xstar[last] != 0.0
    for bump in (("bwd", last), ("dinv", last)):
        x = emulated_solve(c, step, np.random.default_rng(5), bump=bump)
        bad = np.flatnonzero(x != c.x)
        assert bad.tolist() == [last], (bump, bad[:8])
        assert abs(x[last] - c.x[last]) <= 2 * np.spacing(abs(c.x[last])), bump    # (one ulp, no more: the data has no slack)
    # the same seeds without the bump: exact
    assert np.array_equal(emulated_solve(c, step, np.random.default_rng(5)), c.x)
    cp = solve_case(n, 100 + n, True, 0)
    x = emulated_solve(cp, step, np.random.default_rng(5), bump=("bwd", last))
    assert x[last] != cp.x[last] and np.array_equal(x[:last], cp.x[:last])

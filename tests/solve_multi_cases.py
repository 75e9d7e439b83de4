"""Exact systems with several right-hand sides for the blocked solve (SOLVE_BLOCKED, csrc/solve_multi.hip); helper module of
tests/test_solve_multi_cpu.py and tests/test_hip_solve_multi.py, not collected by pytest.

One matrix of tests/solve_exact.py per (n, algorithm, scale_bits) and R distinct dyadic solutions: column r is drawn like the
x* of `solve_case` under a seed of its own, and some columns are multiplied by +-2^k (a power of two commutes with every
operation of the solve, so it changes no bit budget).  B = A X* column by column from the sparse factors.  Every column keeps
`bit_budget` <= BIT_CAP (asserted when the case is built), so every grouping of the sums of the two sweeps -- the MFMA's too --
returns X* bit for bit, and `emulated_solve` does so column by column (tests/test_solve_multi_cpu.py)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests.solve_exact import SolveCase, bit_budget, solve_case

BIT_CAP = 40                        # the cap of tests/test_hip_solve_exact.py
COLUMN_SCALES = (0, 0, 3, 0, -2, 7)  # exponent of column r's factor: 2^COLUMN_SCALES[r % 6], negated for every fourth column

CHOLESKY_LIKE, LDL_LIKE = True, False   # `positive` of solve_case

# (n, right-hand sides, scale_bits) of the GPU tests, W = 64 being the chunk width the planner reports: every order with at least
# two widths, every width with n = 700; n = 4100 is built on the device
W = 64
WIDTHS = (4, 15, 16, 17, W - 1, W, W + 1, 2 * W + 2)
GPU_CASES = ([(700, r, 0) for r in WIDTHS] +
             [(1, 4, 0), (1, 17, 0), (63, 15, 0), (63, W + 1, 0), (65, 16, 0), (65, W - 1, 0), (256, 4, 0), (256, W, 0),
              (257, 17, 0), (257, 2 * W + 2, 0), (1300, 16, 0), (1300, W + 1, 0), (257, 17, 40)])
DEVICE_CASE = (4100, W + 1, 0)


@dataclasses.dataclass
class MultiCase:
    base: SolveCase          # the matrix (and column 0's unscaled solution)
    xstars: np.ndarray       # n x R: the unscaled solutions, before the columns' own factors
    colscale: np.ndarray     # R: +-2^k per column

    @property
    def n(self):
        return self.base.n

    @property
    def R(self):
        return self.xstars.shape[1]

    def column(self, r) -> SolveCase:
        """The single-vector case of column r without its factor."""
        return dataclasses.replace(self.base, xstar=self.xstars[:, r])

    @property
    def X(self):
        """The solution of the scaled system, n x R column-major."""
        return np.asfortranarray(np.stack([self.column(r).x * self.colscale[r] for r in range(self.R)], axis=1))

    @property
    def B(self):
        return np.asfortranarray(np.stack([self.column(r).b * self.colscale[r] for r in range(self.R)], axis=1))

    def budgets(self):
        return [bit_budget(self.column(r)) for r in range(self.R)]


@functools.lru_cache(maxsize=None)
def multi_case(n: int, positive: bool, scale_bits: int, R: int, variant: int = 0) -> MultiCase:
    """The case of order n (seed 100 + n, as the single-vector tests; `variant`: another matrix of the same order) with R
    right-hand sides; dense on the host below 2000 rows."""
    seed = 100 + n + 7919 * variant
    base = solve_case(n, seed, positive, scale_bits, dense=n < 2000)
    xs = np.empty((n, R))
    for r in range(R):
        rng = np.random.default_rng([seed, 77, r])
        xs[:, r] = rng.integers(-8, 9, size=n) * rng.choice([1.0, 0.5, 0.25], size=n)
    colscale = np.array([np.ldexp(-1.0 if r % 4 == 3 else 1.0, COLUMN_SCALES[r % len(COLUMN_SCALES)]) for r in range(R)])
    mc = MultiCase(base, xs, colscale)
    budgets = mc.budgets()
    assert max(budgets) <= BIT_CAP, (n, positive, scale_bits, R, max(budgets))
    return mc

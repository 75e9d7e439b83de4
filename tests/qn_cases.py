"""Inputs and yardstick shared by the quasi-Newton tests (tests/test_quasi_newton_cpu.py, tests/test_hip_quasi_newton.py).

Yardstick: the update written out directly in `np.longdouble`,

    B' = B - (B s)(B s)' / (s' B s) + r r' / (r' s),      B = Symmetric(lower triangle), r = y (BFGS) or the damped r,

with the error bound of item 1 of the issue: an entry of B' is a length-n product (B s) followed by O(1) operations, so
a float64 implementation stays within a small multiple of n eps of the sizes of its three terms,
`scale = max|B| + max|B s|^2 / (s' B s) + max|r|^2 / |r' s|`.

Two families of inputs:

* `random_case`: well conditioned on purpose (s'y and s'Bs are not small against |s||y|, |s||Bs|: y = M s with M SPD), so
  that the bound above is the right yardstick; the strict upper triangle holds NaN (whoever reads it fails).
* `exact_case`: integer B, s in {0, +-1}, integer y, s'Bs and s'y powers of two (theta = 1 for the damped update): every
  intermediate is a small dyadic rational, any summation order gives the same bits, and results are compared with
  `np.array_equal`.
"""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def sym_lower(B, dtype=np.float64):
    """Symmetric(B, :L) as a full matrix."""
    L = np.tril(np.asarray(B, dtype=dtype))
    return L + np.tril(L, -1).T


def formula(B, s, y, kind, first=False):
    """The update in longdouble.  kind: "bfgs" / "damped_bfgs"; `first`: the diagonal is first overwritten with s'y / s's.
    Returns a dict: `B1` (full symmetric, longdouble), `performed`, the scalars and `scale`."""
    n = len(s)
    Bs = sym_lower(B, LD)
    s, y = np.asarray(s, LD), np.asarray(y, LD)
    sy = s @ y
    if kind == "bfgs" and float(s.astype(np.float64) @ y.astype(np.float64)) < 1e-8:
        return dict(B1=Bs, performed=False, sy=sy, sBs=LD(0), theta=LD(1), rs=sy, scale=float(np.abs(Bs).max()))
    if first:
        Bs[np.diag_indices(n)] = sy / (s @ s)
    bs = Bs @ s
    sBs = s @ bs
    theta = LD(1)
    if kind == "damped_bfgs" and sy < LD(0.2) * sBs:
        theta = LD(0.8) * sBs / (sBs - sy)
    r = theta * y + (1 - theta) * bs if kind == "damped_bfgs" else y
    rs = r @ s
    B1 = Bs - np.outer(bs, bs) / sBs + np.outer(r, r) / rs
    scale = float(np.abs(Bs).max() + np.abs(bs).max() ** 2 / sBs + np.abs(r).max() ** 2 / abs(rs))
    return dict(B1=B1, performed=True, sy=sy, sBs=sBs, theta=theta, rs=rs, scale=scale, bs=bs, r=r)


def tril_err(B, ref):
    """max |tril(B - ref)| in longdouble."""
    return float(np.abs(np.tril(np.asarray(B, LD) - ref)).max())


def _spd(rng, n):
    A = rng.standard_normal((n, min(n, 64)))
    return A @ A.T / A.shape[1] + np.eye(n)


def random_case(n, seed, mode="bfgs"):
    """(B, s, y, kind): B is SPD in its lower triangle, NaN in the strict upper one.  mode: "bfgs" (s'y > 0),
    "damped" (theta = 1), "damped_lt1" (s'y < 0.2 s'Bs: theta < 1), "damped_neg" (s'y < 0: BFGS would skip, damped does
    not), "skip" (BFGS with s'y < 1e-8)."""
    rng = np.random.default_rng(seed)
    B = _spd(rng, n)
    s = rng.standard_normal(n)
    M = _spd(rng, n)
    bs = sym_lower(B) @ s
    if mode in ("bfgs", "damped"):
        y = 2.0 * (M @ s)                 # s'y = 2 s'Ms >= 2 s's, s'Bs of the same size: theta = 1
        if mode == "damped":
            y = bs + 0.5 * (M @ s)        # s'y > s'Bs
    elif mode == "damped_lt1":
        y = 0.05 * bs + 0.01 * (M @ s)    # s'y ~ 0.06 s'Bs < 0.2 s'Bs
    elif mode == "damped_neg":
        y = -0.5 * (M @ s)
    elif mode == "skip":
        y = -(M @ s)
    else:
        raise ValueError(mode)
    B = np.asfortranarray(np.tril(B))
    B[np.triu_indices(n, 1)] = np.nan
    kind = "bfgs" if mode in ("bfgs", "skip") else "damped_bfgs"
    return B, s, y, kind


def exact_case(n, seed, kind, first=False):
    """(B, s, y): integers with s'y = s'Bs = a power of two (so theta = 1), s in {0, +-1}.  With `first` the number of
    nonzeros of s is a power of two as well, so that the diagonal reset s'y / s's is dyadic, and s'Bs is a power of two
    AFTER the reset.  The strict upper triangle holds NaN."""
    rng = np.random.default_rng(seed)
    nnz = max(2, 1 << int(np.log2(max(2, (2 * n) // 3))))        # a power of two <= n
    nnz = min(nnz, 1 << int(np.log2(n)))
    s = np.zeros(n)
    idx = np.sort(rng.choice(n, nnz, replace=False))
    s[idx] = rng.choice([-1.0, 1.0], nnz)
    B = np.tril(rng.integers(-3, 4, (n, n)).astype(np.float64))
    y = rng.integers(-4, 5, n).astype(np.float64)
    P = float(1 << int(np.ceil(np.log2(16.0 * n))))               # the common value of s'y and s'Bs
    y[idx[0]] += s[idx[0]] * (P - s @ y)
    assert s @ y == P
    if first:
        B[np.diag_indices(n)] = P / nnz                           # what the reset will write (the update must not need it)
        q = s @ (sym_lower(B) @ s)                                # = P + 2 sum_{i > j} s_i s_j B_ij
        i, j = idx[1], idx[0]
        B[i, j] += s[i] * s[j] * (P - q) / 2.0
        Bchk = B.copy()
        B[np.diag_indices(n)] = rng.integers(-3, 4, n)            # overwritten by the reset
    else:
        q = s @ (sym_lower(B) @ s)
        B[idx[0], idx[0]] += P - q
        Bchk = B
    assert s @ (sym_lower(Bchk) @ s) == P
    B = np.asfortranarray(B)
    B[np.triu_indices(n, 1)] = np.nan
    return B, s, y

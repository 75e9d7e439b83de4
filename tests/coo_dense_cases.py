"""Shared builders of the tests of COO callbacks on the dense KKT systems (`IPMOptions.callback = "sparse"` with
`sparse=False`; csrc/dense_coo.hip): the "hyperbola" model with its closed-form answer, random COO structures, and the
sequential host scatters the device kernels must reproduce bit for bit."""
import numpy as np

from madnlp_jl_amd.tape_model import TapeModel, V

# min x0^2 + x1^2  s.t.  x0 x1 = 1,  x0 + x1^2 <= 3,  0.1 <= x <= 10,  from (2, 0.3).  On x0 x1 = 1 the objective x0^2 + 1 / x0^2
# is minimal at x0 = 1: x = (1, 1), f = 2; there x0 + x1^2 = 2 < 3 is inactive and (2, 2) + y0 (1, 1) = 0 gives y = (-2, 0).
HYPERBOLA_X, HYPERBOLA_F, HYPERBOLA_Y = np.array([1.0, 1.0]), 2.0, np.array([-2.0, 0.0])


def hyperbola_model():
    M = TapeModel(2, 2, np.array([2.0, 0.3]), 0.1, 10.0, np.array([1.0, -np.inf]), np.array([1.0, 3.0]), name="hyperbola")
    xy = np.array([[0, 1]])
    M.add_objective(V(0) * V(0) + V(1) * V(1), xy)
    M.add_constraint(V(0) * V(1), np.array([0]), xy)
    M.add_constraint(V(0) + V(1) * V(1), np.array([1]), xy)
    return M.finalize()


SIZES = [(1, 1), (3, 5), (70, 130), (257, 300)]     # (m, n); the last: more than 256 distinct destinations, no multiple of 256
MAX_DUP = 40


def _feed(rng, dests, ndup_first):
    """COO positions for the distinct destinations `dests` (k x 2): the first one `ndup_first` times, the others 1 .. 3 times,
    all shuffled."""
    reps = rng.integers(1, 4, len(dests))
    reps[0] = ndup_first
    out = np.repeat(dests, reps, axis=0)
    return out[rng.permutation(len(out))]


def random_structure(m, n, seed=0):
    """dict(jac_I, jac_J, hess_I, hess_J), int32, 0-based: up to MAX_DUP duplicates on one destination; diagonal, lower and
    upper Hessian entries (also both orientations of one pair); empty rows and columns where the size leaves room for them."""
    rng = np.random.default_rng(1000 * m + n + seed)
    rows = np.sort(rng.choice(m, max(1, m - m // 4), replace=False))           # a quarter of the rows / columns stay empty
    cols = np.sort(rng.choice(n, max(1, n - n // 4), replace=False))
    nd = min(len(rows) * len(cols), 2 * (m + n))
    flat = rng.choice(len(rows) * len(cols), nd, replace=False)
    jd = np.stack([rows[flat // len(cols)], cols[flat % len(cols)]], axis=1)
    J = _feed(rng, jd, MAX_DUP)
    npairs = min(len(cols) * (len(cols) + 1) // 2, 3 * n)
    tri = np.stack(np.tril_indices(len(cols)), axis=1)
    hd = cols[tri[rng.choice(len(tri), npairs, replace=False)]]                # i >= j
    if len(cols) > 1:                                                          # a diagonal and an off-diagonal pair for certain
        hd[0] = (cols[0], cols[0])
        hd[1] = (cols[1], cols[0])
        hd = np.unique(hd, axis=0)
        hd = hd[rng.permutation(len(hd))]
    H = _feed(rng, hd, MAX_DUP)
    flip = rng.random(len(H)) < 0.5                                            # the upper-triangular orientation
    H[flip] = H[flip][:, ::-1]
    S = dict(jac_I=J[:, 0], jac_J=J[:, 1], hess_I=H[:, 0], hess_J=H[:, 1])
    S = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in S.items()}
    # what the tests rely on
    jcount = np.unique(J, axis=0, return_counts=True)[1]
    hcount = np.unique(np.sort(H, axis=1), axis=0, return_counts=True)[1]
    assert jcount.max() == MAX_DUP and hcount.max() == MAX_DUP
    if n > 1:
        assert (S["hess_I"] == S["hess_J"]).any() and (S["hess_I"] > S["hess_J"]).any() and (S["hess_I"] < S["hess_J"]).any()
    if m > 3 and n > 3:
        assert len(np.unique(S["jac_I"])) < m and len(np.unique(S["jac_J"])) < n and len(np.unique(H)) < n
    if (m, n) == SIZES[-1]:
        for cnt in (len(jcount), len(hcount)):
            assert cnt > 256 and cnt % 256 != 0, cnt
    return S


def host_scatter_jac(m, n, I, J, v):
    """Zero, then the values added entry by entry in COO order (`np.add.at` is that loop)."""
    out = np.zeros((m, n), order="F")
    np.add.at(out, (np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)), v)
    return out


def host_scatter_hess(n, I, J, v):
    """The reference's loop (nlpmodels.jl:863-881): hess[i, j] += v and, where i != j, hess[j, i] += v, in COO order."""
    out = np.zeros((n, n), order="F")
    for i, j, t in zip(np.asarray(I).tolist(), np.asarray(J).tolist(), np.asarray(v).tolist()):
        out[i, j] += t
        if i != j:
            out[j, i] += t
    return out


def host_jtprod(n, I, J, v, y):
    """out[j] = sum over the entries of column j, in COO order, of v[k] * y[I[k]], from 0."""
    out = np.zeros(n)
    np.add.at(out, np.asarray(J, dtype=np.int64), v * y[np.asarray(I, dtype=np.int64)])
    return out


def spread_values(rng, k):
    """Magnitudes spread over 1e-8 .. 1e8, mixed signs."""
    return rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-8, 8, k)

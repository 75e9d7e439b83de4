"""`SchurComplementKKTSystem` on the MI355X: the reference's KKT system for two-stage stochastic programs
(`src/KKT/Schur/schur.jl:72-1146`) around the HIP `S` stage of `schur.py` / `csrc/schur.hip`.

Variable layout `[v_1 .. v_ns (nv each), d (nd)]`, constraint layout `[c_1 .. c_ns (nc each)]`.  Per iteration
(`build_kkt!`, reference :927-1001) every scenario contributes a block

    A_k  = [ H_kk + Sigma_k + J_I,k' D_I J_I,k    J_E,k' ]        C_dk = [ H_dk + J_I,d' D_I J_I,k    J_E,d' ]
           [ J_E,k                                 du_diag_E ]               (nd x blk)

of order blk = nv + (equality rows per scenario) -- the scenario's INEQUALITY rows are condensed (D_I = Sigma_s /
(1 - Sigma_d Sigma_s), the `diag_buffer` of the condensed systems), its equality rows stay -- and the design block starts as
`S = H_dd + Sigma_d + sum_k J_I,d' D_I J_I,d`.  The device then factors the ns blocks as ONE batch, forms
`S -= sum_k C_dk A_k^-1 C_dk'` on the matrix cores and factors S (`mnk_schur_build_local`, `mnk_schur_factorize_s`);
`solve_kkt!` (:1040-1110) runs the forward / design / backward steps of the stage between the host-side condensation and
recovery of the inequality rows.  Inertia is judged on S alone, as the reference does (:901-903).

What is host-side here by default: the vector algebra around the three device steps; with `device_kkt_ops=True` all of
`solve_kkt!`, `mul!`, `jtprod!` and `mul_hess_blk!` runs inside the handle instead (`mnk_schur_solve_kkt` and its kin, on host
vectors or device tensors), and `solve_kkt_ordered` / `mul_ordered` / `jtprod_ordered` / `mul_hess_blk_ordered` mirror those
kernels operation by operation on the host (the comparator of tests/test_hip_schur_device_ops.py).  The scatter of the COO values into the dense
blocks (the reference: precomputed index maps on the CPU, nine @atomic kernels in its CUDA extension) runs on the device since
round 6 (`mnk_schur_set_structure` once, `mnk_schur_assemble` per iteration).  The product path has no CPU fallback for the factorizations and solves: they are the HIP stage's."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from fractions import Fraction

from . import _lib as L
from .kkt import _KKTCommon
from .linear_solver import HipContext, _LIVE_OBJECTS, _ptr
from .schur import OP_H, OP_J, OP_JT, SPMV_DEFAULT_T, SchurDenseStage, spmv_plan


def ordered_spmv(ptr, idx, perm, vals, x, T, alpha=1.0, beta=0.0, y=None):
    """`alpha Op x (+ beta y when beta != 0)` in the order of the device kernels (`schur_spmv_rows_kernel`,
    `schur_spmv_long_kernel`, csrc/schur.hip), operation by operation in fp64 and without fused multiply-adds: the products
    vals[perm[q]] * x[idx[q]] are rounded; a row of at most T entries is summed front to back; a longer one in 64 lanes -- lane l
    sums its entries l, l + 64, ... in ascending order -- whose partials a xor-butterfly with offsets 32, 16, ..., 1 combines."""
    ptr = np.asarray(ptr, dtype=np.int64)
    rows = len(ptr) - 1
    acc = np.zeros(rows)
    lane = np.arange(64)
    for r in range(rows):
        q0, q1 = ptr[r], ptr[r + 1]
        if q1 == q0:
            continue
        t = vals[perm[q0:q1]] * x[idx[q0:q1]]
        if q1 - q0 <= T:
            acc[r] = np.add.accumulate(t)[-1]
            continue
        part = np.zeros(64)
        for j in range(0, len(t), 64):
            c = t[j:j + 64]
            part[:len(c)] = part[:len(c)] + c
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[lane ^ off]
        acc[r] = part[0]
    out = alpha * acc
    if beta != 0.0:
        out = out + beta * np.asarray(y)
    return out


def _fma(a, b, c):
    """round(a * b + c) entry by entry (the bound kernels of csrc/kkt_vec.h are compiled with contraction: their fused
    multiply-adds are part of the device result's bits)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def build_schur_symbolic(n, m, ns, nv, nd, nc, hess_I, hess_J, jac_I, jac_J, ind_eq, ind_ineq):
    """The layout checks of the reference's `_build_schur_symbolic` (schur.jl:140-600; error cases of test/schur_test.jl:176-236)
    and the per-scenario row sets.  0-based indices.  Raises ValueError where the reference throws an ErrorException:
    a Hessian entry that couples two scenarios, a constraint that reaches another scenario's variables, equality / inequality
    counts that differ between scenarios, a sparsity pattern that differs between scenarios."""
    if n != ns * nv + nd or m != ns * nc:
        raise ValueError(f"SchurComplementKKTSystem: n = {n}, m = {m} do not match ns * nv + nd = {ns * nv + nd}, ns * nc = {ns * nc}")
    hess_I, hess_J, jac_I, jac_J = (np.asarray(a, dtype=np.int64) for a in (hess_I, hess_J, jac_I, jac_J))
    off = ns * nv
    scen_of_var = np.where(np.arange(n) < off, np.arange(n) // max(nv, 1), -1)   # -1: design
    hi, hj = scen_of_var[hess_I], scen_of_var[hess_J]
    if ((hi >= 0) & (hj >= 0) & (hi != hj)).any():
        raise ValueError("SchurComplementKKTSystem: a Hessian entry couples two scenarios")
    con_s = jac_I // max(nc, 1)
    vs = scen_of_var[jac_J]
    if ((vs >= 0) & (vs != con_s)).any():
        raise ValueError("SchurComplementKKTSystem: a constraint reaches the variables of another scenario")
    ind_eq, ind_ineq = np.asarray(ind_eq, dtype=np.int64), np.asarray(ind_ineq, dtype=np.int64)
    eq_rows = [np.sort(ind_eq[ind_eq // max(nc, 1) == k]) for k in range(ns)]
    ineq_pos = [np.nonzero(ind_ineq // max(nc, 1) == k)[0] for k in range(ns)]      # positions in ind_ineq (= slack index)
    if len({len(r) for r in eq_rows}) > 1 or len({len(r) for r in ineq_pos}) > 1:
        raise ValueError("SchurComplementKKTSystem: the scenarios have different numbers of equality / inequality constraints")
    # the same local pattern in every scenario (the reference builds ONE symbolic block and reuses it)
    def local_pattern(k):
        lo_i, lo_j = np.maximum(hess_I, hess_J), np.minimum(hess_I, hess_J)
        sel = (scen_of_var[lo_i] == k) & (scen_of_var[lo_j] == k)
        hp = set(zip((lo_i[sel] - k * nv).tolist(), (lo_j[sel] - k * nv).tolist()))
        selj = (con_s == k) & (vs == k)
        jp = set(zip((jac_I[selj] - k * nc).tolist(), (jac_J[selj] - k * nv).tolist()))
        return hp, jp
    if ns > 0:
        p0 = local_pattern(0)
        for k in range(1, ns):
            if local_pattern(k) != p0:
                raise ValueError("SchurComplementKKTSystem: the sparsity pattern differs between scenarios")
    return dict(eq_rows=eq_rows, ineq_pos=ineq_pos, nc_eq=len(eq_rows[0]) if ns else 0, nc_ineq=len(ineq_pos[0]) if ns else 0)


class _DesignSolver:
    """What the interior-point loop sees as `kkt.linear_solver`: the solver of the design block S (reference :868-870,
    `factorize_kkt!` :1003-1005).  The scenario blocks are factored inside `build_kkt!`."""

    def __init__(self, stage):
        self.stage = stage
        self.info = 0

    def factorize(self):
        self.info = self.stage.factorize_kkt()
        return self

    def inertia(self):
        return self.stage.inertia()

    def is_inertia(self):
        return True

    def improve(self):
        return False

    def introduce(self):
        return "HIP-MI355X Schur stage (scenario blocks: batched LDL', design block: dense LDL')"


class SchurComplementKKTSystem(_KKTCommon):
    """reference `src/KKT/Schur/schur.jl:72-140` (fields), `:927-1001` (`build_kkt!`), `:1040-1110` (`solve_kkt!`),
    `:1113-1146` (`mul!`, `mul_hess_blk!`)."""

    _PFX = "mnk_schur"
    device_assembly = True     # False: the host assembly of rounds 4-5 (diagnostic A/B runs)
    device_kkt_ops = False     # True: solve_kkt! / mul! / jtprod! / mul_hess_blk! inside the handle (mnk_schur_solve_kkt and its kin)

    def __init__(self, n, m, jac_I, jac_J, hess_I, hess_J, ind_ineq, ind_eq, ind_lb, ind_ub, ns, nv, nd, nc, ctx=None, gram_row_threshold=None,
                 device_kkt_ops=False, spmv_row_threshold=None):
        import torch
        self.torch = torch
        sym = build_schur_symbolic(n, m, ns, nv, nd, nc, hess_I, hess_J, jac_I, jac_J, ind_eq, ind_ineq)
        self.n, self.m, self.ns, self.nv, self.nd, self.nc = n, m, ns, nv, nd, nc
        self.n_ineq, self.n_eq = len(ind_ineq), len(ind_eq)
        self.nc_eq, self.nc_ineq = sym["nc_eq"], sym["nc_ineq"]
        self.blk = nv + self.nc_eq
        self.eq_rows, self.ineq_pos = sym["eq_rows"], sym["ineq_pos"]
        self.ind_ineq = np.asarray(ind_ineq, dtype=np.int64)
        self.ind_eq = np.asarray(ind_eq, dtype=np.int64)
        self.ind_lb = np.asarray(ind_lb, dtype=np.int64)
        self.ind_ub = np.asarray(ind_ub, dtype=np.int64)
        self.jac_I, self.jac_J = np.asarray(jac_I, dtype=np.int64), np.asarray(jac_J, dtype=np.int64)
        hI, hJ = np.asarray(hess_I, dtype=np.int64), np.asarray(hess_J, dtype=np.int64)
        self.hess_I, self.hess_J = np.maximum(hI, hJ), np.minimum(hI, hJ)       # force_lower_triangular!
        self.hess = np.zeros(len(hI))
        self.jac = np.zeros(len(self.jac_I))
        nt = n + self.n_ineq
        self.reg, self.pr_diag, self.du_diag = np.zeros(nt), np.zeros(nt), np.zeros(m)
        nlb, nub = len(ind_lb), len(ind_ub)
        self.l_diag, self.u_diag = np.ones(nlb), np.ones(nub)
        self.l_lower, self.u_lower = np.zeros(nlb), np.zeros(nub)
        self.diag_buffer = np.zeros(self.n_ineq)
        self.buffer = np.zeros(m)
        self.J = sp.csr_matrix((m, n))
        self.H = sp.csr_matrix((n, n))
        self.ctx = ctx or HipContext()
        zA = [np.eye(self.blk) for _ in range(ns)]
        zC = [np.zeros((nd, self.blk)) for _ in range(ns)]
        self.stage = SchurDenseStage(zA, zC, np.eye(nd), nd, self.blk, ctx=self.ctx)
        # the index maps of `_build_schur_symbolic` (reference :460-700) live in the library: one source list per touched entry of
        # A_k / C_dk / S0, built from the COO patterns once; inequality rows with more than `gram_row_threshold` entries are condensed
        # as Gram products on the matrix cores instead (None: the library's default)
        # ... and so do the row lists of J, J' and Symmetric(H, :L) the device-side products run over; a row with more than
        # `spmv_row_threshold` entries (the design rows collect entries of every scenario) gets a wavefront instead of a thread
        self.stage.set_structure(n, m, nv, nc, self.hess_I, self.hess_J, self.jac_I, self.jac_J, self.ind_ineq, self.ind_eq,
                                 gram_row_threshold=gram_row_threshold, spmv_row_threshold=spmv_row_threshold)
        self.spmv_T = SPMV_DEFAULT_T if spmv_row_threshold is None or spmv_row_threshold < 0 else int(spmv_row_threshold)
        self._row_lists = None
        self.device_kkt_ops = bool(device_kkt_ops)
        self._set_bounds()
        self.aug_com = self.stage.S
        self.linear_solver = _DesignSolver(self.stage)
        self._order = nd
        _LIVE_OBJECTS.add(self)

    # ---- interface pieces
    @property
    def _h(self):
        """The `mnk_schur` handle the shared device entry points of `_KKTCommon` go to."""
        return self.stage._h

    def _solve_kkt_solver(self):
        return ()

    def num_variables(self):
        return self.n

    def is_inertia_correct(self, num_pos, num_zero, num_neg):
        """reference :901-903."""
        return num_zero == 0 and num_pos == self.nd

    def should_regularize_dual(self, num_pos, num_zero, num_neg):
        """reference :905."""
        return True

    def compress_jacobian(self):
        """reference :917-919 (COO -> CSC transfer): here the CSR matrix the products use."""
        self.J = sp.csr_matrix((self.jac, (self.jac_I, self.jac_J)), shape=(self.m, self.n))
        if self.device_kkt_ops:   # jtprod! runs on the handle's copy of the values, and before the next build_kkt!
            self._call("_compress_jacobian", self.jac.ctypes.data, L.MNK_HOST)

    def compress_hessian(self):
        """reference :921-923."""
        Lo = sp.csr_matrix((self.hess, (self.hess_I, self.hess_J)), shape=(self.n, self.n))
        self.H = Lo + sp.tril(Lo, -1).T
        if self.device_kkt_ops:
            self._call("_compress_hessian", self.hess.ctypes.data, L.MNK_HOST)

    def jtprod(self, y, x):
        """reference :907-915."""
        if self.device_kkt_ops:
            return self.jtprod_device(y, x)
        y[:self.n] = self.J.T @ x
        y[self.n:self.n + self.n_ineq] = -x[self.ind_ineq]
        return y

    # ---- build_kkt! (reference :927-1001)
    def assemble_blocks(self):
        """CHECKER ONLY since round 6 (tests; `build_kkt` assembles on the device): the scenario blocks A_k, the coupling blocks
        C_dk and the design block before the Schur products (S0) as dense host arrays by matrix slicing -- what the reference
        scatters into `A_kk.nzval`, `C_dk` and `aug_com` (:935-972, :993-996)."""
        n, ns, nv, nd = self.n, self.ns, self.nv, self.nd
        off = ns * nv
        if self.n_ineq > 0:
            Ss = self.pr_diag[n:n + self.n_ineq]
            Sd = self.du_diag[self.ind_ineq]
            self.diag_buffer[:] = Ss / (1.0 - Sd * Ss)
        J, H = self.J.tocsr(), self.H.tocsr()
        Jd_all = J[:, off:].toarray()                     # m x nd
        S0 = H[off:, off:].toarray() + np.diag(self.pr_diag[off:n])
        A, Cd = [], []
        for k in range(ns):
            v = slice(k * nv, (k + 1) * nv)
            E, Ipos = self.eq_rows[k], self.ineq_pos[k]
            Irows = self.ind_ineq[Ipos]
            Hvv = H[v, v].toarray() + np.diag(self.pr_diag[v])
            Hdv = H[off:, v].toarray()
            Jv = J[:, v]
            JvE, JvI = Jv[E].toarray(), Jv[Irows].toarray()
            JdE, JdI = Jd_all[E], Jd_all[Irows]
            D = self.diag_buffer[Ipos]
            Ak = np.zeros((self.blk, self.blk))
            Ak[:nv, :nv] = Hvv + JvI.T @ (D[:, None] * JvI)
            Ak[nv:, :nv] = JvE
            Ak[:nv, nv:] = JvE.T
            Ak[nv:, nv:] = np.diag(self.du_diag[E])
            Ck = np.zeros((nd, self.blk))
            Ck[:, :nv] = Hdv + JdI.T @ (D[:, None] * JvI)
            Ck[:, nv:] = JdE.T
            S0 += JdI.T @ (D[:, None] * JdI)
            A.append(Ak)
            Cd.append(Ck)
        return A, Cd, S0

    def build_kkt(self):
        """reference :927-1001.  The scatter of the callback values into A_k / C_dk / S0 runs on the device (`mnk_schur_assemble`:
        four uploads -- hess, jac, pr_diag, du_diag -- and one launch instead of ns (blk^2 + nd blk) doubles assembled with numpy
        and uploaded every iteration); the host keeps its copy of `diag_buffer` for the vector algebra of `solve_kkt!`."""
        if not self.device_assembly:     # (rounds 4-5, kept for the before / after record of tools/bench_schur_kkt.py only)
            A, Cd, S0 = self.assemble_blocks()
            self.stage.set_blocks(A, Cd, S0)
            self.stage.build_kkt()
            return
        if self.n_ineq > 0:
            Ss = self.pr_diag[self.n:self.n + self.n_ineq]
            Sd = self.du_diag[self.ind_ineq]
            self.diag_buffer[:] = Ss / (1.0 - Sd * Ss)
        self.stage.assemble(self.hess, self.jac, self.pr_diag, self.du_diag)
        self.stage.build_kkt()          # device: the ns blocks as one batch, S -= sum_k C_dk A_k^-1 C_dk'
        if self.device_kkt_ops:
            self.upload_barrier_terms()

    def build_kkt_device(self, hess=None, jac=None):
        """`build_kkt!` from the diagonals the handle keeps itself (after `set_aug_diagonal_device`); `hess` / `jac`: the COO
        values (host arrays or device tensors; default: the host fields the callbacks wrote)."""
        keep = [np.ascontiguousarray(a, dtype=np.float64) if isinstance(a, np.ndarray) else a
                for a in (self.hess if hess is None else hess, self.jac if jac is None else jac)]
        (ph, l0), (pj, l1) = (_ptr(a) for a in keep)
        assert l0 == l1
        self._call("_assemble", ph, pj, None, None, l0)
        self.stage._assembled = True
        self.stage.build_kkt()

    def factorize_kkt(self):
        return self.linear_solver.factorize()

    # ---- solve_kkt! (reference :1040-1110)
    def solve_kkt(self, w):
        if self.device_kkt_ops:
            return self.solve_kkt_device(w)
        n, ns, nv, nd, ni = self.n, self.ns, self.nv, self.nd, self.n_ineq
        off = ns * nv
        full = w.values
        wx, ws, wy = full[:n], full[n:n + ni], w.dual()
        Ss = self.pr_diag[n:n + ni]
        self._reduce_rhs(w)
        self.buffer[:] = 0.0
        if ni > 0:                                             # step 1: condense the inequality rows
            self.buffer[self.ind_ineq] = self.diag_buffer * (wy[self.ind_ineq] + ws / Ss)
            wx += self.J.T @ self.buffer
        rk = np.empty((ns, self.blk))                          # step 2: per-scenario right-hand sides
        for k in range(ns):
            rk[k, :nv] = wx[k * nv:(k + 1) * nv]
            rk[k, nv:] = wy[self.eq_rows[k]]
        rd = np.ascontiguousarray(wx[off:])
        self.stage.solve_host(rk, rd)                          # steps 3-5 on the device (mnk_schur_solve)
        for k in range(ns):                                    # step 6: write back
            wx[k * nv:(k + 1) * nv] = rk[k, :nv]
            wy[self.eq_rows[k]] = rk[k, nv:]
        wx[off:] = rd
        if ni > 0:                                             # step 7: inequality duals and slacks
            wy_eq = wy[self.ind_eq].copy()
            wy[:] = self.J @ wx
            wy[self.ind_eq] = wy_eq
            wy[self.ind_ineq] = self.diag_buffer * wy[self.ind_ineq] - self.buffer[self.ind_ineq]
            ws[:] = (ws + wy[self.ind_ineq]) / Ss
        self._finish_aug_solve(w)
        return w

    # ---- mul! / mul_hess_blk! (reference :1113-1146)
    def mul(self, w, x, alpha=1.0, beta=0.0):
        if self.device_kkt_ops:
            return self.mul_device(w, x, alpha, beta)
        n = self.n
        wp, xp = w.primal(), x.primal()
        wx, ws = wp[:n], wp[n:]
        xx, xs = xp[:n], xp[n:]
        wy, xy = w.dual(), x.dual()
        wx[:] = beta * wx + alpha * (self.H @ xx)
        if self.m > 0:
            wx += alpha * (self.J.T @ xy)
            wy[:] = alpha * (self.J @ xx) + beta * wy
        else:
            wy[:] = beta * wy
        ws[:] = beta * ws - alpha * xy[self.ind_ineq]
        wy[self.ind_ineq] -= alpha * xs
        self._kktmul(w, x, alpha, beta)
        return w

    def mul_hess_blk(self, wx, t):
        if self.device_kkt_ops:
            return self.mul_hess_blk_device(wx, t)
        n = self.n
        wx[:n] = self.H @ t[:n]
        wx[n:] = 0.0
        wx += t * self.pr_diag
        return wx

    # ---- jtprod! / mul_hess_blk! inside the handle (host arrays or device tensors; `solve_kkt_device` / `mul_device`,
    # the feeders and `get_diagonals_device` are `_KKTCommon`'s)
    def jtprod_device(self, y, x):
        assert all(a.flags.c_contiguous for a in (y, x) if isinstance(a, np.ndarray))
        (py, l0), (px, l1) = _ptr(y), _ptr(x)
        assert l0 == l1
        self._call("_jtprod", py, px, l0)
        return y

    def mul_hess_blk_device(self, wx, t):
        assert all(a.flags.c_contiguous for a in (wx, t) if isinstance(a, np.ndarray))
        (pw, l0), (pt, l1) = _ptr(wx), _ptr(t)
        assert l0 == l1
        self._call("_mul_hess_blk", pw, pt, l0)
        return wx

    # ---- the host mirror of the device entry points: numpy code that performs the device kernels' operations in the kernels'
    # order (csrc/schur.hip, csrc/kkt_vec.h), so that a device result can be held to it bit for bit on arbitrary data -- the host
    # path above sums in scipy's order and cannot serve for that.  It reads the host fields (hess, jac, pr_diag, du_diag, reg, the
    # bound terms) as they were at the last `build_kkt`.
    def row_lists(self):
        """{OP_J, OP_JT, OP_H: (row_ptr, col_idx, perm)} of the structure in force (`mnk_schur_spmv_plan`)."""
        if self._row_lists is None:
            self._row_lists = {w: spmv_plan(self.n, self.m, self.nv, self.nc, self.hess_I, self.hess_J, self.jac_I, self.jac_J, self.ind_ineq,
                                            self.ind_eq, self.spmv_T, w)[:3] for w in (OP_J, OP_JT, OP_H)}
        return self._row_lists

    def _spmv(self, which, x, alpha=1.0, beta=0.0, y=None):
        vals = self.hess if which == OP_H else self.jac
        return ordered_spmv(*self.row_lists()[which], vals, x, self.spmv_T, alpha, beta, y)

    def _condense_weights(self):
        """D of `schur_condense_weights_kernel`: Sigma_s / fma(-Sigma_d, Sigma_s, 1) -- the assembly's kernel is compiled with
        contraction, its `1 - Sigma_d Sigma_s` is one fused operation."""
        Ss = self.pr_diag[self.n:self.n + self.n_ineq]
        return Ss / _fma(-self.du_diag[self.ind_ineq], Ss, 1.0)

    def solve_kkt_ordered(self, w):
        """`mnk_schur_solve_kkt` on the host; steps 3-5 through `stage.solve_host` (the stage's own kernels)."""
        n, ns, nv, ni, blk = self.n, self.ns, self.nv, self.n_ineq, self.blk
        off = ns * nv
        v = w.values
        wx, ws, wy = v[:n], v[n:n + ni], w.dual()
        Ss = self.pr_diag[n:n + ni]
        v[w.ind_lb] = v[w.ind_lb] - w.dual_lb() / self.l_diag          # reduce_rhs_kernel, one side after the other
        v[w.ind_ub] = v[w.ind_ub] - w.dual_ub() / self.u_diag
        buffer = np.zeros(self.m)
        if ni > 0:
            D = self._condense_weights()
            buffer[self.ind_ineq] = D * (wy[self.ind_ineq] + ws / Ss)
            wx[:] = self._spmv(OP_JT, buffer, 1.0, 1.0, wx)
        eq = np.sort(self.ind_eq).reshape(ns, self.nc_eq) if ns else np.zeros((0, 0), dtype=np.int64)
        rk = np.empty((ns, blk))
        rk[:, :nv] = wx[:off].reshape(ns, nv)
        rk[:, nv:] = wy[eq]
        rd = np.ascontiguousarray(wx[off:])
        self.stage.solve_host(rk, rd)
        wx[:off] = rk[:, :nv].reshape(-1)
        wy[eq] = rk[:, nv:]
        wx[off:] = rd
        if ni > 0:
            jx = self._spmv(OP_J, wx)
            y = D * jx[self.ind_ineq] - buffer[self.ind_ineq]
            wy[self.ind_ineq] = y
            ws[:] = (ws + y) / Ss
        dlb, dub = w.dual_lb(), w.dual_ub()                             # finish_aug_kernel: fma(lower, w, -d) / diag, fma(-lower, w, d) / diag
        dlb[:] = _fma(self.l_lower, v[w.ind_lb], -dlb) / self.l_diag
        dub[:] = _fma(-self.u_lower, v[w.ind_ub], dub) / self.u_diag
        return w

    def mul_ordered(self, w, x, alpha=1.0, beta=0.0):
        """`mnk_schur_mul` on the host."""
        n, ni, m = self.n, self.n_ineq, self.m
        wv, xv = w.values, x.values
        wx, ws, wy = wv[:n], wv[n:n + ni], w.dual()
        xx, xs, xy = xv[:n], xv[n:n + ni], x.dual()
        wx[:] = self._spmv(OP_H, xx, alpha, beta, wx)
        if m > 0:
            wx[:] = self._spmv(OP_JT, xy, alpha, 1.0, wx)
            wy[:] = self._spmv(OP_J, xx, alpha, beta, wy)
        ws[:] = beta * ws - alpha * xy[self.ind_ineq]                    # schur_mul_slack_kernel
        wy[self.ind_ineq] = wy[self.ind_ineq] - alpha * xs
        w.primal()[:] = w.primal() + (alpha * self.reg) * x.primal()     # schur_mul_diag_kernel
        wy[:] = wy + (alpha * self.du_diag) * xy
        # kktmul_bound_kernel (kkt_vec.h, compiled with contraction): w[p] -+= alpha xb (two roundings), then
        # wb = fma(beta, wb, alpha * fma(x[p], lower, -+(xb * diag))); the lower side first
        xl, xu = x.dual_lb(), x.dual_ub()
        wv[w.ind_lb] = wv[w.ind_lb] - alpha * xl
        w.dual_lb()[:] = _fma(beta, w.dual_lb(), alpha * _fma(xv[x.ind_lb], self.l_lower, -(xl * self.l_diag)))
        wv[w.ind_ub] = wv[w.ind_ub] + alpha * xu
        w.dual_ub()[:] = _fma(beta, w.dual_ub(), alpha * _fma(xv[x.ind_ub], self.u_lower, xu * self.u_diag))
        return w

    def jtprod_ordered(self, y, x):
        """`mnk_schur_jtprod` on the host."""
        y[:self.n] = self._spmv(OP_JT, x)
        y[self.n:self.n + self.n_ineq] = -x[self.ind_ineq]
        return y

    def mul_hess_blk_ordered(self, wx, t):
        """`mnk_schur_mul_hess_blk` on the host."""
        n = self.n
        wx[:n] = self._spmv(OP_H, t[:n])
        wx[n:] = 0.0
        wx[:] = wx + t * self.pr_diag
        return wx

    def close(self):
        if getattr(self, "stage", None) is not None:
            self.stage.close()
            self.stage = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""Device-resident back-end of the IPM mirror: the iterate, the multipliers, the KKT vectors and the
right-hand sides live in HBM; per iteration only scalars cross PCIe.  The algorithm is `madnlp_jl_amd.ipm.MadNLPSolver`'s
(which documents the reference lines): `DeviceMadNLPSolver` overrides its vector primitives (`ipm.BACKEND_PRIMITIVES`) and
nothing of its control flow except the first trial of the inertia correction.  The vector work goes through

  * the KKT handle:   `set_aug_diagonal!`, `regularize_diagonal!`, `build_kkt!`, `factorize!`, `solve_kkt!`, `mul!`, SpMV
  * `mnk_ipm_*`:      the reductions and elementwise pieces of reference `src/IPM/kernels.jl`, and the loop's plain vector
                      work (`mnk_ipm_vec_*`, `mnk_ipm_get_dot`, `mnk_ipm_gemv`)
  * `mnk_ipm_quality_function`: the adaptive barrier update's quality function for up to four centering parameters per call
                      (`barrier = "quality_function"`), the step `aff + sigma cen` never stored
  * `mnk_ipm_krylov_*` (csrc/krylov.hip): the Gram-Schmidt, normalization and solution updates of the GMRES refinement
                      (`iterator = "krylov"`), one synchronization per Arnoldi step
  * `device_callbacks`: each `eval_*` is one call into the callbacks object, which evaluates the model on the device (`mnk_opf_*`,
                      `mnk_tape_*`, `mnk_fix_*`, the QPs through the KKT handle's SpMV or `mnk_ipm_gemv`) and owns NLP scaling
                      and the objective sense (`mnk_ipm_vec_mul`, `mnk_ipm_scale_cons`, `mnk_ipm_scale_grad`, csrc/nlp_scale.hip)
  * torch:            device memory only (allocation, uploads, the final download) -- no torch kernel runs in the loop

Scope: `SparseCondensedKKTSystem` (all constraints relaxed to inequalities, as the reference's preset does) and
`DenseCondensedKKTSystem` (equalities allowed), with the models of `device_callbacks.callbacks_class`: the AC-OPF NLP and any
`TapeModel` (the sparse condensed system, or with `callback = "sparse"` the dense one: their COO values are scattered into its
device buffers, csrc/dense_coo.hip), the sparse and the dense QP.  Initialization runs once on the host and is uploaded.

With `hessian_approximation = "bfgs" / "damped_bfgs"` (dense systems) the Hessian approximation lives in the KKT handle's
device buffer and is updated there (`mnk_dc_qn_update`, csrc/qn.hip): the model's Hessian is never loaded.  With
`"compact_lbfgs"` (sparse condensed system) the history, U and V live in an `mnk_lbfgs` handle attached to the KKT handle
(csrc/lbfgs.hip), whose `solve_kkt!` / `mul!` apply the low-rank term: the loop below does not know about it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from .device_callbacks import (DeviceDenseQPCallbacks, DeviceFixedVariableCallbacks, DeviceFixedVariables,  # noqa: F401
                               DeviceHessianProduct, DeviceOPFCallbacks, DeviceQPCallbacks, DeviceScaling, DeviceTapeCallbacks,
                               _DevicePointer, _up, callbacks_class, device_callbacks)
from .ipm import IPMOptions, MadNLPSolver, unpack_solution
from .ipm_device import IPMDeviceKernels


class DeviceMadNLPSolver(MadNLPSolver):
    def __init__(self, nlp, kkt_factory, opt: IPMOptions | None = None, device="cuda", sparse=True):
        callback = "auto" if opt is None else opt.callback
        if getattr(nlp, "is_tape_model", False) and not sparse and callback == "auto":
            raise NotImplementedError("DeviceMadNLPSolver evaluates a TapeModel for the sparse condensed KKT handle only "
                                      "(DeviceTapeCallbacks feed COO values to its compressors): use sparse=True with "
                                      "relax_equality, callback = 'sparse' for the dense condensed handle, or MadNLPSolver "
                                      "with host callbacks")
        if callback == "sparse" and not sparse and callbacks_class(nlp, sparse, callback) is DeviceDenseQPCallbacks:
            raise NotImplementedError(f"callback = 'sparse' on a dense system with the dense QP device callbacks "
                                      f"({type(nlp).__name__}): they load dense P and A; use callback = 'auto', a TapeModel or "
                                      "the AC-OPF model")
        if (opt is not None and opt.fixed_variable_treatment == "make_parameter" and sparse
                and callbacks_class(nlp, sparse) is DeviceQPCallbacks
                and (np.asarray(nlp.lvar, float) == np.asarray(nlp.uvar, float)).any()):
            raise NotImplementedError("fixed_variable_treatment = 'make_parameter' with fixed variables on the sparse QP device "
                                      "callbacks (DeviceQPCallbacks): they evaluate f, grad f and c through the reduced KKT "
                                      "handle's SpMV, and the fixed part of H x and J x would need constant offsets that are "
                                      "not implemented; use 'relax_bound', a TapeModel, or MadNLPSolver")
        super().__init__(nlp, kkt_factory, opt, sparse=sparse)
        if self.inertia_correction_method != "inertia_based":
            if hasattr(self.kkt, "close"):
                self.kkt.close()
            raise NotImplementedError(
                f"DeviceMadNLPSolver runs the inertia-based correction only (resolved method: {self.inertia_correction_method}; "
                f"a linear solver without inertia selects inertia_free): use MadNLPSolver for inertia-free or ignore")
        assert not sparse or self.ns == self.m, "device driver: all-inequality (RelaxEquality) sparse condensed systems"
        self.dev = torch.device(device)
        self._on_device = False

    # ------------------------------------------------------------------ host initialization, then upload
    def _upload(self):
        ctx = self.kkt.linear_solver.ctx
        for name in ("x", "xl", "xu", "zl", "zu", "f", "y", "c", "rhs", "jacl", "x_trial", "c_trial"):
            setattr(self, name, _up(getattr(self, name), self.dev))
        nt, m, nlb, nub = self.n + self.ns, self.m, len(self.ind_lb), len(self.ind_ub)
        self.nt = nt
        self._lw = nt + m + nlb + nub
        self.K = IPMDeviceKernels(nt, self.ind_lb, self.ind_ub, ctx=ctx)
        self.K.set_perturbation_sets(self.ind_llb, self.ind_uub)
        self.d, self.p, self._w1, self._w4 = (self._new_vec(self._lw) for _ in range(4))   # flat device KKT vectors
        if self.lbfgs:               # the host mirror (kkt.LowRankHessianKKT) comes off: the handle applies the low-rank term itself
            self.kkt = self.iterator.kkt = self.kkt.inner
        # NLP scaling / the sense: the scaled launches replace the plain ones only when there is something to apply
        self._scaled = bool(self.opt.nlp_scaling) or self.obj_sign != 1.0
        scaling = DeviceScaling(self.K, self.dev, self.n, self.ns, self.ind_ineq, self.rhs, self._scaled, self.obj_sign,
                                self.obj_scale, self.con_scale, self.jac_scale)
        self.ind_ineq_t, self.slack_pos_t = scaling.ind_ineq, scaling.slack_pos
        # variables made parameters (`fixed_handler`): the callbacks are built on the FULL model (self.nlp)
        if self.coo_dense:           # the model's COO callbacks scatter into the dense handle's device buffers
            self.kkt.attach_coo(*self._coo)
        self.cb = device_callbacks(self.nlp, self.kkt, self.dev, self.K, self.sparse, scaling, fixed=self.fixed_handler,
                                   own_hessian=self.lbfgs, callback=self.opt.callback)
        self.kkt.device_kkt_ops = True
        if self.coo_dense:
            # the device buffers get what the host initialization evaluated: J(x0), scaled, and the Lagrangian Hessian at
            # (x0, y0) -- or the quasi-Newton init!, with J(x0) kept for J(x_0)' l_1 of the first secant pair
            self.cb.eval_jac(self.x)
            if self.qn is None:
                self.cb.eval_lag_hess(self.x, self.y, 1.0)
            else:
                self._qn_upload()
                self.kkt.keep_jacobian_device()
        elif not self.sparse:        # the dense handle reads Hessian / Jacobian from its own device copies
            self.cb.load_jac()
            if self.qn is None:
                self.cb.load_hess()
            else:
                self._qn_upload()
        elif self.lbfgs:
            self._lbfgs_upload()
        self._on_device = True
        self._sync = ctx.synchronize

    # slices of a flat KKT vector (reference src/KKT/rhs.jl:90-150)
    def _primal(self, v): return v[:self.nt]
    def _dual(self, v): return v[self.nt:self.nt + self.m]
    def _dual_lb(self, v): return v[self.nt + self.m:self.nt + self.m + len(self.ind_lb)]
    def _dual_ub(self, v): return v[self.nt + self.m + len(self.ind_lb):]

    # ------------------------------------------------------------------ callbacks: scaling and the sense are `self.cb`'s
    def eval_f(self, x):
        return self.cb.eval_f(x) if self._on_device else super().eval_f(x)

    def eval_grad(self, x):
        if not self._on_device:
            return super().eval_grad(x)
        self.cb.eval_grad(self.f, x)
        self.cnt.obj_grad_cnt += 1

    def eval_cons(self, c, x):
        return self.cb.eval_cons(c, x) if self._on_device else super().eval_cons(c, x)

    def eval_jac(self, x):
        return self.cb.eval_jac(x) if self._on_device else super().eval_jac(x)

    def eval_lag_hess(self, x, y, is_resto=False):
        if not self._on_device:
            return super().eval_lag_hess(x, y, is_resto)
        if self.lbfgs:
            return self._eval_lag_hess_lbfgs_device(x, y)
        if self.qn is not None:
            return self._eval_lag_hess_qn_device(x, y)
        self.cb.eval_lag_hess(x, y, 0.0 if is_resto else 1.0)        # objective weight 0 in robust!
        self.cnt.lag_hess_cnt += 1

    def _qn_backups(self, *more):
        """The backups of callbacks.jl:184-186 as device vectors (`qn_dev`), x and grad f saved; `more`: further n-vectors."""
        n = self.n
        d = self.qn_dev = SimpleNamespace(**{k: self._new_vec(n) for k in ("sk", "yk", "last_x", "last_g", "last_jv") + more})
        self.K.vec_copy(d.last_x, self.x[:n])
        self.K.vec_copy(d.last_g, self.f[:n])
        return d

    # ------------------------------------------------------------------ quasi-Newton Hessian in the handle's device buffer
    def _qn_upload(self):
        """The host initialization has run `init!` on the host copy; the device buffer gets its own `init!` from the
        uploaded gradient and objective (`mnk_dc_qn_init`), and the backups of callbacks.jl:184-186 become device vectors.
        From here on the approximation exists on the device only: it is never loaded from the host or from the model."""
        self.kkt.qn_init_device(self.qn.kind, self.f[:self.n], self.obj_val)
        self._qn_backups()

    def _eval_lag_hess_qn_device(self, x, y):
        """`MadNLPSolver._eval_lag_hess_qn` on device vectors: one transposed Jacobian product of the callbacks, one launch for
        s, y and the backups (`mnk_dc_qn_secant`: the same operations in the same order as the host mirror), then
        `mnk_dc_qn_update`; nothing crosses PCIe."""
        n, d = self.n, self.qn_dev
        assert self.cnt.obj_grad_cnt >= 2, "the first call (init!) belongs to the host initialization"
        jl = jv = None
        if self.m > 0:
            jl = self.jacl[:n]                                      # J(x+)' l+ (current: see the host mirror)
            if self.coo_dense:       # from the COO values kept at the previous call, already scaled: no callback launch
                self.kkt.jtprod_coo_device(L.MNK_DC_JAC_KEPT, y, d.last_jv)
            else:
                self.cb.eval_jtprod_at(d.last_x, y, d.last_jv)
            jv = d.last_jv
        self.kkt.qn_secant_device(x[:n], self.f[:n], jl, jv, d.last_x, d.last_g, d.sk, d.yk)
        if self.coo_dense:
            self.kkt.keep_jacobian_device()
        self.kkt.qn_update_device(d.sk, d.yk)

    # ------------------------------------------------------------------ compact L-BFGS in a handle attached to the KKT handle
    def _lbfgs_upload(self):
        """The host initialization has run `init!` on the mirror; the device handle is created with the same options, attached
        to the KKT handle and runs its own `init!` from the uploaded gradient (the same ordered sum, the same sigma).  The
        backups of callbacks.jl:184-186 become device vectors, and the compressed Jacobian of the initial point is kept for
        J(x_0)' l_1.  From here on no Hessian callback is launched."""
        qd = self.kkt.attach_quasi_newton(self.qn.options)
        d = self._qn_backups("hess")
        self.K.vec_fill(d.hess, qd.init(self.f[:self.n], self.obj_val))
        self.kkt.compress_hessian(d.hess)
        self.kkt.keep_jacobian_device()

    def _eval_lag_hess_lbfgs_device(self, x, y):
        """`MadNLPSolver._eval_lag_hess_qn` for `CompactLBFGS` on device vectors.  J(x_k)' l_+ comes from the Jacobian values the
        handle kept at the previous call (already scaled: no con_scale product, no model call), s, y and the backups from one
        launch (`mnk_sc_qn_secant`), then `mnk_lbfgs_update` (one synchronization).  A performed update changes sigma: the
        diagonal Hessian is refilled and compressed."""
        n, d = self.n, self.qn_dev
        assert self.cnt.obj_grad_cnt >= 2, "the first call (init!) belongs to the host initialization"
        jl = jv = None
        if self.m > 0:
            jl = self.jacl[:n]
            self.kkt.spmv_device(L.MNK_SC_JT_KEPT, 0, 1.0, y, 0.0, d.last_jv)
            jv = d.last_jv
        self.kkt.qn_secant_device(x[:n], self.f[:n], jl, jv, d.last_x, d.last_g, d.sk, d.yk)
        self.kkt.keep_jacobian_device()
        performed, sigma = self.kkt.qn_dev.update(d.sk, d.yk)
        if performed:
            self.K.vec_fill(d.hess, sigma)
            self.kkt.compress_hessian(d.hess)

    def jtprod(self, out, y):
        """`jtprod!` reference src/KKT/Sparse/condensed.jl:150-156."""
        self.cb.jtprod_x(out[:self.n], y)
        if self.ns == self.m:
            self.K.vec_axpby(out[self.n:], -1.0, y)
        else:
            self.K.vec_gather(out[self.n:], -1.0, y, self.ind_ineq_t)

    # ------------------------------------------------------------------ factorization glue
    def factorize_wrapper(self):
        if not self._on_device:
            return super().factorize_wrapper()
        self.kkt.build_kkt_device()
        self.kkt.linear_solver.factorize_async()
        self.cnt.factorization_cnt += 1

    def solve_refine(self, x, b, w):
        """Richardson refinement (reference src/LinearSolvers/backsolve.jl:27-76) or, with `iterator = "krylov"`, restarted
        GMRES (the capability of lib/MadNLPKrylov) on device vectors."""
        from .linear_solver import SolveException
        refine = self._solve_refine_krylov if self.opt.iterator == "krylov" else self._solve_refine
        try:
            ok = refine(x, b, w)
            self.kkt.linear_solver.check_solve()   # the stream is idle here (the norms synchronized)
        except SolveException:
            # a one-launch solve gave up (its workgroups were not co-resident): the solver has switched to the stepwise
            # solve; the refinement is repeated from the right-hand side
            ok = refine(x, b, w)
            self.kkt.linear_solver.check_solve()
        return ok

    def _solve_refine(self, x, b, w):
        # One host synchronization per Richardson step: solve -> x += w -> w = b - K x -> the norms are enqueued back to back
        # and read together; the norm of the right-hand side rides along with the first step's norms (round 4 fetched it on
        # its own in front of the loop: one more stream synchronization per solve_refine, ~25 per AC-OPF run).  A zero
        # right-hand side is then solved once instead of not at all: x = K^-1 0 = 0 exactly, reported as the reference
        # reports it (no step, ratio 0).
        it = self.iterator
        residual_ratio = 0.0
        K = self.K
        K.vec_fill(x, 0.0)
        it.ir = 0
        K.vec_copy(w, b)
        norm_b = None
        while True:
            self.kkt.solve_kkt_device(w)
            K.vec_axpby(x, 1.0, x, 1.0, w)
            K.vec_copy(w, b)
            self.kkt.mul_device(w, x, -1.0, 1.0)
            with K.batch():
                b_b = K.get_norms(b) if norm_b is None else None
                b_w = K.get_norms(w)
                b_x = K.get_norms(x)
            if norm_b is None:
                norm_b = b_b[0]
                if norm_b == 0:
                    K.vec_fill(x, 0.0)
                    break
            norm_w, norm_x = b_w[0], b_x[0]
            residual_ratio = norm_w / (min(norm_x, 1e6 * norm_b) + norm_b)
            it.ir += 1
            if it.ir >= it.richardson_max_iter or residual_ratio < it.richardson_tol:
                break
        it.residual_ratio = residual_ratio
        return residual_ratio < it.richardson_acceptable_tol

    def _solve_refine_krylov(self, x, b, w):
        """`KrylovIterator.solve_refine` (backsolve.py) on device vectors: the same operations in the
        same order, the host scalars through the same `GmresCycle`.  One synchronization per `solve_kkt`: cycle 0 is
        Richardson's first step with the 2-norm riding along; an Arnoldi step enqueues mul -> solve -> dots -> project ->
        dots -> project -> normalize and reads h1, h2 and the norm together (the first step of a cycle also the cycle's
        beta); the solution update and the residual ratio close a cycle with one more."""
        it, K, kkt = self.iterator, self.K, self.kkt
        it.ir = it.steps = it.cycles = 0
        it.trace = []
        K.vec_copy(w, b)
        kkt.solve_kkt_device(w)               # cycle 0 (a zero right-hand side is solved once, as in _solve_refine)
        K.vec_copy(x, w)
        with K.batch():
            b_b = K.get_norms(b)
            b_0 = K.get_norm2(w)
            b_w, b_x = self._krylov_residual(x, b, w)
        norm_b, beta0 = b_b[0], b_0[0]
        if norm_b == 0:
            K.vec_fill(x, 0.0)
            it.residual_ratio = 0.0
            return True
        it.ir = 1
        r = b_w[0] / (min(b_x[0], 1e6 * norm_b) + norm_b)
        while not (r < it.richardson_tol or it.ir >= it.max_iter):
            self._krylov_cycle(x, w, beta0)
            with K.batch():
                b_w, b_x = self._krylov_residual(x, b, w)
            r = b_w[0] / (min(b_x[0], 1e6 * norm_b) + norm_b)
        it.residual_ratio = r
        return r < it.richardson_acceptable_tol

    def _krylov_residual(self, x, b, w):
        """Enqueue w = b - K x and the two norms of the residual ratio (inside the caller's batch)."""
        self.K.vec_copy(w, b)
        self.kkt.mul_device(w, x, -1.0, 1.0)
        return self.K.get_norms(w), self.K.get_norms(x)

    def _krylov_cycle(self, x, w, beta0):
        from .backsolve import GmresCycle
        it, K, kkt = self.iterator, self.K, self.kkt
        kkt.solve_kkt_device(w)               # z = K^-1 (b - K x)
        it.ir += 1
        if it.ir >= it.max_iter:              # a single solve left: a Richardson step
            K.vec_axpby(x, 1.0, x, 1.0, w)
            return
        V = getattr(self, "_krylov_V", None)
        if V is None or V.shape[0] != it.restart + 1:
            V = self._krylov_V = self._new_vec((it.restart + 1) * self._lw).view(it.restart + 1, self._lw)   # the basis
        it.cycles += 1
        cyc = None
        for j in range(it.restart):
            k = j + 1
            with K.batch():
                b_beta = K.krylov_normalize(V[0], w, False) if j == 0 else None
                kkt.mul_device(w, V[j], 1.0, 0.0)
                kkt.solve_kkt_device(w)       # u = K^-1 K v_j
                b_h1 = K.krylov_dots(V, k, w)
                K.krylov_project(w, V, k)
                b_h2 = K.krylov_dots(V, k, w)
                K.krylov_project(w, V, k)
                b_hn = K.krylov_normalize(V[k], w, True)
            it.ir += 1
            it.steps += 1
            if cyc is None:
                cyc = GmresCycle(b_beta[0], it.restart)
                it.trace.append((b_beta[0], cyc.rho))
                if not b_beta[0] > 0:         # (a singular solve: nothing to build a basis from)
                    return
            hn = b_hn[0]
            rho = cyc.add_column(list(b_h1)[:k], list(b_h2)[:k], hn)
            if rho <= it.krylov_tol * beta0 or hn == 0 or it.ir >= it.max_iter:
                break
        K.krylov_axpy(x, V, cyc.k, cyc.solution())

    def solve_refine_wrapper(self, d, p, w):
        if not self._on_device:
            return super().solve_refine_wrapper(d, p, w)
        ok = self.solve_refine(d, p, w)
        self.cnt.backsolve_cnt += self.iterator.ir
        return ok

    # ------------------------------------------------------------------ kernels
    def set_aug_diagonal(self):
        o = self.opt
        self.kkt.set_aug_diagonal_device(self.x, self.xl, self.xu, self.zl, self.zu, o.default_primal_regularization,
                                         o.default_dual_regularization)

    def set_aug_rhs(self, c):
        p = self.p
        self.K.set_aug_rhs(self.f, self.zl, self.zu, self.jacl, c, self.x, self.xl, self.xu, self.mu, self._primal(p),
                           self._dual(p), self._dual_lb(p), self._dual_ub(p))
        self.K.dual_inf_perturbation(self._primal(p), self.mu, self.opt.kappa_d)

    def inf_compl(self, mu, sc):
        return self.K.get_inf_compl(self.x, self.xl, self.xu, self.zl, self.zu, mu, sc)

    def varphi(self, obj, x):
        return self.K.get_varphi(obj, x, self.xl, self.xu, self.mu)

    def alpha_max(self, dx):
        return self.K.get_alpha_max(self.x, self.xl, self.xu, dx, self.tau)

    # SPECULATIVE first correction (round 6).  On the AC-OPF run of the bench line 17 of 20 iterations take exactly two trials: the
    # unperturbed matrix is rejected, the first perturbation is accepted -- and that perturbation is known BEFORE the verdict on the
    # unperturbed matrix: after an iteration that needed a correction it is max(min_hessian_perturbation, perturb_dec_fact *
    # del_w_last) (reference src/IPM/solver.jl:633-636), and for a system whose should_regularize_dual is `true` whatever the
    # inertia (SparseCondensedKKTSystem: src/KKT/Sparse/condensed.jl:141) del_c depends on mu alone.  Both trials are then
    # assembled back to back and factorized as ONE batch of two (a second solver on the same KKT handle, one merged launch: the two
    # fill each other's chain-bound ends, and trial 0 stops at its first non-positive pivot).  The speculative factor is used only
    # if trial 0 is rejected, so the sequence of accepted perturbations -- and every bit of the accepted factors -- is the one
    # the sequential loop produces; if trial 0 is accepted after all, reg / pr_diag / du_diag return to the bits they had
    # (`save_diagonals_device`) and the matrix is assembled again.
    #
    # MEASURED, AND OFF BY DEFAULT (profiles/r06_speculative_correction.txt, tools/spec_pair_time.py): on the case1354pegase-shaped
    # system the rejected trial stops at pivot ~2700-3100 of 11 192 -- but a right-looking elimination has done 1 - (1 - 0.25)^3 =
    # 56 % of its flops by then: 4.4 ms alone against 9.2 for the accepted trial, and the merged pair is bulk-bound at the SUM of the
    # two (13.3 ms against 13.7 one after the other: what it saves is one host round trip).  Every wasted speculation costs a whole
    # factorization (+9 ms), and the AC-OPF run ends at 59.7 instead of 65 iterations/s.  The path stays for systems whose
    # rejections come early in the pivot order; `speculate = True` on the solver object arms it.
    speculate = False     # (only ever taken for KKT systems that offer `ensure_spare_solver`)
    speculative_factorizations = 0
    speculative_wasted = 0

    # LEADING-BLOCK PROBE (round 6): lives in the library (`mnk_ls_factorize_sc_async`, option "probe", on by default while early
    # rejection is armed) so that every caller -- this driver, the reference's own inertia_correction! through the Julia glue -- gets
    # it: after a rejection that stopped in the first half of the columns, a matrix that follows an accepted one is first probed
    # through its leading principal block (13 of the AC-OPF run's 17 rejections stop in the same 64 columns; the block of order
    # 3328 is 2.6 % of a factorization's flops where the full elimination has done 63 % by that column).  `probe = False` on the
    # solver object switches it off for A/B runs; `probe_hits` / `probe_misses` read the library's counters.
    probe = True

    @property
    def probe_hits(self):
        return int(self.kkt.linear_solver.get_stat("probe_hits")) if hasattr(self.kkt.linear_solver, "get_stat") else 0

    @property
    def probe_misses(self):
        return int(self.kkt.linear_solver.get_stat("probe_misses")) if hasattr(self.kkt.linear_solver, "get_stat") else 0

    def _can_speculate(self):
        k = self.kkt
        return (self._on_device and self.speculate and self.del_w_last != 0 and hasattr(k, "ensure_spare_solver")
                and k.should_regularize_dual(0, 0, 0) and k.should_regularize_dual(0, 1, 0))

    def _first_trial(self):
        """The first trial of the base class's correction loop, with what belongs to this back-end: the `probe` option of the
        linear solver and, when armed, the speculative pair."""
        from .linear_solver import factorize_batch
        o, k = self.opt, self.kkt
        if self._on_device and getattr(self, "_probe_applied", None) != self.probe and hasattr(k.linear_solver, "set_option"):
            k.linear_solver.set_option("probe", 1 if self.probe else 0)
            self._probe_applied = self.probe
        if not self._can_speculate():
            return super()._first_trial()
        dw1 = max(o.min_hessian_perturbation, o.perturb_dec_fact * self.del_w_last)
        dc1 = o.jacobian_regularization_value * self.mu ** o.jacobian_regularization_exponent
        spare = k.ensure_spare_solver()
        k.save_diagonals_device()
        with factorize_batch():
            k.build_kkt_device()
            k.linear_solver.factorize_async()       # trial 0: the matrix as it is
            k.regularize_diagonal_device(dw1, dc1)  # trial 1: exactly the sequential loop's first correction (dw1 - 0, dc1 - 0)
            k.build_kkt_device()
            spare.factorize_async()
        self.cnt.factorization_cnt += 1
        self.speculative_factorizations += 1
        inertia = k.linear_solver.inertia()
        correct = k.is_inertia_correct(*inertia)
        if correct:
            # trial 0 stands: the handle goes back to the unperturbed system (diagonals bit for bit, matrix and condensation
            # buffers rebuilt from them) before the solve, whose refinement multiplies with that matrix
            k.restore_diagonals_device()
            k.build_kkt_device()
            self.speculative_wasted += 1
        ok = self._solve_newton() if correct else False
        if self.on_trial is not None:
            self.on_trial(self, 0, inertia, correct, ok)
        if correct:
            return 0, inertia, ok
        # trial 0 rejected: the speculative factorization IS the sequential loop's next trial (the handle's diagonals and
        # matrix are already that trial's)
        self.del_w, self.del_c = dw1, dc1
        k.swap_solvers()
        self.cnt.factorization_cnt += 1
        return (1,) + self._trial(1)

    # ------------------------------------------------------------------ back-end primitives (`ipm.BACKEND_PRIMITIVES`): the whole
    # driver of the base class -- regular!, its line search and corrections, restore!, robust! -- runs unchanged on device tensors
    # through these
    def _new_vec(self, n):
        v = torch.empty(n, dtype=torch.float64, device=self.dev)
        self.K.vec_fill(v, 0.0)
        return v

    def _clone(self, v):
        w = torch.empty_like(v)
        self.K.vec_copy(w, v)
        return w

    def _vcopy(self, dst, src): self.K.vec_copy(dst, src)

    def _vaxpy(self, y, a, x): self.K.vec_axpby(y, 1.0, y, a, x)

    def _vaxpby(self, dst, x, a, d): self.K.vec_axpby(dst, 1.0, x, a, d)

    def _vfill(self, v, value): self.K.vec_fill(v, value)

    def _theta(self, c): return self.K.get_norms(c)[1]

    def _norm_inf(self, v): return self.K.get_norms(v)[0]

    def _norm2(self, v): return self.K.get_norm2(v)

    def _regularize(self, dw, dc): self.kkt.regularize_diagonal_device(dw, dc)

    def _sd_sc(self): return self.K.get_sd_sc(self.y, self.zl, self.zu, self.opt.s_max)

    def _inf_du(self, sd): return self.K.get_inf_du(self.f, self.zl, self.zu, self.jacl, sd)

    def _iteration_scalars(self):
        """the five reductions of the iteration header in ONE synchronization (`mnk_ipm_batch_*`)."""
        K = self.K
        with K.batch():
            b_s = K.get_sd_sc(self.y, self.zl, self.zu, self.opt.s_max)
            b_n = K.get_norms(self.c)
            b_d = K.get_inf_du(self.f, self.zl, self.zu, self.jacl, 1.0)
            b_c = K.get_inf_compl(self.x, self.xl, self.xu, self.zl, self.zu, 0.0, 1.0)
        sd, sc = b_s[0], b_s[1]
        return sd, sc, b_n[0], b_d[0] / sd, b_c[0] / sc

    def _jtprod(self): self.jtprod(self.jacl, self.y)

    def _alpha_z(self, tau): return self.K.get_alpha_z(self.zl, self.zu, self._dzl(), self._dzu(), tau)

    def _bound_dual_axpy(self, a): self.K.bound_dual_axpy(self.zl, self.zu, a, self._dzl(), self._dzu())

    def _bound_dual_fill(self, v): self.K.bound_dual_fill(self.zl, self.zu, v)

    def _adjust_boundary(self): self.K.adjust_boundary(self.x, self.xl, self.xu, self.mu)

    def _reset_bound_dual(self, mu):
        self.K.reset_bound_dual(self.zl, self.zu, self.x, self.xl, self.xu, mu, self.opt.kappa_sigma)

    def _get_F(self):
        return self.K.get_F(self.c, self.f, self.zl, self.zu, self.jacl, self.x, self.xl, self.xu, self.mu)

    def _set_initial_rhs(self):
        p = self.p
        self.K.set_initial_rhs(self.f, self.zl, self.zu, self._primal(p), self._dual(p), self._dual_lb(p), self._dual_ub(p))

    def _kkt_initialize(self):
        """`initialize!(kkt)` (reference src/KKT/Sparse/utils.jl:52-62) on the handle's device state: zero Hessian, and
        reg = pr_diag = 1, du_diag = 0, l_diag = u_diag = 1, l_lower = u_lower = 0 through the feeder (x = 0, xl = 1,
        xu = -1, zl = zu = 0, primal_reg = 1)."""
        self.kkt.initialize()
        if not self.lbfgs:         # (compact L-BFGS: the handle's diagonal Hessian was zeroed just above, the model's is never loaded)
            self.cb.zero_hess()    # (a dense quasi-Newton run too: the reference's initialize!(kkt) zeroes its approximation here)
        nt = self.nt
        z = np.zeros(nt)
        self.kkt.set_aug_diagonal_device(z, np.ones(nt), -np.ones(nt), z, z, 1.0, 0.0)

    def _rel_search_norm(self): return self.K.get_rel_search_norm(self.x, self._dx())

    def _line_search_scalars(self):
        """the six reductions in front of the line search in ONE synchronization."""
        K, dx = self.K, self._dx()
        with K.batch():
            b_n = K.get_norms(self.c)
            b_v = K.get_varphi(self.obj_val, self.x, self.xl, self.xu, self.mu)
            b_d = K.get_varphi_d(self.f, self.x, self.xl, self.xu, dx, self.mu)
            b_a = K.get_alpha_max(self.x, self.xl, self.xu, dx, self.tau)
            b_z = K.get_alpha_z(self.zl, self.zu, self._dzl(), self._dzu(), self.tau)
            b_r = K.get_rel_search_norm(self.x, dx)
        return b_n[1], b_v[0], b_d[0], b_a[0], b_z[0], b_r[0]

    def _trial_scalars(self):
        K = self.K
        with K.batch():
            b_n = K.get_norms(self.c_trial)
            b_v = K.get_varphi(self.obj_val_trial, self.x_trial, self.xl, self.xu, self.mu)
        return b_n[1], b_v[0]

    # adaptive barrier rules
    def _average_complementarity(self):
        return self.K.get_average_complementarity(self.x, self.xl, self.xu, self.zl, self.zu)

    def _min_complementarity(self):
        return self.K.get_min_complementarity(self.x, self.xl, self.xu, self.zl, self.zu)

    def _set_affine_rhs(self):
        p = self.p
        self.K.set_aug_rhs(self.f, self.zl, self.zu, self.jacl, self.c, self.x, self.xl, self.xu, 0.0, self._primal(p),
                           self._dual(p), self._dual_lb(p), self._dual_ub(p))

    def _set_centering_rhs(self, mu):
        p, K = self.p, self.K
        K.vec_fill(self._primal(p), 0.0)
        K.vec_fill(self._dual(p), 0.0)
        K.vec_fill(self._dual_lb(p), mu)
        K.vec_fill(self._dual_ub(p), -mu)
        K.dual_inf_perturbation(self._primal(p), mu, self.opt.kappa_d)

    def _solve_kkt_plain(self, w):
        """One `solve_kkt!` of a copy of p on the device; the solver's verdict on a one-launch solve is read once the stream
        is idle, and the solve repeated stepwise if it gave up (as `solve_refine` does)."""
        from .linear_solver import SolveException
        for attempt in (0, 1):
            self.K.vec_copy(w, self.p)
            self.kkt.solve_kkt_device(w)
            self._sync()
            try:
                return self.kkt.linear_solver.check_solve()
            except SolveException:
                if attempt:
                    raise

    def _quality_terms(self, sigmas, step_aff, step_cen):
        """`mnk_ipm_quality_function`: one call of four launches and one synchronization for the whole batch of sigmas."""
        a, c = step_aff, step_cen
        return self.K.quality_function(sigmas, self.x, self.xl, self.xu, self.zl, self.zu, self._primal(a), self._dual_lb(a),
                                       self._dual_ub(a), self._primal(c), self._dual_lb(c), self._dual_ub(c), self.tau)

    # robust restorer (`mnk_ipm_*_R`)
    def _rr_init_vectors(self, RR, mu_R, rho):
        self.K.initialize_robust_restorer(self.x, self.c, mu_R, rho, RR.x_ref, RR.D_R, RR.nn, RR.pp, RR.zp, RR.zn, self.zl, self.zu)
        self.K.vec_fill(RR.f_R, 0.0)
        self.K.vec_fill(self.y, 0.0)

    def _rr_obj_val(self, pp, nn, x):
        RR = self.RR
        return self.K.get_obj_val_R(pp, nn, RR.D_R, x, RR.x_ref, self.opt.rho, RR.zeta)

    def _rr_theta(self, c, pp, nn): return self.K.get_theta_R(c, pp, nn)

    def _rr_inf_pr(self): return self.K.get_inf_pr_R(self.c, self.RR.pp, self.RR.nn)

    def _rr_inf_du(self, sd):
        RR = self.RR
        return self.K.get_inf_du_R(RR.f_R, self.y, self.zl, self.zu, self.jacl, RR.zp, RR.zn, self.opt.rho, sd)

    def _rr_inf_compl(self, mu, sc):
        RR = self.RR
        return self.K.get_inf_compl_R(self.x, self.xl, self.xu, self.zl, self.zu, RR.pp, RR.zp, RR.nn, RR.zn, mu, sc)

    def _rr_varphi(self, obj, x, pp, nn):
        return self.K.get_varphi_R(obj, x, self.xl, self.xu, pp, nn, self.RR.mu_R)

    def _rr_varphi_d(self):
        RR = self.RR
        return self.K.get_varphi_d_R(RR.f_R, self.x, self.xl, self.xu, self._dx(), RR.pp, RR.nn, RR.dpp, RR.dnn, RR.mu_R,
                                     self.opt.rho)

    def _rr_alpha_max(self):
        RR = self.RR
        return self.K.get_alpha_max_R(self.x, self.xl, self.xu, self._dx(), RR.pp, RR.dpp, RR.nn, RR.dnn, RR.tau_R)

    def _rr_alpha_z(self):
        RR = self.RR
        return self.K.get_alpha_z_R(self.zl, self.zu, self._dzl(), self._dzu(), RR.zp, RR.dzp, RR.zn, RR.dzn, RR.tau_R)

    def _rr_set_aug(self):
        o, RR = self.opt, self.RR
        self.kkt.set_aug_RR_device(self.x, self.xl, self.xu, self.zl, self.zu, RR.D_R, RR.pp, RR.zp, RR.nn, RR.zn, RR.zeta,
                                   o.default_primal_regularization, o.default_dual_regularization)

    def _rr_set_rhs(self):
        p, RR = self.p, self.RR
        self.K.set_aug_rhs_RR(RR.f_R, self.zl, self.zu, self.jacl, self.c, self.y, RR.pp, RR.nn, RR.zp, RR.zn, self.x, self.xl,
                              self.xu, RR.mu_R, self.opt.rho, self._primal(p), self._dual(p), self._dual_lb(p), self._dual_ub(p))

    def _rr_finish(self):
        RR = self.RR
        self.K.finish_aug_solve_RR(RR.dpp, RR.dnn, RR.dzp, RR.dzn, self.y, self._dy(), RR.pp, RR.nn, RR.zp, RR.zn, RR.mu_R,
                                   self.opt.rho)

    def _rr_set_f(self):
        RR = self.RR
        self.K.set_f_RR(RR.f_R, RR.D_R, self.x, RR.x_ref, RR.zeta)

    def _rr_reset_slack_duals(self):
        RR, ks = self.RR, self.opt.kappa_sigma
        self.K.reset_bound_dual_1(RR.zp, RR.pp, RR.mu_R, ks)
        self.K.reset_bound_dual_1(RR.zn, RR.nn, RR.mu_R, ks)

    # ------------------------------------------------------------------ solve!: host initialization, upload, then the base
    # class's phases (regular! / restore! / robust!) on the device tensors
    def solve(self):
        if self.status == "INITIAL":
            self.initialize()          # host (numpy), once
            self._upload()
        return super().solve()

    def close(self):
        """Release the callbacks, the vector kernels and the KKT handle, in that order; before `_upload` only the last exists."""
        for name in ("cb", "K", "kkt"):
            if hasattr(getattr(self, name, None), "close"):
                getattr(self, name).close()

    def solution(self):
        """`MadNLPSolver.solution` from a download of the iterate."""
        return unpack_solution(self, *self.host_state())

    def host_state(self):
        """x, y, zl, zu on the host (tests, reporting)."""
        self._sync()      # the library's stream may not be torch's: the download below must see the finished loop
        return tuple(v.cpu().numpy() for v in (self.x, self.y, self.zl, self.zu))

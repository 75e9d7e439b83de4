"""Minimal interior-point driver that replays MadNLP's call sequence around the KKT hot path.

The IPM loop itself is NOT part of the hot path (host code stays the reference's Julia); this
driver exists because Julia cannot run in the build image and the parity statement of the north
star is about *primal/dual residuals per iteration*.  It follows the regular phase of the
reference closely enough that iteration counts and residual histories are meaningful
(SURVEY.md Appendix A):

  initialize!            src/IPM/solver.jl:14-77, src/Callbacks/nlpmodels.jl:593-636
  regular!               src/IPM/solver.jl:216-298
  update_barrier!        src/IPM/barrier.jl:12-34 (monotone), src/IPM/kernels.jl:697-713; the adaptive rules (`barrier =
                         "loqo" / "quality_function"`) barrier.jl:95-316 with the options of src/IPM/types.jl:76-146
  set_aug_diagonal!/rhs  src/IPM/kernels.jl:4-27,113-130,818-823
  inertia_correction!    src/IPM/solver.jl:611-670 (InertiaBased), :672-737 (InertiaFree, with curv_test :785-788),
                         :739-783 (InertiaIgnore); the method is chosen at construction as IPM.jl:203-207 does
  solve_refine_wrapper!  src/IPM/factorization.jl:1-19 + backsolve.jl
  filter_line_search!    src/IPM/line_search.jl:6-123 (+ second-order correction solver.jl:547-608)
  restore!               src/IPM/solver.jl:300-411 (soft restoration, get_F kernels.jl:572-610)
  robust!                src/IPM/solver.jl:413-545, src/IPM/restoration.jl:39-76, filter_line_search_RR!
                         src/IPM/line_search.jl:128-222, _update_monotone_RR! src/IPM/barrier.jl:39-84

NLP scaling (`nlp_scaling`, off by default) and the objective sense (a model's `minimize` attribute): `set_scaling!`
src/IPM/solver.jl:37-49 with the factor functions of src/Callbacks/nlpmodels.jl:222-264, the callback wrappers :771-906 and
src/IPM/callbacks.jl:9,28-30,82, un-scaled results (`solution()`) nlpmodels.jl:649-661.
Quasi-Newton Hessians (`hessian_approximation = "bfgs" / "damped_bfgs"`, dense KKT systems; `"compact_lbfgs"`, the sparse
condensed system behind `kkt.LowRankHessianKKT`): `quasi_newton.py` and `eval_lag_hess` below (src/IPM/callbacks.jl:145-190).

Fixed variables as parameters (`fixed_variable_treatment = "make_parameter"`, off by default): `fixed_vars.py` -- the solver
evaluates `self.model`, the reduced (sparse) or frozen (dense) view of `self.nlp`, and `unpack_solution` un-reduces.

It is backend agnostic: `kkt_factory(info)` builds any object with the KKT interface -- the HIP
mirror (`madnlp_jl_amd.kkt`) or, in the tests, the CPU oracle.

The whole driver -- regular!, the inertia correction loop, both line searches, the second-order correction, restore!, robust! --
is written once, here, against the vector primitives named in `BACKEND_PRIMITIVES`: numpy in this class, the `mnk_ipm_*`
kernels on device tensors in `ipm_dev.DeviceMadNLPSolver`, which adds no control flow of its own beyond its first correction
trial (the `probe` option and the speculative pair).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from .backsolve import ITERATORS, KrylovIterator, RichardsonIterator
from .fixed_vars import TREATMENTS as FIXED_VARIABLE_TREATMENTS, FixedVariableHandler
from .kkt import LowRankHessianKKT, UnreducedKKTVector
from .quasi_newton import HESSIAN_APPROXIMATIONS, QuasiNewtonOptions, create_quasi_newton

INF = float("inf")
EPS = np.finfo(np.float64).eps


def _pow(a, b):
    """a^b with IEEE overflow to Inf (Python's float power raises OverflowError instead)."""
    try:
        return a ** b
    except OverflowError:
        return INF


@dataclass
class IPMOptions:
    """Defaults of reference src/IPM/options.jl:117-204 and src/IPM/types.jl:66-73."""
    tol: float = 1e-8
    acceptable_tol: float = 1e-6
    acceptable_iter: int = 15
    diverging_iterates_tol: float = 1e20
    max_iter: int = 3000
    s_max: float = 100.0
    kappa_d: float = 1e-5
    bound_relax_factor: float = 1e-8
    default_primal_regularization: float = 0.0
    default_dual_regularization: float = 0.0
    constr_mult_init_max: float = 1e3
    bound_push: float = 1e-2
    bound_fac: float = 1e-2
    dual_initialization: str = "least_squares"  # "zero" for the sparse condensed preset (options.jl:160)
    relax_equality: bool = False                 # RelaxEquality preset of SparseCondensedKKTSystem
    min_hessian_perturbation: float = 1e-20
    first_hessian_perturbation: float = 1e-4
    max_hessian_perturbation: float = 1e20
    perturb_inc_fact_first: float = 1e2
    perturb_inc_fact: float = 8.0
    perturb_dec_fact: float = 1 / 3
    jacobian_regularization_exponent: float = 1 / 4
    jacobian_regularization_value: float = 1e-8
    obj_max_inc: float = 5.0
    max_soc: int = 4
    alpha_min_frac: float = 0.05
    s_theta: float = 1.1
    s_phi: float = 2.3
    eta_phi: float = 1e-4
    kappa_soc: float = 0.99
    gamma_theta: float = 1e-5
    gamma_phi: float = 1e-5
    delta: float = 1.0
    kappa_sigma: float = 1e10
    barrier_tol_factor: float = 10.0
    tau_min: float = 0.99
    mu_init: float = 1e-1
    mu_linear_decrease_factor: float = 0.2
    mu_superlinear_decrease_power: float = 1.5
    rho: float = 1000.0                                  # options.jl:195
    # options.jl:153-154: "auto" (InertiaAuto: inertia_based if the linear solver reveals the inertia, else inertia_free),
    # "inertia_based", "inertia_free", "ignore"
    inertia_correction_method: str = "auto"
    inertia_free_tol: float = 0.0
    soft_resto_pderror_reduction_factor: float = 0.9999  # options.jl:178
    required_infeasibility_reduction: float = 0.9        # options.jl:179
    # options.jl `hessian_approximation`: "exact" (ExactHessian), "bfgs" (BFGS), "damped_bfgs" (DampedBFGS) -- these two on
    # the dense KKT systems only (the reference has no dense BFGS for sparse systems) -- and "compact_lbfgs" (CompactLBFGS) on
    # the sparse condensed system only, with the fields of the reference's QuasiNewtonOptions (quasi_newton.jl:63-69;
    # qn_init_strategy 1 .. 4 = SCALAR1 .. SCALAR4)
    hessian_approximation: str = "exact"
    qn_max_history: int = 6
    qn_init_strategy: int = 1
    qn_init_value: float = 1.0
    qn_sigma_min: float = 1e-8
    qn_sigma_max: float = 1e8
    # options.jl:164-165.  The reference's default is `true`; here it is False because every recorded trajectory, golden file
    # and profile of this project was made without scaling -- switching the default is a change of its own
    nlp_scaling: bool = False
    nlp_scaling_max_gradient: float = 100.0
    # options.jl `barrier`: "monotone" (MonotoneUpdate), "loqo" (LOQOUpdate), "quality_function" (QualityFunctionUpdate); the
    # fields of the two adaptive rules with the defaults of types.jl:101-143 (mu_init, mu_min and the two monotone decrease
    # parameters above are shared by all three)
    barrier: str = "monotone"
    barrier_globalization: bool = True
    barrier_mu_max: float = 1e5
    qf_sigma_min: float = 1e-6
    qf_sigma_max: float = 1e2
    qf_sigma_tol: float = 1e-2
    qf_max_gs_iter: int = 8
    loqo_gamma: float = 0.1
    loqo_r: float = 0.95
    # options.jl `iterator`: "richardson" (RichardsonIterator) or "krylov" (the restarted GMRES of lib/MadNLPKrylov, with its
    # defaults restart = 5, max_iter = 10, tol = 1e-10; the stopping rules are relative here)
    iterator: str = "richardson"
    krylov_restart: int = 5
    krylov_max_iter: int = 10
    krylov_tol: float = 1e-10
    # options.jl `fixed_variable_treatment`: "relax_bound" (RelaxBound) or "make_parameter" (MakeParameter, fixed_vars.py).
    # The reference's default is MakeParameter for every KKT system but the sparse condensed one (options.jl:146); here it is
    # "relax_bound" for all of them because every recorded trajectory, golden file and profile was made with it
    fixed_variable_treatment: str = "relax_bound"
    # options.jl `callback`: "sparse" (SparseCallback: the model's COO callbacks, scattered in COO order into the dense Jacobian
    # and Hessian where the KKT system is dense, nlpmodels.jl:829-842, :863-881), "dense" (DenseCallback: the model's own
    # `jac_dense` / `hess_dense`), or "auto": sparse callbacks for the sparse KKT system, dense ones for the dense systems
    callback: str = "auto"

    @property
    def mu_min(self):
        return min(1e-4, self.tol) / (self.barrier_tol_factor + 1)


@dataclass
class Counters:
    k: int = 0
    l: int = 0
    factorization_cnt: int = 0
    backsolve_cnt: int = 0
    acceptable_cnt: int = 0
    unsuccessful_iterate: int = 0
    restoration_fail_count: int = 0
    t: int = 0
    lag_hess_cnt: int = 0     # exact Lagrangian Hessians evaluated: stays 0 in a quasi-Newton run (test/madnlp_quasi_newton.jl:33)
    obj_grad_cnt: int = 0     # objective gradients evaluated (the quasi-Newton update starts with the second one)
    barrier_update_cnt: int = 0   # quality-function updates (`n_update`, barrier.jl:300)
    probe_solve_cnt: int = 0      # plain KKT solves of the quality-function rule, two per update; not part of backsolve_cnt
    quality_eval_cnt: int = 0     # quality-function values computed (6 to 14 per update)


@dataclass
class RobustRestorer:
    """`RobustRestorer` reference src/IPM/types.jl / src/IPM/restoration.jl:1-37 (vectors are created by the solver: numpy
    arrays here, device tensors in the device-resident driver)."""
    obj_val_R: float = 0.0
    theta_ref: float = 0.0
    obj_val_R_trial: float = 0.0
    inf_pr_R: float = 0.0
    inf_du_R: float = 0.0
    inf_compl_R: float = 0.0
    mu_R: float = 0.0
    tau_R: float = 0.0
    zeta: float = 0.0
    filter: list = field(default_factory=list)


INERTIA_CORRECTION_METHODS = ("auto", "inertia_based", "inertia_free", "ignore")
BARRIER_UPDATES = ("monotone", "loqo", "quality_function")
CALLBACKS = ("auto", "sparse", "dense")


def _clamp(x, lo, hi):
    """Julia's `clamp`: hi above it, lo below it, x itself otherwise (a NaN stays a NaN)."""
    return hi if x > hi else lo if x < lo else x


def _fdiv(a, b):
    """a / b with IEEE results for b == 0 (Python raises ZeroDivisionError instead)."""
    if b != 0:
        return a / b
    return float("nan") if a == 0 or a != a else math.copysign(INF, a) * math.copysign(1.0, b)


def ordered_sum(v, blocks=256, threads=256):
    """sum(v) in the fixed order of the library's sum reductions (`map_reduce_kernel` / `final_reduce_kernel`, csrc/ipm_vec.hip):
    element i goes to lane i mod (blocks threads), every lane adds its elements in increasing order, the lanes of a block are
    added by a halving tree (lane j += lane j + s for s = threads/2 ... 1), and so are the blocks' results.  The same bits as
    `mnk_ipm_get_sum` on the same values; used where a sum enters the iterate and both back-ends must agree exactly."""
    v = np.asarray(v, dtype=np.float64)
    lanes = blocks * threads
    trips = max(1, -(-len(v) // lanes))
    a = np.zeros(trips * lanes)
    a[:len(v)] = v
    a = a.reshape(trips, blocks, threads)
    acc = np.zeros((blocks, threads))
    for t in range(trips):
        acc = acc + a[t]
    s = threads // 2
    while s > 0:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    part = acc[:, 0].copy()
    s = blocks // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return float(part[0])


def golden_section(q, lo, hi, max_iter, tol, bracket=None):
    """`_run_golden_search!` barrier.jl:205-246, restated as written: the minimizer of a (supposedly unimodal) function over
    [lo, hi] by at most `max_iter` golden-section steps, stopped early once the bracket is narrower than `tol` times its upper
    end.  `q` takes a LIST of points and returns their values: the four initial points lo, hi, mid1, mid2 are asked for in one
    call, every step asks for one more, so there are at most 4 + max_iter evaluations.  Two things are the reference's own:
    after the re-evaluation in the else branch phi_mid2 receives the NEW phi_mid1 (:230-231, not the value that moved to mid2),
    and the end-point correction (:240-244) returns an end of the initial interval that was never left and whose value is
    below the search's.  `bracket`, if a list, receives the final (sigma_1, sigma_2)."""
    gfac = 0.5 * (3.0 - math.sqrt(5.0))
    sigma_1, sigma_2 = lo, hi
    sigma_mid1 = lo + gfac * (hi - lo)
    sigma_mid2 = lo + (1.0 - gfac) * (hi - lo)
    phi_1, phi_2, phi_mid1, phi_mid2 = q([sigma_1, sigma_2, sigma_mid1, sigma_mid2])
    sigma_1_in, sigma_2_in, phi_1_in, phi_2_in = sigma_1, sigma_2, phi_1, phi_2
    for _ in range(max_iter):
        if phi_mid1 > phi_mid2:
            sigma_1 = sigma_mid1
            phi_1 = phi_mid1
            sigma_mid1 = sigma_mid2
            sigma_mid2 = sigma_1 + (1.0 - gfac) * (sigma_2 - sigma_1)
            phi_mid1 = phi_mid2
            phi_mid2, = q([sigma_mid2])
        else:
            sigma_2 = sigma_mid2
            phi_2 = phi_mid2
            sigma_mid2 = sigma_mid1
            sigma_mid1 = sigma_1 + gfac * (sigma_2 - sigma_1)
            phi_mid1, = q([sigma_mid1])
            phi_mid2 = phi_mid1
        if sigma_2 - sigma_1 < tol * sigma_2:
            break
    sigma, phi = (sigma_mid1, phi_mid1) if phi_mid1 < phi_mid2 else (sigma_mid2, phi_mid2)
    if sigma_2 == sigma_2_in and phi_2_in < phi:
        sigma = sigma_2_in
    elif sigma_1 == sigma_1_in and phi_1_in < phi:
        sigma = sigma_1_in
    if bracket is not None:
        bracket.append((sigma_1, sigma_2))
    return sigma


@dataclass
class InertiaFreeCorrector:
    """`InertiaFree` inertiacorrector.jl:7-20: right-hand side / solution of the normal step, the tangential step t, the
    Hessian product wx and the barrier gradient g."""
    p0: object
    d0: object
    t: np.ndarray
    wx: np.ndarray
    g: np.ndarray


def curv_test(t, n, g, kkt, wx, inertia_free_tol):
    """`curv_test` solver.jl:785-788: t'Wt + max(t'W n - g'n, 0) - tol t't >= 0 (W: the Hessian block with its diagonal)."""
    kkt.mul_hess_blk(wx, t)
    return float(np.dot(wx, t)) + max(float(np.dot(wx, n)) - float(np.dot(g, n)), 0.0) - \
        inertia_free_tol * float(np.dot(t, t)) >= 0


@dataclass
class IterRecord:
    k: int
    obj: float
    inf_pr: float
    inf_du: float
    inf_compl: float
    mu: float
    del_w: float
    alpha: float
    ls: int
    phase: str = ""   # "" regular, "r" soft restoration (restore!), "R" robust restoration (robust!)


def parse_indexes(lvar, uvar, lcon, ucon, enforce_equality):
    """`_parse_indexes` reference src/Callbacks/nlpmodels.jl:369-406 (0-based)."""
    m = len(lcon)
    if m > 0 and enforce_equality:
        is_eq = lcon == ucon
        ind_eq = np.nonzero(is_eq)[0]
        ind_ineq = np.nonzero(~is_eq)[0]
    else:
        ind_eq = np.zeros(0, dtype=np.int64)
        ind_ineq = np.arange(m)
    xl = np.concatenate((lvar, lcon[ind_ineq]))
    xu = np.concatenate((uvar, ucon[ind_ineq]))
    ind_llb = np.nonzero((lvar != -INF) & (uvar == INF))[0]
    ind_uub = np.nonzero((lvar == -INF) & (uvar != INF))[0]
    ind_lb = np.nonzero(xl != -INF)[0]
    ind_ub = np.nonzero(xu != INF)[0]
    return dict(xl=xl, xu=xu, ind_eq=ind_eq, ind_ineq=ind_ineq, ind_lb=ind_lb, ind_ub=ind_ub, ind_llb=ind_llb,
                ind_uub=ind_uub)


def _set_initial_bounds(xl, xu, tol):
    """reference src/IPM/kernels.jl:206-218."""
    if tol > 0:
        xl -= np.maximum(1.0, np.abs(xl)) * tol
        xu += np.maximum(1.0, np.abs(xu)) * tol


def _initialize_variables(x, xl, xu, bound_push, bound_fac):
    """reference src/IPM/kernels.jl:638-654."""
    for i in range(len(x)):
        l, u = xl[i], xu[i]
        if l != -INF and u != INF:
            x[i] = min(u - min(bound_push * max(1, abs(u)), bound_fac * (u - l)),
                       max(l + min(bound_push * max(1, abs(l)), bound_fac * (u - l)), x[i]))
        elif l != -INF:
            x[i] = max(l + bound_push * max(1, abs(l)), x[i])
        elif u != INF:
            x[i] = min(u - bound_push * max(1, abs(u)), x[i])


def set_obj_scale(grad, max_gradient):
    """`set_obj_scale!` nlpmodels.jl:225-227: min(1, max_gradient / norm(grad, Inf)); a zero gradient gives 1 (Julia: 100 / 0
    = Inf)."""
    g = float(np.abs(grad).max(initial=0.0))
    return 1.0 if g == 0.0 else min(1.0, max_gradient / g)


def set_con_scale_sparse(m, jac_I, jac, max_gradient):
    """`set_con_scale_sparse!` nlpmodels.jl:229-244: per row min(1, max_gradient / max(1, max |jac entry|)) over the COO
    entries as they are (duplicates are not summed)."""
    row_max = np.ones(m)
    np.maximum.at(row_max, np.asarray(jac_I, dtype=np.int64), np.abs(np.asarray(jac, dtype=float)))
    return np.minimum(1.0, max_gradient / row_max)


def set_con_scale_dense(jac, max_gradient):
    """`set_con_scale_dense!` nlpmodels.jl:254-264: the same from the rows of a dense Jacobian (init = 1)."""
    jac = np.asarray(jac, dtype=float)
    return np.minimum(1.0, max_gradient / np.abs(jac).max(axis=1, initial=1.0))


def scatter_jac_coo(jac, I, J, values):
    """`_eval_jac_wrapper!` of SparseCallback on a dense Jacobian (nlpmodels.jl:829-842): zero, then the COO values added
    entry by entry in COO order (`np.add.at` is that loop)."""
    jac[...] = 0.0
    np.add.at(jac, (I, J), values)


def hess_mirror_coo(I, J):
    """(rows, columns, COO positions) of the reference's Hessian loop (nlpmodels.jl:863-881) unrolled: every entry (i, j)
    followed by its mirror image (j, i), diagonal entries once."""
    k = np.repeat(np.arange(len(I)), 2)
    swap = np.arange(len(k)) % 2 == 1
    keep = ~(swap & (I[k] == J[k]))
    return np.where(swap, J[k], I[k])[keep], np.where(swap, I[k], J[k])[keep], k[keep]


def scatter_hess_coo(hess, mirror, values):
    """`_eval_lag_hess_wrapper!` of SparseCallback on a dense Hessian: zero, then (i, j) and, off the diagonal, (j, i), entry
    by entry in COO order; both triangles are written, whichever the model gives."""
    r, c, k = mirror
    hess[...] = 0.0
    np.add.at(hess, (r, c), values[k])


@dataclass
class Solution:
    """What the reference hands back in `MadNLPExecutionStats`, un-scaled (nlpmodels.jl:649-661).  `constraints` is left out."""
    status: str
    iterations: int
    solution: np.ndarray
    objective: float
    multipliers: np.ndarray
    multipliers_L: np.ndarray
    multipliers_U: np.ndarray


def unpack_solution(solver, x, y, zl, zu):
    """`unpack_obj`, `unpack_x!`, `unpack_y!`, `unpack_z!` on host copies of the iterate.  With variables made parameters
    (`solver.fixed_handler`) x, zl and zu come back with the model's full length: the fixed entries of x are lvar, those of
    zl / zu come from `update_z!` (`FixedVariableHandler.unpack`), once per call, on the host."""
    n, s = solver.n, solver.obj_scale
    xs, ys, zls, zus = np.array(x[:n]), (y * solver.con_scale) * (solver.obj_sign / s), zl[:n] / s, zu[:n] / s
    if solver.fixed_handler is not None:
        xs, zls, zus = solver.fixed_handler.unpack(solver.nlp, xs, zls, zus, ys, solver.obj_sign)
    return Solution(solver.status, solver.cnt.k, xs, solver.obj_sign * solver.obj_val / s, ys, zls, zus)


# What a back-end of `MadNLPSolver` supplies: the methods that touch vectors.  The host class implements them with numpy; a
# subclass that keeps its vectors elsewhere (`ipm_dev.DeviceMadNLPSolver`) overrides ALL of them -- none may fall back to numpy
# on its vectors (tests/test_ipm_driver_structure.py).  The inertia-free corrector's kernels (`_set_g_ifr`, `_set_aug_rhs_ifr`,
# `_ifr_solves`, `curv_test`) are not in the list: that method is host-only so far.
BACKEND_PRIMITIVES = (
    "eval_f", "eval_grad", "eval_cons", "eval_jac", "eval_lag_hess", "factorize_wrapper", "solve_refine_wrapper",
    "set_aug_diagonal", "set_aug_rhs", "inf_compl", "varphi", "alpha_max",
    "_primal", "_dual", "_dual_lb", "_dual_ub", "_new_vec", "_clone", "_vcopy", "_vaxpy", "_vaxpby", "_vfill", "_theta",
    "_norm_inf", "_norm2", "_regularize", "_sd_sc", "_inf_du", "_iteration_scalars", "_jtprod", "_alpha_z", "_bound_dual_axpy",
    "_bound_dual_fill", "_adjust_boundary", "_reset_bound_dual", "_get_F", "_set_initial_rhs", "_kkt_initialize",
    "_rel_search_norm", "_line_search_scalars", "_trial_scalars",
    "_average_complementarity", "_min_complementarity", "_set_affine_rhs", "_set_centering_rhs", "_solve_kkt_plain",
    "_quality_terms",
    "_rr_init_vectors", "_rr_obj_val", "_rr_theta", "_rr_inf_pr", "_rr_inf_du", "_rr_inf_compl", "_rr_varphi", "_rr_varphi_d",
    "_rr_alpha_max", "_rr_alpha_z", "_rr_set_aug", "_rr_set_rhs", "_rr_finish", "_rr_set_f", "_rr_reset_slack_duals",
    "solution",
)


class MadNLPSolver:
    def __init__(self, nlp, kkt_factory, opt: IPMOptions | None = None, sparse=True):
        self.nlp, self.opt, self.sparse = nlp, opt or IPMOptions(), sparse
        o = self.opt
        if o.hessian_approximation not in HESSIAN_APPROXIMATIONS:
            raise ValueError(f"hessian_approximation must be one of {HESSIAN_APPROXIMATIONS}, not {o.hessian_approximation!r}")
        self.lbfgs = o.hessian_approximation == "compact_lbfgs"
        if self.lbfgs and not sparse:
            raise ValueError("hessian_approximation = 'compact_lbfgs' needs the sparse condensed KKT system (sparse=True)")
        if o.hessian_approximation != "exact" and sparse and not self.lbfgs:
            raise ValueError(f"hessian_approximation = {o.hessian_approximation!r} needs a dense KKT system (sparse=False)")
        if o.fixed_variable_treatment not in FIXED_VARIABLE_TREATMENTS:
            raise ValueError(f"fixed_variable_treatment must be one of {FIXED_VARIABLE_TREATMENTS}, not "
                             f"{o.fixed_variable_treatment!r}")
        # MakeParameter (fixed_vars.py): None for a model without fixed variables -- then nothing below differs from
        # "relax_bound".  `self.model` is what the callbacks evaluate: the reduced (sparse) or frozen (dense) view of `nlp`
        if o.callback not in CALLBACKS:
            raise ValueError(f"callback must be one of {CALLBACKS}, not {o.callback!r}")
        # `coo_dense`: the model's COO callbacks feed a dense KKT system (`scatter_jac_coo`, `scatter_hess_coo`)
        self.coo_dense = o.callback == "sparse" and not sparse
        if o.callback == "dense" and (sparse or not hasattr(nlp, "jac_dense")):
            raise NotImplementedError("callback = 'dense' " + ("with the sparse KKT system (sparse=True)" if sparse else
                                      f"with a model that has no jac_dense / hess_dense ({type(nlp).__name__})")
                                      + ": use callback = 'sparse'")
        if (self.coo_dense and o.fixed_variable_treatment == "make_parameter"
                and (np.asarray(nlp.lvar, float) == np.asarray(nlp.uvar, float)).any()):
            raise NotImplementedError("callback = 'sparse' on a dense KKT system (sparse=False) with fixed_variable_treatment = "
                                      "'make_parameter' and fixed variables present: frozen variables are written for the "
                                      "model's dense callbacks only; use 'relax_bound' or callback = 'dense'")
        self.fixed_handler = FixedVariableHandler.create(nlp, sparse) if o.fixed_variable_treatment == "make_parameter" else None
        if self.fixed_handler is not None and o.hessian_approximation != "exact":
            raise ValueError(f"fixed_variable_treatment = 'make_parameter' with fixed variables present needs "
                             f"hessian_approximation = 'exact', not {o.hessian_approximation!r}: the secant pair of a "
                             "quasi-Newton method over frozen / eliminated variables is not implemented")
        self.model = nlp if self.fixed_handler is None else self.fixed_handler.model
        nlp = self.model
        n, m = nlp.n, nlp.m
        qn_opt = QuasiNewtonOptions(init_strategy=o.qn_init_strategy, max_history=o.qn_max_history, init_value=o.qn_init_value,
                                    sigma_min=o.qn_sigma_min, sigma_max=o.qn_sigma_max)
        self.qn = None if o.hessian_approximation == "exact" else create_quasi_newton(o.hessian_approximation, n, qn_opt)
        idx = parse_indexes(np.asarray(nlp.lvar, float), np.asarray(nlp.uvar, float), np.asarray(nlp.lcon, float),
                            np.asarray(nlp.ucon, float), enforce_equality=not o.relax_equality)
        self.idx = idx
        self.n, self.m, self.ns = n, m, len(idx["ind_ineq"])
        self.ind_ineq, self.ind_lb, self.ind_ub = idx["ind_ineq"], idx["ind_lb"], idx["ind_ub"]
        self.ind_llb, self.ind_uub = idx["ind_llb"], idx["ind_uub"]
        if self.lbfgs:
            # the diagonal Hessian pattern the reference's build_hessian_structure gives a quasi-Newton method: the n-vector
            # `get_hessian()` holds sigma.  Factories written for exact Hessians read the model's own pattern instead
            diag = np.arange(n, dtype=np.int64)
            self.kkt = LowRankHessianKKT(kkt_factory(dict(n=n, m=m, hess_I=diag, hess_J=diag, **idx)), self.qn)
        else:
            reduced = {} if self.fixed_handler is None else self.fixed_handler.structure_info()   # (fixed_vars.structure)
            self.kkt = kkt_factory(dict(n=n, m=m, **idx, **reduced))
        nt = n + self.ns
        self.x, self.xl, self.xu = np.zeros(nt), idx["xl"].copy(), idx["xu"].copy()
        self.zl, self.zu, self.f = np.zeros(nt), np.zeros(nt), np.zeros(nt)
        self.y, self.c, self.rhs = np.zeros(m), np.zeros(m), np.zeros(m)
        self.jacl = np.zeros(nt)
        self.x_trial, self.c_trial = np.zeros(nt), np.zeros(m)
        V = lambda: UnreducedKKTVector(nt, m, len(self.ind_lb), len(self.ind_ub), self.ind_lb, self.ind_ub)  # noqa: E731
        self.d, self.p, self._w1, self._w4 = V(), V(), V(), V()
        method = o.inertia_correction_method
        if method not in INERTIA_CORRECTION_METHODS:
            raise ValueError(f"inertia_correction_method must be one of {INERTIA_CORRECTION_METHODS}, not {method!r}")
        if method == "auto":   # IPM.jl:203-207
            method = "inertia_based" if self.kkt.linear_solver.is_inertia() else "inertia_free"
        self.inertia_correction_method = method
        if o.barrier not in BARRIER_UPDATES:
            raise ValueError(f"barrier must be one of {BARRIER_UPDATES}, not {o.barrier!r}")
        self.free_mode = True      # adaptive barrier rules: free mode / monotone mode (types.jl:113,141), solver state
        if method == "inertia_free":   # the corrector's storage, inertiacorrector.jl:7-20 / solver.jl:756-765
            self._ifr = InertiaFreeCorrector(V(), V(), np.zeros(nt), np.zeros(nt), np.zeros(nt))
            self._w3 = V()
        if o.iterator not in ITERATORS:
            raise ValueError(f"iterator must be one of {ITERATORS}, not {o.iterator!r}")
        if o.iterator == "krylov":   # (its constructor checks krylov_restart and krylov_max_iter)
            self.iterator = KrylovIterator(self.kkt, tol=o.tol, restart=o.krylov_restart, max_iter=o.krylov_max_iter,
                                           krylov_tol=o.krylov_tol)
        else:
            self.iterator = RichardsonIterator(self.kkt, tol=o.tol)
        self.cnt = Counters()
        self.filter = []
        self.history: list[IterRecord] = []
        self.del_w = self.del_c = self.del_w_last = 0.0
        self.alpha = self.alpha_z = 0.0
        self.mu = self.tau = 0.0
        self.obj_val = 0.0
        # NLP scaling (all ones until `initialize` sets them) and the objective sense (callbacks.jl:9)
        self.obj_scale = 1.0
        self.obj_sign = 1.0 if getattr(nlp, "minimize", True) else -1.0
        self.con_scale = np.ones(m)
        self.jac_scale = np.ones(len(nlp.jac_I)) if sparse or self.coo_dense else None     # con_scale[jac_I]
        if self.coo_dense:
            self._coo = tuple(np.asarray(getattr(nlp, k), dtype=np.int64) for k in ("jac_I", "jac_J", "hess_I", "hess_J"))
            self._coo_mirror = hess_mirror_coo(*self._coo[2:])
        self.status = "INITIAL"

    # ------------------------------------------------------------------ callbacks (src/IPM/callbacks.jl)
    # The model's raw values take the scaling factors and the sense here (nlpmodels.jl:771-906); with the factors at one every
    # product below is exact.
    def eval_f(self, x):
        return self.obj_sign * (self.model.obj(x[:self.n]) * self.obj_scale)

    def eval_grad(self, x):
        self.f[:self.n] = self.model.grad(x[:self.n])
        self.f[:self.n] *= self.obj_scale
        if self.obj_sign != 1.0:
            self.f[:self.n] *= self.obj_sign
        if self.fixed_handler is not None and not self.sparse:
            # frozen variables: x - lvar, against the unit diagonal of their Hessian rows (nlpmodels.jl:1026-1031); written
            # after the scale AND the sign, so that the Newton step pulls towards lvar in a maximization too
            self.fixed_handler.dense_grad(self.f, x)
        self.f[self.n:] = 0.0
        self.cnt.obj_grad_cnt += 1

    def eval_cons(self, c, x):
        c[:] = self.model.cons(x[:self.n])
        c *= self.con_scale
        c[self.ind_ineq] -= x[self.n:]
        c -= self.rhs

    def eval_jac(self, x):
        if self.sparse:
            self.kkt.get_jacobian()[:] = self.model.jac_coord(x[:self.n]) * self.jac_scale
        elif self.coo_dense:
            scatter_jac_coo(self.kkt.get_jacobian(), *self._coo[:2], self.model.jac_coord(x[:self.n]) * self.jac_scale)
        else:
            self.kkt.get_jacobian()[...] = self.model.jac_dense(x[:self.n]) * self.con_scale[:, None]
        self.kkt.compress_jacobian()

    def eval_lag_hess(self, x, y, is_resto=False):
        """`eval_lag_hess_wrapper!` callbacks.jl:77-95: objective weight 0 in the robust restoration phase."""
        if self.qn is not None:
            return self._eval_lag_hess_qn(x, y)
        w = (0.0 if is_resto else 1.0) * self.obj_sign * self.obj_scale
        if self.sparse:
            self.kkt.get_hessian()[:] = self.model.hess_coord(x[:self.n], y * self.con_scale, w)
        elif self.coo_dense:
            scatter_hess_coo(self.kkt.get_hessian(), self._coo_mirror, self.model.hess_coord(x[:self.n], y * self.con_scale, w))
        else:
            self.kkt.get_hessian()[...] = self.model.hess_dense(x[:self.n], y * self.con_scale, w)
        self.kkt.compress_hessian()
        self.cnt.lag_hess_cnt += 1

    def _model_jtprod(self, x, l):
        """`_eval_jtprod_wrapper!` nlpmodels.jl:791-801: J(x)' (l .* con_scale) through the model's `jtprod` where it has one."""
        l = l * self.con_scale
        if hasattr(self.model, "jtprod"):
            return np.asarray(self.model.jtprod(x, l), dtype=float)
        if self.sparse or self.coo_dense:
            out = np.zeros(self.n)
            np.add.at(out, np.asarray(self.model.jac_J, dtype=np.int64),
                      self.model.jac_coord(x) * l[np.asarray(self.model.jac_I, dtype=np.int64)])
            return out
        return self.model.jac_dense(x).T @ l

    def _eval_lag_hess_qn(self, x, y):
        """The quasi-Newton method of `eval_lag_hess_wrapper!` (callbacks.jl:145-190): no second derivative is evaluated.
        The first call (inside `initialize`, one gradient evaluated) starts the approximation, every later one updates it
        with the secant pair s = x+ - x, y = grad f+ - grad f + (J+' - J') l+ over the n variables (no slacks).  `is_resto`
        is ignored, as in the reference: robust! goes on updating the same matrix."""
        qn, n = self.qn, self.n
        B = self.kkt.get_hessian()
        if self.cnt.obj_grad_cnt >= 2:
            sk = x[:n] - qn.last_x
            yk = self.f[:n] - qn.last_g
            if self.m > 0:
                # jacl already is J(x+)' l+: regular! / restore! / robust! call jtprod! with this Jacobian and these multipliers
                # right in front of this call (the reference computes it once more, callbacks.jl:170: the same bits)
                yk = yk + self.jacl[:n]
                qn.last_jv = self._model_jtprod(qn.last_x, y)
                yk = yk - qn.last_jv
            qn.update(B, sk, yk)
        else:
            qn.init(B, self.f[:n], self.obj_val)
        qn.last_x = x[:n].copy()
        qn.last_g = self.f[:n].copy()
        self.kkt.compress_hessian()

    # ------------------------------------------------------------------ views
    @property
    def x_lr(self): return self.x[self.ind_lb]
    @property
    def x_ur(self): return self.x[self.ind_ub]
    @property
    def xl_r(self): return self.xl[self.ind_lb]
    @property
    def xu_r(self): return self.xu[self.ind_ub]
    @property
    def zl_r(self): return self.zl[self.ind_lb]
    @property
    def zu_r(self): return self.zu[self.ind_ub]

    # ------------------------------------------------------------------ initialize! (solver.jl:14-77)
    def initialize(self):
        o, nlp, n = self.opt, self.model, self.n
        x0, lvar, uvar = self.x[:n], self.xl[:n], self.xu[:n]
        x0[:] = nlp.x0
        self.y[:] = nlp.y0
        lvar[:] = nlp.lvar
        uvar[:] = nlp.uvar
        lcon, ucon = np.array(nlp.lcon, float), np.array(nlp.ucon, float)
        if o.relax_equality:
            _set_initial_bounds(lcon, ucon, o.bound_relax_factor)
        _set_initial_bounds(lvar, uvar, o.bound_relax_factor)
        _initialize_variables(x0, lvar, uvar, o.bound_push, o.bound_fac)
        con = nlp.cons(x0)
        self.xl[n:] = lcon[self.ind_ineq]
        self.xu[n:] = ucon[self.ind_ineq]
        self.rhs[:] = np.where(lcon == ucon, lcon, 0.0)   # Julia: false * -Inf == -0.0 (`false` is a strong zero)
        self.x[n:] = con[self.ind_ineq]
        sl, su = self.xl[n:], self.xu[n:]
        _set_initial_bounds(sl, su, o.bound_relax_factor)
        xs = self.x[n:]
        _initialize_variables(xs, sl, su, o.bound_push, o.bound_fac)
        self.jacl[:] = 0.0
        self.zl[self.ind_lb] = 1.0
        self.zu[self.ind_ub] = 1.0
        if o.nlp_scaling:
            # set_scaling! (solver.jl:37-49, nlpmodels.jl:693-765): the factors from the model's raw Jacobian and gradient at the
            # pushed starting point (this gradient is not one of `cnt.obj_grad_cnt`), then y0, rhs and the slacks with their bounds
            if self.sparse or self.coo_dense:
                self.con_scale[:] = set_con_scale_sparse(self.m, nlp.jac_I, nlp.jac_coord(x0), o.nlp_scaling_max_gradient)
                self.jac_scale[:] = self.con_scale[np.asarray(nlp.jac_I, dtype=np.int64)]
            else:
                # (the dense set_scaling! reads the model itself, not the frozen wrappers: nlpmodels.jl:752-756)
                self.con_scale[:] = set_con_scale_dense(self.nlp.jac_dense(x0), o.nlp_scaling_max_gradient)
            self.obj_scale = set_obj_scale((nlp if self.sparse else self.nlp).grad(x0), o.nlp_scaling_max_gradient)
            con_scale_slk = self.con_scale[self.ind_ineq]
            self.y /= self.con_scale
            self.rhs *= self.con_scale
            self.x[n:] *= con_scale_slk
            self.xl[n:] *= con_scale_slk
            self.xu[n:] *= con_scale_slk
        self.kkt.initialize()
        self.eval_jac(self.x)
        self.eval_grad(self.x)
        if o.dual_initialization == "least_squares":
            self._initialize_dual_least_squares()
        else:
            self.y[:] = 0.0
        self.obj_val = self.eval_f(self.x)
        self.eval_cons(self.c, self.x)
        self.eval_lag_hess(self.x, self.y)
        theta = np.abs(self.c).sum()
        self.theta_max = 1e4 * max(1.0, theta)
        self.theta_min = 1e-4 * max(1.0, theta)
        self.mu = o.mu_init
        self.tau = max(o.tau_min, 1 - o.mu_init)
        self.filter = [(self.theta_max, -INF)]
        self.status = "REGULAR"

    def _initialize_dual_least_squares(self):
        """solver.jl:86-97 with set_initial_rhs! (kernels.jl:220-230)."""
        p = self.p
        p.values[:] = 0.0
        p.primal()[:] = -self.f + self.zl - self.zu
        self.factorize_wrapper()
        ok = self.solve_refine_wrapper(self.d, p, self._w4)
        if (not ok) or np.abs(self.d.dual()).max(initial=0.0) > self.opt.constr_mult_init_max:
            self.y[:] = 0.0
        else:
            self.y[:] = self.d.dual()

    # ------------------------------------------------------------------ factorization glue (factorization.jl:1-27)
    def factorize_wrapper(self):
        self.kkt.build_kkt()
        self.kkt.linear_solver.factorize()
        self.cnt.factorization_cnt += 1

    def solve_refine_wrapper(self, d, p, w):
        ok = self.iterator.solve_refine(d, p, w)
        if not ok and self.kkt.linear_solver.improve():
            ok = self.iterator.solve_refine(d, p, w)
        self.cnt.backsolve_cnt += self.iterator.ir
        return ok

    # ------------------------------------------------------------------ kernels (kernels.jl)
    def set_aug_diagonal(self):
        k, o = self.kkt, self.opt
        k.reg[:] = o.default_primal_regularization
        k.du_diag[:] = -o.default_dual_regularization
        k.l_diag[:] = self.xl_r - self.x_lr
        k.u_diag[:] = self.x_ur - self.xu_r
        k.l_lower[:] = self.zl_r
        k.u_lower[:] = self.zu_r
        k.pr_diag[:] = k.reg
        k.pr_diag[self.ind_lb] -= k.l_lower / k.l_diag
        k.pr_diag[self.ind_ub] -= k.u_lower / k.u_diag

    def set_aug_rhs(self, c):
        p = self.p
        p.primal()[:] = -self.f + self.zl - self.zu - self.jacl
        p.dual()[:] = -c
        p.dual_lb()[:] = (self.xl_r - self.x_lr) * self.zl_r + self.mu
        p.dual_ub()[:] = (self.xu_r - self.x_ur) * self.zu_r - self.mu
        px = p.primal()
        px[self.ind_llb] -= self.mu * self.opt.kappa_d   # dual_inf_perturbation! (kernels.jl:818-823)
        px[self.ind_uub] += self.mu * self.opt.kappa_d

    def inf_compl(self, mu, sc):
        a = np.abs((self.x_lr - self.xl_r) * self.zl_r - mu).max(initial=0.0)
        b = np.abs((self.xu_r - self.x_ur) * self.zu_r - mu).max(initial=0.0)
        return max(a, b) / sc

    def varphi(self, obj, x):
        dl = x[self.ind_lb] - self.xl_r
        du = self.xu_r - x[self.ind_ub]
        if (dl < 0).any() or (du < 0).any():
            return INF
        with np.errstate(divide="ignore"):
            return obj - self.mu * (np.log(dl).sum() + np.log(du).sum())

    def alpha_max(self, dx):
        x, xl, xu, tau = self.x, self.xl, self.xu, self.tau
        a = 1.0
        neg, pos = dx < 0, dx > 0
        with np.errstate(invalid="ignore"):
            if neg.any():
                a = min(a, ((-x[neg] + xl[neg]) * tau / dx[neg]).min())
            if pos.any():
                a = min(a, ((-x[pos] + xu[pos]) * tau / dx[pos]).min())
        return a

    # ------------------------------------------------------------------ inertia_correction! (solver.jl:611-670, :672-737, :739-783)
    on_trial = None   # diagnostics: callable(solver, n_trial, inertia, inertia_correct, accepted) after every trial of inertia_correction

    def inertia_correction(self):
        """The loop the three correctors share: try the matrix as it is, then perturb, factorize and try again until a trial
        is accepted.  What a trial is (`_trial_<method>`) is all that differs between them."""
        self.del_w = self.del_c = 0.0
        if self.inertia_correction_method == "inertia_free":   # once per correction: solver.jl:692-693
            self._set_g_ifr(self._ifr.g)
            self._set_aug_rhs_ifr(self._ifr.p0)
        n_trial, inertia, ok = self._first_trial()
        dw_prev, dc_prev = self.del_w, self.del_c
        while not ok:
            if not self._next_perturbation(n_trial, inertia):
                return False
            self._regularize(self.del_w - dw_prev, self.del_c - dc_prev)
            dw_prev, dc_prev = self.del_w, self.del_c
            self.factorize_wrapper()
            n_trial += 1
            inertia, ok = self._trial(n_trial)
        if self.del_w != 0:
            self.del_w_last = self.del_w
        return True

    def _first_trial(self):
        """Factorize and try the unperturbed matrix: (trials made after it, last inertia, accepted).  A back-end that has
        tried perturbations already leaves them in `del_w`, `del_c` (and on the KKT diagonals) and counts them."""
        self.factorize_wrapper()
        return (0,) + self._trial(0)

    def _trial(self, n_trial):
        """One trial on the current factorization: (inertia, accepted); inertia is None for the methods that have none."""
        inertia, correct, ok = getattr(self, "_trial_" + self.inertia_correction_method)()
        if self.on_trial is not None:
            self.on_trial(self, n_trial, inertia, correct, ok)
        return inertia, ok

    def _trial_inertia_based(self):
        """`inertia_correction!(::InertiaBased)` solver.jl:611-670: solve only if the inertia is the right one."""
        inertia = self.kkt.linear_solver.inertia()
        correct = self.kkt.is_inertia_correct(*inertia)
        return inertia, correct, self._solve_newton() if correct else False

    def _trial_inertia_free(self):
        """`inertia_correction!(::InertiaFree)` solver.jl:672-737: a trial is accepted when both solves succeed and the
        curvature test holds for the tangential component of the step."""
        ic = self._ifr
        ok = self._ifr_solves()
        return None, None, curv_test(ic.t, ic.d0.primal(), ic.g, self.kkt, ic.wx, self.opt.inertia_free_tol) and ok

    def _trial_ignore(self):
        """`inertia_correction!(::InertiaIgnore)` solver.jl:739-783: perturb only when the solve fails."""
        return None, None, self._solve_newton()

    def _next_perturbation(self, n_trial, inertia):
        """del_w, del_c of the trial after `n_trial` perturbed ones (the schedule of all three correctors, solver.jl:640-653);
        False: del_w too big, restoration.  Without an inertia (None) del_c is set unconditionally."""
        o = self.opt
        if n_trial == 0:
            self.del_w = (o.first_hessian_perturbation if self.del_w_last == 0 else
                          max(o.min_hessian_perturbation, o.perturb_dec_fact * self.del_w_last))
        else:
            self.del_w *= o.perturb_inc_fact_first if self.del_w_last == 0 else o.perturb_inc_fact
            if self.del_w > o.max_hessian_perturbation:
                self.cnt.k += 1
                return False
        self.del_c = (o.jacobian_regularization_value * self.mu ** o.jacobian_regularization_exponent
                      if inertia is None or self.kkt.should_regularize_dual(*inertia) else 0.0)
        return True

    def _set_g_ifr(self, g):
        """`set_g_ifr!` kernels.jl:242-248."""
        with np.errstate(divide="ignore"):
            g[:] = self.f - self.mu / (self.x - self.xl) + self.mu / (self.xu - self.x) + self.jacl

    def _set_aug_rhs_ifr(self, p0):
        """`set_aug_rhs_ifr!` kernels.jl:233-240."""
        p0.primal()[:] = 0.0
        p0.dual_lb()[:] = 0.0
        p0.dual_ub()[:] = 0.0
        p0.dual()[:] = -self.c

    def _ifr_solves(self):
        """The two solves of one inertia-free trial: the normal step d0 (p0 = (0, -c, 0, 0)) and the search direction; the
        tangential component t = dx - n."""
        ic = self._ifr
        ok = (self.solve_refine_wrapper(ic.d0, ic.p0, self._w3) and
              self.solve_refine_wrapper(self.d, self.p, self._w4))
        ic.t[:] = self._dx() - ic.d0.primal()
        return ok

    # ------------------------------------------------------------------ barrier (barrier.jl:12-34, :95-316)
    def update_barrier(self, sc):
        """`update_barrier!`: the monotone rule alone (barrier.jl:90-92), or the mode switching the two adaptive rules share
        (`update_barrier!(::AbstractAdaptiveUpdate)` :118-149).  In free mode mu comes from the rule; an iterate the filter
        (with a margin) rejects sends the solver to monotone mode at 0.8 times the average complementarity, where it stays,
        decreasing mu by the monotone rule, until an iterate is accepted again."""
        o = self.opt
        if o.barrier == "monotone":
            return self._update_monotone(sc)
        old_mu = self.mu
        progress = self._check_progress()
        if not self.free_mode:
            if progress:
                self.free_mode = True
            else:
                self._update_monotone(sc)
        elif not progress:
            self.free_mode = False
            self.mu = _clamp(0.8 * self._average_complementarity(), o.mu_min, o.barrier_mu_max)   # get_fixed_mu :99-102
        if self.free_mode:
            self.mu = self._loqo_mu() if o.barrier == "loqo" else self._quality_function_mu()
        if self.mu != old_mu:
            self.tau = max(o.tau_min, 1 - self.mu)
            self.filter = [(self.theta_max, -INF)]

    def _update_monotone(self, sc):
        """`_update_monotone!` barrier.jl:12-34."""
        o = self.opt
        inf_compl_mu = self.inf_compl(self.mu, sc)
        while self.mu > max(o.mu_min, o.tol / 10) and \
                max(self.inf_pr, self.inf_du, inf_compl_mu) <= o.barrier_tol_factor * self.mu:
            a = min(99.0 * o.mu_min / o.tol, 0.01)
            mu_new = max(o.mu_min, a * o.tol, min(o.mu_linear_decrease_factor * self.mu,
                                                   self.mu ** o.mu_superlinear_decrease_power))
            inf_compl_mu = self.inf_compl(self.mu, sc)
            self.tau = max(o.tau_min, 1 - self.mu)
            self.mu = mu_new
            self.filter = [(self.theta_max, -INF)]

    def _check_progress(self):
        """`_check_progress` barrier.jl:104-116: the current iterate, pushed out by a margin of 1e-5 min(1, KKT error), must be
        acceptable to the current filter.  Always true without globalization."""
        if not self.opt.barrier_globalization:
            return True
        theta = self._theta(self.c)
        varphi = self.varphi(self.obj_val, self.x)
        delta = 1e-5 * min(1.0, max(self.inf_pr, self.inf_du, self.inf_compl_v))
        return self._filter_ok(theta + delta, varphi + delta)

    def _n_bounded(self):
        return len(self.ind_lb) + len(self.ind_ub)

    def _loqo_mu(self):
        """`get_adaptive_mu(::LOQOUpdate)` barrier.jl:304-316 ([Nocedal2009] eq. 3.6): the centering parameter from the ratio
        xi of the smallest to the average complementarity product."""
        o = self.opt
        if self._n_bounded() == 0:
            return o.mu_min
        mu = self._average_complementarity()
        xi = _fdiv(self._min_complementarity(), mu)
        t = min((1 - o.loqo_r) * _fdiv(1 - xi, xi), 2)
        sigma = o.loqo_gamma * (t * t * t)
        return _clamp(sigma * mu, o.mu_min, o.barrier_mu_max)

    def _quality_function_mu(self):
        """`get_adaptive_mu(::QualityFunctionUpdate)` barrier.jl:260-302 ([Nocedal2009] section 4): mu = sigma times the average
        complementarity, sigma minimizing the quality function along d(sigma) = d_aff + sigma d_cen.  Both directions are
        APPROXIMATE, as in the reference: one plain solve each (no refinement) against the factorization and the KKT-handle
        state the previous iteration left -- the barrier update runs before set_aug_diagonal! (solver.jl:255-262), and nothing
        here builds or factorizes.  One deviation: while nothing has been factorized yet (iteration 0 with dual_initialization
        = "zero") the current mu is kept; the reference would solve against a factor that was never computed."""
        o = self.opt
        if self._n_bounded() == 0:
            return o.mu_min
        if self.cnt.factorization_cnt == 0:
            return self.mu
        step_aff, step_cen = self._w1, self._w4     # free here: the corrections and the refinement use them later
        self._set_affine_rhs()
        rp = self._norm2(self._dual(self.p))        # `res_primal` :270
        rd = self._norm2(self._primal(self.p))      # `res_dual` :271
        self._solve_kkt_plain(step_aff)
        mu = self._average_complementarity()
        self._set_centering_rhs(mu)
        self._solve_kkt_plain(step_cen)
        self.cnt.probe_solve_cnt += 2
        q = lambda sigmas: self._quality_values(sigmas, step_aff, step_cen, rp, rd)  # noqa: E731
        sigma_1m = 1.0 - 1e-4
        phi1, phi1m = q([1.0, sigma_1m])
        if phi1m > phi1:       # :289-296, Ipopt's heuristic: is the minimizer above 1?
            sigma_min = 1.0
            sigma_max = min(o.qf_sigma_max, _fdiv(o.barrier_mu_max, mu))
        else:
            sigma_min = max(o.qf_sigma_min, _fdiv(o.mu_min, mu))
            sigma_max = min(max(sigma_min, sigma_1m), _fdiv(o.barrier_mu_max, mu))
        sigma = golden_section(q, sigma_min, sigma_max, o.qf_max_gs_iter, o.qf_sigma_tol)
        self.cnt.barrier_update_cnt += 1
        return _clamp(sigma * mu, o.mu_min, o.barrier_mu_max)

    def _quality_values(self, sigmas, step_aff, step_cen, rp, rd):
        """`_evaluate_quality_function` barrier.jl:152-201 for a batch of sigmas, restated as written: the call sites
        (:209-230, :286-288) pass (res_primal, res_dual) where the signature reads (res_dual, res_primal), so the DUAL step
        length weighs the primal residual rp = ||p_dual||_2 (over the number of variables and slacks) and the PRIMAL step length
        the dual residual rd = ||p_primal||_2 (over the number of constraints)."""
        ntot, m, nb = self.n + self.ns, self.m, self._n_bounded()
        self.cnt.quality_eval_cnt += len(sigmas)
        out = []
        for a_pr, a_du, s_lb, s_ub in self._quality_terms(sigmas, step_aff, step_cen):
            inf_pr = (1.0 - a_pr) * (1.0 - a_pr) * (rd * rd) / m if m > 0 else 0.0
            inf_du = (1.0 - a_du) * (1.0 - a_du) * (rp * rp) / ntot
            out.append(inf_du + inf_pr + (s_lb + s_ub) / nb)
        return out

    # ------------------------------------------------------------------ filter line search (line_search.jl:6-123)
    def _filter_ok(self, theta, varphi):
        if not (math.isfinite(theta) and math.isfinite(varphi)):
            return False
        return all(theta <= tF or varphi <= vF for tF, vF in self.filter)

    def _ftype(self, theta, theta_trial, varphi, varphi_trial, switching, armijo):
        o = self.opt
        if not self._filter_ok(theta_trial, varphi_trial):
            return " "
        if varphi_trial >= varphi and varphi_trial > varphi and \
                math.log10(varphi_trial - varphi) > o.obj_max_inc + max(1.0, math.log10(abs(varphi)) if varphi != 0 else -INF):
            return " "
        if theta <= self.theta_min and switching:
            return "f" if armijo else " "
        suff = (self.m > 0 and theta_trial <= (1 - o.gamma_theta) * theta + 10 * EPS * abs(theta)) or \
               (varphi_trial <= varphi - o.gamma_phi * theta + 10 * EPS * abs(varphi))
        return "h" if suff else " "

    def _alpha_min(self, theta, varphi_d):
        """`get_alpha_min` kernels.jl:715-741: the step below which the line search gives up."""
        o = self.opt
        if varphi_d < 0:
            if theta <= self.theta_min:
                return o.alpha_min_frac * min(o.gamma_theta, o.gamma_phi * theta / (-varphi_d),
                                              o.delta * _pow(theta, o.s_theta) / _pow(-varphi_d, o.s_phi))
            return o.alpha_min_frac * min(o.gamma_theta, -o.gamma_phi * theta / varphi_d)
        return o.alpha_min_frac * o.gamma_theta

    def filter_line_search(self):
        o = self.opt
        dx = self._dx()
        theta, varphi, varphi_d, alpha_max, self.alpha_z, rel_norm = self._line_search_scalars()
        alpha_min = self._alpha_min(theta, varphi_d)
        self.cnt.l = 1
        self.alpha = alpha_max
        small = rel_norm < 10 * EPS
        switching = varphi_d < 0 and self.alpha * _pow(-varphi_d, o.s_phi) > o.delta * 2.0 ** o.s_theta
        armijo = False
        unsuccessful = False
        theta_trial = varphi_trial = 0.0
        norm_dx = None
        while True:
            self._vaxpby(self.x_trial, self.x, self.alpha, dx)
            self.obj_val_trial = self.eval_f(self.x_trial)
            self.eval_cons(self.c_trial, self.x_trial)
            theta_trial, varphi_trial = self._trial_scalars()
            armijo = varphi_trial <= varphi + o.eta_phi * self.alpha * varphi_d
            if small:
                break
            ftype = self._ftype(theta, theta_trial, varphi, varphi_trial, switching, armijo)
            if ftype in ("f", "h"):
                break
            if self.cnt.l == 1 and theta_trial >= theta:
                if self._second_order_correction(alpha_max, theta, varphi, theta_trial, varphi_d, switching):
                    theta_trial = self._theta(self.c_trial)
                    varphi_trial = self.varphi(self.obj_val_trial, self.x_trial)
                    break
            unsuccessful = True
            self.alpha /= 2
            self.cnt.l += 1
            if self.alpha < alpha_min:
                self.cnt.k += 1
                return "RESTORE"
            if norm_dx is None:   # at most one reduction per line search
                norm_dx = self._norm2(dx)
            if self.alpha * norm_dx < EPS * 10:
                self.cnt.restoration_fail_count += 1
                if self.cnt.restoration_fail_count >= 4:
                    return "SOLVED_TO_ACCEPTABLE_LEVEL" if self.cnt.acceptable_cnt > 0 else "SEARCH_DIRECTION_BECOMES_TOO_SMALL"
                # the reference's "second chance" (line_search.jl:79-96), as in filter_line_search_RR below: the first three
                # times the regular phase starts again from the current iterate with y = 0, z = 1 and an empty filter
                self._vfill(self.y, 0.0)
                self._bound_dual_fill(1.0)
                self.filter = [(self.theta_max, -INF)]
                self.cnt.k += 1
                return "REGULAR"
        if unsuccessful:
            self.cnt.unsuccessful_iterate += 1
            if self.cnt.unsuccessful_iterate >= 4:
                if self.theta_max / 10 > theta_trial:
                    self.theta_max /= 10
                    self.filter = [(self.theta_max, -INF)]
                self.cnt.unsuccessful_iterate = 0
        else:
            self.cnt.unsuccessful_iterate = 0
        if not switching or not armijo:
            self.filter.append(((1 - o.gamma_theta) * theta_trial, varphi_trial - o.gamma_theta * theta_trial))
        return "LINESEARCH_SUCCEEDED"

    def _second_order_correction(self, alpha_max, theta, varphi, theta_trial, varphi_d, switching):
        """solver.jl:547-608: reuses the factorization, solves only."""
        o = self.opt
        w1 = self._w1
        # wy IS dual(_w1) in the reference (solver.jl:552-554): the solve below overwrites it, and the
        # next correction starts from that overwritten vector.  Mirrored on purpose.
        wy = self._dual(w1)
        self._vaxpby(wy, self.c_trial, alpha_max, self.c)
        theta_soc_old = theta_trial
        for _ in range(o.max_soc):
            self.set_aug_rhs(wy)
            self.solve_refine_wrapper(w1, self.p, self._w4)
            wx = self._primal(w1)
            alpha_soc = self.alpha_max(wx)
            self._vaxpby(self.x_trial, self.x, alpha_soc, wx)
            self.eval_cons(self.c_trial, self.x_trial)
            self.obj_val_trial = self.eval_f(self.x_trial)
            theta_soc = self._theta(self.c_trial)
            varphi_soc = self.varphi(self.obj_val_trial, self.x_trial)
            if not self._filter_ok(theta_soc, varphi_soc):
                break
            if theta <= self.theta_min and switching:
                if varphi_soc <= varphi + o.eta_phi * self.alpha * varphi_d:
                    self.alpha = alpha_soc
                    return True
            else:
                suff = (self.m > 0 and theta_soc <= (1 - o.gamma_theta) * theta + 10 * EPS * abs(theta)) or \
                       (varphi_soc <= varphi - o.gamma_phi * theta + 10 * EPS * abs(varphi))
                if suff:
                    self.alpha = alpha_soc
                    return True
            if theta_soc > o.kappa_soc * theta_soc_old:
                break
            theta_soc_old = theta_soc
        return False

    # ------------------------------------------------------------------ back-end primitives (`BACKEND_PRIMITIVES`)
    # The phases above and below are written once against these; `ipm_dev.DeviceMadNLPSolver` overrides every one of them
    # with the `mnk_ipm_*` kernels on device tensors.  Slices of a KKT vector (reference src/KKT/rhs.jl:90-150):
    def _primal(self, v): return v.primal()
    def _dual(self, v): return v.dual()
    def _dual_lb(self, v): return v.dual_lb()
    def _dual_ub(self, v): return v.dual_ub()

    def _dx(self): return self._primal(self.d)
    def _dy(self): return self._dual(self.d)
    def _dzl(self): return self._dual_lb(self.d)
    def _dzu(self): return self._dual_ub(self.d)

    def _new_vec(self, n): return np.zeros(n)

    def _clone(self, v): return v.copy()

    def _vcopy(self, dst, src): dst[:] = src         # copyto!

    def _vaxpy(self, y, a, x): y += a * x            # axpy!

    def _vaxpby(self, dst, x, a, d): dst[:] = x + a * d   # a trial point in one step

    def _vfill(self, v, value): v[:] = value         # fill!

    def _theta(self, c): return float(np.abs(c).sum())

    def _norm_inf(self, v): return float(np.abs(v).max(initial=0.0))

    def _norm2(self, v): return float(np.linalg.norm(v))

    def _regularize(self, dw, dc): self.kkt.regularize_diagonal(dw, dc)

    def _sd_sc(self):
        o, nl, nu = self.opt, len(self.ind_lb), len(self.ind_ub)
        nz = np.abs(self.zl_r).sum() + np.abs(self.zu_r).sum()
        sd = max(o.s_max, (np.abs(self.y).sum() + nz) / max(1, self.m + nl + nu)) / o.s_max
        return sd, max(o.s_max, nz / max(1, nl + nu)) / o.s_max

    def _inf_du(self, sd): return float(np.abs(self.f - self.zl + self.zu + self.jacl).max(initial=0.0) / sd)

    def _iteration_scalars(self):
        """sd, sc, inf_pr, inf_du, inf_compl(mu = 0) at the top of an iteration (solver.jl:224-234)."""
        sd, sc = self._sd_sc()
        return sd, sc, self._norm_inf(self.c), self._inf_du(sd), self.inf_compl(0.0, sc)

    def _jtprod(self): self.kkt.jtprod(self.jacl, self.y)

    def _alpha_z(self, tau):
        """`get_alpha_z` kernels.jl:373-388."""
        az = 1.0
        for z, dz in ((self.zl_r, self._dzl()), (self.zu_r, self._dzu())):
            neg = dz < 0
            if neg.any():
                az = min(az, (-z[neg] * tau / dz[neg]).min())
        return float(az)

    def _bound_dual_axpy(self, a):
        self.zl[self.ind_lb] += a * self._dzl()
        self.zu[self.ind_ub] += a * self._dzu()

    def _bound_dual_fill(self, v):
        self.zl[self.ind_lb] = v
        self.zu[self.ind_ub] = v

    def _adjust_boundary(self):
        """`adjust_boundary!` kernels.jl:656-673."""
        c1, c2 = EPS * self.mu, EPS ** 0.75
        xl_r, x_lr = self.xl_r, self.x_lr
        adj = x_lr - xl_r < c1
        self.xl[self.ind_lb[adj]] = xl_r[adj] - c2 * np.maximum(1, np.abs(x_lr[adj]))
        xu_r, x_ur = self.xu_r, self.x_ur
        adj = xu_r - x_ur < c1
        self.xu[self.ind_ub[adj]] = xu_r[adj] + c2 * np.maximum(1, np.abs(x_ur[adj]))

    def _reset_bound_dual(self, mu):
        """the two `reset_bound_dual!` calls on the full primal-sized vectors (kernels.jl:788-800)."""
        ks = self.opt.kappa_sigma
        with np.errstate(divide="ignore", invalid="ignore"):
            dl = self.x - self.xl
            self.zl[:] = np.where(np.isfinite(dl), np.maximum(np.minimum(self.zl, ks * mu / dl), mu / ks / dl), self.zl)
            du = self.xu - self.x
            self.zu[:] = np.where(np.isfinite(du), np.maximum(np.minimum(self.zu, ks * mu / du), mu / ks / du), self.zu)

    def _get_F(self):
        """`get_F` kernels.jl:572-610; the upper-bound term as the reference writes it, `(xu_r - xu_r) * zu_r - mu`."""
        mu = self.mu
        x_lr, xl_r, zl_r, xu_r, x_ur, zu_r = self.x_lr, self.xl_r, self.zl_r, self.xu_r, self.x_ur, self.zu_r
        F3 = np.where((x_lr >= xl_r) & (zl_r >= 0), np.abs((x_lr - xl_r) * zl_r - mu), INF).sum()
        with np.errstate(invalid="ignore"):
            F4 = np.where((xu_r >= x_ur) & (zu_r >= 0), np.abs((xu_r - xu_r) * zu_r - mu), INF).sum()
        return float(np.abs(self.c).sum() + np.abs(self.f - self.zl + self.zu + self.jacl).sum() + F3 + F4)

    def _set_initial_rhs(self):
        """`set_initial_rhs!` kernels.jl:220-230."""
        self.p.values[:] = 0.0
        self.p.primal()[:] = -self.f + self.zl - self.zu

    def _kkt_initialize(self): self.kkt.initialize()

    def solution(self):
        """The result as the reference reports it: un-scaled, in the model's own sense."""
        return unpack_solution(self, self.x, self.y, self.zl, self.zu)

    def _record(self, phase=""):
        # (the un-scaled objective, as `print_iter` shows it: IPM/utils.jl:162-179)
        self.history.append(IterRecord(self.cnt.k, self.obj_val / self.obj_scale, self.inf_pr, self.inf_du, self.inf_compl_v,
                                       self.mu, self.del_w, self.alpha, self.cnt.l, phase))

    # robust restorer pieces
    def _rr_init_vectors(self, RR, mu_R, rho):
        """vector part of `initialize_robust_restorer!` restoration.jl:46-70."""
        RR.x_ref[:] = self.x
        with np.errstate(divide="ignore"):
            RR.D_R[:] = np.minimum(1.0, 1.0 / np.abs(RR.x_ref))
        t = (mu_R - rho * self.c) / (2 * rho)
        RR.nn[:] = t + np.sqrt(t * t + mu_R * self.c / (2 * rho))      # populate_RR_nn! kernels.jl:825-829
        RR.pp[:] = self.c + RR.nn
        RR.zp[:] = mu_R / RR.pp
        RR.zn[:] = mu_R / RR.nn
        RR.f_R[:] = 0.0
        self.y[:] = 0.0
        self.zl[self.ind_lb] = np.minimum(rho, self.zl_r)
        self.zu[self.ind_ub] = np.minimum(rho, self.zu_r)

    def _rr_obj_val(self, pp, nn, x):
        RR, o = self.RR, self.opt
        return float((o.rho * (pp + nn)).sum() + (RR.zeta / 2 * RR.D_R ** 2 * (x - RR.x_ref) ** 2).sum())

    def _rr_theta(self, c, pp, nn): return float(np.abs(c - pp + nn).sum())

    def _rr_inf_pr(self): return float(np.abs(self.c - self.RR.pp + self.RR.nn).max(initial=0.0))

    def _rr_inf_du(self, sd):
        RR, rho = self.RR, self.opt.rho
        return float(max(np.abs(RR.f_R - self.zl + self.zu + self.jacl).max(initial=0.0),
                         np.abs(rho - self.y - RR.zp).max(initial=0.0), np.abs(rho + self.y - RR.zn).max(initial=0.0)) / sd)

    def _rr_inf_compl(self, mu, sc):
        RR = self.RR
        return float(max(np.abs((self.x_lr - self.xl_r) * self.zl_r - mu).max(initial=0.0),
                         np.abs((self.xu_r - self.x_ur) * self.zu_r - mu).max(initial=0.0),
                         np.abs(RR.pp * RR.zp - mu).max(initial=0.0), np.abs(RR.nn * RR.zn - mu).max(initial=0.0)) / sc)

    def _rr_varphi(self, obj, x, pp, nn):
        mu = self.RR.mu_R
        dl, du = x[self.ind_lb] - self.xl_r, self.xu_r - x[self.ind_ub]
        if (dl < 0).any() or (du < 0).any() or (pp < 0).any() or (nn < 0).any():
            return -INF
        with np.errstate(divide="ignore"):
            return float(obj - mu * (np.log(dl).sum() + np.log(du).sum() + np.log(pp).sum() + np.log(nn).sum()))

    def _rr_varphi_d(self):
        RR, mu, rho, dx = self.RR, self.RR.mu_R, self.opt.rho, self._dx()
        with np.errstate(divide="ignore"):
            return float(((RR.f_R - mu / (self.x - self.xl) + mu / (self.xu - self.x)) * dx).sum()
                         + ((rho - mu / RR.pp) * RR.dpp).sum() + ((rho - mu / RR.nn) * RR.dnn).sum())

    def _rr_alpha_max(self):
        RR, tau = self.RR, self.RR.tau_R
        keep, self.tau = self.tau, tau
        a = self.alpha_max(self._dx())
        self.tau = keep
        for v, dv in ((RR.pp, RR.dpp), (RR.nn, RR.dnn)):
            neg = dv < 0
            if neg.any():
                a = min(a, (-v[neg] * tau / dv[neg]).min())
        return float(a)

    def _rr_alpha_z(self):
        RR, tau = self.RR, self.RR.tau_R
        a = self._alpha_z(tau)
        for z, dz in ((RR.zp, RR.dzp), (RR.zn, RR.dzn)):
            neg = dz < 0
            if neg.any():
                a = min(a, (-z[neg] * tau / dz[neg]).min())
        return float(a)

    def _rr_set_aug(self):
        """`set_aug_RR!` kernels.jl:72-87."""
        k, o, RR = self.kkt, self.opt, self.RR
        k.reg[:] = o.default_primal_regularization + RR.zeta * RR.D_R ** 2
        k.du_diag[:] = -o.default_dual_regularization - RR.pp / RR.zp - RR.nn / RR.zn
        k.l_lower[:] = self.zl_r
        k.u_lower[:] = self.zu_r
        k.l_diag[:] = self.xl_r - self.x_lr
        k.u_diag[:] = self.x_ur - self.xu_r
        k.pr_diag[:] = k.reg
        k.pr_diag[self.ind_lb] -= k.l_lower / k.l_diag
        k.pr_diag[self.ind_ub] -= k.u_lower / k.u_diag

    def _rr_set_rhs(self):
        """`set_aug_rhs_RR!` kernels.jl:133-158."""
        p, RR, mu, rho, y = self.p, self.RR, self.RR.mu_R, self.opt.rho, self.y
        p.primal()[:] = -RR.f_R + self.zl - self.zu - self.jacl
        p.dual()[:] = -self.c + RR.pp - RR.nn + (mu - (rho - y) * RR.pp) / RR.zp - (mu - (rho + y) * RR.nn) / RR.zn
        p.dual_lb()[:] = (self.xl_r - self.x_lr) * self.zl_r + mu
        p.dual_ub()[:] = (self.xu_r - self.x_ur) * self.zu_r - mu

    def _rr_finish(self):
        """`finish_aug_solve_RR!` kernels.jl:251-257."""
        RR, mu, rho, l, dl = self.RR, self.RR.mu_R, self.opt.rho, self.y, self._dy()
        RR.dzp[:] = rho - l - dl - RR.zp
        RR.dzn[:] = rho + l + dl - RR.zn
        RR.dpp[:] = -RR.pp + mu / RR.zp - (RR.pp / RR.zp) * RR.dzp
        RR.dnn[:] = -RR.nn + mu / RR.zn - (RR.nn / RR.zn) * RR.dzn

    def _rr_set_f(self):
        RR = self.RR
        RR.f_R[:] = RR.zeta * RR.D_R ** 2 * (self.x - RR.x_ref)      # set_f_RR! kernels.jl:106-110

    def _rr_reset_slack_duals(self):
        RR, mu, ks = self.RR, self.RR.mu_R, self.opt.kappa_sigma
        for z, v in ((RR.zp, RR.pp), (RR.zn, RR.nn)):                  # reset_bound_dual!(z, x, mu, ks) kernels.jl:775-786
            with np.errstate(divide="ignore"):
                z[:] = np.maximum(np.minimum(z, (ks * mu) / v), (mu / ks) / v)

    def _rel_search_norm(self): return float((np.abs(self._dx()) / (1 + np.abs(self.x))).max(initial=0.0))

    def _line_search_scalars(self):
        """theta, varphi, varphi_d, alpha_max, alpha_z, the relative norm of the step: what `filter_line_search` reads of the
        iterate and the direction before its first trial point (line_search.jl:7-31)."""
        dx = self._dx()
        with np.errstate(divide="ignore"):
            varphi_d = float(((self.f - self.mu / (self.x - self.xl) + self.mu / (self.xu - self.x)) * dx).sum())
        return (self._theta(self.c), self.varphi(self.obj_val, self.x), varphi_d, self.alpha_max(dx),
                self._alpha_z(self.tau), self._rel_search_norm())

    def _trial_scalars(self):
        """theta and varphi of the trial point (`c_trial`, `x_trial`, `obj_val_trial`)."""
        return self._theta(self.c_trial), self.varphi(self.obj_val_trial, self.x_trial)

    # adaptive barrier rules
    def _average_complementarity(self):
        """`get_average_complementarity` kernels.jl:305-320, as the sum of the products (x_lr - xl_r) zl_r and (xu_r - x_ur)
        zu_r over nlb + nub on both back-ends (the device reduction computes exactly this).  The reference's difference of dot
        products, dot(x_lr, zl_r) - dot(xl_r, zl_r), agrees with it to rounding and cancels badly at active bounds.  The two sums
        are taken in the device reduction's order (`ordered_sum`): under the adaptive rules mu is a multiple of this value and
        enters the iterate, so the two back-ends must produce the same bits, not the same value to rounding."""
        nb = len(self.ind_lb) + len(self.ind_ub)
        if nb == 0:
            return 0.0
        return float((ordered_sum((self.x_lr - self.xl_r) * self.zl_r) + ordered_sum((self.xu_r - self.x_ur) * self.zu_r)) / nb)

    def _min_complementarity(self):
        """`get_min_complementarity` kernels.jl:322-339."""
        a = ((self.x_lr - self.xl_r) * self.zl_r).min(initial=INF)
        b = ((self.xu_r - self.x_ur) * self.zu_r).min(initial=INF)
        return float("nan") if a != a or b != b else float(min(a, b))

    def _set_affine_rhs(self):
        """The affine-scaling right-hand side, barrier.jl:268: `set_aug_rhs!` with mu = 0 (no dual-infeasibility perturbation)."""
        p = self.p
        p.primal()[:] = -self.f + self.zl - self.zu - self.jacl
        p.dual()[:] = -self.c
        p.dual_lb()[:] = (self.xl_r - self.x_lr) * self.zl_r + 0.0      # (+ mu, - mu with mu = 0: a -0.0 product becomes 0.0)
        p.dual_ub()[:] = (self.xu_r - self.x_ur) * self.zu_r - 0.0

    def _set_centering_rhs(self, mu):
        """`set_centering_aug_rhs!` barrier.jl:248-258 and the perturbation of :280."""
        p = self.p
        p.primal()[:] = 0.0
        p.dual()[:] = 0.0
        p.dual_lb()[:] = mu
        p.dual_ub()[:] = -mu
        px = p.primal()
        px[self.ind_llb] -= mu * self.opt.kappa_d
        px[self.ind_uub] += mu * self.opt.kappa_d

    def _solve_kkt_plain(self, w):
        """w = K^-1 p by one `solve_kkt!` on the current factorization, without refinement (barrier.jl:273-274, :282-283)."""
        w.values[:] = self.p.values
        self.kkt.solve_kkt(w)

    def _quality_terms(self, sigmas, step_aff, step_cen):
        """Per sigma the four reductions of `_evaluate_quality_function` (barrier.jl:157-189) along d = step_aff + sigma
        step_cen: (alpha_pr, alpha_du, sum over the lower bounds of ((x_lr + alpha_pr dx_lr - xl_r) (zl_r + alpha_du dzl))^2,
        the same over the upper bounds).  The step lengths start from 1 (`get_alpha_max`, `get_alpha_z`); a NaN anywhere in
        the step makes them NaN (the reference's loops skip it: its comparisons are false)."""
        out = []
        tau, lb, ub = self.tau, self.ind_lb, self.ind_ub
        for sigma in sigmas:
            dx = step_aff.primal() + sigma * step_cen.primal()
            dzl = step_aff.dual_lb() + sigma * step_cen.dual_lb()
            dzu = step_aff.dual_ub() + sigma * step_cen.dual_ub()
            a_pr = float("nan") if np.isnan(dx).any() else float(self.alpha_max(dx))
            a_du = 1.0
            for z, dz in ((self.zl_r, dzl), (self.zu_r, dzu)):
                neg = dz < 0
                if neg.any():
                    a_du = min(a_du, (-z[neg] * tau / dz[neg]).min())
            a_du = float("nan") if np.isnan(dzl).any() or np.isnan(dzu).any() else float(a_du)
            t = (self.x_lr + a_pr * dx[lb] - self.xl_r) * (self.zl_r + a_du * dzl)
            u = (self.xu_r - self.x_ur - a_pr * dx[ub]) * (self.zu_r + a_du * dzu)
            out.append((a_pr, a_du, float((t * t).sum()), float((u * u).sum())))
        return out

    # ------------------------------------------------------------------ restore! (solver.jl:300-411)
    def restore(self):
        o = self.opt
        self.del_w = 0.0
        w1x, w1y, w2c = self._clone(self.x), self._clone(self.y), self._clone(self.c)   # the backups in _w1 / _w2
        F = self._get_F()
        self.alpha_z = 0.0
        while True:
            alpha_max = self.alpha_max(self._dx())
            self.alpha = min(alpha_max, self._alpha_z(self.tau))
            self._vaxpy(self.x, self.alpha, self._dx())
            self._vaxpy(self.y, self.alpha, self._dy())
            self._bound_dual_axpy(self.alpha)
            self.eval_cons(self.c, self.x)
            self.eval_grad(self.x)
            self.obj_val = self.eval_f(self.x)
            self.eval_jac(self.x)
            self._jtprod()
            F_trial = self._get_F()
            if F_trial > o.soft_resto_pderror_reduction_factor * F:
                self._vcopy(self.x, w1x)
                self._vcopy(self.y, w1y)
                self._vcopy(self.c, w2c)
                return "ROBUST"
            self._adjust_boundary()
            F = F_trial
            theta = self._theta(self.c)
            varphi = self.varphi(self.obj_val, self.x)
            self.cnt.k += 1
            if self._filter_ok(theta, varphi):
                return "REGULAR"
            self.cnt.t += 1
            if self.cnt.k >= o.max_iter:
                return "MAXIMUM_ITERATIONS_EXCEEDED"
            sd, sc, self.inf_pr, self.inf_du, self.inf_compl_v = self._iteration_scalars()
            self._record("r")
            self.eval_lag_hess(self.x, self.y)
            self.set_aug_diagonal()
            self.set_aug_rhs(self.c)
            self.factorize_wrapper()
            self._solve_newton()

    def _solve_newton(self):
        return self.solve_refine_wrapper(self.d, self.p, self._w4)

    # ------------------------------------------------------------------ robust! (solver.jl:413-545)
    def _initialize_robust_restorer(self):
        """`initialize_robust_restorer!` restoration.jl:39-76."""
        o = self.opt
        if getattr(self, "RR", None) is None:
            RR = RobustRestorer()
            nt, m = len(self.x), self.m
            for name, n in (("f_R", nt), ("x_ref", nt), ("D_R", nt)) + tuple((v, m) for v in (
                    "pp", "nn", "zp", "zn", "dpp", "dnn", "dzp", "dzn", "pp_trial", "nn_trial")):
                setattr(RR, name, self._new_vec(n))
            self.RR = RR
        RR = self.RR
        RR.theta_ref = self._theta(self.c)
        RR.mu_R = max(self.mu, self._norm_inf(self.c))
        RR.tau_R = max(o.tau_min, 1 - RR.mu_R)
        RR.zeta = math.sqrt(RR.mu_R)
        self._rr_init_vectors(RR, RR.mu_R, o.rho)
        RR.obj_val_R = self._rr_obj_val(RR.pp, RR.nn, self.x)
        RR.filter = [(self.theta_max, -INF)]
        self.cnt.t = 0
        self.del_w = 0.0

    def _update_monotone_RR(self, sc):
        """`_update_monotone_RR!` barrier.jl:39-84."""
        o, RR = self.opt, self.RR
        inf_compl_mu_R = self._rr_inf_compl(RR.mu_R, sc)
        while RR.mu_R >= o.mu_min and max(RR.inf_pr_R, RR.inf_du_R, inf_compl_mu_R) <= o.barrier_tol_factor * RR.mu_R:
            a = min(99.0 * o.mu_min / o.tol, 0.01)
            RR.mu_R = max(o.mu_min, a * o.tol, min(o.mu_linear_decrease_factor * RR.mu_R,
                                                   RR.mu_R ** o.mu_superlinear_decrease_power))
            inf_compl_mu_R = self._rr_inf_compl(RR.mu_R, sc)
            RR.tau_R = max(o.tau_min, 1 - RR.mu_R)
            RR.zeta = math.sqrt(RR.mu_R)
            RR.filter = [(self.theta_max, -INF)]

    def robust(self):
        o = self.opt
        self._initialize_robust_restorer()
        RR = self.RR
        while True:
            self.eval_jac(self.x)
            self._jtprod()
            sd, sc, self.inf_pr, self.inf_du, self.inf_compl_v = self._iteration_scalars()
            RR.inf_pr_R = self._rr_inf_pr()
            RR.inf_du_R = self._rr_inf_du(sd)
            RR.inf_compl_R = self._rr_inf_compl(0.0, sc)
            self._record("R")
            if max(RR.inf_pr_R, RR.inf_du_R, RR.inf_compl_R) <= o.tol:
                return "INFEASIBLE_PROBLEM_DETECTED"
            if self.cnt.k >= o.max_iter:
                return "MAXIMUM_ITERATIONS_EXCEEDED"
            self._update_monotone_RR(sc)
            self.eval_lag_hess(self.x, self.y, is_resto=True)
            self._rr_set_aug()
            self._rr_set_rhs()
            if not self.inertia_correction():
                return "RESTORATION_FAILED"
            self._rr_finish()
            st = self.filter_line_search_RR()
            if st != "LINESEARCH_SUCCEEDED":
                return st
            self._vcopy(self.x, self.x_trial)
            self._vcopy(self.c, self.c_trial)
            self._vcopy(RR.pp, RR.pp_trial)
            self._vcopy(RR.nn, RR.nn_trial)
            RR.obj_val_R = RR.obj_val_R_trial
            self._rr_set_f()
            self._vaxpy(self.y, self.alpha, self._dy())
            self._vaxpy(RR.zp, self.alpha_z, RR.dzp)
            self._vaxpy(RR.zn, self.alpha_z, RR.dzn)
            self._bound_dual_axpy(self.alpha_z)
            self._reset_bound_dual(RR.mu_R)
            self._rr_reset_slack_duals()
            self._adjust_boundary()
            self.obj_val = self.eval_f(self.x)
            self.eval_grad(self.x)
            theta = self._theta(self.c)
            varphi = self.varphi(self.obj_val, self.x)
            if self._filter_ok(theta, varphi) and theta <= o.required_infeasibility_reduction * RR.theta_ref:
                self._set_initial_rhs()
                self._kkt_initialize()
                self.factorize_wrapper()
                self._solve_newton()
                if self._norm_inf(self._dy()) > o.constr_mult_init_max:
                    self._vfill(self.y, 0.0)
                else:
                    self._vcopy(self.y, self._dy())
                self.cnt.k += 1
                self.cnt.t += 1
                return "REGULAR"
            if self.cnt.k >= o.max_iter:
                return "MAXIMUM_ITERATIONS_EXCEEDED"
            self.cnt.k += 1
            self.cnt.t += 1

    def _ftype_RR(self, theta, theta_trial, varphi, varphi_trial, switching, armijo):
        keep, self.filter = self.filter, self.RR.filter
        try:
            return self._ftype(theta, theta_trial, varphi, varphi_trial, switching, armijo)
        finally:
            self.filter = keep

    def filter_line_search_RR(self):
        """`filter_line_search_RR!` line_search.jl:128-222."""
        o, RR = self.opt, self.RR
        theta_R = self._rr_theta(self.c, RR.pp, RR.nn)
        varphi_R = self._rr_varphi(RR.obj_val_R, self.x, RR.pp, RR.nn)
        varphi_d_R = self._rr_varphi_d()
        alpha_max = self._rr_alpha_max()
        self.alpha_z = self._rr_alpha_z()
        alpha_min = self._alpha_min(theta_R, varphi_d_R)
        self.alpha = alpha_max
        self.cnt.l = 1
        small = self._rel_search_norm() < 10 * EPS
        switching = varphi_d_R < 0 and self.alpha * _pow(-varphi_d_R, o.s_phi) > o.delta * _pow(theta_R, o.s_theta)
        armijo = False
        while True:
            self._vcopy(self.x_trial, self.x)
            self._vaxpy(self.x_trial, self.alpha, self._dx())
            self._vcopy(RR.pp_trial, RR.pp)
            self._vaxpy(RR.pp_trial, self.alpha, RR.dpp)
            self._vcopy(RR.nn_trial, RR.nn)
            self._vaxpy(RR.nn_trial, self.alpha, RR.dnn)
            RR.obj_val_R_trial = self._rr_obj_val(RR.pp_trial, RR.nn_trial, self.x_trial)
            self.eval_cons(self.c_trial, self.x_trial)
            theta_R_trial = self._rr_theta(self.c_trial, RR.pp_trial, RR.nn_trial)
            varphi_R_trial = self._rr_varphi(RR.obj_val_R_trial, self.x_trial, RR.pp_trial, RR.nn_trial)
            armijo = varphi_R_trial <= varphi_R + o.eta_phi * self.alpha * varphi_d_R
            if small:
                break
            if self._ftype_RR(theta_R, theta_R_trial, varphi_R, varphi_R_trial, switching, armijo) in ("f", "h"):
                break
            self.alpha /= 2
            self.cnt.l += 1
            if self.alpha < alpha_min:
                self.cnt.restoration_fail_count += 1
                if self.cnt.restoration_fail_count >= 4:
                    return "RESTORATION_FAILED"
                # the reference's "second chance": back to the regular phase from the current iterate
                self._vfill(self.y, 0.0)
                self._bound_dual_fill(1.0)
                self.filter = [(self.theta_max, -INF)]
                self.cnt.k += 1
                self.cnt.t += 1
                return "REGULAR"
            if self.alpha < EPS * 10:
                return "SOLVED_TO_ACCEPTABLE_LEVEL" if self.cnt.acceptable_cnt > 0 else "SEARCH_DIRECTION_BECOMES_TOO_SMALL"
        if not switching or not armijo:
            RR.filter.append(((1 - o.gamma_theta) * theta_R_trial, varphi_R_trial - o.gamma_theta * theta_R_trial))
        return "LINESEARCH_SUCCEEDED"

    # ------------------------------------------------------------------ solve! (solver.jl:119-166)
    def solve(self):
        if self.status == "INITIAL":
            self.initialize()
        while self.status in ("REGULAR", "RESTORE", "ROBUST"):
            if self.status == "REGULAR":
                self.status = self.regular()
            if self.status == "RESTORE":
                self.status = self.restore()
            if self.status == "ROBUST":
                self.status = self.robust()
        return self.status

    # ------------------------------------------------------------------ regular! (solver.jl:216-298)
    def regular(self):
        o = self.opt
        while True:
            if self.cnt.k != 0:
                self.eval_jac(self.x)
            self._jtprod()
            sd, sc, self.inf_pr, self.inf_du, self.inf_compl_v = self._iteration_scalars()
            self._record()
            inf_total = max(self.inf_pr, self.inf_du, self.inf_compl_v)
            if inf_total <= o.tol:
                return "SOLVE_SUCCEEDED"
            if inf_total <= o.acceptable_tol:
                if self.cnt.acceptable_cnt < o.acceptable_iter:
                    self.cnt.acceptable_cnt += 1
                else:
                    return "SOLVED_TO_ACCEPTABLE_LEVEL"
            else:
                self.cnt.acceptable_cnt = 0
            if inf_total >= o.diverging_iterates_tol:
                return "DIVERGING_ITERATES"
            if self.cnt.k >= o.max_iter:
                return "MAXIMUM_ITERATIONS_EXCEEDED"
            if self.cnt.k != 0:
                self.eval_lag_hess(self.x, self.y)
            self.update_barrier(sc)
            self.set_aug_diagonal()
            self.set_aug_rhs(self.c)
            if not self.inertia_correction():
                return "ROBUST"
            st = self.filter_line_search()
            if st != "LINESEARCH_SUCCEEDED":
                return st
            self._vcopy(self.x, self.x_trial)
            self._vcopy(self.c, self.c_trial)
            self.obj_val = self.obj_val_trial
            self._adjust_boundary()
            self._vaxpy(self.y, self.alpha, self._dy())
            self._bound_dual_axpy(self.alpha_z)
            self._reset_bound_dual(self.mu)
            self.eval_grad(self.x)
            self.cnt.k += 1

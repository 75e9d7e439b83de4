/*
 * madnlp_hip.h -- C ABI of libmadnlp_hip.so: the MI355X (gfx950) implementation of
 * MadNLP's per-iteration KKT hot path.
 *
 * This is the drop-in boundary: every entry point below replaces a function (or a
 * group of functions) of MadNLP.jl v0.10.1; the reference file:line each one stands
 * in for is cited next to it.  A Julia maintainer binds these with `ccall`
 * exactly as `src/LinearSolvers/lapack.jl:50-139` binds LAPACK and
 * `src/LinearSolvers/mumps.jl:148-165` binds MUMPS.
 *
 * Conventions
 *   - plain C types only: int32/int64/double pointers and sizes, opaque handles.
 *   - return value: 0 = OK; < 0 = bad argument / HIP runtime error (text via
 *     mnk_last_error_string(); the Julia glue throws SymbolicException /
 *     FactorizationException / SolveException, reference
 *     `src/LinearSolvers/linearsolvers.jl:133-137`).  A *numerically* failed
 *     factorization is NOT an error: it is reported through `info` / the
 *     inertia, as `src/LinearSolvers/lapack_common.jl:96-102` does, so that the
 *     IPM regularizes and refactorizes.
 *   - `loc` arguments say where a caller buffer lives: MNK_HOST (pageable or
 *     pinned host memory, copied over PCIe on the context's stream) or
 *     MNK_DEVICE (HBM of the context's device; no copy).
 *   - index arrays passed in use `index_base` 0 or 1 (Julia passes 1); arrays
 *     handed back are 0-based unless stated.
 *   - all matrices are column-major Float64, symmetric matrices use the lower
 *     triangle ('L'), as everywhere in the reference.
 *   - all work is enqueued on the context's stream; entry points that return
 *     scalars to the host (info, inertia, host-destination copies) synchronize
 *     that stream, everything else is asynchronous.
 *   - one context / KKT system / solver per MadNLPSolver, driven from one
 *     thread; distinct handles may be used concurrently from distinct threads.
 */
#ifndef MADNLP_HIP_H
#define MADNLP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNK_VERSION 100 /* 0.1.0 */

enum { MNK_HOST = 0, MNK_DEVICE = 1 };

/* Same order as the reference's `@enum LinearFactorization`
 * (`src/LinearSolvers/linearsolvers.jl:139-147`): BUNCHKAUFMAN LU QR CHOLESKY LDL EVD.
 * Implemented on device: CHOLESKY (dpotrf semantics), LDL (static-pivot
 * LDL^T, inertia from sign(D); stands in for BUNCHKAUFMAN = dsytrf), QR
 * (blocked Householder QR of the full symmetric matrix, dgeqrf conventions; no inertia), LU
 * (blocked LU with partial pivoting of the full symmetric matrix, dgetrf conventions; no inertia) and EVD
 * (two-sided block Jacobi eigendecomposition, dsyevd('V', 'L') semantics; inertia from the signs of the eigenvalues). */
enum { MNK_BUNCHKAUFMAN = 1, MNK_LU = 2, MNK_QR = 3, MNK_CHOLESKY = 4, MNK_LDL = 5, MNK_EVD = 6 };

typedef struct mnk_ctx mnk_ctx; /* device, stream(s), scratch */
typedef struct mnk_sc mnk_sc;   /* SparseCondensedKKTSystem device state */
typedef struct mnk_dc mnk_dc;   /* DenseCondensedKKTSystem / DenseKKTSystem device state */
typedef struct mnk_ls mnk_ls;   /* AbstractLinearSolver device state */

/* ---------------------------------------------------------------- context -- */
int mnk_version(void);
const char* mnk_last_error_string(void);
/* `stream`: an existing hipStream_t to enqueue on (e.g. the caller's current
 * stream), or NULL to let the context create its own. */
int mnk_ctx_create(int device, void* stream, mnk_ctx** out);
int mnk_ctx_destroy(mnk_ctx* ctx);
int mnk_ctx_synchronize(mnk_ctx* ctx);
void* mnk_ctx_stream(mnk_ctx* ctx);

/* ------------------------------------------- SparseCondensedKKTSystem (sc) -- */
/* Replaces the constructor `create_kkt_system(::Type{SparseCondensedKKTSystem}, ...)`
 * reference `src/KKT/Sparse/condensed.jl:55-133`:
 *   force_lower_triangular! (`src/matrixtools.jl:129-137`), coo_to_csc + get_mapping
 *   for J^T and tril(H) (`src/matrixtools.jl:55-95`) and the one-time symbolic
 *   analysis build_condensed_aug_symbolic (`condensed.jl:201-301`), all on the host
 *   in C++ (integer work), then uploads the maps.
 * jac_I/jac_J: COO pattern of the Jacobian (row = constraint, col = variable),
 * hess_I/hess_J: COO pattern of the Lagrangian Hessian (either triangle).
 * All m constraints are inequalities (the reference errors otherwise, `:68-70`).
 * ctx may be NULL: the handle is then host-only (symbolic analysis and the structure
 * getters work, nothing is allocated on a device) -- used by CPU-side tests. */
int mnk_sc_create(mnk_ctx* ctx, int64_t n, int64_t m,
                  int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J,
                  int64_t nnzh, const int32_t* hess_I, const int32_t* hess_J,
                  int index_base, mnk_sc** out);
int mnk_sc_destroy(mnk_sc* sc);

/* Sizes of the derived structures: nnz(jt_csc), nnz(hess_com), nnz(aug_com), length(jptr). */
int mnk_sc_sizes(mnk_sc* sc, int64_t* nnz_jt, int64_t* nnz_hess, int64_t* nnz_aug, int64_t* len_jptr);
/* Derived CSC structures (0-based), so the host mirror can build `jt_csc`,
 * `hess_com`, `aug_com` (`condensed.jl:110-119`). which: 0 = jt_csc (n x m),
 * 1 = hess_com (n x n lower), 2 = aug_com (n x n lower). colptr has ncol+1 entries. */
enum { MNK_SC_JT = 0, MNK_SC_HESS = 1, MNK_SC_AUG = 2, MNK_SC_DIAGBUF = 3 };
int mnk_sc_get_structure(mnk_sc* sc, int which, int32_t* colptr, int32_t* rowval);
/* COO -> CSC slot maps `jt_csc_map` / `hess_csc_map` (0-based; which = MNK_SC_JT / MNK_SC_HESS). */
int mnk_sc_get_map(mnk_sc* sc, int which, int64_t* map);
/* dptr/hptr/jptr of `build_condensed_aug_symbolic` (0-based), in the reference's order:
 * dptr: dst[n], src[n]; hptr: dst[nnzH], src[nnzH]; jptr: dst[L], c[L], k[L], l[L].
 * Any output pointer may be NULL. */
int mnk_sc_get_ptrs(mnk_sc* sc, int32_t* d_dst, int32_t* d_src, int32_t* h_dst, int32_t* h_src,
                    int32_t* j_dst, int32_t* j_c, int32_t* j_k, int32_t* j_l);

/* compress_jacobian!(::SparseCondensedKKTSystem) `condensed.jl:145-148` = transfer!
 * (`src/matrixtools.jl:79-88`) of the nnzj COO values into jt_csc.nzval. */
int mnk_sc_compress_jacobian(mnk_sc* sc, const double* jac_coo, int loc);
/* compress_hessian!(::AbstractSparseKKTSystem) `src/KKT/Sparse/utils.jl:48-50`. */
int mnk_sc_compress_hessian(mnk_sc* sc, const double* hess_coo, int loc);
/* build_kkt!(::SparseCondensedKKTSystem) `condensed.jl:354-366` +
 * _build_condensed_aug_coord! `:328-345`.  pr_diag has n+m entries, du_diag m. */
int mnk_sc_build(mnk_sc* sc, const double* pr_diag, const double* du_diag, int loc);
/* Read back nzval of jt_csc / hess_com / aug_com, or diag_buffer (which = MNK_SC_*). */
int mnk_sc_get_values(mnk_sc* sc, int which, double* out, int loc);

/* Device-side pieces of solve_kkt!/mul! for the sparse condensed system (reference
 * `src/IPM/factorization.jl:143-167,278-299`): y = alpha*op(A)*x + beta*y with
 * A = jt_csc (which = MNK_SC_JT; trans = 0: n<-m, trans = 1: m<-n) or
 * Symmetric(hess_com, :L) (which = MNK_SC_HESS).  x, y in device memory. */
int mnk_sc_spmv(mnk_sc* sc, int which, int trans, double alpha, const double* x, double beta, double* y);

/* Compact L-BFGS Hessians, hessian_approximation = CompactLBFGS, on the sparse condensed system (csrc/lbfgs.hip; reference
 * `src/quasi_newton.jl:210-437`, `src/IPM/factorization.jl:76-140,253-276`).  B = sigma I - U U' + V V': the handle's Hessian
 * has the DIAGONAL pattern and holds sigma; S, Y, U, V, E = [U V] and H = C^-1 E stay in the mnk_lbfgs handle on the device.
 *
 * mnk_lbfgs_create replaces `create_quasi_newton(CompactLBFGS, ...)` with the fields of `QuasiNewtonOptions`; max_history is
 * 1 .. 32 (a larger value is an error).  mnk_lbfgs_init is `init!`: *xi = 2 rho0 init_value (rho0 as mnk_dc_qn_init, g0'g0 an
 * ordered sum on the device).  mnk_lbfgs_update is `update!` with device vectors s, y: every dot product in one launch pair,
 * ONE synchronization, the p x p algebra on the host, one launch that stores the pair and writes U and V.  *performed: 0 if
 * the pair was skipped (|s| or |y| < 100 eps, or s'y < sqrt(eps) |s| |y|; the second skip since the last reset empties the
 * memory); *sigma: the value the diagonal Hessian holds from now on.
 *
 * mnk_lbfgs_status (synchronizes): out[0 .. 8) = current_mem, updates, skipped, resets, builds of H / T, singular-T events,
 * version (performed + resetting updates), max_history.  mnk_lbfgs_get copies S, Y, U, V (n x current_mem, oldest pair first),
 * L, D (current_mem), T or W = T^-1 (2 current_mem square; after a solve_kkt) to the host, column-major with leading dimension ld.
 * mnk_lbfgs_gram: out (host, qa x qb) = A'B; mnk_lbfgs_apply: y += alpha A (M (B'x)); device operands with n rows, q <= 64: the
 * reduction and rank-q kernels on their own, every sum in the order of mnk_ipm_get_sum.
 *
 * mnk_sc_attach_lbfgs (qn = NULL detaches): mnk_sc_solve_kkt and mnk_sc_mul then include the low-rank term.  The first
 * solve_kkt after a factorization of the solver it is given, or after a performed / resetting update, computes H = C^-1 E
 * (one mnk_ls_solve with 2 current_mem columns), T = P + E'H and W = T^-1 on the device; every solve_kkt then applies
 * w_x -= H (W (E'w_x)) to the condensed solution with two launches and no host round trip.  A zero pivot of T raises a flag:
 * the correction is not applied, a solve_kkt on host vectors returns an error, one on device vectors reports it at the next
 * call; mnk_lbfgs_status counts it.  mnk_sc_step_batch and mnk_ls_solve_batch refuse such a system.
 * mnk_sc_keep_jacobian snapshots the compressed J' values; mnk_sc_spmv reads the snapshot with which = MNK_SC_JT_KEPT.
 * mnk_sc_qn_secant is mnk_dc_qn_secant for this handle. */
/* The handle is an opaque mnk_lbfgs*; like mnk_tape* below, the prototypes spell it void* (mnk_lbfgs_create: void* out =
 * mnk_lbfgs**) because the static header check of tests/test_julia_glue.py knows the handle types by a fixed list of names. */
typedef struct mnk_lbfgs mnk_lbfgs;
enum { MNK_SC_JT_KEPT = 4 };
enum { MNK_LBFGS_SCALAR1 = 1, MNK_LBFGS_SCALAR2 = 2, MNK_LBFGS_SCALAR3 = 3, MNK_LBFGS_SCALAR4 = 4 };
enum { MNK_LBFGS_S = 0, MNK_LBFGS_Y = 1, MNK_LBFGS_U = 2, MNK_LBFGS_V = 3, MNK_LBFGS_L = 4, MNK_LBFGS_D = 5, MNK_LBFGS_T = 6,
       MNK_LBFGS_W = 7 };
int mnk_lbfgs_create(mnk_ctx* ctx, int64_t n, int max_history, int init_strategy, double init_value, double sigma_min,
                     double sigma_max, void* out);
int mnk_lbfgs_destroy(void* qn);
int mnk_lbfgs_init(void* qn, const double* g0, double f0, double* xi);
int mnk_lbfgs_update(void* qn, const double* s, const double* y, int* performed, double* sigma);
int mnk_lbfgs_status(void* qn, int64_t* out);
int mnk_lbfgs_get(void* qn, int which, double* out, int64_t ld);
int mnk_lbfgs_gram(void* qn, const double* A, int64_t lda, int qa, const double* B, int64_t ldb, int qb, int64_t n,
                   double* out);
int mnk_lbfgs_apply(void* qn, double* y, double alpha, const double* A, int64_t lda, const double* M, const double* B,
                    int64_t ldb, const double* x, int q, int64_t n);
int mnk_sc_attach_lbfgs(mnk_sc* sc, void* qn);
int mnk_sc_keep_jacobian(mnk_sc* sc);
int mnk_sc_qn_secant(mnk_sc* sc, const double* x, const double* g, const double* jl, const double* jv, double* last_x,
                     double* last_g, double* s, double* y);

/* ------------------- DenseCondensedKKTSystem / DenseKKTSystem (dc) ---------- */
/* Replaces `create_kkt_system(::Type{DenseCondensedKKTSystem}, ...)`
 * `src/KKT/Dense/condensed.jl:52-111` (condensed = 1, order n + n_eq) and
 * `create_kkt_system(::Type{DenseKKTSystem}, ...)` `src/KKT/Dense/augmented.jl:41-94`
 * (condensed = 0, order n + ns + m).  ind_ineq has ns entries, ind_eq m - ns. */
int mnk_dc_create(mnk_ctx* ctx, int condensed, int64_t n, int64_t m,
                  int64_t ns, const int64_t* ind_ineq, const int64_t* ind_eq,
                  int index_base, mnk_dc** out);
int mnk_dc_destroy(mnk_dc* dc);
/* The callbacks write kkt.hess (n x n) / kkt.jac (m x n) in place in the reference
 * (`get_hessian/get_jacobian`); here they are uploaded (or copied device to device). */
int mnk_dc_set_hess(mnk_dc* dc, const double* hess, int64_t ld, int loc);
int mnk_dc_set_jac(mnk_dc* dc, const double* jac, int64_t ld, int loc);
/* build_kkt!(::DenseCondensedKKTSystem) `condensed.jl:157-186` (_build_ineq_jac!,
 * the J_i' D J_i product, _build_condensed_kkt_system!) or, for condensed = 0,
 * compress_hessian! + build_kkt!(::DenseKKTSystem) `augmented.jl:116-161`.
 * pr_diag has n+ns entries, du_diag m.  Both triangles of aug_com are written. */
int mnk_dc_build(mnk_dc* dc, const double* pr_diag, const double* du_diag, int loc);
int64_t mnk_dc_order(mnk_dc* dc);
/* Copy aug_com (order x order, column-major, ld = order) out. */
int mnk_dc_get_aug(mnk_dc* dc, double* out, int loc);

/* Dense quasi-Newton Hessians, hessian_approximation = BFGS / DampedBFGS on the dense KKT systems (csrc/qn.hip).  The
 * approximation IS the handle's Hessian buffer (kkt.hess, n x n, column-major), which mnk_dc_build reads: it is updated
 * in place on the device and never uploaded.  mnk_dc_set_hess overwrites it.
 *
 * mnk_dc_qn_init replaces `create_quasi_newton` `src/quasi_newton.jl:94-110,144-161` (workspace: allocated here, once per
 * handle) and `init!` `:194-206`: hess = 2 rho0 I with rho0 = 1 if g0'g0 < sqrt(eps), 1 / g0'g0 if f0 == 0, else
 * |f0| / g0'g0 (g0: n entries on the device).  With g0 = NULL the matrix the handle holds is adopted as it is (it counts
 * as instantiated: no diagonal reset in front of the next update).  Asynchronous on the context's stream.
 *
 * mnk_dc_qn_update replaces `update!(::BFGS)` `:112-130` / `update!(::DampedBFGS)` `:163-192` (s, y: n entries on the
 * device): BFGS skips the update when s'y < 1e-8, DampedBFGS never does; the first performed update first overwrites the
 * diagonal with s'y / s's.  Asynchronous on the context's stream: the dot products, the skip test, theta and the
 * reciprocals stay on the device, nothing is allocated, nothing is copied to the host.  Like the reference's dsymv / dsyr
 * with 'L' it reads and writes the LOWER triangle of hess only; the strict upper triangle keeps what it held.  Every
 * consumer of hess reads the lower triangle (the factorizations through the lower triangle of aug_com, mnk_dc_mul, the
 * QR / LU solvers after tril_to_full!); the non-condensed mnk_dc_build copies both triangles of hess into aug_com, so
 * after an update only the lower triangle of that aug_com is meaningful.
 *
 * mnk_dc_qn_status is the one call that synchronizes: updates performed / skipped since mnk_dc_qn_init, and
 * last = [s'y, s'Bs, theta, r's] of the last update (r = y and theta = 1 for BFGS; s'Bs = 0 after a skipped one).
 * mnk_dc_get_hess copies kkt.hess (n x n, column-major, leading dimension ld) out. */
enum { MNK_QN_BFGS = 1, MNK_QN_DAMPED_BFGS = 2 };
int mnk_dc_qn_init(mnk_dc* dc, int kind, const double* g0, double f0);
int mnk_dc_qn_update(mnk_dc* dc, const double* s, const double* y);
int mnk_dc_qn_status(mnk_dc* dc, int64_t* updates, int64_t* skipped, double* last);
/* The secant pair of the quasi-Newton method of `eval_lag_hess_wrapper!` (`src/IPM/callbacks.jl:162-174,184-186`) from device
 * vectors of n entries, in one launch: s = x - last_x, y = ((g - last_g) + jl) - jv with jl = J(x)' l, jv = J(last_x)' l
 * (both NULL without constraints), then the backups last_x = x, last_g = g.  Asynchronous on the context's stream. */
int mnk_dc_qn_secant(mnk_dc* dc, const double* x, const double* g, const double* jl, const double* jv, double* last_x,
                     double* last_g, double* s, double* y);
int mnk_dc_get_hess(mnk_dc* dc, double* out, int64_t ld, int loc);

/* COO callbacks into the dense systems: the reference's SparseCallback on a dense KKT system (`src/Callbacks/nlpmodels.jl:829-842`,
 * `:863-881`) zeroes the dense Jacobian / Hessian and adds the values of jac_coord! / hess_coord! entry by entry in COO order,
 * the Hessian entry (i, j) also to (j, i).  csrc/dense_coo.hip.
 *
 * mnk_dc_coo_attach (once per handle, host work and uploads only) validates the indices (`base` 0 or 1; a Hessian entry may
 * lie in either triangle: its destination is the unordered pair {i, j}) and builds, per matrix, the distinct destinations
 * sorted column-major with an int32 CSR of the COO positions feeding each, ascending, plus one CSR by Jacobian column.  It
 * fails with a message on an index out of range, a second attach, or a count that does not fit int32.  Every entry below
 * fails before it if called before the attach, and launches nothing when it fails.
 *
 * mnk_dc_compress_jacobian / mnk_dc_compress_hessian (values on the host or the device, `loc`): one launch, one thread per
 * destination, no atomics, no contraction: acc = 0.0; acc += v[k] over the destination's positions in COO order; the sum is
 * stored to kkt.jac (column-major, ld = m), resp. to both (i, j) and (j, i) of kkt.hess (ld = n): bit for bit the reference's
 * sequential loop.  Entries outside the structure read as zero: the buffers are zeroed at creation, and the handle remembers
 * whether mnk_dc_set_jac / mnk_dc_set_hess or mnk_dc_qn_init / mnk_dc_qn_update has written one since; only then the scatter
 * is preceded by a clear of the buffer.  nnz = 0 launches nothing.  The Jacobian values given (scaled by the caller, if at all)
 * stay in the handle; mnk_dc_keep_jacobian snapshots them (the twin of mnk_sc_keep_jacobian).
 *
 * mnk_dc_coo_jtprod: out[j] = sum over the COO entries of column j, in COO order, of v[k] * y[jac_I[k]], from 0.0 (n entries;
 * a column nothing feeds gives 0), on the current (MNK_DC_JAC_CURRENT) or the kept (MNK_DC_JAC_KEPT) values; y, out on the device.
 * mnk_dc_get_jac copies kkt.jac (m x n, column-major, leading dimension ld) out.  All asynchronous on the context's stream except
 * for host-resident arguments. */
enum { MNK_DC_JAC_CURRENT = 0, MNK_DC_JAC_KEPT = 1 };
int mnk_dc_coo_attach(mnk_dc* dc, int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t nnzh, const int32_t* hess_I,
                      const int32_t* hess_J, int base);
int mnk_dc_compress_jacobian(mnk_dc* dc, const double* jac_coo, int loc);
int mnk_dc_compress_hessian(mnk_dc* dc, const double* hess_coo, int loc);
int mnk_dc_keep_jacobian(mnk_dc* dc);
int mnk_dc_coo_jtprod(mnk_dc* dc, int which, const double* y, double* out);
int mnk_dc_get_jac(mnk_dc* dc, double* out, int64_t ld, int loc);

/* ------------------------------------------------- linear solver (ls) ------- */
/* Replaces `LapackCPUSolver(A; opt)` `src/LinearSolvers/lapack.jl:21-43` /
 * `LapackROCmSolver` `lib/MadNLPGPU/ext/MadNLPGPUAMDGPUExt/rocsolver.jl`:
 * allocates the private N x N factor buffer.  algo = MNK_CHOLESKY, MNK_LDL or MNK_QR
 * (MNK_BUNCHKAUFMAN is accepted as an alias of MNK_LDL).  MNK_QR (solve_qr!, reference `lapack.jl:187-209`):
 * factorize! mirrors the transferred lower triangle to the full matrix (tril_to_full!) and runs a blocked
 * Householder QR (dgeqrf conventions, 64-column compact-WY panels); info is always 0 and a singular matrix
 * shows up in the solve; mnk_ls_inertia returns an error (no inertia); it is never merged into a factorization
 * batch nor queued in a solve batch (it runs when called); the options that steer the LDL^T / Cholesky schedules
 * are accepted and ignored.  MNK_LU (solve_lu!, reference `lapack.jl:174-187`): factorize! mirrors the transferred
 * lower triangle to the full matrix and factors P A = L U with partial pivoting (dgetrf conventions: idamax's pivot,
 * the smallest row on a tie; 64-column panels); info is dgetrf's (1-based index of the first exactly zero pivot, 0 if
 * none; the elimination goes on past it and factorize! does not fail on it); solve! is dgetrs('N'); mnk_ls_inertia
 * returns an error; batches and ignored options as for MNK_QR.  MNK_EVD (solve_evd!, reference `lapack.jl:211-234`):
 * factorize! computes A = Q diag(lambda) Q^T of the lower triangle (lambda ascending); info is 0, or 1 when the sweep cap
 * was reached (non-finite input); factorize! never fails on a numerical reason and runs to its end before it returns, the
 * *_async entry points included (one host synchronization per sweep); mnk_ls_inertia is (count(lambda > 0), the rest,
 * count(lambda < 0)) over the N eigenvalues, whatever info says; solve! is x <- Q ((Q^T x) ./ lambda) with IEEE division;
 * batches and ignored options as for MNK_QR. */
int mnk_ls_create(mnk_ctx* ctx, int64_t N, int algo, mnk_ls** out);
int mnk_ls_destroy(mnk_ls* ls);
/* Options: "pivot_tol" (LDL: |d| <= pivot_tol counts as a zero pivot; default 0),
 * "outer_block" (outer panel width, multiple of 64; default 0 = by size: 512, and 1024 from 32 768 rows on),
 * "lookahead" (0/1; default 1: factor the next panel while the trailing update runs),
 * "probe" (0/1; default 1, effective while "early_reject" and "accept_only_pd" are set: after an early rejection that stopped in the
 * first half of the columns, a matrix from the same KKT handle that follows an ACCEPTED one is first factorized on its leading
 * principal block alone -- a child solver of that order; a block that is not positive definite settles the verdict at a few
 * percent of a factorization's work; statistics "probe_hits" / "probe_misses"). */
int mnk_ls_set_option(mnk_ls* ls, const char* key, double value);

/* factorize!(M) `src/LinearSolvers/lapack_common.jl:54-66` = transfer_matrix!
 * (`:28`; CSC -> dense zero-fill + scatter, device twin
 * `lib/MadNLPGPU/src/utils.jl:12-23`) + dpotrf('L') / dsytrf('L')
 * (`lapack.jl:145-148,164-167`).  The source is named explicitly:
 *   _sc    : aug_com of a sparse condensed system (CSC on device);
 *   _dc    : aug_com of a dense system (on device);
 *   _dense : caller's dense N x N matrix (host or device), lower triangle read;
 *   _csc   : caller's lower-triangular CSC (host), 0/1-based.
 * *info = 0 on success, k > 0 if pivot k (1-based) is not positive (CHOLESKY) or
 * is zero (LDL).  Synchronizes the stream (info is read back). */
int mnk_ls_factorize_sc(mnk_ls* ls, mnk_sc* sc, int* info);
int mnk_ls_factorize_dc(mnk_ls* ls, mnk_dc* dc, int* info);
int mnk_ls_factorize_dense(mnk_ls* ls, const double* A, int64_t lda, int loc, int* info);
int mnk_ls_factorize_csc(mnk_ls* ls, const int32_t* colptr, const int32_t* rowval,
                         const double* nzval, int index_base, int* info);
/* Asynchronous variants: enqueue only, info/inertia are fetched later with
 * mnk_ls_inertia (which synchronizes). */
int mnk_ls_factorize_sc_async(mnk_ls* ls, mnk_sc* sc);
int mnk_ls_factorize_dc_async(mnk_ls* ls, mnk_dc* dc);
/* Batches of INDEPENDENT factorizations (scenario batches, BASELINE config C5; the reference drives distinct solver
 * instances concurrently, `src/KKT/Schur/schur.jl:927-1001` `@blas_safe_threads for k in 1:ns`).  Between _begin and _end
 * the factorize! calls of the calling thread (any solver, any context of one device) transfer their matrices and are
 * queued; _end launches them together: the task queues of instances of the same order are merged into one persistent
 * launch beside two pivot chains, so that one instance's chain-bound ends are filled with its neighbours' trailing
 * updates (N = 11 192: ~10.7 -> ~9.x ms per instance).  Every instance's factor is bit-identical to the one a lone
 * factorize! produces.  Any call that needs a queued solver's factor (inertia, solve, another factorize!, destroy)
 * launches what is queued first, so a forgotten _end cannot give a stale answer.  Thread-local; _begin / _end pairs nest (the
 * outermost _end launches). */
int mnk_factorize_batch_begin(void);
int mnk_factorize_batch_end(void);
/* ... and of independent solves: between _begin and _end the mnk_ls_solve calls of the calling thread with ONE right-hand
 * side on a DEVICE vector are queued; _end runs them up to four systems per launch (one solve is bound by its chain of
 * hops, not by HBM: four side by side take hardly longer than one; N = 11 192: 0.45 -> ~0.2 ms per solve).  The vectors must
 * stay untouched until _end returns (asynchronously, like any device solve: mnk_ls_check_solve as usual).  Solves that do not
 * qualify run at once; several right-hand sides of one solver keep their order (one per launch).  Results are bit-identical
 * to lone solves.  Thread-local, like the factorization batch. */
int mnk_solve_batch_begin(void);
int mnk_solve_batch_end(void);
/* A process that goes idle next to OTHER GPU processes: destroys the CU-masked streams (= hardware queues) this library keeps
 * per device for its persistent schedules -- a device runs only so many queues side by side, all processes together, and a
 * process that merely holds a dozen idle ones can keep another process' pivot chain and bulk kernel from being scheduled
 * together.  Every stream is made again by the first operation that needs it (~ms, once).  The
 * last context of a device to be destroyed does the same.  No equivalent in the reference (its solvers hold no queues). */
int mnk_release_idle_streams(int device);
/* Array forms for n independent instances (one call per phase of an iteration; hosts with a per-call overhead):
 *   _step_batch    : per instance compress_jacobian! + compress_hessian! + build_kkt! + factorize! (asynchronous), the
 *                    factorizations as ONE batch (mnk_factorize_batch_begin / _end around the loop);
 *   _inertia_batch : inertia of every instance (each waits for its own factorization only);
 *   _solve_batch   : one right-hand side per instance, as ONE solve batch (x[i]: N_i entries, in place). */
int mnk_sc_step_batch(int n, mnk_sc* const* sc, mnk_ls* const* ls, const double* const* jac_coo, const double* const* hess_coo,
                      const double* const* pr_diag, const double* const* du_diag, int loc);
int mnk_ls_inertia_batch(int n, mnk_ls* const* ls, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg);
int mnk_ls_solve_batch(int n, mnk_ls* const* ls, double* const* x, int loc);

/* inertia(M) `lapack_common.jl:96-109`, `lapack.jl:240-268`: (num_pos, num_zero, num_neg).
 * CHOLESKY: info == 0 ? (N,0,0) : (0,N,0).  LDL: signs of D. */
int mnk_ls_inertia(mnk_ls* ls, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg);
/* solve_linear_system!(M, x) `lapack_common.jl:75-81` (dpotrs / dsytrs): in place,
 * nrhs right-hand sides with leading dimension ldx (the reference loops over
 * columns, `src/LinearSolvers/linearsolvers.jl:102-110`).  So does this call, one single-vector solve per column, unless
 * option multi_rhs_min is positive, nrhs >= multi_rhs_min and the factor is the static-pivot tier's (CHOLESKY / LDL, not
 * pivoted): then the columns go through both sweeps in chunks of 64 on the fp64 matrix cores, one pass over the factor per
 * chunk and sweep (statistics "solve_path" = 5, "solve_rhs_chunks"; csrc/solve_multi.hip).  The blocked results are those of
 * the same factor with the sums grouped differently, not the bits of the column loop; a column's bits do not depend on nrhs,
 * on its position in x or on the other columns.  Rows >= N of a strided x and columns >= nrhs are never written. */
int mnk_ls_solve(mnk_ls* ls, double* x, int64_t nrhs, int64_t ldx, int loc);
/* Status of the solves enqueued so far, for callers whose vectors live on the device (loc = MNK_DEVICE):
 * synchronizes the context stream; 0 if every solve completed, -3 if a one-launch ("persistent") solve gave
 * up waiting for a peer workgroup -- its result is invalid, the solver has switched to the stepwise solve and
 * the caller repeats the solve.  Host-resident callers never need it: mnk_ls_solve / mnk_*_solve_kkt with
 * loc = MNK_HOST detect the condition before copying anything back and redo the solve themselves.
 * (SolveException of the contract, reference src/LinearSolvers/linearsolvers.jl:133-137.) */
int mnk_ls_check_solve(mnk_ls* ls);
/* Debug / tests: copy the factor (N x N, ld = N; L in the lower triangle, for
 * LDL unit-lower L with D returned separately) and D (N entries, may be NULL).
 * QR: dgeqrf's layout -- R on and above the diagonal, the Householder vectors below it
 * (unit leading entry implicit) -- and tau in D.
 * LU: dgetrf's layout -- U on and above the diagonal, the unit-lower L below it -- and diag(U) in D.
 * EVD: the eigenvectors Q (full N x N, one per column) and the eigenvalues, ascending, in D. */
int mnk_ls_get_factor(mnk_ls* ls, double* L, double* D, int loc);
/* LU only (an error for every other algorithm): dgetrf's ipiv, 1-based -- row k (1-based) was swapped with row ipiv[k-1]
 * in step k -- N entries, on the host or the device (loc). */
int mnk_ls_get_pivots(mnk_ls* ls, int64_t* ipiv, int loc);

/* BUNCHKAUFMAN is served in two tiers: the static-pivot blocked LDL^T (fast path), and -- when that breaks down on
 * a matrix that is not quasi-definite in the given order -- a Bunch-Kaufman factorization with 1x1 / 2x2 pivots and
 * global partner search (dsytf2's strategy; option "bk_fallback", default 1), so that `inertia` follows the
 * reference rule `num_neg_ev` (`src/LinearSolvers/lapack.jl:240-268`) on such systems too.  This reports which tier
 * produced the current factor: *active = 1 if P A P^T = L D L^T with 2x2 blocks; *count = how many factorizations of
 * this solver took the pivoted tier; perm (N entries: row i of the permuted matrix is row perm[i] of A, 0-based) and
 * doff (N entries: sub-diagonal of D, non-zero at the first index of a 2x2 block) may be NULL. */
int mnk_ls_bk_info(mnk_ls* ls, int* active, int* count, int32_t* perm, double* doff);

/* Diagnostics of the last factorization (tests, tuning): key "panel_algo" = the panel algorithm that produced the
 * current factor (4: persistent panel kernel; 1: one launch per panel piece -- chosen automatically while more than
 * one context of this process lives on the device, or for good after a persistent panel gave up on a dependency),
 * "pp_fallbacks" = how many factorizations of this solver were redone for that reason.  Synchronizes when a
 * factorization is pending (the fallback is decided when `info` is read).  "solve_path" = how the solver's last solve ran
 * (0: none yet, 1: one launch per 256-column step, 2: one launch over 256-column steps, 3: one launch over 512-column
 * steps, 4: a system of a merged launch of a solve batch; csrc/solve_plan.h). */
int mnk_ls_get_stat(mnk_ls* ls, const char* key, double* value);

/* ----------------------------------------------------------- utilities ------ */
/* C (M x N) = / -= A (M x K) * B (N x K)^T on the fp64 MFMA tile kernel used by the
 * factorization's trailing update; exposed for unit tests and microbenchmarks.
 * mode 0: C -= A*B^T, 1: C = A*B^T, 2: as 0 but only tiles on/below the diagonal.
 * All pointers are device memory; M, N multiples of 64, K multiple of 16. */
int mnk_gemm_nt(mnk_ctx* ctx, int mode, int64_t M, int64_t N, int64_t K,
                const double* A, int64_t lda, const double* B, int64_t ldb,
                double* C, int64_t ldc);

/* ---- device-side solve_kkt! / mul! of the sparse condensed system -----------------------------
 * The primal-dual vector w = [x (n); s (m); z (m); zl (nlb); zu (nub)] (UnreducedKKTVector layout, reference
 * src/KKT/rhs.jl:119-129) stays on the device across reduce_rhs! / condensation / solve / expansion /
 * finish_aug_solve!, so one call replaces the host-side vector algebra and the per-solve round trips.
 *   mnk_sc_set_bounds         ind_lb / ind_ub: positions of the bounded entries in the primal block [0, n+m)
 *   mnk_sc_set_barrier_terms  reg (n+m), l_diag, u_diag, l_lower, u_lower of the current iterate
 *                             (pr_diag / du_diag come with mnk_sc_build)
 *   mnk_sc_solve_kkt          solve_kkt!(::SparseCondensedKKTSystem, w)  reference src/IPM/factorization.jl:143-167
 *   mnk_sc_mul                mul!(w, kkt, x, alpha, beta)               reference :289-308 + _kktmul! kernels.jl:161-180 */
int mnk_sc_set_bounds(mnk_sc* sc, int64_t nlb, const int64_t* ind_lb, int64_t nub, const int64_t* ind_ub,
                      int index_base);
int mnk_sc_set_barrier_terms(mnk_sc* sc, const double* reg, const double* l_diag, const double* u_diag,
                             const double* l_lower, const double* u_lower, int loc);
int mnk_sc_solve_kkt(mnk_sc* sc, mnk_ls* ls, double* w, int loc);
int mnk_sc_mul(mnk_sc* sc, double* w, const double* x, double alpha, double beta, int loc);

/* Device-side feeders of build_kkt! (first slice of 8(f).4): with these an iteration needs no host vector.
 *   mnk_sc_set_aug_diagonal    set_aug_diagonal!(kkt, solver)  reference src/IPM/kernels.jl:4-27: x, xl, xu, zl, zu are the
 *                              FULL primal-length vectors (n + m entries: variables and slacks) of the iterate; fills
 *                              reg = primal_reg, du_diag = -dual_reg, l_diag = xl_r - x_lr, u_diag = x_ur - xu_r,
 *                              l_lower = zl_r, u_lower = zu_r and pr_diag = reg - l_lower./l_diag - u_lower./u_diag
 *                              (scattered through ind_lb / ind_ub of mnk_sc_set_bounds) INSIDE the handle; the barrier
 *                              terms of mnk_sc_set_barrier_terms are thereby set too
 *   mnk_sc_regularize_diagonal regularize_diagonal!(kkt, primal, dual)  reference src/KKT/KKTsystem.jl:222-226
 *   mnk_sc_build(sc, NULL, NULL, loc) then builds from the handle's own pr_diag / du_diag
 *   mnk_sc_get_diagonals       host copies for tests (any pointer may be NULL) */
int mnk_sc_set_aug_diagonal(mnk_sc* sc, const double* x, const double* xl, const double* xu, const double* zl,
                            const double* zu, double primal_reg, double dual_reg, int loc);
int mnk_sc_regularize_diagonal(mnk_sc* sc, double primal, double dual);
int mnk_sc_get_diagonals(mnk_sc* sc, double* pr_diag, double* du_diag, double* reg, double* l_diag, double* u_diag,
                         double* l_lower, double* u_lower);
/* The bracket of a speculative trial of inertia_correction! (reference src/IPM/solver.jl:611-670; the speculation itself lives in
 * the caller -- madnlp_jl_amd/ipm_dev.py): reg, pr_diag and du_diag are copied into a buffer of the handle
 * before regularize_diagonal! perturbs them for the trial that is factorized AHEAD of the verdict on the unperturbed matrix, and
 * copied back -- bit for bit -- when that matrix is accepted after all. */
int mnk_sc_save_diagonals(mnk_sc* sc);
int mnk_sc_restore_diagonals(mnk_sc* sc);

/* The dense twins: w = [x (n); s (ns); y (m); zl; zu].  solve_kkt!(::DenseCondensedKKTSystem) reference
 * src/IPM/factorization.jl:190-229, the reduced solve of DenseKKTSystem :41-46, mul!(::AbstractDenseKKTSystem)
 * :310-330 (symv on the lower triangle of hess, two gemv with jac). */
int mnk_dc_set_bounds(mnk_dc* dc, int64_t nlb, const int64_t* ind_lb, int64_t nub, const int64_t* ind_ub,
                      int index_base);
int mnk_dc_set_barrier_terms(mnk_dc* dc, const double* reg, const double* l_diag, const double* u_diag,
                             const double* l_lower, const double* u_lower, int loc);
int mnk_dc_solve_kkt(mnk_dc* dc, mnk_ls* ls, double* w, int loc);
int mnk_dc_mul(mnk_dc* dc, double* w, const double* x, double alpha, double beta, int loc);
/* (vectors of n + ns entries; same semantics as the mnk_sc_* feeders above; mnk_dc_build(dc, NULL, NULL, loc) builds from
 * the handle's own diagonals) */
int mnk_dc_set_aug_diagonal(mnk_dc* dc, const double* x, const double* xl, const double* xu, const double* zl,
                            const double* zu, double primal_reg, double dual_reg, int loc);
int mnk_dc_regularize_diagonal(mnk_dc* dc, double primal, double dual);
int mnk_dc_get_diagonals(mnk_dc* dc, double* pr_diag, double* du_diag, double* reg, double* l_diag, double* u_diag,
                         double* l_lower, double* u_lower);


/* ---- IPM scalar reductions over DEVICE-resident iterates (second slice) ----------------------------------
 * The regular-phase functions of reference src/IPM/kernels.jl:263-388,675-695 (GPU twins: mapreduce calls in
 * lib/MadNLPGPU/src/IPM/kernels.jl:4-116).  Every vector argument is a DEVICE pointer; x, xl, xu, zl, zu, f, jacl, dx are
 * the FULL primal-length vectors (ntot = variables + slacks), the *_r views of the reference are taken through the
 * ind_lb / ind_ub given at creation; dzl / dzu (mnk_ipm_get_alpha_z) are the bound-length blocks dual_lb(d) / dual_ub(d)
 * of a KKT vector.  Each call enqueues one or two one-pass reductions on the context's stream, synchronizes and returns
 * the scalar(s) in *out (host).  max/min-type results are bit-identical to the reference's loops, sum-type results agree to
 * summation-order rounding. */
typedef struct mnk_ipm mnk_ipm;
int mnk_ipm_create(mnk_ctx* ctx, int64_t ntot, int64_t nlb, const int64_t* ind_lb, int64_t nub, const int64_t* ind_ub,
                   int index_base, mnk_ipm** out);
int mnk_ipm_destroy(mnk_ipm* ipm);
int mnk_ipm_get_varphi(mnk_ipm* ipm, double obj_val, const double* x, const double* xl, const double* xu, double mu,
                       double* out);                                                    /* kernels.jl:263-283 */
int mnk_ipm_get_inf_du(mnk_ipm* ipm, const double* f, const double* zl, const double* zu, const double* jacl, double sd,
                       double* out);                                                    /* :285-291 */
int mnk_ipm_get_inf_compl(mnk_ipm* ipm, const double* x, const double* xl, const double* xu, const double* zl,
                          const double* zu, double mu, double sc, double* out);         /* :293-303 */
int mnk_ipm_get_min_complementarity(mnk_ipm* ipm, const double* x, const double* xl, const double* xu, const double* zl,
                                    const double* zu, double* out);                     /* :322-332 */
int mnk_ipm_get_average_complementarity(mnk_ipm* ipm, const double* x, const double* xl, const double* xu,
                                        const double* zl, const double* zu, double* out); /* :305-313 */
int mnk_ipm_get_varphi_d(mnk_ipm* ipm, const double* f, const double* x, const double* xl, const double* xu,
                         const double* dx, double mu, double* out);                     /* :341-354 */
int mnk_ipm_get_alpha_max(mnk_ipm* ipm, const double* x, const double* xl, const double* xu, const double* dx, double tau,
                          double* out);                                                 /* :356-371 */
int mnk_ipm_get_alpha_z(mnk_ipm* ipm, const double* zl, const double* zu, const double* dzl, const double* dzu, double tau,
                        double* out);                                                   /* :373-388 */
int mnk_ipm_get_rel_search_norm(mnk_ipm* ipm, const double* x, const double* dx, double* out);   /* :675-682 */
int mnk_ipm_get_sd_sc(mnk_ipm* ipm, const double* l, int64_t m, const double* zl, const double* zu, double s_max,
                      double* out /* [sd, sc] */);                                      /* :684-695 */
int mnk_ipm_get_norms(mnk_ipm* ipm, const double* c, int64_t m, double* out /* [norm(c, Inf), norm(c, 1)] */);
/* Batch mode: between mnk_ipm_batch_begin and mnk_ipm_batch_end the mnk_ipm_get_* calls (regular and restoration phase) only
 * enqueue their reductions and return at once; batch_end synchronizes ONCE and then stores every result into the `out` pointer
 * its call was given (the pointers must stay valid until then; a scalar that divides a result -- sd, sc -- can be passed as 1
 * and applied by the caller).  At most 32 reductions per batch (each call uses one to four, mnk_ipm_quality_function four
 * per sigma). */
int mnk_ipm_batch_begin(mnk_ipm* ipm);
int mnk_ipm_batch_end(mnk_ipm* ipm);
/* Quality function of the adaptive barrier update (reference src/IPM/barrier.jl:152-201) for nsigma = 1..4 centering parameters
 * (sigmas: HOST array) along d = aff + sigma cen, which is never stored: aff_x / cen_x are the primal blocks (ntot) of the two
 * KKT vectors, aff_zl / cen_zl their dual_lb blocks (nlb), aff_zu / cen_zu their dual_ub blocks (nub); x, xl, xu, zl, zu full
 * length.  out (host, 4 nsigma doubles): per sigma a_pr = get_alpha_max(x, xl, xu, d_x, tau), a_du = get_alpha_z(zl_r, zu_r,
 * d_zl, d_zu, tau), S_lb = sum ((x_lr + a_pr d_x_lr - xl_r) (zl_r + a_du d_zl))^2, S_ub = sum ((xu_r - x_ur - a_pr d_x_ur)
 * (zu_r + a_du d_zu))^2.  A NaN step entry gives NaN step lengths.  Four launches per call; the sums read the step lengths on
 * the device.  Follows the batch protocol (4 nsigma of a batch's 32 reductions); nsigma outside 1..4 or a NULL pointer is an error. */
int mnk_ipm_quality_function(mnk_ipm* ipm, int nsigma, const double* sigmas, const double* x, const double* xl,
                             const double* xu, const double* zl, const double* zu, const double* aff_x, const double* aff_zl,
                             const double* aff_zu, const double* cen_x, const double* cen_zl, const double* cen_zu, double tau,
                             double* out);
/* Elementwise pieces of the regular phase on device-resident vectors (asynchronous on the context's stream):
 *   mnk_ipm_set_aug_rhs            set_aug_rhs!  kernels.jl:113-131: px = -f + zl - zu - jacl, py = -c,
 *                                  pzl = (xl_r - x_lr) zl_r + mu, pzu = (xu_r - x_ur) zu_r - mu  (px ntot, py m, pzl nlb, pzu nub)
 *   mnk_ipm_set_perturbation_sets  ind_llb / ind_uub (entries bounded on one side only), once
 *   mnk_ipm_dual_inf_perturbation  dual_inf_perturbation!  :818-823
 *   mnk_ipm_adjust_boundary        adjust_boundary!  :656-673 (xl, xu full-length, in place)
 *   mnk_ipm_reset_bound_dual       the two reset_bound_dual! calls of an accepted step, :775-801 / solver.jl:280-291
 *                                  (full-length vectors; unbounded entries carry -Inf / +Inf bounds) */
int mnk_ipm_set_perturbation_sets(mnk_ipm* ipm, int64_t nllb, const int64_t* ind_llb, int64_t nuub, const int64_t* ind_uub,
                                  int index_base);
int mnk_ipm_set_aug_rhs(mnk_ipm* ipm, const double* f, const double* zl, const double* zu, const double* jacl,
                        const double* c, int64_t m, const double* x, const double* xl, const double* xu, double mu,
                        double* px, double* py, double* pzl, double* pzu);
int mnk_ipm_dual_inf_perturbation(mnk_ipm* ipm, double* px, double mu, double kappa_d);
int mnk_ipm_adjust_boundary(mnk_ipm* ipm, const double* x, double* xl, double* xu, double mu);
int mnk_ipm_reset_bound_dual(mnk_ipm* ipm, double* zl, double* zu, const double* x, const double* xl, const double* xu,
                             double mu, double kappa_sigma);

/* ---- restoration phase (robust restorer) on device-resident vectors (third slice) -------------------------
 * Reference src/IPM/kernels.jl:390-636 (GPU twins lib/MadNLPGPU/src/IPM/kernels.jl:117-462).  pp / nn / zp / zn / dpp / dnn /
 * dzp / dzn, c, l (= y) and dl are m-vectors (the RobustRestorer of src/IPM/restoration.jl:1-37 and the constraint block),
 * f_R / D_R / x_ref and x, xl, xu, zl, zu, jacl, dx full primal length; dzl / dzu bound-length blocks of a KKT vector.
 * Same conventions as the regular-phase reductions above (one synchronizing call per reference function). */
int mnk_ipm_get_obj_val_R(mnk_ipm* ipm, const double* p, const double* n, int64_t m, const double* D_R, const double* x,
                          const double* x_ref, double rho, double zeta, double* out);   /* kernels.jl:390-407 */
int mnk_ipm_get_theta_R(mnk_ipm* ipm, const double* c, const double* p, const double* n, int64_t m, double* out); /* :411-421 */
int mnk_ipm_get_inf_pr_R(mnk_ipm* ipm, const double* c, const double* p, const double* n, int64_t m, double* out); /* :423-433 */
int mnk_ipm_get_inf_du_R(mnk_ipm* ipm, const double* f_R, const double* l, const double* zl, const double* zu,
                         const double* jacl, const double* zp, const double* zn, int64_t m, double rho, double sd,
                         double* out);                                                  /* :435-454 */
int mnk_ipm_get_inf_compl_R(mnk_ipm* ipm, const double* x, const double* xl, const double* xu, const double* zl,
                            const double* zu, const double* pp, const double* zp, const double* nn, const double* zn,
                            int64_t m, double mu_R, double sc, double* out);            /* :456-484 */
int mnk_ipm_get_alpha_max_R(mnk_ipm* ipm, const double* x, const double* xl, const double* xu, const double* dx,
                            const double* pp, const double* dpp, const double* nn, const double* dnn, int64_t m,
                            double tau_R, double* out);                                 /* :486-515 */
int mnk_ipm_get_alpha_z_R(mnk_ipm* ipm, const double* zl, const double* zu, const double* dzl, const double* dzu,
                          const double* zp, const double* dzp, const double* zn, const double* dzn, int64_t m,
                          double tau_R, double* out);                                   /* :517-542 */
int mnk_ipm_get_varphi_R(mnk_ipm* ipm, double obj_val, const double* x, const double* xl, const double* xu, const double* pp,
                         const double* nn, int64_t m, double mu_R, double* out);        /* :544-570 */
/* get_F (soft restoration, :572-610).  The upper-bound term is the reference's own expression |(xu_r - xu_r) zu_r - mu|
 * (:606, the same in the GPU twin :407-410), restated as written */
int mnk_ipm_get_F(mnk_ipm* ipm, const double* c, int64_t m, const double* f, const double* zl, const double* zu,
                  const double* jacl, const double* x, const double* xl, const double* xu, double mu, double* out);
int mnk_ipm_get_varphi_d_R(mnk_ipm* ipm, const double* f_R, const double* x, const double* xl, const double* xu,
                           const double* dx, const double* pp, const double* nn, const double* dpp, const double* dnn,
                           int64_t m, double mu_R, double rho, double* out);            /* :612-636 */
/* Elementwise pieces (asynchronous on the context's stream):
 *   mnk_ipm_populate_RR_nn              populate_RR_nn!  :825-829
 *   mnk_ipm_initialize_robust_restorer  vector part of initialize_robust_restorer!  src/IPM/restoration.jl:46-70:
 *                                       x_ref = x, D_R = min(1, 1/|x_ref|), nn, pp = c + nn, zp = mu_R/pp, zn = mu_R/nn,
 *                                       zl_r / zu_r = min(rho, .) in place in the full-length zl / zu
 *   mnk_ipm_set_f_RR                    set_f_RR!  :106-110
 *   mnk_ipm_set_aug_rhs_RR              set_aug_rhs_RR!  :133-158
 *   mnk_ipm_finish_aug_solve_RR         finish_aug_solve_RR!  :251-257
 *   mnk_ipm_reset_bound_dual_1          reset_bound_dual!(z, x, mu, kappa_sigma)  :775-786
 *   mnk_ipm_set_initial_bounds          set_initial_bounds!  :206-218
 *   mnk_ipm_set_initial_rhs             set_initial_rhs!  :220-230
 *   mnk_ipm_set_aug_rhs_ifr             set_aug_rhs_ifr!  :233-240
 *   mnk_ipm_set_g_ifr                   set_g_ifr!  :242-248
 *   mnk_ipm_initialize_variables        initialize_variables!  :638-654 (in place)
 *   mnk_sc_set_aug_RR / mnk_dc_set_aug_RR   set_aug_RR!  :72-87 + _set_aug_diagonal!  :22-27 inside the KKT handle */
int mnk_ipm_populate_RR_nn(mnk_ipm* ipm, double* nn, const double* c, int64_t m, double mu, double rho);
int mnk_ipm_initialize_robust_restorer(mnk_ipm* ipm, const double* x, const double* c, int64_t m, double mu_R, double rho,
                                       double* x_ref, double* D_R, double* nn, double* pp, double* zp, double* zn,
                                       double* zl, double* zu);
int mnk_ipm_set_f_RR(mnk_ipm* ipm, double* f_R, const double* D_R, const double* x, const double* x_ref, double zeta);
int mnk_ipm_set_aug_rhs_RR(mnk_ipm* ipm, const double* f_R, const double* zl, const double* zu, const double* jacl,
                           const double* c, const double* y, const double* pp, const double* nn, const double* zp,
                           const double* zn, int64_t m, const double* x, const double* xl, const double* xu, double mu_R,
                           double rho, double* px, double* py, double* pzl, double* pzu);
int mnk_ipm_finish_aug_solve_RR(mnk_ipm* ipm, double* dpp, double* dnn, double* dzp, double* dzn, const double* l,
                                const double* dl, const double* pp, const double* nn, const double* zp, const double* zn,
                                int64_t m, double mu_R, double rho);
int mnk_ipm_reset_bound_dual_1(mnk_ipm* ipm, double* z, const double* x, int64_t n, double mu, double kappa_sigma);
int mnk_ipm_set_initial_bounds(mnk_ipm* ipm, double* xl, double* xu, int64_t n, double tol);
int mnk_ipm_set_initial_rhs(mnk_ipm* ipm, const double* f, const double* zl, const double* zu, double* px, double* py,
                            int64_t m, double* pzl, double* pzu);
int mnk_ipm_set_aug_rhs_ifr(mnk_ipm* ipm, const double* c, int64_t m, double* px, double* py, double* pzl, double* pzu);
int mnk_ipm_set_g_ifr(mnk_ipm* ipm, double* g, const double* f, const double* x, const double* xl, const double* xu,
                      const double* jacl, double mu);
int mnk_ipm_initialize_variables(mnk_ipm* ipm, double* x, const double* xl, const double* xu, int64_t n, double bound_push,
                                 double bound_fac);
int mnk_sc_set_aug_RR(mnk_sc* sc, const double* x, const double* xl, const double* xu, const double* zl, const double* zu,
                      const double* D_R, const double* pp, const double* zp, const double* nn, const double* zn, double zeta,
                      double primal_reg, double dual_reg);
int mnk_dc_set_aug_RR(mnk_dc* dc, const double* x, const double* xl, const double* xu, const double* zl, const double* zu,
                      const double* D_R, const double* pp, const double* zp, const double* nn, const double* zn, double zeta,
                      double primal_reg, double dual_reg);

/* ---- plain vector work of the solver loop on device vectors (callback half) ----------------------------
 * The copyto! / fill! / axpy! / dot / norm calls the reference's regular! / restore! / robust! loops make on the iterate
 * (src/IPM/solver.jl:236-291, :300-411, :413-545; src/IPM/line_search.jl:60-64, :170-176), the Richardson loop's axpy! and
 * norms (src/LinearSolvers/backsolve.jl:27-76) and the products a dense QP model's callbacks need.  Asynchronous on the
 * context's stream; mnk_ipm_get_* follow the batch protocol above.
 *   mnk_ipm_get_dot / _get_sum / _get_norm2     dot(x, y), sum(v), norm(v, 2)
 *   mnk_ipm_vec_copy / _fill / _axpby           copyto!, fill!, out = a x + b y (y = NULL: out = a x; aliasing allowed)
 *   mnk_ipm_vec_scatter_axpy / _gather          y[idx] .+= a .* x ;  out .= a .* x[idx]   (idx: device, 0-based)
 *   mnk_ipm_bound_dual_axpy / _fill             zl_r .+= a dzl, zu_r .+= a dzu ;  zl_r .= v, zu_r .= v
 *   mnk_ipm_gemv                                y = alpha op(A) x + beta y, A column-major m x n */
int mnk_ipm_get_dot(mnk_ipm* ipm, const double* x, const double* y, int64_t n, double* out);
int mnk_ipm_get_sum(mnk_ipm* ipm, const double* v, int64_t n, double* out);
int mnk_ipm_get_norm2(mnk_ipm* ipm, const double* v, int64_t n, double* out);
int mnk_ipm_vec_copy(mnk_ipm* ipm, double* dst, const double* src, int64_t n);
int mnk_ipm_vec_fill(mnk_ipm* ipm, double* v, int64_t n, double value);
int mnk_ipm_vec_axpby(mnk_ipm* ipm, double* out, double a, const double* x, double b, const double* y, int64_t n);
int mnk_ipm_vec_scatter_axpy(mnk_ipm* ipm, double* y, const int64_t* idx, double a, const double* x, int64_t n);
int mnk_ipm_vec_gather(mnk_ipm* ipm, double* out, double a, const double* x, const int64_t* idx, int64_t n);
int mnk_ipm_bound_dual_axpy(mnk_ipm* ipm, double* zl, double* zu, double a, const double* dzl, const double* dzu);
int mnk_ipm_bound_dual_fill(mnk_ipm* ipm, double* zl, double* zu, double v);
int mnk_ipm_gemv(mnk_ipm* ipm, int trans, int64_t m, int64_t n, double alpha, const double* A, int64_t lda, const double* x,
                 double beta, double* y);

/* ---- vector kernels of the restarted GMRES refinement (csrc/krylov.hip) ---------------------------
 * The capability of the reference's lib/MadNLPKrylov: GMRES around solve_kkt! / mul!, selected by the solver option
 * `iterator = "krylov"`.  V is a device buffer of basis columns with leading dimension ldv >= n (column j starts at V + j ldv),
 * u the vector being orthogonalized, k = 1..8 the number of columns a call uses.  Ordinary launches on the context's stream.
 * Every sum is taken in the fixed order of the mnk_ipm_get_* sum reductions, every product, sum and difference is rounded
 * on its own.  One Arnoldi step is dots -> project -> dots -> project -> normalize with one synchronization (a batch).
 *   mnk_ipm_krylov_dots       out[j] = V_j . u (j < k), out[k] = u . u  (host, k + 1 doubles); one pass over u and the
 *                             columns.  Follows the batch protocol (k + 1 of a batch's 32 reductions).  The results also
 *                             stay on the device: mnk_ipm_krylov_last_dots gives their address
 *   mnk_ipm_krylov_last_dots  *coef = device address of the k + 1 results of the most recent mnk_ipm_krylov_dots call; valid
 *                             until the next batch reaches the same position (or the next call outside a batch)
 *   mnk_ipm_krylov_project    u -= sum_j coef[j] V_j, the terms subtracted in the order j = 0 .. k-1; coef: DEVICE, k
 *                             doubles (the preceding dots call's results: nothing goes to the host in between).  Leaves the
 *                             block partial sums of the new u . u in the handle
 *   mnk_ipm_krylov_axpy       x += sum_j y[j] V_j in the order j = 0 .. k-1; y_host: HOST, k doubles, passed by value
 *   mnk_ipm_krylov_normalize  v = u / norm(u, 2), out[0] = norm(u, 2) (host; batch protocol, one reduction).
 *                             after_project = 1: u . u is what the preceding mnk_ipm_krylov_project left, and the call is
 *                             one launch; 0: a launch of its own sums it first.  A zero u gives a non-finite v
 * A NULL pointer, k outside 1..8, n < 0 or ldv < n is an error and launches nothing. */
int mnk_ipm_krylov_dots(mnk_ipm* ipm, const double* V, int64_t ldv, int k, const double* u, int64_t n, double* out);
int mnk_ipm_krylov_last_dots(mnk_ipm* ipm, const double** coef);
int mnk_ipm_krylov_project(mnk_ipm* ipm, double* u, const double* V, int64_t ldv, int k, int64_t n, const double* coef);
int mnk_ipm_krylov_axpy(mnk_ipm* ipm, double* x, const double* V, int64_t ldv, int k, const double* y_host, int64_t n);
int mnk_ipm_krylov_normalize(mnk_ipm* ipm, double* v, const double* u, int64_t n, int after_project, double* out);

/* ---- NLP scaling and objective sense around a model's raw callback values (csrc/nlp_scale.hip) -------------------------
 * The factors the reference's callback wrappers apply (src/Callbacks/nlpmodels.jl:771-906, src/IPM/callbacks.jl:28-49), on
 * device vectors, asynchronous on the context's stream, one launch each; a length of 0 launches nothing.  Every product and
 * difference is rounded on its own (no FMA).
 *   mnk_ipm_vec_mul     out[i] = a[i] * b[i], i < n; out may alias a or b
 *   mnk_ipm_scale_cons  eval_cons_wrapper! after the model's cons!: c[i] = c[i] * con_scale[i], minus the slack of row i,
 *                       minus rhs[i], in this order.  con_scale = NULL: ones.  slack has ns entries; slack_pos (device, m
 *                       entries, 0-based) holds for every row the position of its slack in `slack`, negative for an
 *                       equality row -- the inverse of the solver's ind_ineq; NULL: the identity (ns == m), or unused (ns == 0)
 *   mnk_ipm_scale_grad  f[0 .. n) *= factor (obj_sign * obj_scale), f[n .. ntot) = 0: the slack part of the gradient */
int mnk_ipm_vec_mul(mnk_ipm* ipm, double* out, const double* a, const double* b, int64_t n);
int mnk_ipm_scale_cons(mnk_ipm* ipm, double* c, const double* con_scale, const double* slack, const int64_t* slack_pos,
                       int64_t ns, const double* rhs, int64_t m);
int mnk_ipm_scale_grad(mnk_ipm* ipm, double* f, int64_t n, int64_t ntot, double factor);

/* ---- fixed variables made parameters, fixed_variable_treatment = MakeParameter (csrc/fixed_vars.hip) ---------------------
 * The reference's MakeParameter callback wrappers (src/Callbacks/nlpmodels.jl:912-1033) on device vectors: the model is
 * evaluated at its full length, the solver sees the free variables only.  Index arrays are host, 0-based, int64.
 *   mnk_fix_create      n: the model's variables; free[nfree] and fixed[nfixed] (strictly increasing, disjoint, together all
 *                       of 0 .. n-1) with the fixed values; ind_jac_free[njac]: the model's Jacobian COO entries (of nnzj_full)
 *                       whose column is free; ind_hess_free[nhess]: the Hessian COO entries (of nnzh_full) whose row and column
 *                       are free.  Every index is checked against its range.  Everything is uploaded once; the handle owns a
 *                       device x_full of n entries whose fixed entries are written here and never again
 *   mnk_fix_x_full      the device pointer of x_full (what the model's callbacks are given)
 *   mnk_fix_get_x_full  x_full downloaded to n host doubles (synchronizes; tests and reporting)
 *   mnk_fix_expand      x_full[free[i]] = x[i], i < nfree
 *   mnk_fix_gather      dst[i] = (src_full[idx[i]] * scale[i]) * factor with idx = free / ind_jac_free / ind_hess_free for
 *                       which = MNK_FIX_FREE / _JAC / _HESS; scale = NULL: ones.  Two rounded products (no FMA), the order of
 *                       the host layer: gather, constraint scaling and the objective factor in one launch
 *   mnk_fix_dense_grad  g[fixed[i]] = x[fixed[i]] - value[i]: the gradient entries of variables frozen in a dense system
 * expand, gather and dense_grad are asynchronous on the context's stream, one launch each (none for an empty set), without
 * allocation, atomics or host round trips.  The handle is an opaque mnk_fix*; like mnk_tape* below the prototypes spell it
 * void* (mnk_fix_create: void* out = mnk_fix**). */
typedef struct mnk_fix mnk_fix;
enum { MNK_FIX_FREE = 0, MNK_FIX_JAC = 1, MNK_FIX_HESS = 2 };
int mnk_fix_create(mnk_ctx* ctx, int64_t n, int64_t nfree, const int64_t* free_idx, int64_t nfixed, const int64_t* fixed_idx,
                   const double* fixed_val, int64_t nnzj_full, int64_t njac, const int64_t* ind_jac_free, int64_t nnzh_full,
                   int64_t nhess, const int64_t* ind_hess_free, void* out);
int mnk_fix_destroy(void* fix);
void* mnk_fix_x_full(void* fix);
int mnk_fix_get_x_full(void* fix, double* out);
int mnk_fix_expand(void* fix, const double* x);
int mnk_fix_gather(void* fix, int which, const double* src_full, const double* scale, double factor, double* dst);
int mnk_fix_dense_grad(void* fix, double* g, const double* x);

/* ---- device evaluation of an NLP model's callbacks: polar AC optimal power flow (callback half) --------
 * What eval_f_wrapper / eval_grad_f_wrapper! / eval_cons_wrapper! / eval_jac_wrapper! / eval_lag_hess_wrapper!
 * (reference src/IPM/callbacks.jl:1-96) obtain from the model through NLPModels.obj / grad! / cons! / jac_coord! /
 * hess_coord!.  The model is the polar AC-OPF the reference's GPU benchmarks solve; variable / constraint / COO order are
 * those of `madnlp_jl_amd.problems.ACOPFModel` (see csrc/opf_eval.hip).  Index arrays are host, 0-based; arc_coef is
 * (2 nbranch) x 6 row-major (from sides first), bus_data nbus x 4 (pd, qd, gs, bs), gen_cost ngen x 3 (c2, c1, c0).
 * x, y and every output are device vectors; calls are asynchronous on the context's stream. */
typedef struct mnk_opf mnk_opf;
int mnk_opf_create(mnk_ctx* ctx, int64_t nbus, int64_t ngen, int64_t nbranch, const int32_t* fr, const int32_t* to,
                   const int32_t* gen_bus, const double* arc_coef, const double* bus_data, const double* gen_cost,
                   mnk_opf** out);
int mnk_opf_destroy(mnk_opf* opf);
int mnk_opf_sizes(mnk_opf* opf, int64_t* n, int64_t* m, int64_t* nnzj, int64_t* nnzh);
int mnk_opf_obj_terms(mnk_opf* opf, const double* x, double* terms /* ngen; obj = sum(terms) */);
int mnk_opf_grad(mnk_opf* opf, const double* x, double* g);
int mnk_opf_cons(mnk_opf* opf, const double* x, double* c);
int mnk_opf_jac_coord(mnk_opf* opf, const double* x, double* jac);
int mnk_opf_hess_coord(mnk_opf* opf, const double* x, const double* y, double obj_weight, double* hess);

/* ---- device evaluation of ANY NLP written as patterns: expression tapes (csrc/tape_eval.hip) -----
 * The general form of mnk_opf_*: a model is a list of patterns, each one scalar expression applied to R rows of index and
 * parameter data (objective pattern: f += sum_r e_r; constraint pattern: c[rows[r]] += e_r, several patterns may feed one
 * row, rows fed by none evaluate to 0).  `madnlp_jl_amd.tape_model` compiles an expression to the three tapes a pattern is
 * added with -- 0 value (one output), 1 first derivatives (out_j[o] = local variable), 2 second derivatives (out_j[o] >=
 * out_l[o] = local pair) -- and is the host mirror.  A tape is straight-line code: `code` holds (op, dst_slot, a, b) per
 * instruction, op 0 add 1 sub 2 mul 3 div 4 neg 5 sin 6 cos 7 exp 8 log 9 sqrt 16 pow 17 tan 18 atan 19 tanh 20 abs
 * 21 sign 22 step 23 min 24 max (10 .. 15 are unassigned and refused; 0 .. 3, 16, 23 and 24 read `a` and `b`, the others
 * `a` only); min = (b < a) ? b : a, max = (b > a) ? b : a, step = (a >= 0) ? 1 : 0, sign = (a > 0) ? 1 : (a < 0) ? -1 : 0
 * as written, abs clears the sign bit.  An operand is
 * kind << 24 | index with kind 0 slot (< nslot <= 32), 1 local variable (< k <= 8), 2 parameter column (< q <= 8),
 * 3 constant (< nconst).  var_index is R x k and params R x q, row-major; all index arrays are host, 0-based; a row of
 * var_index names k distinct variables.  mnk_tape_add_pattern checks everything a kernel will index with and returns
 * non-zero (mnk_last_error_string says what) for a bad tape; nothing is uploaded before mnk_tape_finalize.
 * COO layout: pattern-major, output-major, then row -- entry = base[pattern] + o * R + r; Jacobian (rows[r],
 * var_index[r, out_j[o]]), Hessian at (max, min) of the pair's global indices; duplicates across patterns are expected.
 * cons / grad add the contributions of a destination in term order (no atomics).  x, y and every output are device
 * vectors; the evaluation calls are asynchronous on the context's stream. */
/* The handle is an opaque mnk_tape*.  TEMPORARY: the prototypes below spell it void* (mnk_tape_create: void* out = mnk_tape**),
 * at the cost of C type checking on this one handle family, because the static header check of tests/test_julia_glue.py knows
 * the handle types by a fixed list of names; the follow-up adds `tape` to that list and types these prototypes
 * (mnk_tape* / mnk_tape**), which does not change the binary interface. */
typedef struct mnk_tape mnk_tape;
int mnk_tape_create(mnk_ctx* ctx, int64_t n, int64_t m, void* out);
int mnk_tape_destroy(void* tape);
int mnk_tape_add_pattern(void* tape, int kind /* 0 objective, 1 constraint */, int64_t R, int k, int q,
                         const int32_t* var_index, const double* params, const int32_t* rows,
                         int64_t ninstr0, const int32_t* code0, int64_t nconst0, const double* consts0, int64_t nout0,
                         const int32_t* out_operand0, const int32_t* out_j0, const int32_t* out_l0, int nslot0,
                         int64_t ninstr1, const int32_t* code1, int64_t nconst1, const double* consts1, int64_t nout1,
                         const int32_t* out_operand1, const int32_t* out_j1, const int32_t* out_l1, int nslot1,
                         int64_t ninstr2, const int32_t* code2, int64_t nconst2, const double* consts2, int64_t nout2,
                         const int32_t* out_operand2, const int32_t* out_j2, const int32_t* out_l2, int nslot2);
int mnk_tape_finalize(void* tape);
int mnk_tape_sizes(void* tape, int64_t* n, int64_t* m, int64_t* nterms, int64_t* nnzj, int64_t* nnzh);
/* which callback launches have a tape with an opcode from 16 on and therefore run the larger of the two interpreter
 * kernels: the sum of obj 1, grad 2, cons 4, jac 8, hess 16 (0: every launch runs the kernel that knows 0 .. 9 only) */
int mnk_tape_extended(void* tape, int* mask);
int mnk_tape_get_structure(void* tape, int32_t* jac_I, int32_t* jac_J, int32_t* hess_I, int32_t* hess_J);
int mnk_tape_obj_terms(void* tape, const double* x, double* terms /* nterms; obj = sum(terms) */);
int mnk_tape_grad(void* tape, const double* x, double* g);
int mnk_tape_cons(void* tape, const double* x, double* c);
int mnk_tape_jac_coord(void* tape, const double* x, double* jac);
int mnk_tape_hess_coord(void* tape, const double* x, const double* y, double obj_weight, double* hess);

/* ---- dense S stage of the Schur-complement KKT system ----------------------------------------------
 * Reference: `SchurComplementKKTSystem` src/KKT/Schur/schur.jl -- `build_kkt!` :927-1001 (phase 1: factor every
 * scenario block A_k and form A_k^-1 C_dk'; phase 2: S -= C_dk A_k^-1 C_dk'), `factorize_kkt!` :1003-1005, steps 3-5 of
 * `solve_kkt!` :1040-1058.  Scenario blocks arrive DENSE here (the reference factors them with a sparse solver per
 * scenario, which is outside this path); A_k (blk x blk, lower triangle read, symmetric indefinite), C_dk (nd x blk).
 * Scenarios are sharded over the ranks of a multi-GPU job: a handle holds the ns_local scenarios of ONE rank.
 *   mnk_schur_build_local  S_out = S0 - sum_{local k} C_dk A_k^-1 C_dk'   (S0 = H_dd + Sigma_dd + inequality terms on
 *                          the rank that owns it, NULL elsewhere); S_out is caller-owned DEVICE memory, nd x nd; the
 *                          caller sums the ranks' contributions with ONE all-reduce (RCCL), then
 *   mnk_schur_factorize_s  every rank factors S with the dense solver; mnk_schur_inertia_s: reference
 *                          `is_inertia_correct` :901-903 wants (nd, 0, 0)
 *   mnk_schur_forward      r_k <- A_k^-1 r_k (rhs_k: ns_local x blk, device) and contrib_d = -sum_k C_dk r_k (nd, device):
 *                          the caller adds r_d and all-reduces nd doubles
 *   mnk_schur_solve_s      S x_d = r_d
 *   mnk_schur_backward     x_k = r_k - (A_k^-1 C_dk') x_d */
typedef struct mnk_schur mnk_schur;
int mnk_schur_create(mnk_ctx* ctx, int64_t ns_local, int64_t blk, int64_t nd, int algo, mnk_schur** out);
int mnk_schur_destroy(mnk_schur* h);
int mnk_schur_set_block(mnk_schur* h, int64_t k, const double* A_kk, int64_t lda, const double* C_dk, int64_t ldc,
                        int loc);
int mnk_schur_build_local(mnk_schur* h, const double* S0, int64_t lds0, int loc_s0, double* S_out, int64_t lds_out);
int mnk_schur_factorize_s(mnk_schur* h, const double* S, int64_t lds, int loc, int* info);
int mnk_schur_inertia_s(mnk_schur* h, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg);
int mnk_schur_scenario_inertia(mnk_schur* h, int64_t k, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg);
/* Which tier produced scenario k's current factor (mnk_ls_bk_info of its solver): *active = 1 when the pivoted Bunch-Kaufman
 * tier was taken -- mnk_schur_build_local then forms that scenario's term column by column (T_k = A_k^-1 C_dk') instead of on
 * the grouped path; *count = how many factorizations of this scenario took it so far.  Either pointer may be NULL. */
int mnk_schur_scenario_bk_info(mnk_schur* h, int64_t k, int* active, int* count);
int mnk_schur_forward(mnk_schur* h, double* rhs_k, double* contrib_d);
int mnk_schur_solve_s(mnk_schur* h, double* rhs_d);
int mnk_schur_backward(mnk_schur* h, double* rhs_k, const double* x_d);
/* Single-rank conveniences for callers that keep no device memory of their own (the host-driven KKT type of the Julia glue):
 *   mnk_schur_s_buffer  a device buffer of nd x nd doubles owned by the handle (S_out of _build_local, S of _factorize_s);
 *   mnk_schur_solve     steps 3-5 of solve_kkt! (reference :1078-1092) in one call, host (loc = MNK_HOST) or device vectors:
 *                       rhs_k = ns x blk (scenario k at k * blk), rhs_d = nd, both overwritten with the solution. */
void* mnk_schur_s_buffer(mnk_schur* h);
/* Device-side assembly of the scenario blocks (round 6).  Reference: the scatter of the callback values through precomputed index
 * maps in build_kkt! (src/KKT/Schur/schur.jl:935-972, maps built at :460-700) and its GPU twin's nine kernels
 * (lib/MadNLPGPU/ext/MadNLPGPUCUDAExt/kernels_schur.jl:14-174, @atomic adds).
 *   mnk_schur_set_structure  once: the COO patterns of the Lagrangian Hessian (any triangle: forced to the lower one) and of the
 *                            Jacobian (row = constraint, column = variable), the rows of the inequality constraints in slack order
 *                            (ind_ineq) and of the equality constraints (ind_eq); variable layout [v_1 .. v_ns (nv each), d (nd)],
 *                            constraint layout [c_1 .. c_ns (nc each)].  Checks what _build_schur_symbolic checks (:140-236: a Hessian
 *                            entry that couples two scenarios, a constraint that reaches another scenario, unequal row counts) and
 *                            builds, per touched entry of A_k (order nv + equality rows per scenario, both triangles), C_dk (nd x blk)
 *                            and S0 (nd x nd), the list of its sources in the reference's scatter order.  ns_global / local_scen:
 *                            the global scenario of every local block when the scenarios are sharded over ranks (NULL: all local);
 *                            own_design: this rank adds H_dd + Sigma_d to its S0 (exactly one rank does).
 *   mnk_schur_assemble       per build_kkt!: hess / jac (COO values), pr_diag (n + n_ineq), du_diag (m), host or device (pr_diag =
 *                            du_diag = NULL: the handle's own, see mnk_schur_set_aug_diagonal below) -> A_k, C_dk of
 *                            every local scenario and S0 (mnk_schur_s0_buffer, device) in one launch, every entry summed by one thread
 *                            in the reference's order (the bits of a sequential scatter-add, the same in every run); then
 *                            mnk_schur_build_local(h, mnk_schur_s0_buffer(h), nd, MNK_DEVICE, ...)
 *   mnk_schur_get_block      host copies of one assembled block pair and / or of S0 (tests; any pointer may be NULL) */
int mnk_schur_set_structure(mnk_schur* h, int64_t n, int64_t m, int64_t nv, int64_t nc, int64_t nnzh, const int32_t* hess_I,
                            const int32_t* hess_J, int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t n_ineq,
                            const int64_t* ind_ineq, int64_t n_eq, const int64_t* ind_eq, int index_base, int64_t ns_global,
                            const int64_t* local_scen, int own_design);
int mnk_schur_assemble(mnk_schur* h, const double* hess, const double* jac, const double* pr_diag, const double* du_diag, int loc);
void* mnk_schur_s0_buffer(mnk_schur* h);
int mnk_schur_get_block(mnk_schur* h, int64_t k, double* A_kk, double* C_dk, double* S0);
int mnk_schur_solve(mnk_schur* h, double* rhs_k, double* rhs_d, int loc);
/* Long inequality rows.  The source list of an inequality row holds one term per pair of its COO entries: it grows with the square
 * of the row's length (a second-stage constraint that touches all of 400 design variables: 160 000 terms per row).  A row with MORE
 * than `row_entries` COO entries (duplicates counted) therefore adds no pairs: mnk_schur_assemble stages the entries of such rows
 * into dense zero-padded operands (duplicates summed in COO order) and adds J' D J of them to A_k, C_dk and S0 as weighted Gram
 * products on the fp64 matrix cores, behind the source lists' kernel.  Every destination entry is owned by one workgroup and summed
 * in a fixed order: the bits depend on the structure and the values alone.  A problem whose inequality rows all have at most
 * `row_entries` entries keeps the bits of the source lists.
 *   mnk_schur_set_gram_threshold  the threshold of the NEXT mnk_schur_set_structure; negative: the built-in default (64),
 *                                 INT64_MAX: never (every row keeps its pairs)
 *   mnk_schur_assembly_stats      of the structure in force: out[0] = terms of the source lists, out[1] = their segments (touched
 *                                 entries), out[2] = long rows over the local scenarios, out[3] = doubles of the staging operands,
 *                                 out[4] = the threshold in force; cap >= 5 */
int mnk_schur_set_gram_threshold(mnk_schur* h, int64_t row_entries);
int mnk_schur_assembly_stats(mnk_schur* h, int64_t* out, int cap);
/* The KKT-handle contract on the Schur handle (what mnk_sc_* / mnk_dc_* give the condensed and dense systems): bound / barrier state,
 * device-side feeders, solve_kkt!, mul!, jtprod! and mul_hess_blk! on host (loc = MNK_HOST) or device vectors.  SINGLE RANK only: all
 * scenarios local and the design block owned (local_scen = NULL, own_design = 1 in mnk_schur_set_structure); a sharded handle is
 * refused.  Vectors are laid out as the reference's UnreducedKKTVector: w = (x (n), s (n_ineq), y (m), z_l (nlb), z_u (nub)).
 *   mnk_schur_set_bounds           once: the positions of the bounded entries in the primal block [0, n + n_ineq)
 *   mnk_schur_set_barrier_terms    reg (n + n_ineq), l_diag, u_diag, l_lower, u_lower of the iterate
 *   mnk_schur_set_aug_diagonal     set_aug_diagonal! inside the handle (x, xl, xu, zl, zu of length n + n_ineq): the handle then owns
 *   mnk_schur_regularize_diagonal  reg, pr_diag (n + n_ineq) and du_diag (m); mnk_schur_assemble with pr_diag = du_diag = NULL uses them
 *   mnk_schur_get_diagonals        host copies (any pointer may be NULL)
 * mnk_schur_assemble keeps device copies of the COO values and diagonals it was given and of the condensation weights D; the
 * products below read the values of the LAST assemble and are refused before the first.  They run over three row lists built once
 * by mnk_schur_set_structure (J, J' and Symmetric(H, :L) with a permutation into the COO value arrays: duplicates stay separate terms
 * in COO order).  A row with at most `row_entries` entries is summed by one thread in list order; a longer one (the design rows of J'
 * and H collect entries from every scenario) by one 64-lane wavefront: lane l sums entries l, l + 64, ... in ascending order, a fixed
 * xor-butterfly (offsets 32, 16, ..., 1) combines the partials.  Every multiply and add is rounded on its own and nothing is added
 * atomically: the bits depend on the lists and the values alone.  y = alpha acc (+ beta y when beta != 0).
 *   mnk_schur_compress_jacobian    compress_jacobian! / compress_hessian! (:917-923): the kept COO values of the Jacobian / the Hessian as
 *   mnk_schur_compress_hessian     of now, without an assemble (the interior-point loop calls jtprod! on a fresh Jacobian before it
 *                                  builds the next KKT system); mnk_schur_jtprod works from the first compress_jacobian on
 *   mnk_schur_set_spmv_threshold   `row_entries` of the NEXT mnk_schur_set_structure; negative: the default (64), INT64_MAX: never
 *   mnk_schur_solve_kkt            solve_kkt! (reference src/KKT/Schur/schur.jl:1007-1109) after mnk_schur_build_local and
 *                                  mnk_schur_factorize_s; a scenario or design solve that gave up ends the call with its error, as
 *                                  mnk_schur_solve does
 *   mnk_schur_mul                  w = alpha K x + beta w (:1112-1139)
 *   mnk_schur_jtprod               y (n + n_ineq) = [J' x ; -x[ind_ineq]], x (m) (:907-915)
 *   mnk_schur_mul_hess_blk         wx = [Symmetric(H, :L) t[0:n] ; 0] + t .* pr_diag (:1141-1146)
 *   mnk_schur_spmv_plan            host only, no device is opened: the row lists mnk_schur_set_structure would build from the same
 *                                  pattern arguments with threshold T, for `which` = 0 (J, m rows), 1 (J', n rows), 2 (H, n rows):
 *                                  counts = {rows, entries, long rows, T in force}; row_ptr (rows + 1), col_idx, perm (entries) and
 *                                  long_rows (ascending) may each be NULL (a first call sizes the arrays) */
int mnk_schur_set_bounds(mnk_schur* h, int64_t nlb, const int64_t* ind_lb, int64_t nub, const int64_t* ind_ub, int index_base);
int mnk_schur_set_barrier_terms(mnk_schur* h, const double* reg, const double* l_diag, const double* u_diag, const double* l_lower,
                                const double* u_lower, int loc);
int mnk_schur_set_aug_diagonal(mnk_schur* h, const double* x, const double* xl, const double* xu, const double* zl, const double* zu,
                               double primal_reg, double dual_reg, int loc);
int mnk_schur_regularize_diagonal(mnk_schur* h, double primal, double dual);
int mnk_schur_get_diagonals(mnk_schur* h, double* pr_diag, double* du_diag, double* reg, double* l_diag, double* u_diag, double* l_lower,
                            double* u_lower);
int mnk_schur_compress_jacobian(mnk_schur* h, const double* jac, int loc);
int mnk_schur_compress_hessian(mnk_schur* h, const double* hess, int loc);
int mnk_schur_set_spmv_threshold(mnk_schur* h, int64_t row_entries);
int mnk_schur_solve_kkt(mnk_schur* h, double* w, int loc);
int mnk_schur_mul(mnk_schur* h, double* w, const double* x, double alpha, double beta, int loc);
int mnk_schur_jtprod(mnk_schur* h, double* y, const double* x, int loc);
int mnk_schur_mul_hess_blk(mnk_schur* h, double* wx, const double* t, int loc);
int mnk_schur_spmv_plan(int64_t n, int64_t m, int64_t nv, int64_t nc, int64_t nnzh, const int32_t* hess_I, const int32_t* hess_J,
                        int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t n_ineq, const int64_t* ind_ineq, int64_t n_eq,
                        const int64_t* ind_eq, int index_base, int64_t ns_global, const int64_t* local_scen, int own_design, int64_t T,
                        int which, int32_t* row_ptr, int32_t* col_idx, int32_t* perm, int32_t* long_rows, int64_t* counts);

/* Diagnostics: with option "solve_trace" = 1 the persistent solve kernel stamps the forward sweep's critical
 * path (8 x 100 MHz timer values per 64-row block); this copies them out (n = number of uint64 to copy). */
int mnk_ls_debug_solve_trace(mnk_ls* ls, unsigned long long* out, int64_t n);

/* Diagnostics: with option "dag_debug" = 1 a factorization of the task-DAG schedule that runs into its bounded waits keeps the
 * schedule's progress words (two queue counters | front[Np / 64] | af[ntile^2] | tprog[ntile^2]) and 8 words per pivot-chain
 * strip saying what it was waiting for ({site, strip-column, strip, word, target, value, spins >> 20, 0}) as the time-out left
 * them, before the factorization is redone.  Copies up to `nflags` / `nchain` ints; *have = 1 if a time-out was recorded. */
int mnk_ls_debug_dag_state(mnk_ls* ls, int* flags, int64_t nflags, int* chain, int64_t nchain, int* have);

/* Size of a persistent grid on the CU-mask bits [cu_first + first, cu_first + num_cu) with `per_cu` workgroups per CU: the
 * workgroups the hardware places AT LAUNCH (the dispatcher deals a grid out evenly per XCD and shader engine -- mask bit b is
 * CU b / 8 of XCD b % 8, shader engine (b / 8) % 4 --, so the engine the mask leaves the fewest CUs bounds it).  Pure host
 * arithmetic (no device needed); the task-DAG schedule sizes its bulk kernel with it: 672 beside the 16-CU chain of a 256-CU
 * part, not 3 x 240 (workgroups placed in mid-kernel were the schedule's rare time-out). */
int mnk_debug_grid_at_launch(int cu_first, int num_cu, int first, int per_cu);
/* Which CU-mask bits the two streams of a CU-masked pair get on a device of `num_cu` CUs (csrc/stream_plan.hip; host only, no device
 * is opened).  kind: 0 the task-DAG schedule's pivot chain | bulk kernel, 1 its deep band, 2 the second chain partition | bulk
 * stream of batches, 3 the chains of a round of small systems (arg = their CUs) | the rest, 4 the look-ahead pair of the
 * launch-per-panel schedules (arg = the panel stream's CUs; negative: the default); dag_cus / dag_cus2 = the chain CUs of kinds 0
 * and 1.  split = {chain_first, chain_count, rest_first, rest_count}; chain_mask / rest_mask receive the (num_cu + 31) / 32 mask
 * words of the two streams.  Returns 1, 0 where no such pair is made (split and masks are zero then), -1 on bad arguments. */
int mnk_debug_stream_split(int kind, int num_cu, int dag_cus, int dag_cus2, int arg, int* split, int32_t* chain_mask, int32_t* rest_mask);
/* Rounds of a batch of small factorizations of `strips` 64-row strips each (host only): out[0] = the CUs the bulk kernel keeps at
 * least (0 without bulk tasks), out[1] = the systems of a round at most (< 2: no round), out[2] = the CUs of the chains' partition
 * for a round of k systems.  Returns 0, -1 on bad arguments. */
int mnk_debug_small_rounds(int strips, int num_cu, int has_bulk, int k, int* out);
/* Diagnostics (bench.py `clocks`): the shader clock the chip sustains under fp64 MFMA load right now, MHz (s_memtime against the
 * 100 MHz s_memrealtime over the second of two ~2.5 ms launches of MFMAs on every CU, on the context's stream). */
int mnk_debug_shader_clock(mnk_ctx* ctx, double* mhz);

/* Diagnostics / tests (host only): the task list of the task-DAG factorization schedule (csrc/dag_plan.hip) for a matrix of `ntile`
 * 128-row tiles: 4 ints per task (flags | chunk index << 8, tile row I, tile column J, kbeg | kend << 16) in queue order, at most
 * `cap` tasks written; returns the number of tasks (negative: bad arguments). */
int mnk_debug_dag_tasks(int ntile, int chunk, int band_tiles, int js2, int taper0, int* out, int cap, int* first_phase);
/* ... and the merged queue of a batch of `ninst` instances shifted by `period` tile columns of chain position (with the
 * zero-fill tasks of the next factorization's buffer if `fill`): the instance index sits in bits 16.. of the second int. */
int mnk_debug_dag_merged_tasks(int ntile, int chunk, int band_tiles, int js2, int taper0, int fill, int ninst, int period,
                               int* out, int cap);
/* ... and that list dealt into `nq` per-XCD queues per phase, as the bulk kernel of a single factorization pops them (options
 * dag_xcd_queues, dag_gang; ninst > 1: the merged list, one phase).  tasks_out: the list (4 ints per task); order: list positions,
 * queue after queue, first phase first; off: 2 x (nq + 1) offsets into `order`.  Returns the number of tasks. */
int mnk_debug_dag_deal(int ntile, int chunk, int band_tiles, int js2, int taper0, int fill, int ninst, int period, int nq, int gang,
                       int* tasks_out, int* order, int cap, int* off, int* first_phase);
/* The plan shape of that schedule for a padded order Np (a multiple of 64; host only): js2, the first strip-column (256 columns) from
 * which every remaining row is a 64-row strip of the pivot chain's deep band -- 0: from the first column on, ceil(Np / 256): never
 * (band + bulk kernel throughout).  dag_cus2: the CUs of the deep band's partition (0: there is none, js2 = ceil(Np / 256));
 * dag_deep_rows, js2_override: the options "dag_deep_rows" and "dag_js2" (negative: by size).  A js2 that would leave more than
 * dag_cus2 strips to the deep band is raised to ceil((Np - 64 dag_cus2) / 256).  Returns js2 (the statistic "dag_js2"), -1 on bad
 * arguments. */
int mnk_debug_dag_js2(int64_t Np, int dag_cus2, int64_t dag_deep_rows, int js2_override);

/* Diagnostics / tests (host only): the envelope per 128-row tile row that a solver of order `order` (<= the handle's n) uses when
 * it factors this KKT handle's condensed matrix: tile_env[I] = (first nonzero column over the rows of tile I) / 128, truncated to
 * the (order + 127) / 128 tiles of that order.  At most `cap` entries written; returns the number of tiles (negative: bad arguments). */
int mnk_sc_debug_tile_env(mnk_sc* sc, int64_t order, int32_t* out, int cap);
/* ... and the one mnk_ls_factorize_csc derives from a lower CSC matrix of order n. */
int mnk_debug_tile_env_csc(int64_t n, const int32_t* colptr, const int32_t* rowval, int index_base, int32_t* out, int cap);
/* The same per 64-row HALF of a tile row, in 64-column units (option "envelope_half" of a linear solver, default 1, ignored with
 * "envelope" = 0: the waves of a bulk chunk skip the k-tiles left of the envelopes of their own halves and the upper quadrant of a
 * diagonal tile): two entries per tile row, envh[2I] and envh[2I + 1]; tile_env[I] = min(envh[2I], envh[2I + 1]) / 2.  Returns the
 * number of halves, 2 * ((order + 127) / 128). */
int mnk_sc_debug_tile_envh(mnk_sc* sc, int64_t order, int32_t* out, int cap);
int mnk_debug_tile_envh_csc(int64_t n, const int32_t* colptr, const int32_t* rowval, int index_base, int32_t* out, int cap);
/* The statistics "envh_ksteps" (count[0]) and "envh_ksteps_skipped" (count[1]) of mnk_ls_get_stat for the task list of `ntile`
 * tiles: half-tile k-steps (a 64 x 64 quadrant of a tile over 64 columns) that the tile envelope `env` leaves of the bulk tasks /
 * of them skipped with the half-tile envelope `envh` (NULL: none).  Returns the number of tasks. */
int mnk_debug_envh_ksteps(int ntile, int chunk, int band_tiles, int js2, int taper0, const int* env, const int* envh, int64_t* count);
/* The schedule of the leading-block probe (option "probe") for a solver of order N over `n` verdicts (host only, no device is
 * opened): cols[i] is the column at which verdict i was rejected early, or -1 for an acceptance; orders[i] receives the order of the
 * leading block through which the matrix of verdict i would be probed first (0: no probe), i.e. before verdict i is noted. */
int mnk_debug_probe_schedule(int64_t N, int n, const int64_t* cols, int64_t* orders);
/* The steps of one factorization under the launch-per-panel schedules (option "panel_algo" 1 or 4; csrc/factor_plan.hip; host only,
 * no device is opened) for a padded order Np (a multiple of 64): 16 ints per step in the order of FactorStep's members (kind, stream,
 * col, n, rows, src, K, variant, slot, cus, whalf, wko, rhalf, rko, event, index), in the order the host enqueues them; at most `cap`
 * steps written.  shape[0] receives the number of outer panels, shape[1] whether the look-ahead streams are used (NULL: neither).
 * Returns the number of steps, -1 on bad arguments. */
int mnk_debug_factor_plan(int64_t Np, int ldl, int algo_now, int lookahead, int64_t outer_width, int64_t pp_fuse_rows, int share,
                          int small_tiles, int num_cu, int panel_cus, int32_t* out, int cap, int* shape);
/* How solve! would run for a solver described by plain numbers (csrc/solve_plan.hip; host only, no device is opened): padded order Np
 * (a multiple of 64), the context's CUs, and the flags of SolveShape (the factor is the pivoted tier's, options persistent_solve and
 * solve512, the 512-row inverses exist, the context is a CU partition, an abort is pending, debug_ps_missing is set, solve_trace is
 * on, LDL^T) plus option linv_mfma.  out[0] = the path as the statistic "solve_path" of mnk_ls_get_stat reports it (1: one launch
 * per 256-column step, 2: one launch over 256-column steps, 3: one launch over 512-column steps; 4, a system of a merged launch of a
 * solve batch, is never planned here; the statistic is 0 before the first solve), out[1] = the grid of a one-launch path (0:
 * stepwise), out[2] = a solve batch may queue it, out[3] = a solver of this order gets the 512-row inverses with solve512,
 * out[4] = the inverses of a batch of small factorizations come from one launch.  Returns 0, -1 on bad arguments. */
int mnk_debug_solve_plan(int64_t Np, int num_cu, int pivoted, int persistent_opt, int solve512_opt, int have_linv512, int partitioned,
                         int abort_raised, int debug_missing, int tracing, int ldl, int linv_mfma, int* out);
/* ... and a solve of `nrhs` right-hand sides with option multi_rhs_min (the same shape arguments, without linv_mfma): out[0] = the
 * path -- 5 (blocked, csrc/solve_multi.hip) exactly when the factor is not pivoted, multi_rhs_min > 0 and nrhs >= multi_rhs_min,
 * otherwise the path of every column of the column loop as mnk_debug_solve_plan gives it --, out[1] = the chunk width W (right-hand
 * sides per pass over the factor), out[2] = the chunks, out[3] = the padded width of the last chunk's working block (a multiple
 * of 16), out[4] = the grid of the column loop's one-launch path; out[1..3] are 0 for the column loop.  Returns 0, -1 on bad
 * arguments. */
int mnk_debug_solve_plan_multi(int64_t Np, int num_cu, int pivoted, int persistent_opt, int solve512_opt, int have_linv512, int partitioned,
                               int abort_raised, int debug_missing, int tracing, int ldl, int64_t nrhs, int64_t multi_rhs_min, int* out);
/* The launches a solve batch makes of `n` queued solves (in queue order: solver identity, device, padded order, LDL^T or not and the
 * CUs of its context): launch l runs the requests idx[begin[l] .. begin[l + 1]) with G[l] workgroups per system; a launch of one
 * request is an ordinary solve (G[l] = 0).  begin holds n + 1, idx and G n entries.  Returns the number of launches, -1 on bad
 * arguments. */
int mnk_debug_solve_batch_groups(int n, const int64_t* solver_id, const int32_t* device, const int64_t* Np, const int32_t* ldl,
                                 const int32_t* num_cu, int32_t* begin, int32_t* idx, int32_t* G);
/* What mnk_schur_set_structure would plan for a stage of `ns_local` scenarios of block order `blk` and `nd` design variables
 * (csrc/schur_plan.hip; host only, no device is opened): the pattern arguments of mnk_schur_set_structure, then the stage's three
 * numbers and the Gram row threshold T (negative: the default, INT64_MAX: never).  Runs the same checks and fills out[0..4] as
 * mnk_schur_assembly_stats does; cap >= 5.  Returns 0, or a negative value with the error string set. */
int mnk_debug_schur_assembly_plan(int64_t n, int64_t m, int64_t nv, int64_t nc, int64_t nnzh, const int32_t* hess_I,
                                  const int32_t* hess_J, int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t n_ineq,
                                  const int64_t* ind_ineq, int64_t n_eq, const int64_t* ind_eq, int index_base, int64_t ns_global,
                                  const int64_t* local_scen, int own_design, int64_t ns_local, int64_t blk, int64_t nd, int64_t T,
                                  int64_t* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MADNLP_HIP_H */

// What the sparse and the dense KKT units share (reference src/IPM/kernels.jl:161-204): the elementwise kernels of solve_kkt! /
// mul! (reduce_rhs!, finish_aug_solve!, the bound part of _kktmul!), the bound / barrier state of a handle with the entry points
// that only touch it, and the frames of solve_kkt! / mul! around each unit's matrix part.
#pragma once
#include <cstring>

#include "ls.h"

namespace mnk {

// ---- device-side solve_kkt! / mul! pieces (reference src/IPM/kernels.jl:161-204, factorization.jl:143-167,289-308)
// reduce_rhs!: xp_lr -= wl ./ l_diag (one launch per bound side: a variable may carry both bounds)
static __global__ void reduce_rhs_kernel(double* __restrict__ w, const int64_t* __restrict__ ind, const double* __restrict__ wb,
                                  const double* __restrict__ diag, int64_t nb) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < nb) w[ind[i]] -= wb[i] / diag[i];
}
// finish_aug_solve!: dlb = (-dlb + l_lower .* xp_lr) ./ l_diag ; dub = (dub - u_lower .* xp_ur) ./ u_diag
static __global__ void finish_aug_kernel(double* __restrict__ db, const double* __restrict__ w, const int64_t* __restrict__ ind,
                                  const double* __restrict__ lower, const double* __restrict__ diag, int64_t nb, int upper) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < nb) db[i] = upper ? (db[i] - lower[i] * w[ind[i]]) / diag[i] : (-db[i] + lower[i] * w[ind[i]]) / diag[i];
}
// _kktmul!, bound part.  side 0: xp_lr -= alpha dlb(x) ; dlb(w) = beta dlb(w) + alpha (x_lr l_lower - dlb(x) l_diag)
//                        side 1: xp_ur += alpha dub(x) ; dub(w) = beta dub(w) + alpha (x_ur u_lower + dub(x) u_diag)
static __global__ void kktmul_bound_kernel(double* __restrict__ w, double* __restrict__ wb, const double* __restrict__ x,
                                    const double* __restrict__ xb, const int64_t* __restrict__ ind,
                                    const double* __restrict__ lower, const double* __restrict__ diag, double alpha,
                                    double beta, int64_t nb, int upper) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int64_t p = ind[i];
    if (upper) {
        w[p] += alpha * xb[i];
        wb[i] = beta * wb[i] + alpha * (x[p] * lower[i] + xb[i] * diag[i]);
    } else {
        w[p] -= alpha * xb[i];
        wb[i] = beta * wb[i] + alpha * (x[p] * lower[i] - xb[i] * diag[i]);
    }
}

// ---- device-side feeders of build_kkt!: set_aug_diagonal! (reference src/IPM/kernels.jl:4-27) and
// regularize_diagonal! (src/KKT/KKTsystem.jl:222-226), so that an iteration needs no host vector at all:
//   l_diag = xl_r - x_lr, l_lower = zl_r      (upper = 0)      u_diag = x_ur - xu_r, u_lower = zu_r     (upper = 1)
static __global__ void aug_terms_kernel(double* __restrict__ diag, double* __restrict__ lower, const double* __restrict__ x,
                                        const double* __restrict__ xb, const double* __restrict__ z,
                                        const int64_t* __restrict__ ind, int64_t nb, int upper) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int64_t p = ind[i];
    diag[i] = upper ? x[p] - xb[p] : xb[p] - x[p];
    lower[i] = z[p];
}
//   pr_diag[ind] -= lower ./ diag   (one launch per bound side: a variable may carry both bounds)
static __global__ void aug_diag_sub_kernel(double* __restrict__ pr_diag, const double* __restrict__ lower,
                                           const double* __restrict__ diag, const int64_t* __restrict__ ind, int64_t nb) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < nb) pr_diag[ind[i]] -= lower[i] / diag[i];
}
static __global__ void vec_fill2_kernel(double* __restrict__ a, double* __restrict__ b, double v, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) { a[i] = v; if (b) b[i] = v; }
}
static __global__ void vec_shift2_kernel(double* __restrict__ a, double* __restrict__ b, double v, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) { a[i] += v; if (b) b[i] += v; }
}

// ---- the bound / barrier state of a KKT handle (sparse condensed, dense condensed, dense augmented) and the entry points
// that touch nothing else.  The handles differ in their matrix; each unit's private struct embeds one KktVecState and passes
// its own sizes: npr = length of the primal block (n + m sparse, n + ns dense), npd = primal + dual length of w (n + 2m sparse,
// n + ns + m dense; the Schur handle: n + n_ineq and n + n_ineq + m).  `who` is the C entry point's name: errors read "<who>: ...",
// and where a message names another entry point of the same handle kind it takes the kind's prefix from who: the name up to its
// second underscore ("mnk_sc" / "mnk_dc" / "mnk_schur": kkt_pfx).
struct KktVecState {
    int64_t nlb = 0, nub = 0;
    DevBuf<int64_t> ind_lb, ind_ub;               // positions in the primal block [0, npr)
    DevBuf<double> reg, l_diag, u_diag, l_lower, u_lower;
    DevBuf<double> wdev, xdev;                    // staging of a host-resident w / x: npd + nlb + nub each
    DevBuf<double> feed;                          // staging of host iterates for kkt_set_aug_diagonal (5 * npr)
    bool have_bounds = false, have_terms = false, have_diag = false;
    DevBuf<double> saved_diag;                    // reg | pr_diag | du_diag of kkt_save_diagonals
    bool have_saved_diag = false;
};

static inline int kkt_pfx(const char* who) {
    const char* u = std::strchr(who + 4, '_');
    return u ? (int)(u - who) : (int)std::strlen(who);
}

#define KKT_REQUIRE(cond, ...) do { if (!(cond)) { mnk::set_error(__VA_ARGS__); return -1; } } while (0)

// What every entry point on this state starts with: a handle that has a context and its private struct (a sparse handle made
// without a context is host-only and has neither; `what` carries that wording), on the handle's device.
template <class Handle>
static inline int kkt_enter(Handle* h, bool args_ok, const char* who, const char* what) {
    KKT_REQUIRE(h && h->ctx && h->extra && args_ok, "%s: %s", who, what);
    MNK_HIP(hipSetDevice(h->ctx->device));
    return 0;
}

static inline int kkt_set_bounds(KktVecState& st, mnk_ctx* ctx, const char* who, int64_t npr, int64_t npd, int64_t nlb,
                                 const int64_t* ind_lb, int64_t nub, const int64_t* ind_ub, int index_base) {
    std::vector<int64_t> lb(nlb), ub(nub);
    for (int64_t i = 0; i < nlb; ++i) {
        lb[i] = ind_lb[i] - index_base;
        KKT_REQUIRE(lb[i] >= 0 && lb[i] < npr, "%s: lower-bound index out of range", who);
    }
    for (int64_t i = 0; i < nub; ++i) {
        ub[i] = ind_ub[i] - index_base;
        KKT_REQUIRE(ub[i] >= 0 && ub[i] < npr, "%s: upper-bound index out of range", who);
    }
    hipStream_t s = ctx->stream;
    const size_t lw = (size_t)(npd + nlb + nub);
    int rc = st.ind_lb.upload(lb, s);
    rc |= st.ind_ub.upload(ub, s);
    rc |= st.reg.alloc(npr);
    rc |= st.l_diag.alloc(nlb);
    rc |= st.l_lower.alloc(nlb);
    rc |= st.u_diag.alloc(nub);
    rc |= st.u_lower.alloc(nub);
    rc |= st.wdev.alloc(lw);
    rc |= st.xdev.alloc(lw);
    if (rc) return rc;
    st.nlb = nlb;
    st.nub = nub;
    st.have_bounds = true;
    return 0;
}

static inline int kkt_set_barrier_terms(KktVecState& st, mnk_ctx* ctx, const char* who, int64_t npr, const double* reg,
                                        const double* l_diag, const double* u_diag, const double* l_lower,
                                        const double* u_lower, int loc) {
    KKT_REQUIRE(st.have_bounds, "%s: call %.*s_set_bounds first", who, kkt_pfx(who), who);
    hipStream_t s = ctx->stream;
    auto put = [&](double* dst, const double* src, int64_t cnt) -> int {
        if (cnt <= 0) return 0;
        KKT_REQUIRE(src != nullptr, "%s: NULL vector", who);
        if (loc == MNK_DEVICE) MNK_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
        else MNK_HIP(mnk::h2d_copy(dst, src, cnt * sizeof(double), s));
        return 0;
    };
    int rc = put(st.reg.p, reg, npr);
    rc |= put(st.l_diag.p, l_diag, st.nlb);
    rc |= put(st.u_diag.p, u_diag, st.nub);
    rc |= put(st.l_lower.p, l_lower, st.nlb);
    rc |= put(st.u_lower.p, u_lower, st.nub);
    if (rc) return rc;
    if (loc != MNK_DEVICE) MNK_HIP(mnk::stream_wait(s));  // the host arrays may change after return
    st.have_terms = true;
    return 0;
}

// One view over the diagonal state of a KKT handle: the shared state plus the handle's own pr_diag / du_diag.
struct AugDiagView {
    mnk_ctx* ctx;
    KktVecState* st;
    int64_t npr, ndu, nlb, nub;  // lengths of pr_diag / du_diag / the bound sides
    double *reg, *pr_diag, *du_diag, *l_diag, *u_diag, *l_lower, *u_lower;
    const int64_t *ind_lb, *ind_ub;
    DevBuf<double>* feed;        // staging for host-resident iterates (5 * npr)
};

static inline int kkt_diag_view(AugDiagView& v, KktVecState& st, mnk_ctx* ctx, const char* who, int64_t npr, int64_t ndu,
                                double* pr_diag, double* du_diag) {
    KKT_REQUIRE(st.have_bounds, "%s: call %.*s_set_bounds first", who, kkt_pfx(who), who);
    v = AugDiagView{ctx, &st, npr, ndu, st.nlb, st.nub, st.reg.p, pr_diag, du_diag, st.l_diag.p,
                    st.u_diag.p, st.l_lower.p, st.u_lower.p, st.ind_lb.p, st.ind_ub.p, &st.feed};
    return 0;
}

#define MNK_G1(cnt) dim3((unsigned)(((cnt) + 255) / 256)), dim3(256), 0, s
// _set_aug_diagonal! (reference src/IPM/kernels.jl:22-27), the tail of both feeders below: the bound terms from device vectors
// and their share of pr_diag; the handle then has its terms and its diagonals.
static inline int kkt_bound_terms(const AugDiagView& v, const double* x, const double* xl, const double* xu, const double* zl,
                                  const double* zu) {
    hipStream_t s = v.ctx->stream;
    if (v.nlb > 0) {
        hipLaunchKernelGGL(aug_terms_kernel, MNK_G1(v.nlb), v.l_diag, v.l_lower, x, xl, zl, v.ind_lb, v.nlb, 0);
        hipLaunchKernelGGL(aug_diag_sub_kernel, MNK_G1(v.nlb), v.pr_diag, v.l_lower, v.l_diag, v.ind_lb, v.nlb);
    }
    if (v.nub > 0) {
        hipLaunchKernelGGL(aug_terms_kernel, MNK_G1(v.nub), v.u_diag, v.u_lower, x, xu, zu, v.ind_ub, v.nub, 1);
        hipLaunchKernelGGL(aug_diag_sub_kernel, MNK_G1(v.nub), v.pr_diag, v.u_lower, v.u_diag, v.ind_ub, v.nub);
    }
    MNK_HIP(hipGetLastError());
    v.st->have_terms = v.st->have_diag = true;
    return 0;
}

static inline int kkt_set_aug_diagonal(const AugDiagView& v, const char* who, const double* x, const double* xl,
                                       const double* xu, const double* zl, const double* zu, double primal_reg,
                                       double dual_reg, int loc) {
    KKT_REQUIRE(x && xl && xu && zl && zu, "%s: NULL vector", who);
    hipStream_t s = v.ctx->stream;
    const double* in[5] = {x, xl, xu, zl, zu};
    if (loc != MNK_DEVICE) {
        if (v.feed->n < (size_t)(5 * v.npr)) {
            int rc = v.feed->alloc((size_t)(5 * v.npr));
            if (rc) return rc;
        }
        for (int k = 0; k < 5; ++k) {
            MNK_HIP(mnk::h2d_copy(v.feed->p + k * v.npr, in[k], v.npr * sizeof(double), s));
            in[k] = v.feed->p + k * v.npr;
        }
        MNK_HIP(mnk::stream_wait(s));  // the caller's arrays are only valid for the duration of the call
    }
    hipLaunchKernelGGL(vec_fill2_kernel, MNK_G1(v.npr), v.reg, v.pr_diag, primal_reg, v.npr);
    if (v.ndu > 0) hipLaunchKernelGGL(vec_fill2_kernel, MNK_G1(v.ndu), v.du_diag, (double*)nullptr, -dual_reg, v.ndu);
    return kkt_bound_terms(v, in[0], in[1], in[2], in[3], in[4]);
}

// set_aug_RR! (reference src/IPM/kernels.jl:72-87) + _set_aug_diagonal! (:22-27): the robust restorer's diagonals from
// DEVICE-resident vectors: reg = primal_reg + zeta D_R^2, du_diag = -dual_reg - pp/zp - nn/zn, bound terms as above.
static __global__ void rr_reg_kernel(double* __restrict__ reg, double* __restrict__ pr_diag, const double* __restrict__ D,
                                     double primal_reg, double zeta, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = primal_reg + zeta * (D[i] * D[i]);
    reg[i] = v;
    pr_diag[i] = v;
}
static __global__ void rr_du_kernel(double* __restrict__ du_diag, const double* __restrict__ pp, const double* __restrict__ zp,
                                    const double* __restrict__ nn, const double* __restrict__ zn, double dual_reg, int64_t m) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < m) du_diag[i] = -dual_reg - pp[i] / zp[i] - nn[i] / zn[i];
}
static inline int kkt_set_aug_RR(const AugDiagView& v, const char* who, const double* x, const double* xl, const double* xu,
                                 const double* zl, const double* zu, const double* D_R, const double* pp, const double* zp,
                                 const double* nn, const double* zn, double zeta, double primal_reg, double dual_reg) {
    KKT_REQUIRE(x && xl && xu && zl && zu && D_R && (v.ndu == 0 || (pp && zp && nn && zn)), "%s: NULL vector", who);
    hipStream_t s = v.ctx->stream;
    hipLaunchKernelGGL(rr_reg_kernel, MNK_G1(v.npr), v.reg, v.pr_diag, D_R, primal_reg, zeta, v.npr);
    if (v.ndu > 0) hipLaunchKernelGGL(rr_du_kernel, MNK_G1(v.ndu), v.du_diag, pp, zp, nn, zn, dual_reg, v.ndu);
    return kkt_bound_terms(v, x, xl, xu, zl, zu);
}

static inline int kkt_regularize_diagonal(const AugDiagView& v, const char* who, double primal, double dual) {
    KKT_REQUIRE(v.st->have_diag, "%s: call %.*s_set_aug_diagonal first", who, kkt_pfx(who), who);
    hipStream_t s = v.ctx->stream;
    hipLaunchKernelGGL(vec_shift2_kernel, MNK_G1(v.npr), v.reg, v.pr_diag, primal, v.npr);
    if (v.ndu > 0) hipLaunchKernelGGL(vec_shift2_kernel, MNK_G1(v.ndu), v.du_diag, (double*)nullptr, -dual, v.ndu);
    MNK_HIP(hipGetLastError());
    return 0;
}

static inline int kkt_get_diagonals(const AugDiagView& v, double* pr_diag, double* du_diag, double* reg, double* l_diag,
                                    double* u_diag, double* l_lower, double* u_lower) {
    hipStream_t s = v.ctx->stream;
    auto get = [&](double* dst, const double* src, int64_t n) -> int {
        if (dst && n > 0) MNK_HIP(mnk::d2h_copy(dst, src, n * sizeof(double), s));
        return 0;
    };
    int rc = get(pr_diag, v.pr_diag, v.npr) | get(du_diag, v.du_diag, v.ndu) | get(reg, v.reg, v.npr) |
             get(l_diag, v.l_diag, v.nlb) | get(u_diag, v.u_diag, v.nub) | get(l_lower, v.l_lower, v.nlb) |
             get(u_lower, v.u_lower, v.nub);
    if (rc) return rc;
    MNK_HIP(mnk::stream_wait(s));
    return 0;
}
// reg, pr_diag and du_diag as they are, into a buffer of the state / back from it (device copies on the handle's stream): the
// bracket of a SPECULATIVE trial of inertia_correction! (madnlp_jl_amd.ipm_dev: the trial with the next perturbation is factorized
// together with the unperturbed one; when the unperturbed matrix is accepted after all, the diagonals return to the bits they had
// -- pr_diag + dw - dw would not)
static inline int kkt_save_diagonals(const AugDiagView& v, const char* who) {
    KktVecState& st = *v.st;
    KKT_REQUIRE(st.have_diag, "%s: call %.*s_set_aug_diagonal first", who, kkt_pfx(who), who);
    const size_t npr = (size_t)v.npr, ndu = (size_t)v.ndu;
    if (st.saved_diag.n < 2 * npr + ndu && st.saved_diag.alloc(2 * npr + ndu)) {
        const std::string why = mnk_last_error_string();   // (the allocation's own message: which hipMalloc failed and why)
        set_error("%s: no device memory for the saved diagonals: %s", who, why.c_str());
        return -1;
    }
    hipStream_t s = v.ctx->stream;
    MNK_HIP(hipMemcpyAsync(st.saved_diag.p, v.reg, npr * sizeof(double), hipMemcpyDeviceToDevice, s));
    MNK_HIP(hipMemcpyAsync(st.saved_diag.p + npr, v.pr_diag, npr * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (ndu > 0) MNK_HIP(hipMemcpyAsync(st.saved_diag.p + 2 * npr, v.du_diag, ndu * sizeof(double), hipMemcpyDeviceToDevice, s));
    st.have_saved_diag = true;
    return 0;
}

static inline int kkt_restore_diagonals(const AugDiagView& v, const char* who) {
    const KktVecState& st = *v.st;
    KKT_REQUIRE(st.have_saved_diag, "%s: nothing saved (%.*s_save_diagonals)", who, kkt_pfx(who), who);
    const size_t npr = (size_t)v.npr, ndu = (size_t)v.ndu;
    hipStream_t s = v.ctx->stream;
    MNK_HIP(hipMemcpyAsync(v.reg, st.saved_diag.p, npr * sizeof(double), hipMemcpyDeviceToDevice, s));
    MNK_HIP(hipMemcpyAsync(v.pr_diag, st.saved_diag.p + npr, npr * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (ndu > 0) MNK_HIP(hipMemcpyAsync(v.du_diag, st.saved_diag.p + 2 * npr, ndu * sizeof(double), hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---- the frames of solve_kkt! / mul! (reference src/IPM/factorization.jl:41-46,143-167,190-229,289-330): everything but the
// matrix.  A handle passes its middle as a lambda (inlined: nothing on this path allocates or calls through a pointer).
// solve_kkt!: reduce_rhs!, `middle(d)` on the device vector d (the condensed or reduced solve with `ls`), finish_aug_solve!.
template <class Middle>
static inline int kkt_solve_kkt(KktVecState& st, mnk_ctx* ctx, const char* who, mnk_ls* ls, int64_t npd, double* w, int loc,
                                Middle&& middle) {
    KKT_REQUIRE(st.have_bounds && st.have_terms, "%s: call %.*s_set_bounds / %.*s_set_barrier_terms / %.*s_build first", who,
                kkt_pfx(who), who, kkt_pfx(who), who, kkt_pfx(who), who);
    hipStream_t s = ctx->stream;
    const int64_t nlb = st.nlb, nub = st.nub, lw = npd + nlb + nub;
    // Host-resident caller: the host still owns `w` until the final copy-back, so a persistent solve that gave
    // up (abort word raised, solve.hip) is detected HERE, after the stream synchronization and before anything
    // is copied back, and the whole solve_kkt! is redone once with the stepwise solve.
    for (int attempt = 0; attempt < 2; ++attempt) {
        double* d = w;
        if (loc != MNK_DEVICE) {
            d = st.wdev.p;
            MNK_HIP(mnk::h2d_copy(d, w, lw * sizeof(double), s));
        }
        double *wl = d + npd, *wu = wl + nlb;
        if (nlb > 0) hipLaunchKernelGGL(reduce_rhs_kernel, MNK_G1(nlb), d, st.ind_lb.p, wl, st.l_diag.p, nlb);
        if (nub > 0) hipLaunchKernelGGL(reduce_rhs_kernel, MNK_G1(nub), d, st.ind_ub.p, wu, st.u_diag.p, nub);
        int rc = middle(d);
        if (rc) return rc;
        if (nlb > 0) hipLaunchKernelGGL(finish_aug_kernel, MNK_G1(nlb), wl, d, st.ind_lb.p, st.l_lower.p, st.l_diag.p, nlb, 0);
        if (nub > 0) hipLaunchKernelGGL(finish_aug_kernel, MNK_G1(nub), wu, d, st.ind_ub.p, st.u_lower.p, st.u_diag.p, nub, 1);
        MNK_HIP(hipGetLastError());
        if (loc == MNK_DEVICE) break;  // device-resident caller: mnk_ls_check_solve() reports an abort
        MNK_HIP(mnk::stream_wait(s));
        if (attempt == 0 && mnk_ls_take_solve_abort(ls)) continue;  // redo with the stepwise solve
        MNK_HIP(mnk::d2h_copy(w, d, lw * sizeof(double), s));
        break;
    }
    return 0;
}

// mul!: `matrix(dw, dx)` is the handle's part on the device vectors (Hessian / Jacobian products and its diagonal kernel), then
// the bound part of _kktmul!.
template <class Matrix>
static inline int kkt_mul(KktVecState& st, mnk_ctx* ctx, const char* who, int64_t npd, double* w, const double* x, double alpha,
                          double beta, int loc, Matrix&& matrix) {
    KKT_REQUIRE(st.have_bounds && st.have_terms, "%s: call %.*s_set_bounds / %.*s_set_barrier_terms first", who, kkt_pfx(who), who,
                kkt_pfx(who), who);
    hipStream_t s = ctx->stream;
    const int64_t nlb = st.nlb, nub = st.nub, lw = npd + nlb + nub;
    double* dw = w;
    const double* dx = x;
    if (loc != MNK_DEVICE) {
        dw = st.wdev.p;
        MNK_HIP(mnk::h2d_copy(st.wdev.p, w, lw * sizeof(double), s));
        MNK_HIP(mnk::h2d_copy(st.xdev.p, x, lw * sizeof(double), s));
        dx = st.xdev.p;
    }
    int rc = matrix(dw, dx);
    if (rc) return rc;
    if (nlb > 0)
        hipLaunchKernelGGL(kktmul_bound_kernel, MNK_G1(nlb), dw, dw + npd, dx, dx + npd, st.ind_lb.p, st.l_lower.p, st.l_diag.p,
                           alpha, beta, nlb, 0);
    if (nub > 0)
        hipLaunchKernelGGL(kktmul_bound_kernel, MNK_G1(nub), dw, dw + npd + nlb, dx, dx + npd + nlb, st.ind_ub.p, st.u_lower.p,
                           st.u_diag.p, alpha, beta, nub, 1);
    MNK_HIP(hipGetLastError());
    if (loc != MNK_DEVICE) {
        MNK_HIP(mnk::d2h_copy(w, dw, lw * sizeof(double), s));
    }
    return 0;
}
#undef MNK_G1

}  // namespace mnk

// Dense quasi-Newton Hessians on the device (mnk_dc_qn_*): hessian_approximation = BFGS / DampedBFGS of the dense KKT
// systems, reference src/quasi_newton.jl:72-206 (update!, init!).  The approximation B lives in the dense handle's Hessian
// buffer (mnk_dc::hess, n x n, column-major, ld = n), which mnk_dc_build reads; it is UPDATED there, never uploaded.
//
// The reference's update is dsymv 'L' + a few dots + two dsyr 'L' (three sweeps over the triangle and more).  Here one update is
//   1. qn_dots_kernel     (1 workgroup)  s'y, s's; the skip test (BFGS, s'y < 1e-8), the "first update" diagonal value
//   2. qn_symv_kernel     (tiles)        ONE read of the lower triangle: tile (I, J), I >= J, gives B_IJ s_J for bs_I and, off the
//                                        diagonal, B_IJ' s_I for bs_J; every tile STORES its two 64-vectors into its own slots of
//                                        a slab (slot k of destination block D: tile (D, k) for k <= D, tile (k, D) for k > D)
//   3. qn_bs_kernel       (n / 256)      bs = the slab's slots summed in the order k = 0, 1, ..; per-workgroup partials of s'bs
//   4. qn_scalars_kernel  (1 workgroup)  s'Bs, theta, r = theta y + (1 - theta) bs, r's, -1 / s'Bs, 1 / r's
//   5. qn_rank2_kernel    (tiles)        ONE read and ONE write of the lower triangle: B_ij = (B_ij - bs_i bs_j / s'Bs) + r_i r_j / r's
// so the algorithmic traffic is 1.5 x 8 n^2 bytes.  Every number a later kernel needs (the dots, the skip flag, theta, the
// reciprocals, the "instantiated" flag, the counters) stays in a scalar block on the device: the host only enqueues.  No
// floating-point atomics: every sum is taken in one fixed order, so an update is bitwise reproducible run to run.  The strict
// upper triangle of B is neither read nor written.
#pragma clang fp contract(off)

#include "ls.h"

namespace mnk {

constexpr int QT = 64;           // tile edge
constexpr int QN_MAX_GRID = 2048;

struct QnScal {
    double sy, ss, sbs, theta, rs, na1, a2, dval;   // s'y, s's, s'Bs, theta, r's, -1 / s'Bs, 1 / r's, value of a diagonal reset
    long long updates, skipped;
    int skip;      // this update is skipped (BFGS, s'y < 1e-8): the passes over the matrix return at once
    int reset;     // this update first overwrites the diagonal with dval (folded into the two passes: they read dval for B_ii)
    int inst;      // is_instantiated of the reference: an update has been performed (or the matrix was adopted)
    int kind;
};

// fixed-order sum of one value per thread of a 256-thread workgroup
__device__ inline double block_sum_256(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) sh[t] = sh[t] + sh[t + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// init!: rho0 by the Gilbert-Lemarechal rule (quasi_newton.jl:195-203); dval = 2 rho0
__global__ __launch_bounds__(256) void qn_init_scal_kernel(QnScal* __restrict__ sc, const double* __restrict__ g0, int64_t n,
                                                           double f0, int kind) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) a += g0[i] * g0[i];
    const double gg = block_sum_256(a, sh);
    if (threadIdx.x == 0) {
        double rho0;
        if (gg < 1.4901161193847656e-08) rho0 = 1.0;   // sqrt(eps)
        else if (f0 == 0.0) rho0 = 1.0 / gg;
        else rho0 = fabs(f0) / gg;
        QnScal z = {};
        z.dval = 2.0 * rho0;
        z.theta = 1.0;
        z.kind = kind;
        *sc = z;
    }
}
__global__ __launch_bounds__(256) void qn_adopt_scal_kernel(QnScal* __restrict__ sc, int kind) {
    if (threadIdx.x == 0) {
        QnScal z = {};
        z.theta = 1.0;
        z.kind = kind;
        z.inst = 1;
        *sc = z;
    }
}
// B = dval I (the whole buffer, as the reference's zeroed matrix with its diagonal set)
__global__ __launch_bounds__(256) void qn_fill_kernel(double* __restrict__ B, int64_t n, const QnScal* __restrict__ sc) {
    const double d = sc->dval;
    const int64_t total = n * n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
        B[e] = (e / n == e % n) ? d : 0.0;
}

// step 1
__global__ __launch_bounds__(256) void qn_dots_kernel(QnScal* __restrict__ sc, const double* __restrict__ s,
                                                      const double* __restrict__ y, int64_t n) {
    __shared__ double sh[256];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        a += s[i] * y[i];
        b += s[i] * s[i];
    }
    const double sy = block_sum_256(a, sh);
    const double ss = block_sum_256(b, sh);
    if (threadIdx.x == 0) {
        sc->sy = sy;
        sc->ss = ss;
        const bool skip = sc->kind == MNK_QN_BFGS && sy < 1e-8;
        sc->skip = skip ? 1 : 0;
        sc->reset = 0;
        if (skip) {
            sc->skipped += 1;
            sc->sbs = 0.0;
            sc->theta = 1.0;
            sc->rs = sy;
        } else {
            sc->updates += 1;
            if (!sc->inst) {     // Nocedal & Wright p. 143 (quasi_newton.jl:118-122)
                sc->dval = sy / ss;
                sc->reset = 1;
                sc->inst = 1;
            }
        }
    }
}

// tile t of the lower triangle in row-major order of (I, J), J <= I
__device__ inline void tile_of(int64_t t, int& I, int& J) {
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((int64_t)i * (i + 1) / 2 > t) --i;
    while ((int64_t)(i + 1) * (i + 2) / 2 <= t) ++i;
    I = i;
    J = (int)(t - (int64_t)i * (i + 1) / 2);
}

// The two rows r, r + 1 of column c a thread owns: one 16-byte access where the pair is inside the matrix, inside the lower
// triangle and 16-byte aligned (the buffer is, so (r + c n) even), else one access per entry that is.  Entries outside read 0.
__device__ inline void load_pair(const double* __restrict__ B, int64_t n, int64_t r, int64_t c, bool colok, bool reset,
                                 double dval, double& v0, double& v1) {
    v0 = v1 = 0.0;
    if (!colok) return;
    const int64_t e = r + c * n;
    if (r >= c && r + 1 < n && (e & 1) == 0) {
        const double2 v = *reinterpret_cast<const double2*>(B + e);
        v0 = v.x;
        v1 = v.y;
    } else {
        if (r >= c && r < n) v0 = B[e];
        if (r + 1 >= c && r + 1 < n) v1 = B[e + 1];
    }
    if (reset) {
        if (r == c) v0 = dval;
        if (r + 1 == c) v1 = dval;
    }
}

// step 2.  256 threads per 64 x 64 tile: thread (rp, cg) owns the rows 2 rp, 2 rp + 1 of the columns cg, cg + 8, ..: the 32 lanes
// of a half-wave read 512 contiguous bytes of a column.
__global__ __launch_bounds__(256) void qn_symv_kernel(const double* __restrict__ B, int64_t n, const double* __restrict__ s,
                                                      const QnScal* __restrict__ sc, double* __restrict__ slab, int nt) {
    if (sc->skip) return;
    __shared__ double rowp[8][QT];
    __shared__ double colp[QT];
    const bool reset = sc->reset != 0;
    const double dval = sc->dval;
    const int rp = threadIdx.x & 31, cg = threadIdx.x >> 5;
    const int64_t ntiles = (int64_t)nt * (nt + 1) / 2;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int I, J;
        tile_of(t, I, J);
        const int64_t r = (int64_t)I * QT + 2 * rp;
        const double s0 = r < n ? s[r] : 0.0, s1 = r + 1 < n ? s[r + 1] : 0.0;
        double v0[8], v1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t c = (int64_t)J * QT + cg + 8 * k;
            load_pair(B, n, r, c, c < n, reset, dval, v0[k], v1[k]);
        }
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t c = (int64_t)J * QT + cg + 8 * k;
            const double scv = c < n ? s[c] : 0.0;
            a0 += v0[k] * scv;
            a1 += v1[k] * scv;
            // the transposed contribution of the entries strictly below the diagonal
            double cv = (r > c ? v0[k] * s0 : 0.0) + (r + 1 > c ? v1[k] * s1 : 0.0);
            for (int off = 16; off > 0; off >>= 1) cv += __shfl_xor(cv, off);   // within the half-wave that owns the column
            if (rp == 0) colp[cg + 8 * k] = cv;
        }
        rowp[cg][2 * rp] = a0;
        rowp[cg][2 * rp + 1] = a1;
        __syncthreads();
        if (threadIdx.x < QT) {
            const int q = threadIdx.x;
            double rs = rowp[0][q];
#pragma unroll
            for (int g = 1; g < 8; ++g) rs += rowp[g][q];
            const int64_t ri = (int64_t)I * QT + q, ci = (int64_t)J * QT + q;
            if (I == J) {
                if (ri < n) slab[(int64_t)I * n + ri] = rs + colp[q];
            } else {
                if (ri < n) slab[(int64_t)J * n + ri] = rs;        // slot J of destination block I
                if (ci < n) slab[(int64_t)I * n + ci] = colp[q];   // slot I of destination block J
            }
        }
        __syncthreads();
    }
}

// step 3
__global__ __launch_bounds__(256) void qn_bs_kernel(double* __restrict__ bs, const double* __restrict__ slab, int nt, int64_t n,
                                                    const double* __restrict__ s, const QnScal* __restrict__ sc,
                                                    double* __restrict__ part) {
    if (sc->skip) return;
    __shared__ double sh[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0, p = 0.0;
    if (i < n) {
        for (int k = 0; k < nt; ++k) v += slab[(int64_t)k * n + i];
        bs[i] = v;
        p = s[i] * v;
    }
    const double tot = block_sum_256(p, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// step 4
__global__ __launch_bounds__(256) void qn_scalars_kernel(QnScal* __restrict__ sc, const double* __restrict__ part, int nblk,
                                                         const double* __restrict__ s, const double* __restrict__ y,
                                                         const double* __restrict__ bs, double* __restrict__ rv, int64_t n) {
    if (sc->skip) return;
    __shared__ double sh[256];
    __shared__ double sbs_sh;
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int b = 0; b < nblk; ++b) a += part[b];
        sbs_sh = a;
    }
    __syncthreads();
    const double sbs = sbs_sh, sy = sc->sy;
    double theta = 1.0;
    if (sc->kind == MNK_QN_DAMPED_BFGS && sy < 0.2 * sbs) theta = 0.8 * sbs / (sbs - sy);   // Nocedal & Wright, procedure 18.2
    const bool damped = sc->kind == MNK_QN_DAMPED_BFGS;
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double r = damped ? theta * y[i] + (1.0 - theta) * bs[i] : y[i];
        rv[i] = r;
        a += r * s[i];
    }
    const double rs = damped ? block_sum_256(a, sh) : sy;
    if (threadIdx.x == 0) {
        sc->sbs = sbs;
        sc->theta = theta;
        sc->rs = rs;
        sc->na1 = -(1.0 / sbs);
        sc->a2 = 1.0 / rs;
    }
}

// step 5 (same thread layout as step 2)
__global__ __launch_bounds__(256) void qn_rank2_kernel(double* __restrict__ B, int64_t n, const double* __restrict__ bs,
                                                       const double* __restrict__ rv, const QnScal* __restrict__ sc, int nt) {
    if (sc->skip) return;
    const bool reset = sc->reset != 0;
    const double dval = sc->dval, na1 = sc->na1, a2 = sc->a2;
    const int rp = threadIdx.x & 31, cg = threadIdx.x >> 5;
    const int64_t ntiles = (int64_t)nt * (nt + 1) / 2;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int I, J;
        tile_of(t, I, J);
        const int64_t r = (int64_t)I * QT + 2 * rp;
        const double b0 = r < n ? bs[r] : 0.0, b1 = r + 1 < n ? bs[r + 1] : 0.0;
        const double r0 = r < n ? rv[r] : 0.0, r1 = r + 1 < n ? rv[r + 1] : 0.0;
        double v0[8], v1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t c = (int64_t)J * QT + cg + 8 * k;
            load_pair(B, n, r, c, c < n, reset, dval, v0[k], v1[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t c = (int64_t)J * QT + cg + 8 * k;
            if (c >= n) continue;
            const double t1 = na1 * bs[c], t2 = a2 * rv[c];   // dsyr 'L': column c receives v * (alpha v[c])
            const double w0 = (v0[k] + b0 * t1) + r0 * t2;
            const double w1 = (v1[k] + b1 * t1) + r1 * t2;
            const int64_t e = r + c * n;
            if (r >= c && r + 1 < n && (e & 1) == 0) {
                *reinterpret_cast<double2*>(B + e) = make_double2(w0, w1);
            } else {
                if (r >= c && r < n) B[e] = w0;
                if (r + 1 >= c && r + 1 < n) B[e + 1] = w1;
            }
        }
    }
}

// The secant pair of the quasi-Newton method of eval_lag_hess_wrapper! (callbacks.jl:162-174, 184-186) in one launch:
// s = x - last_x ; y = ((g - last_g) + jl) - jv (the two Jacobian terms only when there are constraints) ; last_x = x ; last_g = g
__global__ __launch_bounds__(256) void qn_secant_kernel(const double* __restrict__ x, const double* __restrict__ g,
                                                        const double* __restrict__ jl, const double* __restrict__ jv,
                                                        double* __restrict__ last_x, double* __restrict__ last_g,
                                                        double* __restrict__ s, double* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double xi = x[i], gi = g[i];
        s[i] = xi - last_x[i];
        double yv = gi - last_g[i];
        if (jl != nullptr) yv = (yv + jl[i]) - jv[i];
        y[i] = yv;
        last_x[i] = xi;
        last_g[i] = gi;
    }
}

struct QnState {
    int kind = 0;
    int nt = 0, nblk = 0;
    DevBuf<QnScal> scal;
    DevBuf<double> slab, bs, rv, part;
};

}  // namespace mnk

using namespace mnk;

static QnState* qn_of(mnk_dc* dc) { return static_cast<QnState*>(dc->qn); }

void mnk_dc_qn_release(mnk_dc* dc) {
    delete qn_of(dc);
    dc->qn = nullptr;
}

extern "C" {

int mnk_dc_qn_init(mnk_dc* dc, int kind, const double* g0, double f0) {
    MNK_REQUIRE(dc, "mnk_dc_qn_init: NULL argument");
    MNK_REQUIRE(kind == MNK_QN_BFGS || kind == MNK_QN_DAMPED_BFGS, "mnk_dc_qn_init: kind must be MNK_QN_BFGS or MNK_QN_DAMPED_BFGS");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    hipStream_t s = dc->ctx->stream;
    const int64_t n = dc->n;
    QnState* q = qn_of(dc);
    if (q == nullptr) {
        q = new QnState();
        q->nt = (int)((n + QT - 1) / QT);
        q->nblk = (int)((n + 255) / 256);
        int rc = q->scal.alloc(1);
        rc |= q->slab.alloc((size_t)q->nt * n);
        rc |= q->bs.alloc(n);
        rc |= q->rv.alloc(n);
        rc |= q->part.alloc(q->nblk);
        if (rc) { delete q; return -2; }
        dc->qn = q;
    }
    q->kind = kind;
    if (g0 == nullptr) {
        hipLaunchKernelGGL(qn_adopt_scal_kernel, dim3(1), dim3(256), 0, s, q->scal.p, kind);
    } else {
        hipLaunchKernelGGL(qn_init_scal_kernel, dim3(1), dim3(256), 0, s, q->scal.p, g0, n, f0, kind);
        const int64_t blocks = std::min<int64_t>((n * n + 255) / 256, QN_MAX_GRID);
        dc->hess_dirty = true;
        hipLaunchKernelGGL(qn_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dc->hess.p, n, q->scal.p);
    }
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_dc_qn_update(mnk_dc* dc, const double* sk, const double* yk) {
    MNK_REQUIRE(dc && sk && yk, "mnk_dc_qn_update: NULL argument");
    QnState* q = qn_of(dc);
    MNK_REQUIRE(q != nullptr, "mnk_dc_qn_update: call mnk_dc_qn_init first");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    hipStream_t s = dc->ctx->stream;
    const int64_t n = dc->n;
    const int64_t ntiles = (int64_t)q->nt * (q->nt + 1) / 2;
    const unsigned tgrid = (unsigned)std::min<int64_t>(ntiles, QN_MAX_GRID);
    dc->hess_dirty = true;
    hipLaunchKernelGGL(qn_dots_kernel, dim3(1), dim3(256), 0, s, q->scal.p, sk, yk, n);
    hipLaunchKernelGGL(qn_symv_kernel, dim3(tgrid), dim3(256), 0, s, dc->hess.p, n, sk, q->scal.p, q->slab.p, q->nt);
    hipLaunchKernelGGL(qn_bs_kernel, dim3((unsigned)q->nblk), dim3(256), 0, s, q->bs.p, q->slab.p, q->nt, n, sk, q->scal.p,
                       q->part.p);
    hipLaunchKernelGGL(qn_scalars_kernel, dim3(1), dim3(256), 0, s, q->scal.p, q->part.p, q->nblk, sk, yk, q->bs.p, q->rv.p, n);
    hipLaunchKernelGGL(qn_rank2_kernel, dim3(tgrid), dim3(256), 0, s, dc->hess.p, n, q->bs.p, q->rv.p, q->scal.p, q->nt);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_dc_qn_secant(mnk_dc* dc, const double* x, const double* g, const double* jl, const double* jv, double* last_x,
                     double* last_g, double* sk, double* yk) {
    MNK_REQUIRE(dc && x && g && last_x && last_g && sk && yk, "mnk_dc_qn_secant: NULL argument");
    MNK_REQUIRE((jl == nullptr) == (jv == nullptr), "mnk_dc_qn_secant: jl and jv are given together or not at all");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    const int64_t blocks = std::min<int64_t>((dc->n + 255) / 256, QN_MAX_GRID);
    hipLaunchKernelGGL(qn_secant_kernel, dim3((unsigned)blocks), dim3(256), 0, dc->ctx->stream, x, g, jl, jv, last_x, last_g, sk, yk,
                       dc->n);
    MNK_HIP(hipGetLastError());
    return 0;
}

// the same launch for the sparse condensed handle (compact L-BFGS, lbfgs.hip)
int mnk_sc_qn_secant(mnk_sc* sc, const double* x, const double* g, const double* jl, const double* jv, double* last_x,
                     double* last_g, double* sk, double* yk) {
    MNK_REQUIRE(sc && sc->ctx && x && g && last_x && last_g && sk && yk, "mnk_sc_qn_secant: NULL argument or host-only handle");
    MNK_REQUIRE((jl == nullptr) == (jv == nullptr), "mnk_sc_qn_secant: jl and jv are given together or not at all");
    MNK_HIP(hipSetDevice(sc->ctx->device));
    const int64_t blocks = std::min<int64_t>((sc->n + 255) / 256, QN_MAX_GRID);
    hipLaunchKernelGGL(qn_secant_kernel, dim3((unsigned)blocks), dim3(256), 0, sc->ctx->stream, x, g, jl, jv, last_x, last_g, sk, yk,
                       sc->n);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_dc_qn_status(mnk_dc* dc, int64_t* updates, int64_t* skipped, double* last) {
    MNK_REQUIRE(dc, "mnk_dc_qn_status: NULL argument");
    QnState* q = qn_of(dc);
    MNK_REQUIRE(q != nullptr, "mnk_dc_qn_status: call mnk_dc_qn_init first");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    QnScal h;
    MNK_HIP(mnk::d2h_copy(&h, q->scal.p, sizeof(QnScal), dc->ctx->stream));
    if (updates) *updates = h.updates;
    if (skipped) *skipped = h.skipped;
    if (last) {
        last[0] = h.sy;
        last[1] = h.sbs;
        last[2] = h.theta;
        last[3] = h.rs;
    }
    return 0;
}

int mnk_dc_get_hess(mnk_dc* dc, double* out, int64_t ld, int loc) {
    MNK_REQUIRE(dc && out, "mnk_dc_get_hess: NULL argument");
    MNK_REQUIRE(ld >= dc->n, "mnk_dc_get_hess: leading dimension smaller than n");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    const size_t w = dc->n * sizeof(double);
    if (loc == MNK_DEVICE)
        MNK_HIP(hipMemcpy2DAsync(out, ld * sizeof(double), dc->hess.p, w, w, dc->n, hipMemcpyDeviceToDevice, dc->ctx->stream));
    else
        MNK_HIP(mnk::d2h_copy_2d(out, ld * sizeof(double), dc->hess.p, w, w, dc->n, dc->ctx->stream));
    return 0;
}

}  // extern "C"

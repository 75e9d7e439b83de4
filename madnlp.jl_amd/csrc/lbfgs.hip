// Compact L-BFGS Hessians of the sparse condensed KKT system on the device (mnk_lbfgs_*): hessian_approximation = CompactLBFGS,
// reference src/quasi_newton.jl:210-437 (update!, init!) and the Sherman-Morrison-Woodbury solve of
// src/IPM/factorization.jl:76-140, applied here around the CONDENSED matrix:
//     K = C + E P E',   C = xi I + Sigma_x + J' D J (what the linear solver factors),   E = [U V],   P = diag(-I_p, I_p),
//     K^-1 r = C^-1 r - H W E' C^-1 r,   H = C^-1 E,   T = P + E' H,   W = T^-1.
// Everything of length n lives in the handle: the history S, Y (a ring of max_history columns), E = [U V], H.  Host mirror:
// madnlp.jl_amd/quasi_newton.py (CompactLBFGS, gram, lowrank_apply), kkt.LowRankHessianKKT.
//
// update!:  lb_dots_kernel + lb_final_kernel   all ordered dot products (s's, s'y, y'y, S's, Y's) -> pinned host memory, ONE
//                                              synchronization; 16 (1 + p) n bytes read
//           host (C++, O(p^3))                 skip / reset, S'S and L grown by a row, D, sigma, M, its Cholesky factor and the
//                                              coefficients of U = S A1 + Y A2, V = Y D^-1/2 (copied from pinned memory, no wait)
//           lb_uv_kernel                       stores the pair into its ring slot and writes E = [U V] and P; 16 p n bytes read,
//                                              16 p n written (the history is read p times per row from L1 / L2)
// per factorization (or performed / resetting update), in front of the first solve_kkt!:
//           copy E -> H, mnk_ls_solve(H, 2p)   the blocked multi-right-hand-side solve from 2p >= 4 (solve_multi.hip)
//           lb_gram_kernel + lb_tfinal_kernel  T = P + E'H: (2p)^2 ordered sums, 8 (1 + 8) n bytes per 8 of them
//           lb_invert_kernel                   W = T^-1: LU with partial pivoting in LDS, one workgroup; a zero pivot raises the flag
// per solve_kkt! / mul!:
//           lb_gram_kernel                     t = E'w_x (2p ordered sums, partials in device memory); 8 (2p + 1) n bytes read
//           lb_apply_kernel                    w_x += alpha A (M t) with (A, M, alpha) = (H, W, -1) or (E, P, alpha); every workgroup
//                                              adds the partials itself; 8 (2p + 2) n bytes moved
// Ordinary grid launches on the context's stream with the lane mapping of krylov.hip: element i belongs to lane i mod 65536
// (IPM_BLOCKS x IPM_THREADS), a lane adds its terms in increasing i, lanes and blocks are added by halving trees: every sum has
// the bits of `ordered_sum` (ipm.py).  Workgroups that would own no element are not launched; their partials count as zero,
// which is what they would have stored.  No atomics, no FMA contraction: a call is bitwise reproducible.
#pragma clang fp contract(off)
#include <cmath>

#include "ipm_handle.h"
#include "ls.h"

namespace mnk {

constexpr int LB_MAX_HIST = 32;               // max_history: E's 2p <= 64 columns are one chunk of the blocked solve
constexpr int LB_MAX_Q = 2 * LB_MAX_HIST;
constexpr int LB_TILE = 8;                    // dot products per workgroup
constexpr int LB_MAX_DOTS = 72;               // 3 + 2 LB_MAX_HIST, rounded up to LB_TILE
static_assert(IPM_BLOCKS == IPM_THREADS, "the final tree adds one partial per thread");

struct LbDotList {
    const double* a[LB_MAX_DOTS];
    const double* b[LB_MAX_DOTS];
    int count;
};

__device__ __forceinline__ double lb_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = IPM_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// part[pair * IPM_BLOCKS + block] = the block's share of a_pair . b_pair ; grid (blocks, ceil(count / LB_TILE))
__global__ __launch_bounds__(IPM_THREADS) void lb_dots_kernel(LbDotList dl, int64_t n, double* __restrict__ part) {
    __shared__ double sh[IPM_THREADS];
    const int p0 = blockIdx.y * LB_TILE;
    const int cnt = min(LB_TILE, dl.count - p0);
    double acc[LB_TILE];
#pragma unroll
    for (int k = 0; k < LB_TILE; ++k) acc[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS) {
#pragma unroll
        for (int k = 0; k < LB_TILE; ++k)
            if (k < cnt) acc[k] += dl.a[p0 + k][i] * dl.b[p0 + k][i];
    }
#pragma unroll
    for (int k = 0; k < LB_TILE; ++k) {
        if (k < cnt) {   // (cnt is uniform)
            const double r = lb_block_sum(acc[k], sh);
            if (threadIdx.x == 0) part[(int64_t)(p0 + k) * IPM_BLOCKS + blockIdx.x] = r;
        }
    }
}

// part[(i qb + j) * IPM_BLOCKS + block] = the block's share of A_i . B_j ; grid (blocks, qa, ceil(qb / LB_TILE))
__global__ __launch_bounds__(IPM_THREADS) void lb_gram_kernel(const double* __restrict__ A, int64_t lda,
                                                               const double* __restrict__ B, int64_t ldb, int qb, int64_t n,
                                                               double* __restrict__ part) {
    __shared__ double sh[IPM_THREADS];
    const int ia = blockIdx.y, j0 = blockIdx.z * LB_TILE;
    const int cnt = min(LB_TILE, qb - j0);
    const double* a = A + (int64_t)ia * lda;
    double acc[LB_TILE];
#pragma unroll
    for (int k = 0; k < LB_TILE; ++k) acc[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS) {
        const double ai = a[i];
#pragma unroll
        for (int k = 0; k < LB_TILE; ++k)
            if (k < cnt) acc[k] += ai * B[(int64_t)(j0 + k) * ldb + i];
    }
#pragma unroll
    for (int k = 0; k < LB_TILE; ++k) {
        if (k < cnt) {
            const double r = lb_block_sum(acc[k], sh);
            if (threadIdx.x == 0) part[((int64_t)ia * qb + j0 + k) * IPM_BLOCKS + blockIdx.x] = r;
        }
    }
}

// block `pair`: out[pair] = the halving tree over the partials of the nblk launched blocks (the others count as zero)
__global__ __launch_bounds__(IPM_THREADS) void lb_final_kernel(const double* __restrict__ part, int nblk,
                                                                double* __restrict__ out) {
    __shared__ double sh[IPM_THREADS];
    const double v = (int)threadIdx.x < nblk ? part[(int64_t)blockIdx.x * IPM_BLOCKS + threadIdx.x] : 0.0;
    const double r = lb_block_sum(v, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// block i q + j: T[i + q j] = P[i + q j] + (E_i . H_j), the sum from its partials as above
__global__ __launch_bounds__(IPM_THREADS) void lb_tfinal_kernel(const double* __restrict__ part, int nblk, int q,
                                                                 const double* __restrict__ Pm, double* __restrict__ T) {
    __shared__ double sh[IPM_THREADS];
    const double v = (int)threadIdx.x < nblk ? part[(int64_t)blockIdx.x * IPM_BLOCKS + threadIdx.x] : 0.0;
    const double r = lb_block_sum(v, sh);
    if (threadIdx.x == 0) {
        const int i = blockIdx.x / q, j = blockIdx.x % q;
        T[i + q * j] = Pm[i + q * j] + r;
    }
}

// y[i] += alpha sum_j A[i, j] c[j],  c = M t,  t[j] = the tree over part[j * IPM_BLOCKS + .]  (q <= LB_MAX_Q; M column-major).
// `flag` != NULL and *flag != 0 (the T behind M = W was singular): y is left alone.
__global__ __launch_bounds__(IPM_THREADS) void lb_apply_kernel(double* __restrict__ y, double alpha, const double* __restrict__ A,
                                                                int64_t lda, const double* __restrict__ M, int q,
                                                                const double* __restrict__ part, int nblk, int64_t n,
                                                                const int* __restrict__ flag) {
    __shared__ double sh[LB_TILE][IPM_THREADS];
    __shared__ double t[LB_MAX_Q], c[LB_MAX_Q];
    if (flag != nullptr && *flag != 0) return;
    const int tid = threadIdx.x;
    for (int j0 = 0; j0 < q; j0 += LB_TILE) {
#pragma unroll
        for (int k = 0; k < LB_TILE; ++k) sh[k][tid] = (j0 + k < q && tid < nblk) ? part[(int64_t)(j0 + k) * IPM_BLOCKS + tid] : 0.0;
        __syncthreads();
        for (int s = IPM_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int k = 0; k < LB_TILE; ++k) sh[k][tid] = sh[k][tid] + sh[k][tid + s];
            }
            __syncthreads();
        }
        if (tid < LB_TILE && j0 + tid < q) t[j0 + tid] = sh[tid][0];
        __syncthreads();
    }
    if (tid < q) {
        double a = 0.0;
        for (int j = 0; j < q; ++j) a = a + M[tid + q * j] * t[j];
        c[tid] = a;
    }
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + tid; i < n; i += (int64_t)gridDim.x * IPM_THREADS) {
        double a = 0.0;
        for (int j = 0; j < q; ++j) a = a + A[(int64_t)j * lda + i] * c[j];
        y[i] = y[i] + alpha * a;
    }
}

// W = T^-1 (q x q, column-major, q <= LB_MAX_Q): LU with partial pivoting in LDS by one workgroup, then thread j solves for
// column j.  A pivot that is zero (or NaN) stops the elimination: *flag_dev = 1 and the pinned word *flag_pin = 1, W is not
// written; otherwise *flag_dev = 0.
__global__ __launch_bounds__(IPM_THREADS) void lb_invert_kernel(const double* __restrict__ T, double* __restrict__ W, int q,
                                                                 int* __restrict__ flag_dev, int* __restrict__ flag_pin) {
    __shared__ double a[LB_MAX_Q * LB_MAX_Q];
    __shared__ int piv[LB_MAX_Q];
    __shared__ int sing;
    const int tid = threadIdx.x;
    for (int e = tid; e < q * q; e += IPM_THREADS) a[e] = T[e];
    if (tid == 0) sing = 0;
    __syncthreads();
    for (int k = 0; k < q; ++k) {
        if (tid == 0) {
            int p = k;
            double best = fabs(a[k + q * k]);
            for (int r = k + 1; r < q; ++r) {
                const double v = fabs(a[r + q * k]);
                if (v > best) { best = v; p = r; }
            }
            piv[k] = p;
            if (!(best > 0.0)) sing = 1;
        }
        __syncthreads();
        if (sing) break;   // (shared: every thread leaves)
        const int p = piv[k];
        if (p != k && tid < q) {
            const double v = a[k + q * tid];
            a[k + q * tid] = a[p + q * tid];
            a[p + q * tid] = v;
        }
        __syncthreads();
        const double d = a[k + q * k];
        for (int r = k + 1 + tid; r < q; r += IPM_THREADS) a[r + q * k] = a[r + q * k] / d;
        __syncthreads();
        const int w = q - k - 1;
        for (int e = tid; e < w * w; e += IPM_THREADS) {
            const int r = k + 1 + e % w, cc = k + 1 + e / w;
            a[r + q * cc] = a[r + q * cc] - a[r + q * k] * a[k + q * cc];
        }
        __syncthreads();
    }
    if (sing) {
        if (tid == 0) {
            *flag_dev = 1;
            __hip_atomic_store(flag_pin, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (tid == 0) *flag_dev = 0;
    if (tid < q) {
        double* x = W + (int64_t)q * tid;   // column tid of the inverse: L U x = (row swaps) e_tid
        int pos = tid;
        for (int k = 0; k < q; ++k) {
            if (pos == k) pos = piv[k];
            else if (pos == piv[k]) pos = k;
        }
        for (int r = 0; r < q; ++r) {
            double v = r == pos ? 1.0 : 0.0;
            for (int cc = 0; cc < r; ++cc) v = v - a[r + q * cc] * x[cc];
            x[r] = v;
        }
        for (int r = q - 1; r >= 0; --r) {
            double v = x[r];
            for (int cc = r + 1; cc < q; ++cc) v = v - a[r + q * cc] * x[cc];
            x[r] = v / a[r + q * r];
        }
    }
}

// The accepted pair goes into ring slot `slot`, then E = [U V] with U = S A1 + Y A2 (columns of S, then of Y, in the order of
// the history) and V_c = Y_c delta_c; block 0 also writes P = diag(-I_k, I_k).  coef: A1 (k x k, column-major) | A2 | delta (k) |
// the ring slots of the k pairs, oldest first (as doubles).  S and Y are read after this thread's own store.
__global__ __launch_bounds__(IPM_THREADS) void lb_uv_kernel(double* S, double* Y, int64_t ld, const double* __restrict__ s,
                                                             const double* __restrict__ y, int slot, int k,
                                                             const double* __restrict__ coef, double* __restrict__ E,
                                                             double* __restrict__ Pm, int64_t n) {
    __shared__ double A1[LB_MAX_HIST * LB_MAX_HIST], A2[LB_MAX_HIST * LB_MAX_HIST], dl[LB_MAX_HIST];
    __shared__ int ph[LB_MAX_HIST];
    const int tid = threadIdx.x;
    for (int e = tid; e < k * k; e += IPM_THREADS) {
        A1[e] = coef[e];
        A2[e] = coef[k * k + e];
    }
    if (tid < k) {
        dl[tid] = coef[2 * k * k + tid];
        ph[tid] = (int)coef[2 * k * k + k + tid];
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        const int q = 2 * k;
        for (int e = tid; e < q * q; e += IPM_THREADS) {
            const int r = e % q, cc = e / q;
            Pm[e] = r != cc ? 0.0 : (r < k ? -1.0 : 1.0);
        }
    }
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + tid; i < n; i += (int64_t)gridDim.x * IPM_THREADS) {
        S[(int64_t)slot * ld + i] = s[i];
        Y[(int64_t)slot * ld + i] = y[i];
        for (int cc = 0; cc < k; ++cc) {
            double u = 0.0;
            for (int j = 0; j < k; ++j) u = u + S[(int64_t)ph[j] * ld + i] * A1[j + k * cc];
            for (int j = 0; j < k; ++j) u = u + Y[(int64_t)ph[j] * ld + i] * A2[j + k * cc];
            E[(int64_t)cc * ld + i] = u;
            E[(int64_t)(k + cc) * ld + i] = Y[(int64_t)ph[cc] * ld + i] * dl[cc];
        }
    }
}

inline int lb_blocks(int64_t n) { return (int)std::min<int64_t>(IPM_BLOCKS, (n + IPM_THREADS - 1) / IPM_THREADS); }

}  // namespace mnk

using namespace mnk;

struct mnk_lbfgs {
    mnk_ctx* ctx = nullptr;
    int64_t n = 0, ld = 0;
    int pmax = 0, strategy = 1;
    double init_value = 1.0, sigma_min = 1e-8, sigma_max = 1e8, sigma = 0.0;
    // the history: `cur` pairs, the oldest in ring slot `head`; S'S, tril(S'Y, -1) and diag(S'Y) in the order of the history
    int cur = 0, head = 0, skipped_iter = 0;
    std::vector<double> StS, L, D;
    int64_t updates = 0, skipped = 0, resets = 0, builds = 0, singular = 0, version = 0;
    DevBuf<double> S, Y, E, H;            // ld x pmax, ld x pmax, ld x 2 pmax, ld x 2 pmax
    DevBuf<double> Pm, T, W, coef, res;   // (2 pmax)^2 each; 2 pmax^2 + 2 pmax; LB_MAX_DOTS
    DevBuf<double> part;                  // (2 pmax)^2 x IPM_BLOCKS partials
    DevBuf<int> flag;                     // the T behind W was singular (what lb_apply_kernel reads)
    double* pin = nullptr;                // pinned: LB_MAX_DOTS results | the coefficient block | the singular-T word
    int* pin_flag = nullptr;
    // what H, T, W were built for: the solver, its factorization, its solve path, this object's version
    const mnk_ls* key_ls = nullptr;
    int64_t key_serial = -1, key_version = -1;
    int key_persistent = -1;
    bool key_valid = false;
    size_t coef_words() const { return (size_t)2 * pmax * pmax + 2 * pmax; }
    int slot_of(int j) const { return (head + j) % pmax; }
    void reset() {
        cur = head = skipped_iter = 0;
        ++resets;
        ++version;
    }
};

// the count dot products of `dl` -> qn->pin[0 .. count), complete on return (the one synchronization of init! / update!)
static int lb_dots(mnk_lbfgs* qn, const LbDotList& dl) {
    hipStream_t s = qn->ctx->stream;
    const int nblk = lb_blocks(qn->n);
    hipLaunchKernelGGL(lb_dots_kernel, dim3(nblk, (dl.count + LB_TILE - 1) / LB_TILE), dim3(IPM_THREADS), 0, s, dl, qn->n,
                       qn->part.p);
    hipLaunchKernelGGL(lb_final_kernel, dim3(dl.count), dim3(IPM_THREADS), 0, s, qn->part.p, nblk, qn->res.p);
    MNK_HIP(hipGetLastError());
    MNK_HIP(hipMemcpyAsync(qn->pin, qn->res.p, dl.count * sizeof(double), hipMemcpyDeviceToHost, s));
    MNK_HIP(mnk::stream_wait(s));
    return 0;
}

// t = B'x into the partials, then y += alpha A (M t): the pair of launches behind solve_kkt!, mul! and mnk_lbfgs_apply
static int lb_apply(mnk_lbfgs* qn, double* y, double alpha, const double* A, int64_t lda, const double* M, const double* B,
                    int64_t ldb, const double* x, int q, int64_t n, const int* flag) {
    hipStream_t s = qn->ctx->stream;
    const int nblk = lb_blocks(n);
    hipLaunchKernelGGL(lb_gram_kernel, dim3(nblk, 1, (q + LB_TILE - 1) / LB_TILE), dim3(IPM_THREADS), 0, s, x, n, B, ldb, q, n,
                       qn->part.p);
    hipLaunchKernelGGL(lb_apply_kernel, dim3(nblk), dim3(IPM_THREADS), 0, s, y, alpha, A, lda, M, q, qn->part.p, nblk, n, flag);
    MNK_HIP(hipGetLastError());
    return 0;
}

int64_t mnk_lbfgs_order(const mnk_lbfgs* qn) { return qn->n; }

int mnk_lbfgs_check(mnk_lbfgs* qn, const char* who) {
    if (qn->pin_flag != nullptr && *(volatile int*)qn->pin_flag != 0) {
        set_error("%s: T = P + E' C^-1 E of the compact L-BFGS correction is singular (zero pivot): the low-rank term was not "
                  "applied", who);
        return -4;
    }
    return 0;
}

int mnk_lbfgs_solve_correct(mnk_lbfgs* qn, mnk_ls* ls, double* wx) {
    if (qn->cur == 0) return 0;
    MNK_REQUIRE(ls->N == qn->n, "mnk_sc_solve_kkt: the attached compact L-BFGS handle has another order than the solver");
    { int rc_q = mnk_solve_sync_deferred(ls); if (rc_q) return rc_q; }   // (a solve batch of this thread may hold the solve of wx)
    hipStream_t s = qn->ctx->stream;
    const int q = 2 * qn->cur;
    const bool same = qn->key_valid && qn->key_ls == ls && qn->key_serial == ls->verdict.serial &&
                      qn->key_persistent == ls->solves.persistent_solve && qn->key_version == qn->version;
    if (same) {
        int rc = mnk_lbfgs_check(qn, "mnk_sc_solve_kkt");
        if (rc) return rc;
    } else {
        *(volatile int*)qn->pin_flag = 0;
        qn->key_valid = false;
        MNK_HIP(hipMemcpyAsync(qn->H.p, qn->E.p, (size_t)q * qn->ld * sizeof(double), hipMemcpyDeviceToDevice, s));
        int rc = mnk_ls_solve(ls, qn->H.p, q, qn->ld, MNK_DEVICE);   // H = C^-1 E
        if (rc) return rc;
        const int nblk = lb_blocks(qn->n);
        hipLaunchKernelGGL(lb_gram_kernel, dim3(nblk, q, (q + LB_TILE - 1) / LB_TILE), dim3(IPM_THREADS), 0, s, qn->E.p, qn->ld,
                           qn->H.p, qn->ld, q, qn->n, qn->part.p);
        hipLaunchKernelGGL(lb_tfinal_kernel, dim3(q * q), dim3(IPM_THREADS), 0, s, qn->part.p, nblk, q, qn->Pm.p, qn->T.p);
        hipLaunchKernelGGL(lb_invert_kernel, dim3(1), dim3(IPM_THREADS), 0, s, qn->T.p, qn->W.p, q, qn->flag.p, qn->pin_flag);
        MNK_HIP(hipGetLastError());
        qn->key_ls = ls;
        qn->key_serial = ls->verdict.serial;
        qn->key_persistent = ls->solves.persistent_solve;
        qn->key_version = qn->version;
        qn->key_valid = true;
        ++qn->builds;
    }
    return lb_apply(qn, wx, -1.0, qn->H.p, qn->ld, qn->W.p, qn->E.p, qn->ld, wx, q, qn->n, qn->flag.p);
}

int mnk_lbfgs_mul_add(mnk_lbfgs* qn, double* wx, const double* xx, double alpha) {
    if (qn->cur == 0) return 0;
    return lb_apply(qn, wx, alpha, qn->E.p, qn->ld, qn->Pm.p, qn->E.p, qn->ld, xx, 2 * qn->cur, qn->n, nullptr);
}

extern "C" {

int mnk_lbfgs_create(mnk_ctx* ctx, int64_t n, int max_history, int init_strategy, double init_value, double sigma_min,
                     double sigma_max, void* out_) {
    mnk_lbfgs** out = static_cast<mnk_lbfgs**>(out_);
    MNK_REQUIRE(n > 0, "mnk_lbfgs_create: n must be positive");
    MNK_REQUIRE(max_history >= 1 && max_history <= LB_MAX_HIST, "mnk_lbfgs_create: max_history must be 1 to 32");
    MNK_REQUIRE(init_strategy >= MNK_LBFGS_SCALAR1 && init_strategy <= MNK_LBFGS_SCALAR4,
                "mnk_lbfgs_create: init_strategy must be MNK_LBFGS_SCALAR1 .. MNK_LBFGS_SCALAR4");
    MNK_REQUIRE(ctx && out, "mnk_lbfgs_create: NULL argument");
    MNK_HIP(hipSetDevice(ctx->device));
    mnk_lbfgs* qn = new mnk_lbfgs();
    qn->ctx = ctx;
    qn->n = n;
    qn->ld = round_up(n, 8);
    qn->pmax = max_history;
    qn->strategy = init_strategy;
    qn->init_value = init_value;
    qn->sigma_min = sigma_min;
    qn->sigma_max = sigma_max;
    const size_t pm = (size_t)max_history, qm = 2 * pm, ld = (size_t)qn->ld;
    int rc = qn->S.alloc(ld * pm) | qn->Y.alloc(ld * pm) | qn->E.alloc(ld * qm) | qn->H.alloc(ld * qm) | qn->Pm.alloc(qm * qm) |
             qn->T.alloc(qm * qm) | qn->W.alloc(qm * qm) | qn->coef.alloc(qn->coef_words()) | qn->res.alloc(LB_MAX_DOTS) |
             qn->part.alloc(std::max<size_t>(qm * qm, LB_MAX_DOTS) * IPM_BLOCKS) | qn->flag.alloc(1);
    const size_t pin_bytes = (LB_MAX_DOTS + qn->coef_words()) * sizeof(double) + sizeof(int);
    if (!rc && hipHostMalloc((void**)&qn->pin, pin_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        qn->pin = nullptr;
        rc = -2;
    }
    if (rc) {
        if (qn->pin) { LaunchLock lock; quiesce_persistent(); (void)hipHostFree(qn->pin); }
        delete qn;
        set_error("mnk_lbfgs_create: no memory for n = %lld, max_history = %d", (long long)n, max_history);
        return -2;
    }
    qn->pin_flag = reinterpret_cast<int*>(qn->pin + LB_MAX_DOTS + qn->coef_words());
    *qn->pin_flag = 0;
    hipStream_t s = ctx->stream;
    MNK_HIP(hipMemsetAsync(qn->S.p, 0, ld * pm * sizeof(double), s));
    MNK_HIP(hipMemsetAsync(qn->Y.p, 0, ld * pm * sizeof(double), s));
    MNK_HIP(hipMemsetAsync(qn->E.p, 0, ld * qm * sizeof(double), s));
    MNK_HIP(hipMemsetAsync(qn->H.p, 0, ld * qm * sizeof(double), s));
    MNK_HIP(hipMemsetAsync(qn->flag.p, 0, sizeof(int), s));
    qn->StS.assign(pm * pm, 0.0);
    qn->L.assign(pm * pm, 0.0);
    qn->D.assign(pm, 0.0);
    mnk_ctx_child_added(ctx);
    *out = qn;
    return 0;
}

int mnk_lbfgs_destroy(void* qn_) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    if (!qn) return 0;
    (void)hipSetDevice(qn->ctx->device);
    (void)mnk::stream_wait(qn->ctx->stream);
    if (qn->pin) { LaunchLock lock; quiesce_persistent(); (void)hipHostFree(qn->pin); }
    mnk_ctx* ctx = qn->ctx;
    delete qn;
    mnk_ctx_child_gone(ctx);
    return 0;
}

// init! (quasi_newton.jl:425-437): xi = 2 rho0 init_value by the Gilbert-Lemarechal rule, g0'g0 an ordered sum on the device
int mnk_lbfgs_init(void* qn_, const double* g0, double f0, double* xi) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    MNK_REQUIRE(qn && g0 && xi, "mnk_lbfgs_init: NULL argument");
    MNK_HIP(hipSetDevice(qn->ctx->device));
    LbDotList dl = {};
    dl.a[0] = dl.b[0] = g0;
    dl.count = 1;
    int rc = lb_dots(qn, dl);
    if (rc) return rc;
    const double gg = qn->pin[0];
    double rho0;
    if (gg < 1.4901161193847656e-08) rho0 = 1.0;   // sqrt(eps)
    else if (f0 == 0.0) rho0 = 1.0 / gg;
    else rho0 = std::fabs(f0) / gg;
    qn->sigma = 2.0 * rho0 * qn->init_value;
    *xi = qn->sigma;
    return 0;
}

// update! (quasi_newton.jl:366-423) with the device vectors s, y
int mnk_lbfgs_update(void* qn_, const double* sv, const double* yv, int* performed, double* sigma) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    MNK_REQUIRE(qn && sv && yv && performed && sigma, "mnk_lbfgs_update: NULL argument");
    MNK_HIP(hipSetDevice(qn->ctx->device));
    hipStream_t st = qn->ctx->stream;
    const int p = qn->cur, pm = qn->pmax;
    LbDotList dl = {};
    dl.a[0] = sv; dl.b[0] = sv;
    dl.a[1] = sv; dl.b[1] = yv;
    dl.a[2] = yv; dl.b[2] = yv;
    for (int j = 0; j < p; ++j) {
        dl.a[3 + j] = qn->S.p + (int64_t)qn->slot_of(j) * qn->ld; dl.b[3 + j] = sv;
        dl.a[3 + p + j] = qn->Y.p + (int64_t)qn->slot_of(j) * qn->ld; dl.b[3 + p + j] = sv;
    }
    dl.count = 3 + 2 * p;
    int rc = lb_dots(qn, dl);
    if (rc) return rc;
    const double* r = qn->pin;
    const double ss = r[0], sy = r[1], yy = r[2];
    const double eps = 2.220446049250313e-16, ns = std::sqrt(ss), ny = std::sqrt(yy);
    *performed = 0;
    *sigma = qn->sigma;
    if (ns < 100.0 * eps || ny < 100.0 * eps || sy < std::sqrt(eps) * ns * ny) {
        ++qn->skipped;
        if (++qn->skipped_iter >= 2) qn->reset();
        return 0;
    }
    // the history after this pair: the oldest one goes when the memory is full
    const int drop = p == pm ? 1 : 0, k = p - drop + 1;
    std::vector<double> StS((size_t)k * k, 0.0), L((size_t)k * k, 0.0), D(k), delta(k);
    for (int i = 0; i + 1 < k; ++i) {
        for (int j = 0; j + 1 < k; ++j) {
            StS[i + k * j] = qn->StS[(i + drop) + pm * (j + drop)];
            L[i + k * j] = qn->L[(i + drop) + pm * (j + drop)];
        }
        StS[(k - 1) + k * i] = StS[i + k * (k - 1)] = r[3 + i + drop];
        L[(k - 1) + k * i] = r[3 + p + i + drop];   // s_k . y_i
        D[i] = qn->D[i + drop];
    }
    StS[(k - 1) + k * (k - 1)] = ss;
    D[k - 1] = sy;
    double sg;
    if (qn->strategy == MNK_LBFGS_SCALAR1) sg = sy / ss;
    else if (qn->strategy == MNK_LBFGS_SCALAR2) sg = yy / sy;
    else if (qn->strategy == MNK_LBFGS_SCALAR3) sg = ((sy / ss) + (yy / sy)) / 2;
    else sg = std::sqrt((sy / ss) * (yy / sy));
    sg = sg > qn->sigma_max ? qn->sigma_max : sg < qn->sigma_min ? qn->sigma_min : sg;
    for (int i = 0; i < k; ++i) delta[i] = 1.0 / std::sqrt(D[i]);
    // DL = D^-1/2 L' ; M = sigma S'S + DL' DL ; M = J J'
    std::vector<double> DL((size_t)k * k), J((size_t)k * k, 0.0), Ji((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) DL[i + k * j] = delta[i] * L[j + k * i];
    bool pd = true;
    for (int j = 0; j < k && pd; ++j)
        for (int i = j; i < k; ++i) {
            double v = sg * StS[i + k * j];
            for (int t = 0; t < k; ++t) v += DL[t + k * i] * DL[t + k * j];
            for (int t = 0; t < j; ++t) v -= J[i + k * t] * J[j + k * t];
            if (i == j) {
                if (!(v > 0.0) || !std::isfinite(v)) { pd = false; break; }
                J[j + k * j] = std::sqrt(v);
            } else {
                J[i + k * j] = v / J[j + k * j];
            }
        }
    if (!pd) {   // (the reference raises PosDefException here; the mirror resets too)
        ++qn->skipped;
        qn->reset();
        return 0;
    }
    for (int c = 0; c < k; ++c)   // Ji = J^-1 (lower), column by column
        for (int i = c; i < k; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int t = c; t < i; ++t) v -= J[i + k * t] * Ji[t + k * c];
            Ji[i + k * c] = v / J[i + k * i];
        }
    // U = (sigma S + Y D^-1/2 DL) J^-T = S A1 + Y A2
    double* coef = qn->pin + LB_MAX_DOTS;
    double *A1 = coef, *A2 = coef + (size_t)k * k, *dlt = coef + (size_t)2 * k * k, *ph = dlt + k;
    for (int c = 0; c < k; ++c)
        for (int j = 0; j < k; ++j) {
            A1[j + k * c] = sg * Ji[c + k * j];
            double v = 0.0;
            for (int t = 0; t < k; ++t) v += DL[j + k * t] * Ji[c + k * t];
            A2[j + k * c] = delta[j] * v;
        }
    // commit: the ring, the small matrices, the counters
    int slot;
    if (drop) { slot = qn->head; qn->head = (qn->head + 1) % pm; }
    else { slot = qn->slot_of(p); qn->cur = k; }
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < k; ++j) {
            qn->StS[i + pm * j] = StS[i + k * j];
            qn->L[i + pm * j] = L[i + k * j];
        }
        qn->D[i] = D[i];
        dlt[i] = delta[i];
        ph[i] = (double)qn->slot_of(i);
    }
    qn->sigma = sg;
    ++qn->updates;
    ++qn->version;
    const size_t words = (size_t)2 * k * k + 2 * k;
    MNK_HIP(hipMemcpyAsync(qn->coef.p, coef, words * sizeof(double), hipMemcpyHostToDevice, st));   // (pinned source: no wait)
    hipLaunchKernelGGL(lb_uv_kernel, dim3(lb_blocks(qn->n)), dim3(IPM_THREADS), 0, st, qn->S.p, qn->Y.p, qn->ld, sv, yv, slot, k,
                       qn->coef.p, qn->E.p, qn->Pm.p, qn->n);
    MNK_HIP(hipGetLastError());
    *performed = 1;
    *sigma = sg;
    return 0;
}

int mnk_lbfgs_status(void* qn_, int64_t* out) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    MNK_REQUIRE(qn && out, "mnk_lbfgs_status: NULL argument");
    MNK_HIP(hipSetDevice(qn->ctx->device));
    MNK_HIP(mnk::stream_wait(qn->ctx->stream));
    if (*(volatile int*)qn->pin_flag != 0 && qn->key_valid) {   // one event per singular T
        ++qn->singular;
        qn->key_valid = false;
        *(volatile int*)qn->pin_flag = 0;
    }
    out[0] = qn->cur; out[1] = qn->updates; out[2] = qn->skipped; out[3] = qn->resets;
    out[4] = qn->builds; out[5] = qn->singular; out[6] = qn->version; out[7] = qn->pmax;
    return 0;
}

int mnk_lbfgs_get(void* qn_, int which, double* out, int64_t ld) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    MNK_REQUIRE(qn && out, "mnk_lbfgs_get: NULL argument");
    MNK_HIP(hipSetDevice(qn->ctx->device));
    hipStream_t s = qn->ctx->stream;
    const int p = qn->cur, q = 2 * p, pm = qn->pmax;
    const size_t w = qn->n * sizeof(double);
    if (which == MNK_LBFGS_S || which == MNK_LBFGS_Y || which == MNK_LBFGS_U || which == MNK_LBFGS_V) {
        MNK_REQUIRE(ld >= qn->n, "mnk_lbfgs_get: leading dimension smaller than n");
        for (int j = 0; j < p; ++j) {
            const double* src = which == MNK_LBFGS_S ? qn->S.p + (int64_t)qn->slot_of(j) * qn->ld
                              : which == MNK_LBFGS_Y ? qn->Y.p + (int64_t)qn->slot_of(j) * qn->ld
                              : which == MNK_LBFGS_U ? qn->E.p + (int64_t)j * qn->ld
                                                     : qn->E.p + (int64_t)(p + j) * qn->ld;
            MNK_HIP(mnk::d2h_copy(out + j * ld, src, w, s));
        }
        return 0;
    }
    if (which == MNK_LBFGS_L) {
        MNK_REQUIRE(ld >= p, "mnk_lbfgs_get: leading dimension smaller than current_mem");
        for (int j = 0; j < p; ++j)
            for (int i = 0; i < p; ++i) out[i + ld * j] = qn->L[i + pm * j];
        return 0;
    }
    if (which == MNK_LBFGS_D) {
        for (int i = 0; i < p; ++i) out[i] = qn->D[i];
        return 0;
    }
    if (which == MNK_LBFGS_T || which == MNK_LBFGS_W) {
        MNK_REQUIRE(ld >= q, "mnk_lbfgs_get: leading dimension smaller than 2 current_mem");
        MNK_REQUIRE(qn->key_valid, "mnk_lbfgs_get: T and W exist after the first solve_kkt of a factorization");
        const double* src = which == MNK_LBFGS_T ? qn->T.p : qn->W.p;
        if (q > 0) MNK_HIP(mnk::d2h_copy_2d(out, ld * sizeof(double), src, q * sizeof(double), q * sizeof(double), q, s));
        return 0;
    }
    set_error("mnk_lbfgs_get: bad selector %d", which);
    return -1;
}

// out (host, qa x qb, column-major) = A'B of device matrices with n rows: the reduction kernels on their own
int mnk_lbfgs_gram(void* qn_, const double* A, int64_t lda, int qa, const double* B, int64_t ldb, int qb, int64_t n,
                   double* out) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    MNK_REQUIRE(qn && A && B && out, "mnk_lbfgs_gram: NULL argument");
    MNK_REQUIRE(n > 0 && lda >= n && ldb >= n && qa >= 1 && qb >= 1 && (size_t)qa * qb * IPM_BLOCKS <= qn->part.n,
                "mnk_lbfgs_gram: bad sizes (qa qb may not exceed (2 max_history)^2)");
    MNK_HIP(hipSetDevice(qn->ctx->device));
    hipStream_t s = qn->ctx->stream;
    const int nblk = lb_blocks(n);
    DevBuf<double> res;
    if (res.alloc((size_t)qa * qb)) return -2;
    hipLaunchKernelGGL(lb_gram_kernel, dim3(nblk, qa, (qb + LB_TILE - 1) / LB_TILE), dim3(IPM_THREADS), 0, s, A, lda, B, ldb, qb, n,
                       qn->part.p);
    hipLaunchKernelGGL(lb_final_kernel, dim3(qa * qb), dim3(IPM_THREADS), 0, s, qn->part.p, nblk, res.p);
    MNK_HIP(hipGetLastError());
    std::vector<double> h((size_t)qa * qb);
    MNK_HIP(mnk::d2h_copy(h.data(), res.p, h.size() * sizeof(double), s));
    for (int i = 0; i < qa; ++i)
        for (int j = 0; j < qb; ++j) out[i + (size_t)qa * j] = h[(size_t)i * qb + j];
    return 0;
}

// y += alpha A (M (B'x)) on device vectors (A, B: n x q, M: q x q column-major): the pair of launches on its own
int mnk_lbfgs_apply(void* qn_, double* y, double alpha, const double* A, int64_t lda, const double* M, const double* B,
                    int64_t ldb, const double* x, int q, int64_t n) {
    mnk_lbfgs* qn = static_cast<mnk_lbfgs*>(qn_);
    MNK_REQUIRE(qn && y && A && M && B && x, "mnk_lbfgs_apply: NULL argument");
    MNK_REQUIRE(n > 0 && lda >= n && ldb >= n && q >= 1 && q <= LB_MAX_Q && (size_t)q * IPM_BLOCKS <= qn->part.n,
                "mnk_lbfgs_apply: bad sizes (q may not exceed 64 or (2 max_history)^2)");
    MNK_HIP(hipSetDevice(qn->ctx->device));
    return lb_apply(qn, y, alpha, A, lda, M, B, ldb, x, q, n, nullptr);
}

}  // extern "C"

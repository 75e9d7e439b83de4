// LU linear solver: lapack_algorithm = LU of LapackCPUSolver / LapackROCmSolver (reference src/LinearSolvers/lapack.jl:174-187,
// lib/MadNLPGPU/ext/MadNLPGPUAMDGPUExt/rocsolver.jl: getrf / getrs): factorize! mirrors the transferred lower triangle to the
// full matrix (tril_to_full!, src/LinearSolvers/lapack_common.jl) and factors P A = L U with partial pivoting, LAPACK dgetrf's
// conventions; solve! applies the row interchanges, then L y = b (unit diagonal) and U x = y (dgetrs 'N').
//
// Storage (what mnk_ls_get_factor / mnk_ls_get_pivots hand out): the factor buffer holds the unit-lower L strictly below the
// diagonal and U on and above it, dvec holds diag(U), ipiv[k] (0-based on the device, 1-based at the ABI) is the row swapped
// with row k.  Pivot choice is idamax's: the largest |a|, the smallest row index on a tie (a NaN counts as larger than
// everything, so it spreads instead of hiding).  Multipliers are a * (1 / pivot) when |pivot| >= DBL_MIN, a / pivot otherwise
// (dgetf2); an exactly zero pivot scales nothing and info is the 1-based index of the first one (elimination goes on).  The
// padding block of the factor buffer is the identity and its rows are zero in the real columns: never chosen, never moved.
//
// Schedule of one factorization (everything is enqueued on the context's stream; no host synchronization, no wait across
// workgroups -- every dependency is a kernel boundary):
//   per 64-column panel (columns j0 .. j0 + 63, rows j0 .. Np):
//     1. lu_panel_kernel, 65 launches: launch c picks the pivot of panel column c from the per-256-row-block candidates of the
//        previous launch (reduced in a fixed order by every workgroup), swaps rows inside the panel, scales column c and applies
//        the rank-1 update to the panel's remaining columns; then it forms the next column's candidates: each block's
//        (max |a|, row) and that row's 64 panel entries, plus the row the next pivot replaces.
//     2. lu_laswp_kernel: the panel's 64 interchanges, composed into one gather of at most 128 rows, on every column outside
//        the panel; workgroup 0 also folds them into the full row permutation that the solves gather with.
//     3. lu_trsm_kernel: U12 = L11^-1 A12 (unit lower, one column per thread), in place and transposed into a workspace.
//     4. A22 -= L21 U12 on the MFMA pipes (the factorization's NT tile kernel, U12^T as its B operand).
// Nothing depends on timing or on atomics: two factorizations of the same matrix are bit-identical.
#include <cfloat>
#include <climits>
#include <vector>

#include "gemm_tile.h"
#include "ls.h"

namespace mnk {

constexpr int LB = 64;       // panel width
constexpr int LU_RB = 256;   // rows per workgroup of the panel and solve kernels (one row per thread)

// idamax's order on (|a|, row): larger |a| first, then the smaller row.  The key is the bit pattern of |a|, which orders the
// non-negative doubles and puts every NaN above +Inf; -1 marks "no candidate".  A total order, so a butterfly leaves the same
// winner in every lane and the result does not depend on the order of the reduction.
__device__ __forceinline__ long long lu_key(double a) { return __double_as_longlong(fabs(a)); }
__device__ __forceinline__ bool lu_better(long long ka, int ra, long long kb, int rb) {
    return ka > kb || (ka == kb && ra < rb);
}
__device__ __forceinline__ void lu_wave_argmax(long long& k, int& r) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const long long ko = __shfl_xor(k, h);
        const int ro = __shfl_xor(r, h);
        if (lu_better(ko, ro, k, r)) {
            k = ko;
            r = ro;
        }
    }
}

// ipiv / perm start as the identity (padding columns keep it), info as 0
__global__ __launch_bounds__(256) void lu_init_kernel(int* __restrict__ ipiv, int* __restrict__ perm, int64_t Np,
                                                      int* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < Np) {
        ipiv[i] = (int)i;
        perm[i] = (int)i;
    }
    if (i == 0) *info = 0;
}

// One column step of the panel factorization (unblocked dgetf2 on the m x 64 panel at F(j0, j0), m = Np - j0).
// APPLY: column c.  The candidates of the previous launch are, per 256-row block b, the row Iin[b] with the largest |a(., j)|
// among the block's rows >= j and its 64 panel entries Pin[64 b ..]; Rin holds row j's entries.  Every workgroup reduces the
// candidates in the same order to the pivot row p, so all of them see the same pivot row (read from Pin, never from F, which
// this launch rewrites).  Row j takes row p's entries, row p takes Rin, every row r > j gets l = a(r, j) / pivot and
// a(r, k) -= l u(k) for k > c.
// Then (c < 63, or !APPLY for column 0) the candidates of the next column into Iout / Pout and its row into Rout.
template <bool APPLY>
__global__ __launch_bounds__(256) void lu_panel_kernel(double* __restrict__ F, int64_t ld, int64_t j0, int64_t Np, int c,
                                                       const double* __restrict__ Pin, const int* __restrict__ Iin,
                                                       const double* __restrict__ Rin, double* __restrict__ Pout,
                                                       int* __restrict__ Iout, double* __restrict__ Rout, int* __restrict__ ipiv,
                                                       double* __restrict__ dvec, int* __restrict__ info, int nb) {
    __shared__ double prow[64], wrow[64];
    __shared__ long long redk[4];
    __shared__ int redr[4], s_p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = j0 + (int64_t)blockIdx.x * LU_RB + tid;
    const bool valid = r < Np;
    const int64_t j = j0 + c;
    const bool live = valid && r >= (APPLY ? j : j0);
    double a[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) a[k] = live ? F[r + (j0 + k) * ld] : 0.0;
    if (APPLY) {
        if (wave == 0) {   // the pivot: candidates of blocks lane, lane + 64, ... in order, then the butterfly
            long long kb = -1;
            int rb = INT_MAX;
            for (int b = lane; b < nb; b += 64) {
                const long long kk = lu_key(Pin[b * 64 + c]);
                const int rr = Iin[b];
                if (lu_better(kk, rr, kb, rb)) {
                    kb = kk;
                    rb = rr;
                }
            }
            lu_wave_argmax(kb, rb);
            if (lane == 0) s_p = rb < Np ? rb : (int)j;   // (every block has a candidate: rb is a row of the panel)
        }
        __syncthreads();
        const int64_t p = s_p;
        const int w = (int)((p - j0) / LU_RB);
        if (tid < 64) prow[tid] = Pin[w * 64 + tid];
        __syncthreads();
        const double piv = prow[c];
        if (blockIdx.x == 0 && tid == 0) {
            ipiv[j] = (int)p;
            dvec[j] = piv;
            if (piv == 0.0 && *info == 0) *info = (int)(j + 1);
        }
        if (live) {
            if (r == j) {   // the pivot row: row p's entries (its L part included)
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    a[k] = prow[k];
                    F[r + (j0 + k) * ld] = a[k];
                }
            } else {
                const bool moved = r == p;   // row p takes the old row j
                if (moved) {
#pragma unroll
                    for (int k = 0; k < 64; ++k) a[k] = Rin[k];
                }
                double x = 0.0;
#pragma unroll
                for (int k = 0; k < 64; ++k)
                    if (k == c) x = a[k];
                const double l = piv == 0.0 ? x : (fabs(piv) >= DBL_MIN ? x * (1.0 / piv) : x / piv);
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    if (k == c) a[k] = l;
                    else if (k > c) a[k] -= l * prow[k];
                    if (k >= c || moved) F[r + (j0 + k) * ld] = a[k];
                }
            }
        }
    }
    const int cn = APPLY ? c + 1 : 0;   // the next column
    if (cn >= LB) return;
    const int64_t jn = j0 + cn;
    long long kb = -1;
    int rb = INT_MAX;
    if (valid && r >= jn) {
#pragma unroll
        for (int k = 0; k < 64; ++k)
            if (k == cn) kb = lu_key(a[k]);
        rb = (int)r;
    }
    if (r == jn) {
#pragma unroll
        for (int k = 0; k < 64; ++k) Rout[k] = a[k];
    }
    lu_wave_argmax(kb, rb);
    if (lane == 0) {
        redk[wave] = kb;
        redr[wave] = rb;
    }
    __syncthreads();
    kb = redk[0];
    rb = redr[0];
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (lu_better(redk[q], redr[q], kb, rb)) {
            kb = redk[q];
            rb = redr[q];
        }
    if (r == rb) {
#pragma unroll
        for (int k = 0; k < 64; ++k) wrow[k] = a[k];
    }
    __syncthreads();
    if (tid < 64) Pout[(int64_t)blockIdx.x * 64 + tid] = wrow[tid];
    if (tid == 0) Iout[blockIdx.x] = rb;
}

// The panel's interchanges (row j0 + k <-> ipiv[j0 + k], k = 0 .. 63, in order) on the columns outside the panel.  Wave 0
// composes them into slots: slot s < 64 is row j0 + s, the others the pivot rows below the panel, in order of first use; after
// the 64 swaps, row dst[s] holds what row src[s] held.  Every workgroup then gathers its 16 columns; workgroup 0 also applies
// the gather to perm (perm[i]: the row of the original matrix that row i of P A is).
__global__ __launch_bounds__(256) void lu_laswp_kernel(double* __restrict__ F, int64_t ld, int64_t j0, int64_t Np,
                                                       const int* __restrict__ ipiv, int* __restrict__ perm) {
    __shared__ int pv[64], dst[128], src[128], s_ns;
    const int tid = threadIdx.x;
    if (tid < 64) pv[tid] = ipiv[j0 + tid];
    __syncthreads();
    if (tid < 64) {
        const int lane = tid;
        int xr = -1;   // the row of slot 64 + lane
        int nx = 0;
        if (lane == 0)
            for (int s = 0; s < 64; ++s) dst[s] = src[s] = (int)j0 + s;
        for (int k = 0; k < 64; ++k) {
            const int p = pv[k];
            int sp;
            if (p < j0 + 64) {
                sp = p - (int)j0;
            } else {
                const unsigned long long m = __ballot(xr == p);
                if (m) {
                    sp = 64 + __ffsll((long long)m) - 1;
                } else {
                    sp = 64 + nx;
                    if (lane == nx) xr = p;
                    if (lane == 0) dst[sp] = src[sp] = p;
                    ++nx;
                }
            }
            if (lane == 0 && sp != k) {
                const int t = src[k];
                src[k] = src[sp];
                src[sp] = t;
            }
        }
        if (lane == 0) s_ns = 64 + nx;
    }
    __syncthreads();
    const int ns = s_ns;
    const int s = tid & 127, cg = tid >> 7;
    const bool moves = s < ns && src[s] != dst[s];
    if (blockIdx.x == 0) {
        const int v = moves ? perm[src[s]] : 0;
        __syncthreads();
        if (cg == 0 && moves) perm[dst[s]] = v;
    }
    const int64_t ncols = Np - LB;
    const int64_t q0 = (int64_t)blockIdx.x * 16;
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t q = q0 + cg + 2 * i;
        const int64_t col = q < j0 ? q : q + LB;
        v[i] = moves && q < ncols ? F[src[s] + col * ld] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t q = q0 + cg + 2 * i;
        const int64_t col = q < j0 ? q : q + LB;
        if (moves && q < ncols) F[dst[s] + col * ld] = v[i];
    }
}

// U12 = L11^-1 A12 for the n2 columns right of the panel (unit lower L11 staged in LDS; one column per thread, forward
// substitution in dtrsm's order), written in place and transposed into Ut (n2 x 64, leading dimension ldt).
__global__ __launch_bounds__(64) void lu_trsm_kernel(double* __restrict__ F, int64_t ld, int64_t j0, double* __restrict__ Ut,
                                                     int64_t ldt) {
    __shared__ double Ls[64 * 65];
    const int tid = threadIdx.x;
    for (int e = tid; e < 64 * 64; e += 64) {
        const int rr = e & 63, i = e >> 6;
        Ls[rr * 65 + i] = F[j0 + rr + (j0 + i) * ld];
    }
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * 64 + tid;
    double* col = F + j0 + (j0 + LB + q) * ld;
    double x[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) x[i] = col[i];
#pragma unroll
    for (int i = 0; i < 64; ++i)
#pragma unroll
        for (int rr = i + 1; rr < 64; ++rr) x[rr] -= Ls[rr * 65 + i] * x[i];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        col[i] = x[i];
        Ut[q + i * ldt] = x[i];
    }
}

// ---- solve: y = P b (one gather), L z = y by 64-row blocks (unit diagonal), U x = z (the QR solver's back substitution) ----
__global__ __launch_bounds__(256) void lu_gather_kernel(const double* __restrict__ b, int64_t N, int64_t Np,
                                                        const int* __restrict__ perm, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Np) return;
    const int p = perm[i];
    y[i] = p < N ? b[p] : 0.0;
}

// Block q of the forward substitution: every workgroup solves L_qq z_q = y_q (one wave, L_qq staged in LDS), workgroup 0
// stores z_q, and every workgroup subtracts L(r, q-block) z_q from its 256 rows r >= 64 (q + 1) of y.
__global__ __launch_bounds__(256) void lu_lsolve_kernel(const double* __restrict__ F, int64_t ld, int64_t Np, int q,
                                                        double* __restrict__ y, double* __restrict__ z) {
    __shared__ double Ls[64 * 65], zs[64];
    const int tid = threadIdx.x;
    const int64_t d0 = (int64_t)q * LB;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int l = e & 63, i = e >> 6;
        Ls[l * 65 + i] = F[d0 + l + (d0 + i) * ld];
    }
    __syncthreads();
    if (tid < 64) {
        double yl = y[d0 + tid], zv = 0.0;
        for (int i = 0; i < LB; ++i) {
            const double zi = __shfl(yl, i);
            if (tid == i) zv = zi;
            if (tid > i) yl -= Ls[tid * 65 + i] * zi;
        }
        zs[tid] = zv;
        if (blockIdx.x == 0) z[d0 + tid] = zv;
    }
    __syncthreads();
    const int64_t r = d0 + LB + (int64_t)blockIdx.x * LU_RB + tid;
    if (r < Np) {
        double yr = y[r];
#pragma unroll 8
        for (int i = 0; i < LB; ++i) yr -= F[r + (d0 + i) * ld] * zs[i];
        y[r] = yr;
    }
}

__global__ __launch_bounds__(256) void lu_pivots_out_kernel(const int* __restrict__ ipiv, int64_t N, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) out[i] = (int64_t)ipiv[i] + 1;
}

static int lu_nblk(int64_t Np) { return (int)((Np + LU_RB - 1) / LU_RB); }

struct LuSolver final : mnk_ls_alt {
    // U12^T of the current panel (B operand of the trailing update), the panel's pivot candidates (64 entries and the row per
    // 256-row block, two sets used alternately) and the row the next pivot replaces; the pivots (0-based), the row permutation
    // they compose to (what the solves gather with) and getrf's info
    DevBuf<double> lu_ut, lu_p;
    DevBuf<int> lu_cand, lu_ipiv, lu_perm, lu_info;

    int alloc(mnk_ls* ls) override {
        const int64_t Np = ls->Np;
        const int nblk = lu_nblk(Np);
        int rc = lu_ut.alloc((size_t)Np * LB + SLACK * LB);
        rc |= lu_p.alloc((size_t)2 * nblk * 64 + 2 * 64);
        rc |= lu_cand.alloc((size_t)2 * nblk);
        rc |= lu_ipiv.alloc((size_t)Np);
        rc |= lu_perm.alloc((size_t)Np);
        rc |= lu_info.alloc(1);
        return rc;
    }

    // factorize! of an LU solver: the matrix has been transferred (lower triangle); mirror it and factor it (see the top).
    int factor(mnk_ls* ls) override {
        hipStream_t s = ls->ctx->stream;
        double* F = ls->fact.p;
        const int64_t ld = ls->ld, N = ls->N, Np = ls->Np;
        const int np = (int)(Np / LB), nblk = lu_nblk(Np);
        int rc = mnk_launch_tril_to_full(s, F, ld, N, Np);
        if (rc) return rc;
        double* P[2] = {lu_p.p, lu_p.p + (int64_t)nblk * 64};
        double* R[2] = {lu_p.p + (int64_t)2 * nblk * 64, lu_p.p + (int64_t)2 * nblk * 64 + 64};
        int* I[2] = {lu_cand.p, lu_cand.p + nblk};
        int *ipiv = lu_ipiv.p, *perm = lu_perm.p, *info = lu_info.p;
        double* Ut = lu_ut.p;
        hipLaunchKernelGGL(lu_init_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, s, ipiv, perm, Np, info);
        for (int p = 0; p < np; ++p) {
            const int64_t j0 = (int64_t)p * LB, m = Np - j0, n2 = m - LB;
            const int nb = (int)((m + LU_RB - 1) / LU_RB);
            hipLaunchKernelGGL(lu_panel_kernel<false>, dim3(nb), dim3(256), 0, s, F, ld, j0, Np, -1, nullptr, nullptr, nullptr,
                               P[0], I[0], R[0], ipiv, ls->dvec.p, info, nb);
            for (int c = 0; c < LB; ++c)
                hipLaunchKernelGGL(lu_panel_kernel<true>, dim3(nb), dim3(256), 0, s, F, ld, j0, Np, c, P[c & 1], I[c & 1],
                                   R[c & 1], P[(c + 1) & 1], I[(c + 1) & 1], R[(c + 1) & 1], ipiv, ls->dvec.p, info, nb);
            const unsigned gs = (unsigned)std::max<int64_t>(1, (Np - LB + 15) / 16);
            hipLaunchKernelGGL(lu_laswp_kernel, dim3(gs), dim3(256), 0, s, F, ld, j0, Np, ipiv, perm);
            if (n2 > 0) {
                hipLaunchKernelGGL(lu_trsm_kernel, dim3((unsigned)(n2 / 64)), dim3(64), 0, s, F, ld, j0, Ut, Np);
                MNK_HIP(hipGetLastError());
                rc = launch_gemm_nt(s, 0, n2, n2, LB, F + j0 + LB + j0 * ld, ld, Ut, Np, F + j0 + LB + (j0 + LB) * ld, ld,
                                    nullptr, nullptr, 0, nullptr);
                if (rc) return rc;
            }
        }
        MNK_HIP(hipGetLastError());
        return 0;
    }

    // getrf's info of the factorization queued last (waits for it): the first exactly zero pivot (1-based), 0 if none
    int fetch_info(mnk_ls* ls) override {
        int info = 0;
        MNK_HIP(d2h_copy(&info, lu_info.p, sizeof(int), ls->ctx->stream));
        ls->verdict.accept(info, 0, 0, 0);
        return 0;
    }

    // solve_lu! (reference src/LinearSolvers/lapack.jl:183-187): P b, then L^-1, then U^-1 on the padded vectors y, z, xo; the
    // first N entries of xo go to x.
    int solve_vec(mnk_ls* ls, const double* b, double* x) override {
        hipStream_t s = ls->ctx->stream;
        const double* F = ls->fact.p;
        const int64_t ld = ls->ld, N = ls->N, Np = ls->Np;
        const int np = (int)(Np / LB);
        double* y = ls->xwork.p + Np;
        double* z = ls->xwork.p + 2 * Np;
        double* xo = ls->xwork.p + 3 * Np;
        hipLaunchKernelGGL(lu_gather_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, s, b, N, Np, lu_perm.p, y);
        for (int q = 0; q < np; ++q) {
            const int64_t below = Np - (int64_t)(q + 1) * LB;
            const unsigned g = (unsigned)std::max<int64_t>(1, (below + LU_RB - 1) / LU_RB);
            hipLaunchKernelGGL(lu_lsolve_kernel, dim3(g), dim3(256), 0, s, F, ld, Np, q, y, z);
        }
        MNK_HIP(hipGetLastError());
        int rc = mnk_launch_upper_bsolve(s, F, ld, Np, z, xo);
        if (rc) return rc;
        MNK_HIP(hipMemcpyAsync(x, xo, N * sizeof(double), hipMemcpyDeviceToDevice, s));
        return 0;
    }

    const char* no_inertia_message() const override { return "mnk_ls_inertia: an LU factorization reveals no inertia (is_inertia is false for LU)"; }
};

}  // namespace mnk

using namespace mnk;

std::unique_ptr<mnk_ls_alt> mnk_lu_new() { return std::make_unique<LuSolver>(); }

extern "C" {

int mnk_ls_get_pivots(mnk_ls* ls, int64_t* ipiv, int loc) {
    MNK_REQUIRE(ls && ipiv, "mnk_ls_get_pivots: NULL argument");
    MNK_REQUIRE(ls->algo == MNK_LU, "mnk_ls_get_pivots: only an LU factorization has row interchanges");
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    MNK_REQUIRE(ls->verdict.has_factorization(), "mnk_ls_get_pivots: factorize first");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    hipStream_t s = ls->ctx->stream;
    const int64_t N = ls->N;
    const int* lu_ipiv = static_cast<const LuSolver*>(ls->alt.get())->lu_ipiv.p;   // (checked above: the alt is this unit's)
    if (loc == MNK_DEVICE) {
        hipLaunchKernelGGL(lu_pivots_out_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, lu_ipiv, N, ipiv);
        MNK_HIP(hipGetLastError());
        MNK_HIP(stream_wait(s));
        return 0;
    }
    std::vector<int> h((size_t)N);
    MNK_HIP(d2h_copy(h.data(), lu_ipiv, N * sizeof(int), s));
    for (int64_t i = 0; i < N; ++i) ipiv[i] = (int64_t)h[i] + 1;
    return 0;
}

}  // extern "C"

// QR linear solver: lapack_algorithm = QR of LapackCPUSolver / LapackROCmSolver (reference
// src/LinearSolvers/lapack.jl:187-209, lib/MadNLPGPU/ext/MadNLPGPUAMDGPUExt/rocsolver.jl): factorize! mirrors the
// transferred lower triangle to the full matrix (tril_to_full!, src/LinearSolvers/lapack_common.jl) and runs a blocked
// Householder QR with LAPACK dgeqrf's conventions; solve! is ormqr('L','T') followed by trsv('U','N','N').
//
// Storage (what mnk_ls_get_factor hands out): the factor buffer holds R on and above the diagonal and the Householder
// vectors below it (v(1) = 1 implicit), dvec holds one tau per column -- exactly where dgeqrf puts them.  The padding
// block of the factor buffer is the identity: its reflectors are H = I (tau = 0) and it never touches the N x N block.
//
// Schedule of one factorization (everything is enqueued on the context's stream; no host synchronization, no wait
// across workgroups -- every dependency is a kernel boundary):
//   per 64-column panel p (columns j0 = 64 p ..., rows j0 .. Np):
//     1. qr_panel_kernel, 65 launches: launch c applies the reflector of panel column c (its dlarfg scalars from the
//        partial sums of the previous launch, reduced in a fixed order by every workgroup) to the panel's remaining
//        columns and forms the partial sums (x.x and x.a_k per 256-row block) the next column needs.
//     2. qr_extract_v_kernel + qr_tn_kernel + qr_form_t_kernel: V (unit lower trapezoid, zero above), G = V^T V, and the
//        compact-WY T of the panel (dlarft, forward / columnwise).  Every panel's T is kept for the solves.
//     3. trailing update A2 = (I - V T^T V^T) A2 on the MFMA pipes: W^T = A2^T V (qr_tn_kernel: split over K, the splits
//        reduced in a fixed order), W^T <- W^T T (qr_wt_kernel), A2 -= V (W^T)^T (the factorization's NT tile kernel).
// Nothing depends on timing or on atomics: two factorizations of the same matrix are bit-identical.
#include "gemm_tile.h"
#include "ls.h"

namespace mnk {

constexpr int QB = 64;       // panel width (columns per compact-WY block)
constexpr int QR_RB = 256;   // rows per workgroup of the panel and solve kernels (one row per thread)
constexpr int QR_SMAX = 16;  // at most this many K-splits of a W^T = A2^T V product

// Sum of v[k] over the 64 lanes of a wave for all 64 k at once: recursive halving, 63 shuffles.  On return v[0] of lane l
// holds the sum for k = l.  Every column is summed in a fixed order (independent of the data).
template <int H>
__device__ __forceinline__ void qr_tr_step(double (&v)[64], int lane) {
    const bool hi = (lane & H) != 0;
#pragma unroll
    for (int q = 0; q < H; ++q) {
        const double send = hi ? v[q] : v[q + H];
        const double keep = hi ? v[q + H] : v[q];
        v[q] = keep + __shfl_xor(send, H);
    }
}
__device__ __forceinline__ double qr_transpose_reduce(double (&v)[64], int lane) {
    qr_tr_step<32>(v, lane);
    qr_tr_step<16>(v, lane);
    qr_tr_step<8>(v, lane);
    qr_tr_step<4>(v, lane);
    qr_tr_step<2>(v, lane);
    qr_tr_step<1>(v, lane);
    return v[0];
}

// Block sum of v[k] (256 threads): out[k] for k < 64, four waves added in order.
__device__ __forceinline__ void qr_block_reduce_store(double (&v)[64], double* red /* LDS [4][64] */, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    red[wave * 64 + lane] = qr_transpose_reduce(v, lane);
    __syncthreads();
    if (threadIdx.x < 64) {
        const int k = threadIdx.x;
        out[k] = ((red[k] + red[64 + k]) + red[128 + k]) + red[192 + k];
    }
}

// upper(F) = lower(F)^T on the N x N block, 0 elsewhere above the diagonal (tril_to_full!).  32 x 32 tiles; only the tiles
// on or above the diagonal are written, from their mirror images below it (which the transfer wrote).
__global__ __launch_bounds__(256) void qr_mirror_kernel(double* __restrict__ F, int64_t ld, int64_t N) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t br = blockIdx.x, bc = blockIdx.y;
    if (br > bc) return;
    const int64_t r0 = br * 32, c0 = bc * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = ty + 8 * q;
        tile[j][tx] = F[(c0 + tx) + (r0 + j) * ld];   // tile[j][i] = F(c0 + i, r0 + j)
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = ty + 8 * q;
        const int64_t r = r0 + tx, c = c0 + j;
        if (r < c) F[r + c * ld] = c < N ? tile[tx][j] : 0.0;   // F(r, c) = F(c, r)
    }
}

// One column step of the panel factorization (unblocked dgeqr2 on the m x 64 panel at F(j0, j0), m = Np - j0).
// APPLY: reflector of panel column c, from the partial sums Pin (per 256-row block b: Pin[64 b + k] = sum over the block's
// rows r > j0 + c of A(r, j0 + c) A(r, j0 + k)) and the pivot row Rin[k] = A(j0 + c, j0 + k):
//   dlarfg: alpha = A(j, j), xnorm^2 = sum Pin[.][c]; beta = -sign(alpha) sqrt(alpha^2 + xnorm^2), tau = (beta - alpha) / beta,
//   v = x / (alpha - beta) (tau = 0, nothing changes, when x = 0); then A(j:, k) -= tau v (v^T A(j:, k)) for k > c.
// Then (c < 63, or !APPLY for column 0) the partial sums and pivot row of the next column, into Pout / Rout.
template <bool APPLY>
__global__ __launch_bounds__(256) void qr_panel_kernel(double* __restrict__ F, int64_t ld, int64_t j0, int64_t Np, int c,
                                                       const double* __restrict__ Pin, const double* __restrict__ Rin,
                                                       double* __restrict__ Pout, double* __restrict__ Rout,
                                                       double* __restrict__ tau_out, int nb) {
    __shared__ double S[64], tw[64], sc[3], red[256];
    const int tid = threadIdx.x;
    const int64_t r = j0 + (int64_t)blockIdx.x * QR_RB + tid;
    const bool valid = r < Np;
    const int64_t j = j0 + c;
    double vr = 0.0;
    if (APPLY) {
        // S[k] = sum over the blocks of Pin[.][k]: four threads per column (blocks b = q mod 4), their sums added in order
        {
            const int k = tid & 63, q = tid >> 6;
            double s = 0.0;
            if (k >= c)
                for (int b = q; b < nb; b += 4) s += Pin[b * 64 + k];
            red[tid] = s;
        }
        __syncthreads();
        if (tid < 64 && tid >= c) S[tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
        __syncthreads();
        if (tid == 0) {
            const double alpha = Rin[c], xn2 = S[c];
            double beta = alpha, tau = 0.0, scal = 0.0;
            if (xn2 != 0.0) {
                const double h = sqrt(alpha * alpha + xn2);
                beta = alpha >= 0.0 ? -h : h;
                tau = (beta - alpha) / beta;
                scal = 1.0 / (alpha - beta);
            }
            sc[0] = beta;
            sc[1] = tau;
            sc[2] = scal;
            if (blockIdx.x == 0) tau_out[j] = tau;
        }
        __syncthreads();
        if (tid < 64 && tid > c) tw[tid] = -sc[1] * (Rin[tid] + sc[2] * S[tid]);   // -tau w_k, w_k = v^T A(j:, k)
        __syncthreads();
        if (valid && r >= j) {
            if (r == j) {
                vr = 1.0;
                F[j + j * ld] = sc[0];
            } else if (sc[1] != 0.0) {
                vr = F[r + j * ld] * sc[2];
                F[r + j * ld] = vr;
            }
        }
    }
    const int cn = APPLY ? c + 1 : 0;   // the next column
    if (cn >= QB) return;
    const int64_t jn = j0 + cn;
    double prod[64];
    double piv = 0.0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        prod[k] = 0.0;
        if (k >= cn && valid && r >= j) {
            double* p = F + r + (j0 + k) * ld;
            double a;
            if (APPLY) {
                a = (r == j ? Rin[k] : *p) + vr * tw[k];
                *p = a;
            } else {
                a = *p;
            }
            if (k == cn) piv = a;
            if (r > jn) prod[k] = piv * a;
            if (r == jn) Rout[k] = a;
        }
    }
    qr_block_reduce_store(prod, red, Pout + (int64_t)blockIdx.x * 64);
}

// V of panel j0 (m x 64, leading dimension ldv): unit diagonal, Householder vectors below, zeros above.
__global__ __launch_bounds__(256) void qr_extract_v_kernel(const double* __restrict__ F, int64_t ld, int64_t j0, int64_t m,
                                                           double* __restrict__ V, int64_t ldv) {
    const int64_t rr = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (rr >= m) return;
#pragma unroll 8
    for (int i = 0; i < QB; ++i) V[rr + i * ldv] = rr > i ? F[j0 + rr + (j0 + i) * ld] : (rr == i ? 1.0 : 0.0);
}

// Split-K partial products Wp[s] (n2 x 64, leading dimension ldw, split s at Wp + s * wstride) = A(kb:ke, :)^T V(kb:ke, :)
// with A (K x n2, lda) and V (K x 64, ldv), both contiguous along K.  Workgroup (a-tile, split): a 64 x 64 output tile, four
// waves of 32 x 32 (2 x 2 fp64 MFMA 16x16x4).  The operands are staged through LDS transposed ([k][column]) in k-tiles of 16,
// the next k-tile's loads in flight during the current one's MFMAs.  K-chunks are multiples of 16.
constexpr int QR_TN_LD = 65;
__global__ __launch_bounds__(256) void qr_tn_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ V,
                                                    int64_t ldv, int64_t K, int64_t kchunk, double* __restrict__ Wp,
                                                    int64_t ldw, int64_t wstride) {
    __shared__ double As[16 * QR_TN_LD], Vs[16 * QR_TN_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int wa = wave & 1, wi = wave >> 1;
    const int64_t a0 = (int64_t)blockIdx.x * 64;
    const int64_t kb = (int64_t)blockIdx.y * kchunk;
    const int64_t ke = kb + kchunk < K ? kb + kchunk : K;
    const int nk = kb < ke ? (int)((ke - kb) / 16) : 0;
    v4f64 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = v4f64{0.0, 0.0, 0.0, 0.0};
    double ra[4], rv[4];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = tid + 256 * q, kk = p & 15, col = p >> 4;
            ra[q] = A[(k0 + kk) + (a0 + col) * lda];
            rv[q] = V[(k0 + kk) + col * ldv];
        }
    };
    if (nk > 0) gload(kb);
    for (int t = 0; t < nk; ++t) {
        __syncthreads();   // (the previous k-tile's fragments have been read)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = tid + 256 * q, kk = p & 15, col = p >> 4;
            As[kk * QR_TN_LD + col] = ra[q];
            Vs[kk * QR_TN_LD + col] = rv[q];
        }
        __syncthreads();
        if (t + 1 < nk) gload(kb + (int64_t)(t + 1) * 16);
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
            const int kk = kq * 4 + l4;
            double af[2], vf[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                af[x] = As[kk * QR_TN_LD + wa * 32 + x * 16 + l15];
                vf[x] = Vs[kk * QR_TN_LD + wi * 32 + x * 16 + l15];
            }
            // D = V^T A2 block: row (l4 + 4 r) = column i of V, column l15 = column a of A2
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f64_16x16x4f64(vf[ni], af[mi], acc[ni][mi], 0, 0, 0);
        }
    }
    double* W = Wp + (int64_t)blockIdx.y * wstride;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int64_t i = wi * 32 + ni * 16 + l4 + 4 * rg;
                const int64_t a = a0 + wa * 32 + mi * 16 + l15;
                W[a + i * ldw] = acc[ni][mi][rg];
            }
}

// T of one panel (dlarft 'F','C'): T(i, i) = tau_i, T(0:i, i) = T(0:i, 0:i) (-tau_i G(0:i, i)), G = V^T V = sum of the S
// split partials (fixed order).  T is stored column-major, 64 x 64, zero below the diagonal.
__global__ __launch_bounds__(256) void qr_form_t_kernel(const double* __restrict__ Gp, int64_t ldw, int64_t wstride, int S,
                                                        const double* __restrict__ tau, double* __restrict__ T) {
    __shared__ double G[64 * 65], Ts[64 * 65];
    const int tid = threadIdx.x;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int a = e & 63, i = e >> 6;
        double g = 0.0;
        for (int s = 0; s < S; ++s) g += Gp[s * wstride + a + i * ldw];
        G[a * 65 + i] = g;
        Ts[a * 65 + i] = 0.0;
    }
    __syncthreads();
    for (int i = 0; i < QB; ++i) {
        const double ti = tau[i];
        if (tid < i && ti != 0.0) {
            double t = 0.0;
            for (int q = tid; q < i; ++q) t += Ts[tid * 65 + q] * (-ti * G[q * 65 + i]);
            Ts[tid * 65 + i] = t;
        }
        if (tid == i) Ts[i * 65 + i] = ti;
        __syncthreads();
    }
    for (int e = tid; e < 64 * 64; e += 256) {
        const int l = e & 63, i = e >> 6;
        T[l + i * 64] = Ts[l * 65 + i];
    }
}

// Wt(a, :) = (sum_s Wp[s](a, :)) T for the 64 rows a of this workgroup (fixed order over the splits).
__global__ __launch_bounds__(256) void qr_wt_kernel(const double* __restrict__ Wp, int64_t ldw, int64_t wstride, int S,
                                                    const double* __restrict__ T, double* __restrict__ Wt) {
    __shared__ double Ts[64 * 65], Ws[64 * 65];
    const int tid = threadIdx.x;
    const int64_t a0 = (int64_t)blockIdx.x * 64;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int a = e & 63, i = e >> 6;
        double w = 0.0;
        for (int s = 0; s < S; ++s) w += Wp[s * wstride + a0 + a + i * ldw];
        Ws[a * 65 + i] = w;
        Ts[a * 65 + i] = T[a + i * 64];   // Ts[l][i] = T(l, i)
    }
    __syncthreads();
    const int a = tid & 63, ig = tid >> 6;
#pragma unroll 4
    for (int ii = 0; ii < 16; ++ii) {
        const int i = ig * 16 + ii;
        double t = 0.0;
        for (int l = 0; l <= i; ++l) t += Ws[a * 65 + l] * Ts[l * 65 + i];
        Wt[a0 + a + (int64_t)i * ldw] = t;
    }
}

// ---- solve: x <- Q^T x panel by panel (ormqr 'L','T'), then R x = y by block back substitution (trsv 'U','N','N') -----------
// Q^T y, launch for panel p (APPLY) over the 256-row blocks b >= j0 / 256 (absolute): w = sum_b Pin[b] (= V^T y), z = T^T w,
// y(j0:) -= V z; then the partial sums V_{p+1}^T y of the next panel per block into Pout.  !APPLY: only the partial sums of
// panel 0.
template <bool APPLY>
__global__ __launch_bounds__(256) void qr_qt_kernel(const double* __restrict__ F, int64_t ld, int64_t Np, int p, int np,
                                                    double* __restrict__ y, const double* __restrict__ Tall,
                                                    const double* __restrict__ Pin, double* __restrict__ Pout, int nblk) {
    __shared__ double ws[64], zs[64], red[256];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)(APPLY ? p : 0) * QB;
    const int b = (int)(j0 / QR_RB) + blockIdx.x;
    const int64_t r = (int64_t)b * QR_RB + tid;
    double yr = r < Np ? y[r] : 0.0;
    if (APPLY) {
        {   // w = sum over the blocks b >= j0 / 256 of Pin[b]: four threads per entry, added in order
            const int i = tid & 63, q = tid >> 6;
            double w = 0.0;
            for (int bb = (int)(j0 / QR_RB) + q; bb < nblk; bb += 4) w += Pin[bb * 64 + i];
            red[tid] = w;
        }
        __syncthreads();
        if (tid < 64) ws[tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
        __syncthreads();
        if (tid < 64) {
            const double* T = Tall + (int64_t)p * 4096;
            double z = 0.0;
            for (int l = 0; l <= tid; ++l) z += T[l + tid * 64] * ws[l];
            zs[tid] = z;
        }
        __syncthreads();
        if (r < Np && r >= j0) {
            const int64_t rr = r - j0;
#pragma unroll 8
            for (int i = 0; i < QB; ++i) {
                const double v = rr > i ? F[r + (j0 + i) * ld] : (rr == i ? 1.0 : 0.0);
                yr -= v * zs[i];
            }
            y[r] = yr;
        }
    }
    const int pn = APPLY ? p + 1 : 0;
    if (pn >= np) return;
    const int64_t jn = (int64_t)pn * QB;
    double prod[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int64_t rr = r - jn;
        prod[i] = 0.0;
        if (r < Np && rr >= i) prod[i] = (rr == i ? 1.0 : F[r + (jn + i) * ld]) * yr;
    }
    qr_block_reduce_store(prod, red, Pout + (int64_t)b * 64);
}

// Block q of the back substitution: every workgroup solves R_qq x_q = y_q (one wave, R_qq staged in LDS), workgroup 0 stores
// x_q, and every workgroup subtracts R(r, q-block) x_q from its 256 rows r < 64 q of y.
__global__ __launch_bounds__(256) void qr_rsolve_kernel(const double* __restrict__ F, int64_t ld, int q, double* __restrict__ y,
                                                        double* __restrict__ x) {
    __shared__ double Rs[64 * 65], xs[64];
    const int tid = threadIdx.x;
    const int64_t d0 = (int64_t)q * QB;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int l = e & 63, i = e >> 6;
        Rs[l * 65 + i] = F[d0 + l + (d0 + i) * ld];
    }
    __syncthreads();
    if (tid < 64) {
        double yl = y[d0 + tid], xv = 0.0;
        for (int i = QB - 1; i >= 0; --i) {
            const double xi = __shfl(yl / Rs[i * 65 + i], i);
            if (tid == i) xv = xi;
            if (tid < i) yl -= Rs[tid * 65 + i] * xi;
        }
        xs[tid] = xv;
        if (blockIdx.x == 0) x[d0 + tid] = xv;
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * QR_RB + tid;
    if (r < d0) {
        double yr = y[r];
#pragma unroll 8
        for (int i = 0; i < QB; ++i) yr -= F[r + (d0 + i) * ld] * xs[i];
        y[r] = yr;
    }
}

static int qr_nblk(int64_t Np) { return (int)((Np + QR_RB - 1) / QR_RB); }

// K-splits of a W^T product with n2 output rows: enough workgroups to cover the chip, at least 256 rows of K per split.
static void qr_splits(int64_t K, int64_t n2, int64_t* kchunk, int* S) {
    const int64_t tiles = n2 / 64;
    int64_t s = (512 + tiles - 1) / tiles;
    s = std::max<int64_t>(1, std::min<int64_t>({s, (int64_t)QR_SMAX, K / 256}));
    const int64_t ch = round_up((K + s - 1) / s, 16);
    *kchunk = ch;
    *S = (int)((K + ch - 1) / ch);
}

static int launch_tn(hipStream_t s, const double* A, int64_t lda, const double* V, int64_t ldv, int64_t K, int64_t n2,
                     double* Wp, int64_t ldw, int64_t wstride, int* S) {
    int64_t kchunk;
    qr_splits(K, n2, &kchunk, S);
    hipLaunchKernelGGL(qr_tn_kernel, dim3((unsigned)(n2 / 64), (unsigned)*S), dim3(256), 0, s, A, lda, V, ldv, K, kchunk, Wp,
                       ldw, wstride);
    return 0;
}

struct QrSolver final : mnk_ls_alt {
    // V of the current panel, the T of every panel (kept for the solves), split-K partials of W^T = A2^T V and W^T T, partial
    // sums of the panel / solve kernels
    DevBuf<double> qr_v, qr_t, qr_w, qr_p;

    int alloc(mnk_ls* ls) override {
        const int64_t Np = ls->Np;
        int rc = qr_v.alloc((size_t)Np * QB + SLACK * QB);
        rc |= qr_t.alloc((size_t)(Np / QB) * QB * QB);
        rc |= qr_w.alloc((size_t)(QR_SMAX + 1) * Np * QB + SLACK * QB);
        rc |= qr_p.alloc((size_t)2 * qr_nblk(Np) * 64 + 2 * 64);
        return rc;
    }

    // factorize! of a QR solver: the matrix has been transferred (lower triangle); mirror it and factor it (see the top).
    int factor(mnk_ls* ls) override {
        hipStream_t s = ls->ctx->stream;
        double* F = ls->fact.p;
        const int64_t ld = ls->ld, N = ls->N, Np = ls->Np;
        const int np = (int)(Np / QB), nblk = qr_nblk(Np);
        int rc = mnk_launch_tril_to_full(s, F, ld, N, Np);
        if (rc) return rc;
        double* P[2] = {qr_p.p, qr_p.p + (int64_t)nblk * 64};
        double* R[2] = {qr_p.p + (int64_t)2 * nblk * 64, qr_p.p + (int64_t)2 * nblk * 64 + 64};
        double *V = qr_v.p, *Wp = qr_w.p;
        const int64_t ldw = Np, wstride = Np * QB;
        double* Wt = Wp + (int64_t)QR_SMAX * wstride;
        for (int p = 0; p < np; ++p) {
            const int64_t j0 = (int64_t)p * QB, m = Np - j0, n2 = m - QB;
            const int nb = (int)((m + QR_RB - 1) / QR_RB);
            hipLaunchKernelGGL(qr_panel_kernel<false>, dim3(nb), dim3(256), 0, s, F, ld, j0, Np, -1, nullptr, nullptr, P[0], R[0],
                               ls->dvec.p, nb);
            for (int c = 0; c < QB; ++c)
                hipLaunchKernelGGL(qr_panel_kernel<true>, dim3(nb), dim3(256), 0, s, F, ld, j0, Np, c, P[c & 1], R[c & 1],
                                   P[(c + 1) & 1], R[(c + 1) & 1], ls->dvec.p, nb);
            hipLaunchKernelGGL(qr_extract_v_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, F, ld, j0, m, V, Np);
            int S;
            launch_tn(s, V, Np, V, Np, m, QB, Wp, ldw, wstride, &S);
            double* T = qr_t.p + (int64_t)p * QB * QB;
            hipLaunchKernelGGL(qr_form_t_kernel, dim3(1), dim3(256), 0, s, Wp, ldw, wstride, S, ls->dvec.p + j0, T);
            if (n2 > 0) {
                double* A2 = F + j0 + (j0 + QB) * ld;
                launch_tn(s, A2, ld, V, Np, m, n2, Wp, ldw, wstride, &S);
                hipLaunchKernelGGL(qr_wt_kernel, dim3((unsigned)(n2 / 64)), dim3(256), 0, s, Wp, ldw, wstride, S, T, Wt);
                MNK_HIP(hipGetLastError());
                rc = launch_gemm_nt(s, 0, m, n2, QB, V, Np, Wt, ldw, A2, ld, nullptr, nullptr, 0, nullptr);
                if (rc) return rc;
            }
        }
        MNK_HIP(hipGetLastError());
        return 0;
    }

    // geqrf's info is always 0; a singular matrix shows up in the solve
    int fetch_info(mnk_ls* ls) override {
        MNK_HIP(stream_wait(ls->ctx->stream));
        ls->verdict.accept(0, 0, 0, 0);
        return 0;
    }

    // solve_qr! (reference src/LinearSolvers/lapack.jl:205-209): Q^T then R^-1 on the zero-padded copy y of b; the solution
    // (Np entries) goes to xo and its first N entries to x.
    int solve_vec(mnk_ls* ls, const double* b, double* x) override {
        hipStream_t s = ls->ctx->stream;
        const double* F = ls->fact.p;
        const int64_t ld = ls->ld, N = ls->N, Np = ls->Np;
        const int np = (int)(Np / QB), nblk = qr_nblk(Np);
        double* y = ls->xwork.p + Np;
        double* xo = ls->xwork.p + 2 * Np;
        double* P[2] = {qr_p.p, qr_p.p + (int64_t)nblk * 64};
        MNK_HIP(hipMemsetAsync(y, 0, Np * sizeof(double), s));
        MNK_HIP(hipMemcpyAsync(y, b, N * sizeof(double), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(qr_qt_kernel<false>, dim3(nblk), dim3(256), 0, s, F, ld, Np, -1, np, y, qr_t.p, nullptr, P[0], nblk);
        for (int p = 0; p < np; ++p) {
            const int b0 = (int)((int64_t)p * QB / QR_RB);
            hipLaunchKernelGGL(qr_qt_kernel<true>, dim3(nblk - b0), dim3(256), 0, s, F, ld, Np, p, np, y, qr_t.p, P[p & 1],
                               P[(p + 1) & 1], nblk);
        }
        MNK_HIP(hipGetLastError());
        int rc = mnk_launch_upper_bsolve(s, F, ld, Np, y, xo);
        if (rc) return rc;
        MNK_HIP(hipMemcpyAsync(x, xo, N * sizeof(double), hipMemcpyDeviceToDevice, s));
        return 0;
    }

    const char* no_inertia_message() const override { return "mnk_ls_inertia: a QR factorization reveals no inertia (is_inertia is false for QR)"; }
};

}  // namespace mnk

using namespace mnk;

// (lu.hip) the same mirror and the same block back substitution for the LU solver
int mnk_launch_tril_to_full(hipStream_t s, double* F, int64_t ld, int64_t N, int64_t Np) {
    hipLaunchKernelGGL(qr_mirror_kernel, dim3((unsigned)(Np / 32), (unsigned)(Np / 32)), dim3(256), 0, s, F, ld, N);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_launch_upper_bsolve(hipStream_t s, const double* F, int64_t ld, int64_t Np, double* y, double* x) {
    for (int q = (int)(Np / QB) - 1; q >= 0; --q) {
        const int64_t d0 = (int64_t)q * QB;
        const unsigned g = (unsigned)std::max<int64_t>(1, (d0 + QR_RB - 1) / QR_RB);
        hipLaunchKernelGGL(qr_rsolve_kernel, dim3(g), dim3(256), 0, s, F, ld, q, y, x);
    }
    MNK_HIP(hipGetLastError());
    return 0;
}

std::unique_ptr<mnk_ls_alt> mnk_qr_new() { return std::make_unique<QrSolver>(); }

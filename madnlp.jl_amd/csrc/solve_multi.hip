// Blocked solve! for several right-hand sides (SOLVE_BLOCKED of solve_plan.h): `solve_linear_system!(M, X::AbstractMatrix)` of
// the contract (reference src/LinearSolvers/linearsolvers.jl:102-110), for the static-pivot tier (CHOLESKY / LDL).
//
// The column loop of mnk_ls_solve streams the whole factor through both sweeps once per column.  Here a chunk of up to
// SP_MULTI_W right-hand sides goes through both sweeps together, so each sweep reads the factor once per chunk, and the
// products run on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).
//
// Layout.  The working block is kept transposed, right-hand-side index fastest: P[r + ldr * i] is entry i of column r, ldr =
// the chunk's padded width (a multiple of 16), i < Np.  Two such blocks P and Q swap roles step by step:
//   forward, 256-column step j :  Q_j = linv256_j P_j            ;  P[below] -= L[below, j] Q_j
//   LDL only                   :  Q <- D^-1 Q
//   backward, last step first  :  P_j = linv256t_j Q_j           ;  Q[before] -= L[j, before]^T P_j
// All four are ONE kernel, C (=|-=) A X: a workgroup owns SM_ROWS rows of C and every column of the chunk; its four waves
// take a quarter of the k range each and their partial sums meet in LDS in the fixed order ((0 + 1) + (2 + 3)).  With the
// MFMA operand maps  A[i = lane % 16][k = lane / 16],  B[k = lane / 16][j = lane % 16],  D[i = lane / 16 + 4 reg][j = lane % 16]
// and j = the right-hand side, every operand load and every store of the working block is 16 consecutive doubles, and
// the factor's columns are read in 128-byte pieces without a trip through LDS.  The backward update reads L[j, before]^T:
// its k runs down a column of L, so a lane loads four consecutive k (32 bytes) and uses them in four MFMA steps -- the k
// order within sixteen is permuted, the same way in both operands.
//
// What follows from the form: no atomics, one owner per destination element and a fixed k order, so a solve repeats bit for
// bit; column r of the result depends on column r of the operand only (an MFMA's D[i][j] reads row i of A and column j of
// B), so it is the same bits for any nrhs, any position in X and any contents of the other columns, NaN included; the
// padding columns are zero.  Launches per chunk: 4 per 256-column step (minus the two updates that have no rows) + pack,
// unpack and the D^-1 scaling.  Nothing waits for another workgroup, and the publication buffers of the one-launch solves
// (xwork) are not touched: the workspace is the solver's own `xmulti`, allocated by its first blocked solve.
#include "ls.h"

namespace mnk {

typedef double sm_v4 __attribute__((ext_vector_type(4)));
typedef double sm_v2 __attribute__((ext_vector_type(2)));

constexpr int SM_STEP = 256;           // columns per step (the explicit inverses linv256 / linv256t)
constexpr int SM_RT = 2;               // 16-row MFMA tiles of C per workgroup
constexpr int SM_ROWS = 16 * SM_RT;    // rows of C per workgroup
constexpr int SM_TRI_NONE = 0, SM_TRI_LOWER = 1, SM_TRI_UPPER = 2;

// C[i, :] (=|-=) sum_k A(i, k) X[k, :] for the SM_ROWS rows i of this workgroup and the 16 NT columns of the chunk.
//   TRANS = false: A(i, k) = A[i + lda k]   (the panel of L below a step, or an explicit inverse)
//   TRANS = true : A(i, k) = A[k + lda i]   (the rows of L in a step, read down its columns)
// X[r + ldr k], C[r + ldr i] with ldr = 16 NT.  K: the k range (a multiple of 64, at most 256), wave w takes [w kq, (w + 1) kq) of
// it: kq = 64 without TRANS, a multiple of 16 up to 64 with it.
// `tri`: A is a 256 x 256 explicit inverse whose 64-column quarters right of (SM_TRI_LOWER) / left of (SM_TRI_UPPER) the
// 64-row block of its rows are structurally zero and are skipped, as diag256_kernel skips them.
template <int NT, bool TRANS>
__global__ __launch_bounds__(256) void sm_product_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ X,
                                                         double* __restrict__ C, int K, int kq, int tri, int subtract) {
    constexpr int ldr = 16 * NT;
    constexpr int NACC = SM_RT * NT * 4;
    __shared__ double part[4][NACC][64];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int row0 = blockIdx.x * SM_ROWS;
    const int k0 = w * kq, k1 = k0 + kq < K ? k0 + kq : K;
    const bool wanted = tri == SM_TRI_NONE || (tri == SM_TRI_LOWER ? (k0 >> 6) <= (row0 >> 6) : (k0 >> 6) >= (row0 >> 6));
    sm_v4 acc[SM_RT][NT];
#pragma unroll
    for (int rt = 0; rt < SM_RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = sm_v4{0.0, 0.0, 0.0, 0.0};
    if (wanted && k0 < k1) {   // (uniform over the wave)
        if (!TRANS) {
            // (a wave's k range here is always 64 wide: the quarters of an inverse, or of a full step -- the last, short step
            // has no rows below it)
            const double* Ap = A + row0 + l15 + lda * (int64_t)(k0 + l4);
            const double* Xp = X + l15 + (int64_t)ldr * (k0 + l4);
#pragma unroll 4
            for (int it = 0; it < 16; ++it) {
                double a[SM_RT], x[NT];
#pragma unroll
                for (int rt = 0; rt < SM_RT; ++rt) a[rt] = Ap[16 * rt];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) x[nt] = Xp[16 * nt];
#pragma unroll
                for (int rt = 0; rt < SM_RT; ++rt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], x[nt], acc[rt][nt], 0, 0, 0);
                Ap += 4 * lda;
                Xp += 4 * ldr;
            }
        } else {
            // sixteen k per turn: the lanes of group l4 hold k = 4 l4 + s in MFMA step s, in A and in X alike
            // (at most four turns: all of the wave's part of L is requested before the first product)
            const double* Ap = A + (k0 + 4 * l4) + lda * (int64_t)(row0 + l15);
            const double* Xp = X + l15 + (int64_t)ldr * (k0 + 4 * l4);
            const int nit = (k1 - k0) >> 4;
            sm_v2 a[4][SM_RT][2];
#pragma unroll
            for (int it = 0; it < 4; ++it)
                if (it < nit) {
#pragma unroll
                    for (int rt = 0; rt < SM_RT; ++rt) {
                        const sm_v2* p = reinterpret_cast<const sm_v2*>(Ap + 16 * it + 16 * rt * lda);
                        a[it][rt][0] = p[0];
                        a[it][rt][1] = p[1];
                    }
                }
#pragma unroll
            for (int it = 0; it < 4; ++it)
                if (it < nit) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        double x[NT];
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) x[nt] = Xp[16 * nt + ldr * (16 * it + s)];
#pragma unroll
                        for (int rt = 0; rt < SM_RT; ++rt)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                acc[rt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[it][rt][s >> 1][s & 1], x[nt], acc[rt][nt], 0, 0, 0);
                    }
                }
        }
    }
#pragma unroll
    for (int rt = 0; rt < SM_RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[w][(rt * NT + nt) * 4 + r][lane] = acc[rt][nt][r];
    __syncthreads();
    // wave w adds up and stores register w of every tile: row 16 rt + l4 + 4 w, column 16 nt + l15
#pragma unroll
    for (int rt = 0; rt < SM_RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int e = (rt * NT + nt) * 4 + w;
            const double sum = (part[0][e][lane] + part[1][e][lane]) + (part[2][e][lane] + part[3][e][lane]);
            double* c = C + (16 * nt + l15) + (int64_t)ldr * (row0 + 16 * rt + l4 + 4 * w);
            *c = subtract ? *c - sum : sum;
        }
}

// Q[r + ldr i] *= dinv[i]
__global__ void sm_scale_kernel(double* __restrict__ Q, const double* __restrict__ dinv, int ldr, int64_t n) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < n) Q[e] *= dinv[e / ldr];
}

// The caller's columns src[i + lds r] (i < N, r < cols) into the zero-padded working block P[r + ldr i] (i < Np, r < ldr),
// 64 rows per workgroup, transposed through LDS so that both sides move whole lines.
__global__ __launch_bounds__(256) void sm_pack_kernel(double* __restrict__ P, int ldr, const double* __restrict__ src, int64_t lds,
                                                      int64_t N, int cols) {
    __shared__ double tile[64][65];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 64;
    for (int r = t >> 6; r < ldr; r += 4) {
        const int64_t i = i0 + (t & 63);
        tile[r][t & 63] = (i < N && r < cols) ? src[i + lds * r] : 0.0;
    }
    __syncthreads();
    for (int e = t; e < 64 * ldr; e += 256) P[(int64_t)ldr * i0 + e] = tile[e % ldr][e / ldr];
}

// ... and back: rows < N and columns < cols only
__global__ __launch_bounds__(256) void sm_unpack_kernel(double* __restrict__ dst, int64_t ldd, const double* __restrict__ P, int ldr,
                                                        int64_t N, int cols) {
    __shared__ double tile[64][65];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 64;
    for (int e = t; e < 64 * ldr; e += 256) tile[e % ldr][e / ldr] = P[(int64_t)ldr * i0 + e];
    __syncthreads();
    for (int r = t >> 6; r < cols; r += 4) {
        const int64_t i = i0 + (t & 63);
        if (i < N) dst[i + ldd * r] = tile[r][t & 63];
    }
}

namespace {

template <int NT>
void sm_launch_nt(bool trans, hipStream_t s, int64_t rows, const double* A, int64_t lda, const double* X, double* C, int K, int kq, int tri,
                  int subtract) {
    const dim3 grid((unsigned)(rows / SM_ROWS)), block(256);
    if (trans) hipLaunchKernelGGL((sm_product_kernel<NT, true>), grid, block, 0, s, A, lda, X, C, K, kq, tri, subtract);
    else hipLaunchKernelGGL((sm_product_kernel<NT, false>), grid, block, 0, s, A, lda, X, C, K, kq, tri, subtract);
}

// `rows` rows of C (a multiple of SM_ROWS), chunk of padded width 16 nt
void sm_launch(int nt, bool trans, hipStream_t s, int64_t rows, const double* A, int64_t lda, const double* X, double* C, int K, int kq,
               int tri, int subtract) {
    if (rows <= 0) return;
    switch (nt) {
        case 1: sm_launch_nt<1>(trans, s, rows, A, lda, X, C, K, kq, tri, subtract); break;
        case 2: sm_launch_nt<2>(trans, s, rows, A, lda, X, C, K, kq, tri, subtract); break;
        case 3: sm_launch_nt<3>(trans, s, rows, A, lda, X, C, K, kq, tri, subtract); break;
        default: sm_launch_nt<4>(trans, s, rows, A, lda, X, C, K, kq, tri, subtract); break;
    }
}

}  // namespace
}  // namespace mnk

using namespace mnk;

SolveMultiPlan mnk_ls_plan_multi(const mnk_ls* ls, int64_t nrhs) {
    return solve_plan_multi(mnk_ls_solve_shape(ls), nrhs, ls->solves.multi_rhs_min);
}

// The blocked solve of x (N x nrhs, leading dimension ldx, host or device) as `mp` says (mp.path == SOLVE_BLOCKED).
int mnk_ls_run_solve_multi(mnk_ls* ls, double* x, int64_t nrhs, int64_t ldx, int loc, const SolveMultiPlan& mp) {
    { int rc_q = mnk_solve_sync_deferred(ls); if (rc_q) return rc_q; }   // (queued single solves of this solver keep their place)
    hipStream_t s = ls->ctx->stream;
    const int64_t N = ls->N, Np = ls->Np, ld = ls->ld;
    const int64_t W = mp.W;
    const size_t need = (size_t)(2 * W * Np + W * N);   // P | Q | the staging block of host data
    if (ls->xmulti.n < need && ls->xmulti.alloc(need)) return -2;   // (alloc has called set_error)
    double* P = ls->xmulti.p;
    double* Q = P + W * Np;
    double* S = Q + W * Np;
    const bool ldl = ls->algo == MNK_LDL;
    const int64_t nsteps = (Np + SM_STEP - 1) / SM_STEP;
    const unsigned nblk = (unsigned)(Np / 64);
    for (int64_t c = 0; c < mp.chunks; ++c) {
        const int64_t c0 = c * W;
        const int cols = (int)std::min<int64_t>(W, nrhs - c0);
        const int ldr = c == mp.chunks - 1 ? mp.last_padded : (int)W;
        const int nt = ldr / 16;
        double* xc = x + c0 * ldx;
        double* io = xc;   // what the pack / unpack kernels read and write
        int64_t ldio = ldx;
        if (loc != MNK_DEVICE) {
            MNK_HIP(h2d_copy_2d(S, N * sizeof(double), xc, ldx * sizeof(double), N * sizeof(double), (size_t)cols, s));
            io = S;
            ldio = N;
        }
        hipLaunchKernelGGL(sm_pack_kernel, dim3(nblk), dim3(256), 0, s, P, ldr, (const double*)io, ldio, N, cols);
        for (int64_t k = 0; k < nsteps; ++k) {
            const int64_t j0 = k * SM_STEP;
            const int ncol = (int)std::min<int64_t>(SM_STEP, Np - j0);
            sm_launch(nt, false, s, ncol, ls->linv256.p + k * (int64_t)(SM_STEP * SM_STEP), SM_STEP, P + ldr * j0, Q + ldr * j0, ncol, 64,
                      SM_TRI_LOWER, 0);
            sm_launch(nt, false, s, Np - j0 - ncol, ls->fact.p + (j0 + ncol) + j0 * ld, ld, Q + ldr * j0, P + ldr * (j0 + ncol), ncol, ncol / 4,
                      SM_TRI_NONE, 1);
        }
        if (ldl)
            hipLaunchKernelGGL(sm_scale_kernel, dim3((unsigned)((ldr * Np + 255) / 256)), dim3(256), 0, s, Q, (const double*)ls->dinv.p, ldr,
                               ldr * Np);
        for (int64_t k = nsteps - 1; k >= 0; --k) {
            const int64_t j0 = k * SM_STEP;
            const int nrow = (int)std::min<int64_t>(SM_STEP, Np - j0);
            sm_launch(nt, false, s, nrow, ls->linv256t.p + k * (int64_t)(SM_STEP * SM_STEP), SM_STEP, Q + ldr * j0, P + ldr * j0, nrow, 64,
                      SM_TRI_UPPER, 0);
            sm_launch(nt, true, s, j0, ls->fact.p + j0, ld, P + ldr * j0, Q, nrow, nrow / 4, SM_TRI_NONE, 1);
        }
        hipLaunchKernelGGL(sm_unpack_kernel, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, s, io, ldio, (const double*)P, ldr, N, cols);
        MNK_HIP(hipGetLastError());
        if (loc != MNK_DEVICE)
            MNK_HIP(d2h_copy_2d(xc, ldx * sizeof(double), S, N * sizeof(double), N * sizeof(double), (size_t)cols, s));
    }
    ls->solves.last_path = SOLVE_BLOCKED;
    ls->solves.last_rhs_chunks = mp.chunks;
    return 0;
}

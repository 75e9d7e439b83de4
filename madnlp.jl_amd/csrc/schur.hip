// Dense `S` stage of the Schur-complement KKT system (reference src/KKT/Schur/schur.jl:927-1001 `build_kkt!`,
// :1003-1005 `factorize_kkt!`, :1040-1065 steps 3-5 of `solve_kkt!`): SURVEY 8(f).3.
//
// Two-stage structure: ns scenario blocks A_k (blk x blk, symmetric indefinite) coupled to nd design variables by
// dense C_dk (nd x blk); the Schur complement the dense linear solver sees is
//       S = S0 - sum_k C_dk A_k^-1 C_dk',        S0 = H_dd + Sigma_dd + inequality terms,
// and a solve is   r_k <- A_k^-1 r_k ;  r_d <- r_d - sum_k C_dk r_k ;  S x_d = r_d ;  x_k = r_k - (A_k^-1 C_dk') x_d.
// The reference factors the A_k with a sparse solver per scenario (MUMPS; sparse direct solvers are out of this
// path's scope); here the scenario blocks arrive dense and are factored by the same blocked fp64-MFMA factorization
// as S itself (BUNCHKAUFMAN tiers: the blocks are indefinite).  With a static-pivot factor A_k = L D L' the term is
// C A^-1 C' = (C L^-T) D^-1 (C L^-T)': ONE forward sweep over the nd rows of C_dk (right-side block triangular solve
// on MFMA) and one MFMA rank-blk update of S; a block that needed the pivoted tier falls back to the reference's
// column-by-column T_k = A_k^-1 C_dk' and S -= C_dk T_k.
//
// Multi-GPU: scenarios are sharded over the ranks.  mnk_schur_build_local produces THIS rank's contribution
// (S0 on the rank that owns it, minus its scenarios' terms) into a caller-owned device buffer; the caller sums the
// contributions with ONE all-reduce of nd^2 doubles (RCCL over xGMI) and every rank factors S; a solve needs one more
// all-reduce of nd doubles (mnk_schur_forward's contribution).  The library itself does no communication.
#include <vector>

#include "gemm_tile.h"
#include "kkt_vec.h"
#include "ls.h"
#include "schur_plan.h"

struct mnk_schur {
    mnk_ctx* ctx = nullptr;
    int64_t ns = 0, blk = 0, nd = 0, ndp = 0, blkp = 0;
    int algo = MNK_BUNCHKAUFMAN;
    mnk::DevBuf<double> A;    // ns x (blk x blk)   scenario blocks (lower triangle read)
    mnk::DevBuf<double> C;    // ns x (nd x blk)    coupling blocks
    mnk::DevBuf<double> T;    // blk x nd    A_k^-1 C_dk' of ONE scenario (pivoted-tier fallback only)
    mnk::DevBuf<double> Cp;   // ndp x Npb   X = C_dk L^-T D^-1 (fast path) / zero-padded C_dk (fallback)   (MFMA operand)
    mnk::DevBuf<double> Tt;   // ndp x Npb   V = C_dk L^-T (fast path) / zero-padded T_k' (fallback)         (MFMA operand)
    mnk::DevBuf<double> tmpk; // Npb         C_dk' x_d of one scenario (back-substitution)
    int64_t Npb = 0;          // padded order of a scenario factor (multiple of 128)
    mnk::DevBuf<double> Sp;   // ndp x ndp   accumulator
    std::vector<mnk_ls*> ls_k;
    mnk_ls* ls_s = nullptr;
    std::vector<int> info_k;
    bool built = false;
    // build_kkt!: the forward sweeps of ALL scenarios with a static-pivot factor run as grouped launches (one per 64-column
    // step: blockIdx.y = scenario) on per-scenario X / V buffers, their products X_k V_k' as one batched product into
    // per-scenario partial sums that are added to S in scenario order (the same bits whatever the timing)
    mnk::DevBuf<double> Xall, Vall, Pall;   // ns x (ndp x Npb) | the same (LDL^T only) | ns x (ndp x ndp)
    mnk::DevBuf<char> recs;                 // device copies of the launch records
    mnk::DevBuf<int> fast_k;                // the scenarios on the grouped path
    int64_t chunk = 32;                     // scenarios per pass of the grouped build (their X / V / P buffers are reused)
    char* stage = nullptr;                  // pinned host memory: the launch records + scenario list of one pass (no synchronizing upload)
    size_t stage_bytes = 0;
    hipEvent_t stage_ev = nullptr;          // recorded behind the last upload from `stage`
    mnk::DevBuf<double> Sown;               // nd x nd: the handle's own copy of S (mnk_schur_s_buffer: callers without device memory of their own)
    mnk::DevBuf<double> hostrk, hostrd;     // mnk_schur_solve with host vectors: ns x blk | 2 nd (right-hand side, contribution)
    // ---- device-side assembly of A_k / C_dk / S0 from the callbacks' COO values (mnk_schur_set_structure / mnk_schur_assemble):
    // every touched entry of the three buffers is one SEGMENT of sources, summed by one thread in a fixed order (no atomics)
    struct {
        bool have = false;
        int64_t n = 0, m = 0, nv = 0, nc = 0, nnzh = 0, nnzj = 0, n_ineq = 0, nseg = 0, nsrc = 0;
        mnk::DevBuf<int64_t> seg_dst;           // nseg: virtual offset into [A | C | S0]
        mnk::DevBuf<int32_t> seg_ptr;           // nseg + 1
        mnk::DevBuf<int8_t> src_kind;           // 0 hess[a], 1 jac[a], 2 pr_diag[a], 3 du_diag[a], 4 jac[a] * D[w] * jac[b]
        mnk::DevBuf<int32_t> src_a, src_b, src_w;
        mnk::DevBuf<int64_t> ind_ineq;          // constraint row of slack p
        mnk::DevBuf<double> D, S0, vals;        // n_ineq | nd x nd | staging of host inputs: hess | jac | pr_diag | du_diag
        // long inequality rows (more than T COO entries; schur_plan.h): no pairs -- their entries are staged into dense zero-padded
        // operands and condensed by three weighted Gram products on the matrix cores behind schur_assemble_kernel
        int64_t stats[5] = {0, 0, 0, 0, 0};     // mnk_schur_assembly_stats
        int64_t long_rows = 0, nvp = 0, ndp = 0, Kp = 0, nslot = 0, nchunk = 0;
        mnk::DevBuf<int64_t> slot_dst;          // nslot: offset into W (and DW)
        mnk::DevBuf<int32_t> slot_ptr, slot_src, slot_p;   // nslot + 1 | COO entries of the slots | slack index of a slot's row
        mnk::DevBuf<double> W, DW;              // [Wv_0 .. Wv_ns-1 (nvp x Kp each) | Wd_0 .. Wd_ns-1 (ndp x Kp each)] and its twin D W
        mnk::DevBuf<double> P;                  // nchunk x (nd x nd): the partial sums of the S0 product, one per K chunk
    } as;
    int64_t gram_T = -1;                        // Gram row threshold of the next mnk_schur_set_structure (negative: the default)
    // ---- device-side solve_kkt! / mul! / jtprod! / mul_hess_blk! on ONE rank (mnk_schur_solve_kkt and its kin): the bound / barrier
    // state every KKT handle has (kkt_vec.h; npr = n + n_ineq, npd = n + n_ineq + m), the row lists of J, J' and Symmetric(H, :L)
    // over the COO values of the last mnk_schur_assemble (schur_plan.h), and the work vectors of the solve.  The handle's own
    // pr_diag / du_diag are the last two parts of as.vals: an assemble with explicit diagonals copies them there, one without uses
    // what the feeders (mnk_schur_set_aug_diagonal, mnk_schur_regularize_diagonal) left.
    struct SpmvDev {
        int64_t rows = 0, nlong = 0;
        mnk::DevBuf<int32_t> ptr, idx, perm, long_rows;
    };
    struct {
        bool have = false;                      // false: no structure yet, or a sharded handle
        bool have_vals = false;                 // an assemble has filled as.vals
        bool have_jac = false, have_hess = false;   // ... or a compress call its Jacobian / Hessian part
        mnk::KktVecState st;
        SpmvDev op[3];                          // SCHUR_OP_J, SCHUR_OP_JT, SCHUR_OP_H
        int64_t T = 0, n_eq = 0;
        mnk::DevBuf<int64_t> eq_rows;           // ascending: scenario k's equality rows at [k * nc_eq, (k + 1) * nc_eq)
        mnk::DevBuf<double> buffer, buffer2;    // m each: the condensed inequality right-hand side | J wx
        mnk::DevBuf<double> rk, rd;             // ns x blk | nd: the stage's right-hand sides
        mnk::DevBuf<double> va, vb;             // staging of host vectors of jtprod! / mul_hess_blk! (n + n_ineq + m each)
    } kv;
    int64_t spmv_T = -1;                        // product row threshold of the next mnk_schur_set_structure (negative: the default)
    double* hess_v() { return as.vals.p; }
    double* jac_v() { return as.vals.p + as.nnzh; }
    double* pr_diag() { return as.vals.p + as.nnzh + as.nnzj; }
    double* du_diag() { return as.vals.p + as.nnzh + as.nnzj + as.n + as.n_ineq; }
};

namespace mnk {

// dst (rows_d x cols_d, ld ldd; zero padding beyond the source) = src' or src
__global__ void schur_copy_kernel(double* __restrict__ dst, int64_t ldd, int64_t rows_d, int64_t cols_d,
                                  const double* __restrict__ src, int64_t lds, int64_t rows_s, int64_t cols_s, int trans) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= rows_d * cols_d) return;
    const int64_t r = e % rows_d, c = e / rows_d;
    double v = 0.0;
    if (trans) { if (c < rows_s && r < cols_s) v = src[c + r * lds]; }   // dst[r][c] = src[c][r]
    else { if (r < rows_s && c < cols_s) v = src[r + c * lds]; }
    dst[r + c * ldd] = v;
}

// S += P_0 + P_1 + ... (the scenarios' partial sums, in scenario order)
__global__ void schur_partial_sum_kernel(double* __restrict__ S, const double* __restrict__ P, int64_t np, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = S[i];
    for (int64_t k = 0; k < np; ++k) v += P[k * n + i];
    S[i] = v;
}
// X_i (ndp x Npb, zero padded) = C_dk of scenario k = fast_k[i]   (blockIdx.y = i)
__global__ void schur_copy_batch_kernel(double* __restrict__ Xall, int64_t ndp, int64_t Npb, const double* __restrict__ Call,
                                        int64_t nd, int64_t blk, const int* __restrict__ fast_k) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= ndp * Npb) return;
    const int64_t r = e % ndp, c = e / ndp;
    const double* src = Call + (int64_t)fast_k[blockIdx.y] * nd * blk;
    Xall[(int64_t)blockIdx.y * ndp * Npb + e] = (r < nd && c < blk) ? src[r + c * nd] : 0.0;
}
// The per-scenario vector kernels of a solve, scenario k = blockIdx.y, ONE launch each (ns launches of a few microseconds were
// most of a solve).  Fixed summation orders: deterministic.
// P[k][r] = sum_c C_k[r + c*nd] x_k[c], then y[r] = sum_k alpha P[k][r] in scenario order
__global__ __launch_bounds__(256) void schur_gemv_batch_kernel(double* __restrict__ P, const double* __restrict__ Call, int64_t nd,
                                                               const double* __restrict__ xall, int64_t blk) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, k = blockIdx.y;
    if (r >= nd) return;
    const double* A = Call + k * nd * blk;
    const double* x = xall + k * blk;
    double s0 = 0.0, s1 = 0.0;
    int64_t c = 0;
    for (; c + 1 < blk; c += 2) {
        s0 = fma(A[r + c * nd], x[c], s0);
        s1 = fma(A[r + (c + 1) * nd], x[c + 1], s1);
    }
    if (c < blk) s0 = fma(A[r + c * nd], x[c], s0);
    P[k * nd + r] = s0 + s1;
}
__global__ void schur_contrib_sum_kernel(double* __restrict__ y, const double* __restrict__ P, int64_t ns, int64_t nd, double alpha) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= nd) return;
    double v = 0.0;
    for (int64_t k = 0; k < ns; ++k) v += alpha * P[k * nd + r];
    y[r] = v;
}
// tmp_k[c] = sum_r C_k[r + c*nd] x_d[r]
__global__ __launch_bounds__(256) void schur_gemv_t_batch_kernel(double* __restrict__ tmp, int64_t stride, const double* __restrict__ Call,
                                                                 int64_t nd, const double* __restrict__ x, int64_t blk) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, k = blockIdx.y;
    if (c >= blk) return;
    const double* a = Call + k * nd * blk + c * nd;
    double s0 = 0.0, s1 = 0.0;
    int64_t r = 0;
    for (; r + 1 < nd; r += 2) {
        s0 = fma(a[r], x[r], s0);
        s1 = fma(a[r + 1], x[r + 1], s1);
    }
    if (r < nd) s0 = fma(a[r], x[r], s0);
    tmp[k * stride + c] = s0 + s1;
}
// rhs_k[i] -= tmp_k[i]
__global__ void schur_sub_batch_kernel(double* __restrict__ y, int64_t blk, const double* __restrict__ tmp, int64_t stride) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i < blk) y[k * blk + i] -= tmp[k * stride + i];
}

// y += x (the design right-hand side receives the scenarios' contribution)
__global__ void schur_axpy_kernel(double* __restrict__ y, const double* __restrict__ x, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) y[i] += x[i];
}

}  // namespace mnk

namespace mnk {
// D = Sigma_s / (1 - Sigma_d Sigma_s) of every inequality row (reference schur.jl:929-933), rounded operation by operation
__global__ void schur_condense_weights_kernel(double* __restrict__ D, const double* __restrict__ pr_diag, const double* __restrict__ du_diag,
                                              const int64_t* __restrict__ ind_ineq, int64_t n, int64_t n_ineq) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n_ineq) return;
    const double Ss = pr_diag[n + p], Sd = du_diag[ind_ineq[p]];
    D[p] = __ddiv_rn(Ss, __dsub_rn(1.0, __dmul_rn(Sd, Ss)));
}
// One thread per touched entry of [A | C | S0]: its sources in the order the reference scatters them (Hessian entries, diagonal
// terms, equality-row Jacobian entries, the condensation pairs J' D J row by row: schur.jl:935-972), every operation rounded on
// its own (no contraction into fma): the entry carries the bits a sequential scatter-add produces.  The reference's GPU twin
// (lib/MadNLPGPU/ext/MadNLPGPUCUDAExt/kernels_schur.jl:14-174) adds with @atomic -- an order that changes from run to run.
__global__ void schur_assemble_kernel(int64_t nseg, const int64_t* __restrict__ seg_dst, const int32_t* __restrict__ seg_ptr,
                                      const int8_t* __restrict__ kind, const int32_t* __restrict__ sa, const int32_t* __restrict__ sb,
                                      const int32_t* __restrict__ sw, const double* __restrict__ hess, const double* __restrict__ jac,
                                      const double* __restrict__ pr_diag, const double* __restrict__ du_diag, const double* __restrict__ D,
                                      double* __restrict__ A, int64_t sizeA, double* __restrict__ Cb, int64_t sizeC, double* __restrict__ S0) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= nseg) return;
    double acc = 0.0;
    for (int32_t q = seg_ptr[t]; q < seg_ptr[t + 1]; ++q) {
        const int a = sa[q];
        double v;
        switch (kind[q]) {
            case 0: v = hess[a]; break;
            case 1: v = jac[a]; break;
            case 2: v = pr_diag[a]; break;
            case 3: v = du_diag[a]; break;
            default: v = __dmul_rn(__dmul_rn(jac[a], D[sw[q]]), jac[sb[q]]); break;
        }
        acc = __dadd_rn(acc, v);
    }
    const int64_t d = seg_dst[t];
    if (d < sizeA) A[d] = acc;
    else if (d < sizeA + sizeC) Cb[d - sizeA] = acc;
    else S0[d - sizeA - sizeC] = acc;
}

// ---- long inequality rows: J' D J as weighted Gram products (schur_plan.h) ----
// One thread per staging slot = distinct (long row, column): the sum of its COO entries in COO order into W, D[row] times the sum
// into the twin.  The padding of both buffers was zeroed once (mnk_schur_set_structure) and is never written.
__global__ void schur_gram_stage_kernel(int64_t nslot, const int64_t* __restrict__ slot_dst, const int32_t* __restrict__ slot_ptr,
                                        const int32_t* __restrict__ slot_src, const int32_t* __restrict__ slot_p,
                                        const double* __restrict__ jac, const double* __restrict__ D, double* __restrict__ W,
                                        double* __restrict__ DW) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= nslot) return;
    double w = 0.0;
    for (int32_t q = slot_ptr[t]; q < slot_ptr[t + 1]; ++q) w = __dadd_rn(w, jac[slot_src[q]]);
    const int64_t d = slot_dst[t];
    W[d] = w;
    DW[d] = __dmul_rn(D[slot_p[t]], w);
}

// dst_y (+)= W_y DW_y' for the batch member y = blockIdx.y, one 64 x 64 tile (blockIdx.x; 2 x 2 waves of 32 x 32) per workgroup:
// W_y = W + y * strideW (element (c, k) at c + k * ldw, rows padded to 64), DW_y likewise, K = 16 * nk long rows (the last member:
// 16 * nk_last).  The K-loop is gemm_nt_mainloop on the padded operands (no bounds checks); the epilogue touches rows < rows and
// columns < cols of the unpadded destination only.  add: dst = dst + acc, rounded once (the destination holds what
// schur_assemble_kernel wrote); else dst = acc (a partial sum of the S0 product).  One workgroup owns a destination tile and sums
// its K range front to back: the bits depend on the structure and the values alone.
constexpr int GRAM_WM = 2, GRAM_WN = 2, GRAM_WT = 2, GRAM_BK = (int)SCHUR_GRAM_BK;
constexpr int GRAM_TILE = 16 * GRAM_WT * GRAM_WM;
constexpr int GRAM_LDS_BYTES = 2 * 2 * GRAM_BK * (GRAM_TILE + 16) * 8;
static_assert(GRAM_TILE == SCHUR_GRAM_TILE && 16 * GRAM_WT * GRAM_WN == SCHUR_GRAM_TILE, "the planner pads to the kernel's tile");
constexpr int GRAM_S0_CHUNK = 32;   // k-tiles (of 16 long rows) per partial sum of the S0 product
__global__ __launch_bounds__(64 * GRAM_WM * GRAM_WN) void schur_gram_kernel(const double* __restrict__ W, int64_t ldw, int64_t strideW,
                                                                            const double* __restrict__ DW, int64_t lddw, int64_t strideDW,
                                                                            int nk, int nk_last, double* dst, int64_t ldd, int64_t strideD,
                                                                            int64_t rows, int64_t cols, int ntm, int add) {
    __shared__ __attribute__((aligned(16))) char smem[GRAM_LDS_BYTES];
    const int tid = threadIdx.x;
    const int tm = (int)blockIdx.x % ntm, tn = (int)blockIdx.x / ntm;
    const int64_t y = blockIdx.y;
    const int64_t row0 = (int64_t)tm * GRAM_TILE, col0 = (int64_t)tn * GRAM_TILE;
    v4f64 acc[GRAM_WT][GRAM_WT];
#pragma unroll
    for (int i = 0; i < GRAM_WT; ++i)
#pragma unroll
        for (int j = 0; j < GRAM_WT; ++j) acc[i][j] = v4f64{0.0, 0.0, 0.0, 0.0};
    (void)gemm_nt_mainloop<GRAM_WM, GRAM_WN, GRAM_WT, GRAM_BK>(acc, W + y * strideW + row0, ldw, DW + y * strideDW + col0, lddw,
                                                                y + 1 == (int64_t)gridDim.y ? nk_last : nk, smem, tid);
    // acc[ni][mi] register r of lane (l15, l4) of wave (wm, wn): row wm*32 + mi*16 + l15, column wn*32 + ni*16 + l4 + 4r (gemm_tile.h)
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave % GRAM_WM, wn = wave / GRAM_WM, l15 = lane & 15, l4 = lane >> 4;
    double* D0 = dst + y * strideD;
#pragma unroll
    for (int ni = 0; ni < GRAM_WT; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t col = col0 + wn * 16 * GRAM_WT + ni * 16 + l4 + 4 * r;
            if (col >= cols) continue;
#pragma unroll
            for (int mi = 0; mi < GRAM_WT; ++mi) {
                const int64_t row = row0 + wm * 16 * GRAM_WT + mi * 16 + l15;
                if (row >= rows) continue;
                double* p = D0 + row + col * ldd;
                *p = add ? __dadd_rn(*p, acc[ni][mi][r]) : acc[ni][mi][r];
            }
        }
}
// S0 = (((S0 + P_0) + P_1) + ...): the partial sums of the S0 product in chunk order, every addition rounded on its own
__global__ void schur_gram_reduce_kernel(double* __restrict__ S0, const double* __restrict__ P, int64_t nchunk, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = S0[i];
    for (int64_t c = 0; c < nchunk; ++c) v = __dadd_rn(v, P[c * n + i]);
    S0[i] = v;
}

// ---- the sparse products of solve_kkt! / mul! / jtprod! / mul_hess_blk! (row lists: schur_plan.h) ----
// hipcc contracts a * b + c into one fma by default, and __dmul_rn / __dadd_rn do not stop it: HIP defines them as the plain
// operators in a header that is itself compiled with contraction (schur_condense_weights_kernel's 1 - Sd Ss above IS one fma).  The
// kernels below therefore spell their arithmetic with the operators and switch contraction off in their bodies (`#pragma clang fp
// contract(off)`): every multiply and add is rounded on its own -- the compiled code holds no fma outside the division sequences --
// and the numpy mirror of schur_kkt.py needs no fused operation for them.
// y[r] = alpha acc (+ beta y[r] when beta != 0), acc = the row's terms vals[perm[q]] * x[idx[q]], every multiply and add rounded on
// its own (see above): the bits depend on the lists and the values alone (no atomics, no dependence on the grid).
__device__ __forceinline__ void schur_spmv_store(double* __restrict__ y, int64_t r, double acc, double alpha, double beta) {
#pragma clang fp contract(off)
    double v = alpha * acc;
    if (beta != 0.0) v = v + beta * y[r];
    y[r] = v;
}
// rows of at most T entries: one thread per row, the terms in list order
__global__ void schur_spmv_rows_kernel(int64_t rows, int64_t T, const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                       const int32_t* __restrict__ perm, const double* __restrict__ vals, const double* __restrict__ x,
                                       double alpha, double beta, double* __restrict__ y) {
#pragma clang fp contract(off)
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int32_t q0 = ptr[r], q1 = ptr[r + 1];
    if ((int64_t)q1 - q0 > T) return;   // a long row: schur_spmv_long_kernel's
    double acc = 0.0;
    for (int32_t q = q0; q < q1; ++q) acc = acc + vals[perm[q]] * x[idx[q]];
    schur_spmv_store(y, r, acc, alpha, beta);
}
// rows of more than T entries: one 64-lane wavefront per row (four rows per workgroup).  Lane l sums the entries l, l + 64, ... in
// ascending order; a fixed xor-butterfly (offsets 32, 16, ..., 1) combines the 64 partials -- both operands of every addition are
// the same pair on both sides of an exchange, so all lanes end with the same bits; lane 0 stores.  A wavefront leaves as a whole
// (w >= nlong is uniform over it) and the lanes reconverge behind the loop: all 64 take part in every exchange.
__global__ __launch_bounds__(256) void schur_spmv_long_kernel(int64_t nlong, const int32_t* __restrict__ long_rows,
                                                              const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                              const int32_t* __restrict__ perm, const double* __restrict__ vals,
                                                              const double* __restrict__ x, double alpha, double beta, double* __restrict__ y) {
#pragma clang fp contract(off)
    const int64_t w = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= nlong) return;
    const int64_t r = long_rows[w];
    const int32_t q1 = ptr[r + 1];
    double acc = 0.0;
    for (int32_t q = ptr[r] + lane; q < q1; q += 64) acc = acc + vals[perm[q]] * x[idx[q]];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
    if (lane == 0) schur_spmv_store(y, r, acc, alpha, beta);
}
// solve_kkt! step 1 (reference schur.jl:1028-1030): buffer[ind_ineq[p]] = D_p (wy[ind_ineq[p]] + ws_p / Sigma_s,p) (the rest of
// buffer was zeroed)
__global__ void schur_condense_rhs_kernel(double* __restrict__ buffer, const double* __restrict__ D, const double* __restrict__ ws,
                                          const double* __restrict__ wy, const double* __restrict__ Ss, const int64_t* __restrict__ ind_ineq,
                                          int64_t n_ineq) {
#pragma clang fp contract(off)
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n_ineq) return;
    const int64_t r = ind_ineq[p];
    buffer[r] = D[p] * (wy[r] + ws[p] / Ss[p]);
}
// steps 2 and 6 (:1035-1052, :1072-1086): the per-scenario right-hand sides (wx_k ; wy[equality rows of k]) and the design part, to
// the stage's buffers (back = 0) or back from them (back = 1); one thread per entry of rk | rd
__global__ void schur_rhs_blocks_kernel(double* __restrict__ wx, double* __restrict__ wy, double* __restrict__ rk, double* __restrict__ rd,
                                        const int64_t* __restrict__ eq_rows, int64_t ns, int64_t nv, int64_t blk, int64_t nd, int back) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double *a, *b;
    if (t < ns * blk) {
        const int64_t k = t / blk, i = t - k * blk;
        a = i < nv ? wx + k * nv + i : wy + eq_rows[k * (blk - nv) + (i - nv)];
        b = rk + t;
    } else if (t < ns * blk + nd) {
        a = wx + ns * nv + (t - ns * blk);
        b = rd + (t - ns * blk);
    } else {
        return;
    }
    if (back) *a = *b;
    else *b = *a;
}
// step 7 (:1088-1105) with jx = J wx in a vector of its own (the equality duals in wy stay as the stage left them):
// wy[ind_ineq[p]] = D_p jx[ind_ineq[p]] - buffer[ind_ineq[p]] ; ws_p = (ws_p + wy[ind_ineq[p]]) / Sigma_s,p
__global__ void schur_expand_kernel(double* __restrict__ ws, double* __restrict__ wy, const double* __restrict__ jx,
                                    const double* __restrict__ buffer, const double* __restrict__ D, const double* __restrict__ Ss,
                                    const int64_t* __restrict__ ind_ineq, int64_t n_ineq) {
#pragma clang fp contract(off)
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n_ineq) return;
    const int64_t r = ind_ineq[p];
    const double y = D[p] * jx[r] - buffer[r];
    wy[r] = y;
    ws[p] = (ws[p] + y) / Ss[p];
}
// mul! (:1135-1136): ws_p = beta ws_p - alpha xy[ind_ineq[p]] ; wy[ind_ineq[p]] -= alpha xs_p
__global__ void schur_mul_slack_kernel(double* __restrict__ ws, double* __restrict__ wy, const double* __restrict__ xs,
                                       const double* __restrict__ xy, const int64_t* __restrict__ ind_ineq, double alpha, double beta,
                                       int64_t n_ineq) {
#pragma clang fp contract(off)
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n_ineq) return;
    const int64_t r = ind_ineq[p];
    ws[p] = beta * ws[p] - alpha * xy[r];
    wy[r] = wy[r] - alpha * xs[p];
}
// _kktmul!, diagonal part: w[i] += (alpha d_i) x[i] with d = reg on the primal block [0, npr) and du_diag on the dual block
__global__ void schur_mul_diag_kernel(double* __restrict__ w, const double* __restrict__ x, const double* __restrict__ reg,
                                      const double* __restrict__ du_diag, double alpha, int64_t npr, int64_t npd) {
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= npd) return;
    const double d = i < npr ? reg[i] : du_diag[i - npr];
    w[i] = w[i] + (alpha * d) * x[i];
}
// jtprod! (:907-915), slack part: y[n + p] = -x[ind_ineq[p]]
__global__ void schur_jtprod_slack_kernel(double* __restrict__ ys, const double* __restrict__ x, const int64_t* __restrict__ ind_ineq,
                                          int64_t n_ineq) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p < n_ineq) ys[p] = -x[ind_ineq[p]];
}
// mul_hess_blk! (:1141-1146) behind the Hessian product: wx[i] = (i < n ? wx[i] : 0) + t[i] pr_diag[i]
__global__ void schur_hess_blk_diag_kernel(double* __restrict__ wx, const double* __restrict__ t, const double* __restrict__ pr_diag,
                                           int64_t n, int64_t npr) {
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= npr) return;
    wx[i] = (i < n ? wx[i] : 0.0) + t[i] * pr_diag[i];
}
}  // namespace mnk

using namespace mnk;

extern "C" {

int mnk_schur_create(mnk_ctx* ctx, int64_t ns_local, int64_t blk, int64_t nd, int algo, mnk_schur** out) {
    MNK_REQUIRE(ctx && out, "mnk_schur_create: NULL argument");
    MNK_REQUIRE(ns_local >= 0 && blk > 0 && nd > 0, "mnk_schur_create: bad dimensions");
    MNK_REQUIRE(algo == MNK_CHOLESKY || algo == MNK_LDL || algo == MNK_BUNCHKAUFMAN,
                "mnk_schur_create: CHOLESKY, LDL and BUNCHKAUFMAN are implemented for the Schur-complement system");
    MNK_HIP(hipSetDevice(ctx->device));
    mnk_schur* h = new mnk_schur();
    h->ctx = ctx;
    h->ns = ns_local; h->blk = blk; h->nd = nd; h->algo = algo;
    h->ndp = round_up(nd, 64);
    h->blkp = round_up(blk, 16);
    h->Npb = round_up(blk, PAD);
    int rc = 0;
    rc |= h->A.alloc((size_t)std::max<int64_t>(ns_local, 1) * blk * blk);
    rc |= h->C.alloc((size_t)std::max<int64_t>(ns_local, 1) * nd * blk);
    rc |= h->T.alloc((size_t)blk * nd);
    rc |= h->Cp.alloc((size_t)h->ndp * h->Npb + SLACK);
    rc |= h->Tt.alloc((size_t)h->ndp * h->Npb + SLACK);
    rc |= h->tmpk.alloc((size_t)h->Npb * (size_t)std::max<int64_t>(ns_local, 1));   // (one vector per scenario: their solves run as a batch)
    rc |= h->Sp.alloc((size_t)h->ndp * h->ndp + SLACK);
    {
        const size_t nsl = (size_t)std::max<int64_t>(ns_local, 1);
        const size_t nstep = (size_t)(h->Npb / NBI);
        //  the grouped build works on CHUNKS of at most `chunk` scenarios -- X / V / P buffers of that many, reused
        // from chunk to chunk, the partial sums added to S chunk by chunk in scenario order (the same additions in the same
        // order as one pass over all of them: the same bits) -- instead of ns x nd^2 doubles for P alone (ns = 128, nd = 4096:
        // 17 GB); the solves' per-scenario vectors need ns x nd doubles of P
        // chunk size: as many scenarios as ~4 GB of X / V / P hold, at least 32 (every chunk costs three record uploads with a
        // stream synchronization each: ns = 128, blk = 512, nd = 256 in chunks of 32 built in 10.2 instead of 4.6-7.9 ms)
        const size_t per_scen = (size_t)h->ndp * h->ndp * 8 + 2 * (size_t)h->ndp * h->Npb * 8;
        const size_t by_mem = std::max<size_t>(32, ((size_t)4 << 30) / std::max<size_t>(per_scen, 1));
        h->chunk = (int64_t)std::min<size_t>(nsl, getenv("MNK_SCHUR_CHUNK") ? (size_t)std::max(1, atoi(getenv("MNK_SCHUR_CHUNK"))) : by_mem);
        const size_t nch = (size_t)h->chunk;
        rc |= h->Xall.alloc(nch * h->ndp * h->Npb + SLACK);
        if (algo != MNK_CHOLESKY) rc |= h->Vall.alloc(nch * h->ndp * h->Npb + SLACK);
        rc |= h->Pall.alloc(std::max(nch * h->ndp * h->ndp, nsl * (size_t)h->ndp) + SLACK);
        rc |= h->recs.alloc(nsl * (sizeof(mnk::TrsmBatchRec) + nstep * sizeof(mnk::GemmBatchRec)) + 64);
        rc |= h->fast_k.alloc(nsl);
    }
    if (rc) { (void)hipGetLastError(); delete h; return -2; }
    for (int64_t k = 0; k < ns_local && !rc; ++k) {
        mnk_ls* ls = nullptr;
        rc = mnk_ls_create(ctx, blk, algo, &ls);
        if (!rc) h->ls_k.push_back(ls);
    }
    if (!rc) rc = mnk_ls_create(ctx, nd, algo, &h->ls_s);
    if (rc) {
        for (mnk_ls* l : h->ls_k) mnk_ls_destroy(l);
        if (h->ls_s) mnk_ls_destroy(h->ls_s);
        delete h;
        return rc;
    }
    h->info_k.assign(ns_local, 0);
    mnk_ctx_child_added(ctx);
    *out = h;
    return 0;
}

int mnk_schur_destroy(mnk_schur* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->ctx->device);
    (void)mnk::stream_wait(h->ctx->stream);
    for (mnk_ls* l : h->ls_k) mnk_ls_destroy(l);
    if (h->ls_s) mnk_ls_destroy(h->ls_s);
    mnk_ctx* ctx = h->ctx;
    if (h->stage) { mnk::LaunchLock lock; mnk::quiesce_persistent(); (void)hipHostFree(h->stage); }
    if (h->stage_ev) (void)hipEventDestroy(h->stage_ev);
    delete h;
    mnk_ctx_child_gone(ctx);
    return 0;
}

int mnk_schur_set_block(mnk_schur* h, int64_t k, const double* A_kk, int64_t lda, const double* C_dk, int64_t ldc, int loc) {
    MNK_REQUIRE(h && A_kk && C_dk, "mnk_schur_set_block: NULL argument");
    MNK_REQUIRE(k >= 0 && k < h->ns && lda >= h->blk && ldc >= h->nd, "mnk_schur_set_block: bad scenario index / leading dimension");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (loc == MNK_DEVICE) {
        MNK_HIP(hipMemcpy2DAsync(h->A.p + k * h->blk * h->blk, h->blk * sizeof(double), A_kk, lda * sizeof(double),
                                 h->blk * sizeof(double), h->blk, hipMemcpyDeviceToDevice, s));
        MNK_HIP(hipMemcpy2DAsync(h->C.p + k * h->nd * h->blk, h->nd * sizeof(double), C_dk, ldc * sizeof(double),
                                 h->nd * sizeof(double), h->blk, hipMemcpyDeviceToDevice, s));
    } else {
        MNK_HIP(mnk::h2d_copy_2d(h->A.p + k * h->blk * h->blk, h->blk * sizeof(double), A_kk, lda * sizeof(double),
                                 h->blk * sizeof(double), h->blk, s));
        MNK_HIP(mnk::h2d_copy_2d(h->C.p + k * h->nd * h->blk, h->nd * sizeof(double), C_dk, ldc * sizeof(double),
                                 h->nd * sizeof(double), h->blk, s));
    }
    h->built = false;
    return 0;
}

#define MNK_GRID1(cnt) dim3((unsigned)(((cnt) + 255) / 256)), dim3(256), 0, s

int mnk_schur_build_local(mnk_schur* h, const double* S0, int64_t lds0, int loc_s0, double* S_out, int64_t lds_out) {
    MNK_REQUIRE(h && S_out, "mnk_schur_build_local: NULL argument");
    MNK_REQUIRE(lds_out >= h->nd && (S0 == nullptr || lds0 >= h->nd), "mnk_schur_build_local: bad leading dimension");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const int64_t nd = h->nd, blk = h->blk, ndp = h->ndp, blkp = h->blkp;
    // S <- S0 (or 0), zero padded
    MNK_HIP(hipMemsetAsync(h->Sp.p, 0, (size_t)ndp * ndp * sizeof(double), s));
    if (S0 != nullptr) {
        if (loc_s0 == MNK_DEVICE)
            MNK_HIP(hipMemcpy2DAsync(h->Sp.p, ndp * sizeof(double), S0, lds0 * sizeof(double), nd * sizeof(double), nd,
                                     hipMemcpyDeviceToDevice, s));
        else
            MNK_HIP(mnk::h2d_copy_2d(h->Sp.p, ndp * sizeof(double), S0, lds0 * sizeof(double), nd * sizeof(double), nd, s));
    }
    // Phase 1a (reference :955-990, `@blas_safe_threads for k in 1:ns`): the scenario blocks are factored TOGETHER -- one
    // batch (dag_batch.hip): the pivot chains of up to 32 blocks side by side in one launch instead of one whole-chip factorization
    // and one host synchronization per scenario (a 512-row block is chain-bound at 0.03 of the peak on its own)
    {
        int rc = mnk_factorize_batch_begin();
        if (rc) return rc;
        for (int64_t k = 0; k < h->ns && !rc; ++k) rc = mnk_ls_factorize_dense_dev_async(h->ls_k[k], h->A.p + k * blk * blk, blk);
        const int rc_end = mnk_factorize_batch_end();
        if (rc || rc_end) return rc ? rc : rc_end;
    }
    // (the tier that produced each factor is known first: the info fetch of a batch member waits for its own factorization)
    std::vector<int> fast, slow;
    for (int64_t k = 0; k < h->ns; ++k) {
        int rc = mnk_ls_fetch_info(h->ls_k[k]);
        if (rc) return rc;
        h->info_k[k] = h->ls_k[k]->verdict.info;
        const bool grouped = !h->ls_k[k]->verdict.is_pivoted() && h->info_k[k] == 0 && h->ls_k[k]->algo == h->ls_k[0]->algo &&
                             h->ls_k[k]->ld == h->ls_k[0]->ld;
        (grouped ? fast : slow).push_back((int)k);
    }
    const int64_t Npb = h->Npb;
    // Phase 1b, fast path (static-pivot factor A_k = L D L' or L L'):  C A^-1 C' = (C L^-T) D^-1 (C L^-T)', so only the
    // FORWARD sweep is needed, as a right-side triangular solve of the nd rows of C_dk -- left-looking over the 64-column
    // blocks of L: an MFMA update with the finished blocks, then block substitution on MFMA against the diagonal block.
    // One launch of each per step for ALL scenarios of a chunk (round 3: ~20 launches per scenario, 13.3 ms for 16 of them;
    // four streams side by side: 5.2 ms; the host's launch rate was the bound).
    for (size_t c0 = 0; c0 < fast.size(); c0 += (size_t)h->chunk) {
        const int nf = (int)std::min<size_t>((size_t)h->chunk, fast.size() - c0);
        const int* fk = fast.data() + c0;
        const bool ldl = h->ls_k[fk[0]]->algo == MNK_LDL;
        const int nstep = (int)(Npb / NBI);
        // the records of this pass go through pinned host memory, laid out like the device buffer: one asynchronous copy (a
        // pageable source costs the launch mutex and a stream synchronization per upload -- three per pass)
        const size_t gr_off = (size_t)h->ns * sizeof(mnk::TrsmBatchRec);
        const size_t fk_off = gr_off + (size_t)nstep * h->chunk * sizeof(mnk::GemmBatchRec);
        const size_t need = fk_off + (size_t)h->chunk * sizeof(int);
        if (h->stage_ev == nullptr) MNK_HIP(hipEventCreateWithFlags(&h->stage_ev, hipEventDisableTiming));
        else MNK_HIP(hipEventSynchronize(h->stage_ev));   // (the previous pass' upload has left the staging memory)
        if (h->stage_bytes < need) {
            mnk::LaunchLock lock;
            if (h->stage) { mnk::quiesce_persistent(); (void)hipHostFree(h->stage); h->stage = nullptr; h->stage_bytes = 0; }
            MNK_HIP(hipHostMalloc((void**)&h->stage, need, hipHostMallocDefault));
            h->stage_bytes = need;
        }
        mnk::TrsmBatchRec* tr = reinterpret_cast<mnk::TrsmBatchRec*>(h->stage);
        mnk::GemmBatchRec* gr = reinterpret_cast<mnk::GemmBatchRec*>(h->stage + gr_off);
        int* fk_st = reinterpret_cast<int*>(h->stage + fk_off);
        for (int i = 0; i < nf; ++i) fk_st[i] = fk[i];
        for (int i = 0; i < nf; ++i) {
            mnk_ls* ls = h->ls_k[fk[i]];
            double* X = h->Xall.p + (size_t)i * ndp * Npb;
            double* V = ldl ? h->Vall.p + (size_t)i * ndp * Npb : X;
            tr[i] = {X, ldl ? V : nullptr, ls->dblk.p, ls->inv16.p, ls->dinv.p, ls->info_dev.p};
            for (int j = 1; j < nstep; ++j)   // X[:, block j] -= V[:, 0 : 64 j] L[block j, 0 : 64 j]'
                gr[(size_t)(j - 1) * nf + i] = {V, ls->fact.p + (int64_t)j * NBI, X + (int64_t)j * NBI * ndp, ls->info_dev.p};
            gr[(size_t)(nstep - 1) * nf + i] = {X, V, h->Pall.p + (size_t)i * ndp * ndp, ls->info_dev.p};   // P_i -= X V'
        }
        char* rdev = h->recs.p;
        mnk::TrsmBatchRec* tr_dev = reinterpret_cast<mnk::TrsmBatchRec*>(rdev);
        mnk::GemmBatchRec* gr_dev = reinterpret_cast<mnk::GemmBatchRec*>(rdev + (size_t)h->ns * sizeof(mnk::TrsmBatchRec));
        MNK_HIP(hipMemcpyAsync(rdev, h->stage, gr_off + (size_t)nstep * nf * sizeof(mnk::GemmBatchRec), hipMemcpyHostToDevice, s));
        MNK_HIP(hipMemcpyAsync(h->fast_k.p, fk_st, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
        MNK_HIP(hipEventRecord(h->stage_ev, s));
        hipLaunchKernelGGL(schur_copy_batch_kernel, dim3((unsigned)((ndp * Npb + 255) / 256), (unsigned)nf), dim3(256), 0, s,
                           h->Xall.p, ndp, Npb, h->C.p, nd, blk, h->fast_k.p);
        const int64_t ldf = h->ls_k[fk[0]]->ld;
        int rc = 0;
        for (int j = 0; j < nstep && !rc; ++j) {
            if (j > 0) rc = launch_gemm_nt_batch(s, ndp, NBI, (int64_t)j * NBI, gr_dev + (size_t)(j - 1) * nf, nf, ndp, ldf, ndp);
            if (!rc) rc = mnk_launch_trsm64_batch(s, ldl, tr_dev, nf, (int64_t)j * NBI, ndp, ndp);
        }
        if (rc) return rc;
        // Phase 2 (reference :993-999): S -= sum_k X_k V_k'
        MNK_HIP(hipMemsetAsync(h->Pall.p, 0, (size_t)nf * ndp * ndp * sizeof(double), s));
        rc = launch_gemm_nt_batch(s, ndp, ndp, Npb, gr_dev + (size_t)(nstep - 1) * nf, nf, ndp, ndp, ndp);
        if (rc) return rc;
        hipLaunchKernelGGL(schur_partial_sum_kernel, MNK_GRID1(ndp * ndp), h->Sp.p, h->Pall.p, (int64_t)nf, ndp * ndp);
        MNK_HIP(hipGetLastError());
    }
    for (int k : slow) {
        // Pivoted (Bunch-Kaufman tier) or failed factor: T_k = A_k^-1 C_dk' column by column, as the reference does
        mnk_ls* ls = h->ls_k[k];
        const double* Ck = h->C.p + (int64_t)k * nd * blk;
        double* Tk = h->T.p;
        hipLaunchKernelGGL(schur_copy_kernel, MNK_GRID1(blk * nd), Tk, blk, blk, nd, Ck, nd, nd, blk, 1);
        int rc = mnk_ls_solve(ls, Tk, nd, blk, MNK_DEVICE);
        if (!rc) rc = mnk_ls_check_solve(ls);   // (T_k feeds the Schur complement: an aborted solve must not get that far)
        if (rc) return rc;
        hipLaunchKernelGGL(schur_copy_kernel, MNK_GRID1(ndp * blkp), h->Cp.p, ndp, ndp, blkp, Ck, nd, nd, blk, 0);
        hipLaunchKernelGGL(schur_copy_kernel, MNK_GRID1(ndp * blkp), h->Tt.p, ndp, ndp, blkp, Tk, blk, blk, nd, 1);
        MNK_HIP(hipGetLastError());
        rc = launch_gemm_nt(s, 0, ndp, ndp, blkp, h->Cp.p, ndp, h->Tt.p, ndp, h->Sp.p, ndp, nullptr, nullptr, 0, nullptr);
        if (rc) return rc;
    }
    MNK_HIP(hipMemcpy2DAsync(S_out, lds_out * sizeof(double), h->Sp.p, ndp * sizeof(double), nd * sizeof(double), nd,
                             hipMemcpyDeviceToDevice, s));
    h->built = true;
    return 0;
}

int mnk_schur_factorize_s(mnk_schur* h, const double* S, int64_t lds, int loc, int* info) {
    MNK_REQUIRE(h && S, "mnk_schur_factorize_s: NULL argument");
    return mnk_ls_factorize_dense(h->ls_s, S, lds, loc, info);
}

int mnk_schur_inertia_s(mnk_schur* h, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg) {
    MNK_REQUIRE(h, "mnk_schur_inertia_s: NULL argument");
    return mnk_ls_inertia(h->ls_s, num_pos, num_zero, num_neg);
}

int mnk_schur_scenario_inertia(mnk_schur* h, int64_t k, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg) {
    MNK_REQUIRE(h && k >= 0 && k < h->ns, "mnk_schur_scenario_inertia: bad argument");
    return mnk_ls_inertia(h->ls_k[k], num_pos, num_zero, num_neg);
}

int mnk_schur_scenario_bk_info(mnk_schur* h, int64_t k, int* active, int* count) {
    MNK_REQUIRE(h && k >= 0 && k < h->ns, "mnk_schur_scenario_bk_info: bad argument");
    return mnk_ls_bk_info(h->ls_k[k], active, count, nullptr, nullptr);
}

// The solves above run on device-resident vectors and return before the device is done.  A one-launch (persistent) solve
// that gives up raises a pinned abort word: every stage checks its solvers once at its end (one stream synchronization) and
// reports the failure now -- the solver has then switched to the stepwise solve, the caller repeats the stage.
static int schur_check_solves(mnk_schur* h, bool scenarios, bool design) {
    if (scenarios)
        for (mnk_ls* l : h->ls_k) {
            int rc = mnk_ls_check_solve(l);
            if (rc) return rc;
        }
    if (design && h->ls_s) return mnk_ls_check_solve(h->ls_s);
    return 0;
}

// Step 3 of solve_kkt! (reference :1040-1049): r_k <- A_k^-1 r_k for the local scenarios, and this rank's
// contribution  -sum_k C_dk r_k  to the design right-hand side (the caller adds r_d and all-reduces).
int mnk_schur_forward(mnk_schur* h, double* rhs_k, double* contrib_d) {
    MNK_REQUIRE(h && contrib_d && (rhs_k || h->ns == 0), "mnk_schur_forward: NULL argument");
    MNK_REQUIRE(h->built, "mnk_schur_forward: call mnk_schur_build_local first");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (h->ns == 0) MNK_HIP(hipMemsetAsync(contrib_d, 0, h->nd * sizeof(double), s));
    {   // the scenarios' solves as ONE batch (solve.hip: up to 32 small systems per launch), then the contributions in order
        int rc = mnk_solve_batch_begin();
        for (int64_t k = 0; k < h->ns && !rc; ++k) rc = mnk_ls_solve(h->ls_k[k], rhs_k + k * h->blk, 1, h->blk, MNK_DEVICE);
        int rc_end = mnk_solve_batch_end();
        // (inside a batch the CALLER opened the end above is a no-op: the contributions below need the solutions now)
        if (!rc && !rc_end) rc_end = mnk_solve_batch_flush_pending();
        if (rc || rc_end) return rc ? rc : rc_end;
    }
    if (h->ns > 0) {
        hipLaunchKernelGGL(schur_gemv_batch_kernel, dim3((unsigned)((h->nd + 255) / 256), (unsigned)h->ns), dim3(256), 0, s, h->Pall.p,
                           h->C.p, h->nd, rhs_k, h->blk);
        hipLaunchKernelGGL(schur_contrib_sum_kernel, MNK_GRID1(h->nd), contrib_d, h->Pall.p, h->ns, h->nd, -1.0);
    }
    MNK_HIP(hipGetLastError());
    return schur_check_solves(h, true, false);
}

// Step 4: S x_d = r_d (in place, device vector)
int mnk_schur_solve_s(mnk_schur* h, double* rhs_d) {
    MNK_REQUIRE(h && rhs_d, "mnk_schur_solve_s: NULL argument");
    int rc = mnk_ls_solve(h->ls_s, rhs_d, 1, h->nd, MNK_DEVICE);
    return rc ? rc : schur_check_solves(h, false, true);
}

// Step 5 (reference :1055-1058): x_k = r_k - (A_k^-1 C_dk') x_d, applied as one more solve with A_k on C_dk' x_d
// (the reference multiplies by the stored blk x nd matrix A_k^-1 C_dk'; the fast build path never forms it).
int mnk_schur_backward(mnk_schur* h, double* rhs_k, const double* x_d) {
    MNK_REQUIRE(h && x_d && (rhs_k || h->ns == 0), "mnk_schur_backward: NULL argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (h->ns > 0)
        hipLaunchKernelGGL(schur_gemv_t_batch_kernel, dim3((unsigned)((h->blk + 255) / 256), (unsigned)h->ns), dim3(256), 0, s, h->tmpk.p,
                           h->Npb, h->C.p, h->nd, x_d, h->blk);
    {
        int rc = mnk_solve_batch_begin();
        for (int64_t k = 0; k < h->ns && !rc; ++k) rc = mnk_ls_solve(h->ls_k[k], h->tmpk.p + k * h->Npb, 1, h->blk, MNK_DEVICE);
        int rc_end = mnk_solve_batch_end();
        if (!rc && !rc_end) rc_end = mnk_solve_batch_flush_pending();   // (as in the forward stage)
        if (rc || rc_end) return rc ? rc : rc_end;
    }
    if (h->ns > 0)
        hipLaunchKernelGGL(schur_sub_batch_kernel, dim3((unsigned)((h->blk + 255) / 256), (unsigned)h->ns), dim3(256), 0, s, rhs_k, h->blk,
                           h->tmpk.p, h->Npb);
    MNK_HIP(hipGetLastError());
    return schur_check_solves(h, true, false);
}

// The Gram row threshold of the next mnk_schur_set_structure and the numbers of the structure in force (schur_plan.h).
int mnk_schur_set_gram_threshold(mnk_schur* h, int64_t row_entries) {
    MNK_REQUIRE(h, "mnk_schur_set_gram_threshold: NULL handle");
    h->gram_T = row_entries < 0 ? -1 : row_entries;
    return 0;
}

int mnk_schur_assembly_stats(mnk_schur* h, int64_t* out, int cap) {
    MNK_REQUIRE(h && h->as.have, "mnk_schur_assembly_stats: call mnk_schur_set_structure first");
    MNK_REQUIRE(out && cap >= 5, "mnk_schur_assembly_stats: out needs room for five numbers");
    std::copy(h->as.stats, h->as.stats + 5, out);
    return 0;
}

// The lists come from the host-only planner (schur_plan.hip); this uploads them and zeroes the staging operands of the long rows.
int mnk_schur_set_structure(mnk_schur* h, int64_t n, int64_t m, int64_t nv, int64_t nc, int64_t nnzh, const int32_t* hess_I,
                            const int32_t* hess_J, int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t n_ineq,
                            const int64_t* ind_ineq, int64_t n_eq, const int64_t* ind_eq, int index_base, int64_t ns_global,
                            const int64_t* local_scen, int own_design) {
    MNK_REQUIRE(h, "mnk_schur_set_structure: NULL handle");
    const int64_t nd = h->nd;
    const SchurPatterns in{h->ns, h->blk, nd, n, m, nv, nc, nnzh, hess_I, hess_J, nnzj, jac_I, jac_J, n_ineq, ind_ineq,
                           n_eq, ind_eq, index_base, ns_global, local_scen, own_design, h->gram_T};
    SchurAssemblyPlan plan;
    const char* err = schur_assembly_plan(in, plan);
    MNK_REQUIRE(!err, err);
    MNK_REQUIRE(plan.long_rows == 0 || (h->ns <= 65535 && h->ns * plan.Kp / GRAM_BK <= (int64_t)65535 * GRAM_S0_CHUNK),
                "mnk_schur_set_structure: too many local scenarios / long rows for the Gram products' grids");
    // the row lists of the device-side products: a single rank's only (a sharded handle keeps the stage and the assembly)
    const bool single_rank = local_scen == nullptr && own_design;
    SchurSpmvPlan sp;
    if (single_rank) {
        err = schur_spmv_plan(in, h->spmv_T, sp);
        MNK_REQUIRE(!err, err);
    }
    MNK_HIP(hipSetDevice(h->ctx->device));
    auto& as = h->as;
    auto& kv = h->kv;
    as.have = false;
    kv.have = kv.have_vals = kv.have_jac = kv.have_hess = false;
    kv.st.have_diag = kv.st.have_saved_diag = false;   // (the handle's diagonals live in as.vals, allocated anew below)
    as.n = n; as.m = m; as.nv = nv; as.nc = nc; as.nnzh = nnzh; as.nnzj = nnzj; as.n_ineq = n_ineq;
    as.nseg = plan.nseg(); as.nsrc = plan.nsrc();
    plan.stats(as.stats);
    as.long_rows = plan.long_rows; as.nvp = plan.nvp; as.ndp = plan.ndp; as.Kp = plan.Kp;
    as.nslot = (int64_t)plan.slot_dst.size();
    as.nchunk = (h->ns * plan.Kp / GRAM_BK + GRAM_S0_CHUNK - 1) / GRAM_S0_CHUNK;
    hipStream_t st = h->ctx->stream;
    int rc = as.seg_dst.upload(plan.seg_dst, st) | as.seg_ptr.upload(plan.seg_ptr, st) | as.src_kind.upload(plan.kind, st) |
             as.src_a.upload(plan.a, st) | as.src_b.upload(plan.b, st) | as.src_w.upload(plan.w, st) | as.ind_ineq.upload(plan.ineq0, st) |
             as.D.alloc((size_t)std::max<int64_t>(n_ineq, 1)) | as.S0.alloc((size_t)nd * nd + 8) |
             as.vals.alloc((size_t)(nnzh + nnzj + n + n_ineq + m) + 8);
    if (!rc && as.long_rows > 0) {
        const size_t nw = (size_t)(plan.size_wv() + plan.size_wd());
        rc = as.slot_dst.upload(plan.slot_dst, st) | as.slot_ptr.upload(plan.slot_ptr, st) | as.slot_src.upload(plan.slot_src, st) |
             as.slot_p.upload(plan.slot_p, st) | as.W.alloc(nw + 8) | as.DW.alloc(nw + 8) | as.P.alloc((size_t)as.nchunk * nd * nd + 8);
        if (!rc) {   // the padding never changes: zeroed once
            MNK_HIP(hipMemsetAsync(as.W.p, 0, (nw + 8) * sizeof(double), st));
            MNK_HIP(hipMemsetAsync(as.DW.p, 0, (nw + 8) * sizeof(double), st));
            MNK_HIP(mnk::stream_wait(st));
        }
    } else if (!rc) {
        as.slot_dst.release(); as.slot_ptr.release(); as.slot_src.release(); as.slot_p.release();
        as.W.release(); as.DW.release(); as.P.release();
    }
    if (!rc && single_rank) {
        for (int w = 0; w < 3 && !rc; ++w) {
            auto& d = kv.op[w];
            d.rows = sp.op[w].rows;
            d.nlong = (int64_t)sp.op[w].long_rows.size();
            rc = d.ptr.upload(sp.op[w].ptr, st) | d.idx.upload(sp.op[w].idx, st) | d.perm.upload(sp.op[w].perm, st) |
                 d.long_rows.upload(sp.op[w].long_rows, st);
        }
        kv.T = sp.T;
        kv.n_eq = n_eq;
        const size_t npd = (size_t)(n + n_ineq + m);
        if (!rc)
            rc = kv.eq_rows.upload(sp.eq_rows, st) | kv.buffer.alloc((size_t)m + 8) | kv.buffer2.alloc((size_t)m + 8) |
                 kv.rk.alloc((size_t)(h->ns * h->blk) + 8) | kv.rd.alloc((size_t)nd + 8) | kv.va.alloc(npd + 8) | kv.vb.alloc(npd + 8);
    }
    if (rc) { (void)hipGetLastError(); set_error("mnk_schur_set_structure: out of device memory"); return -2; }
    as.have = true;
    kv.have = single_rank;
    return 0;
}

int mnk_schur_assemble(mnk_schur* h, const double* hess, const double* jac, const double* pr_diag, const double* du_diag, int loc) {
    MNK_REQUIRE(h && h->as.have, "mnk_schur_assemble: call mnk_schur_set_structure first");
    auto& as = h->as;
    // NULL pr_diag and du_diag: the handle's own (what mnk_schur_set_aug_diagonal / mnk_schur_regularize_diagonal left), as
    // mnk_sc_build(NULL, NULL)
    const bool own_diag = pr_diag == nullptr && du_diag == nullptr;
    MNK_REQUIRE((hess || as.nnzh == 0) && (jac || as.nnzj == 0) && (own_diag || (pr_diag && (du_diag || as.m == 0))),
                "mnk_schur_assemble: NULL argument");
    MNK_REQUIRE(!own_diag || h->kv.st.have_diag, "mnk_schur_assemble: NULL diagonals: call mnk_schur_set_aug_diagonal first");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    {   // the handle keeps the values it assembles from (as.vals: hess | jac | pr_diag | du_diag): the device-side products of
        // solve_kkt! / mul! read "the values of the last assemble" (the role of jt_csc / hess_csc in the reference)
        const size_t np = (size_t)(as.n + as.n_ineq);
        auto put = [&](double* dst, const double* src, size_t cnt) -> int {
            if (cnt == 0 || src == nullptr) return 0;
            if (loc == MNK_DEVICE) MNK_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
            else MNK_HIP(mnk::h2d_copy(dst, src, cnt * sizeof(double), s));
            return 0;
        };
        int rc = put(h->hess_v(), hess, (size_t)as.nnzh) | put(h->jac_v(), jac, (size_t)as.nnzj);
        if (!own_diag) rc |= put(h->pr_diag(), pr_diag, np) | put(h->du_diag(), du_diag, (size_t)as.m);
        if (rc) return rc;
        hess = h->hess_v(); jac = h->jac_v(); pr_diag = h->pr_diag(); du_diag = h->du_diag();
        h->kv.have_vals = h->kv.have_jac = h->kv.have_hess = true;
    }
    const int64_t sizeA = h->ns * h->blk * h->blk, sizeC = h->ns * h->nd * h->blk;
    if (sizeA > 0) MNK_HIP(hipMemsetAsync(h->A.p, 0, (size_t)sizeA * sizeof(double), s));
    if (sizeC > 0) MNK_HIP(hipMemsetAsync(h->C.p, 0, (size_t)sizeC * sizeof(double), s));
    MNK_HIP(hipMemsetAsync(as.S0.p, 0, (size_t)h->nd * h->nd * sizeof(double), s));
    if (as.n_ineq > 0)
        hipLaunchKernelGGL(mnk::schur_condense_weights_kernel, dim3((unsigned)((as.n_ineq + 255) / 256)), dim3(256), 0, s, as.D.p, pr_diag, du_diag,
                           as.ind_ineq.p, as.n, as.n_ineq);
    if (as.nseg > 0)
        hipLaunchKernelGGL(mnk::schur_assemble_kernel, dim3((unsigned)((as.nseg + 255) / 256)), dim3(256), 0, s, as.nseg, as.seg_dst.p, as.seg_ptr.p,
                           as.src_kind.p, as.src_a.p, as.src_b.p, as.src_w.p, hess, jac, pr_diag, du_diag, as.D.p, h->A.p, sizeA, h->C.p, sizeC,
                           as.S0.p);
    if (as.long_rows > 0) {   // J' D J of the long rows, added behind the segments' `=` on the same stream
        const double* Wv = as.W.p;
        const double* DWv = as.DW.p;
        const int64_t sizeWv = h->ns * as.nvp * as.Kp, nv = as.nv, nd = h->nd, nvp = as.nvp, ndp = as.ndp, Kp = as.Kp;
        const double* Wd = Wv + sizeWv;
        const double* DWd = DWv + sizeWv;
        const int tv = (int)(nvp / GRAM_TILE), td = (int)(ndp / GRAM_TILE), nk = (int)(Kp / GRAM_BK);
        const dim3 blkdim(64 * GRAM_WM * GRAM_WN);
        hipLaunchKernelGGL(mnk::schur_gram_stage_kernel, dim3((unsigned)((as.nslot + 255) / 256)), dim3(256), 0, s, as.nslot, as.slot_dst.p,
                           as.slot_ptr.p, as.slot_src.p, as.slot_p.p, jac, as.D.p, as.W.p, as.DW.p);
        // A_k[0:nv, 0:nv] += Wv_k DWv_k'  |  C_dk[0:nd, 0:nv] += Wd_k DWv_k'   (blockIdx.y = local scenario)
        hipLaunchKernelGGL(mnk::schur_gram_kernel, dim3((unsigned)(tv * tv), (unsigned)h->ns), blkdim, 0, s, Wv, nvp, nvp * Kp, DWv, nvp,
                           nvp * Kp, nk, nk, h->A.p, h->blk, h->blk * h->blk, nv, nv, tv, 1);
        hipLaunchKernelGGL(mnk::schur_gram_kernel, dim3((unsigned)(td * tv), (unsigned)h->ns), blkdim, 0, s, Wd, ndp, ndp * Kp, DWv, nvp,
                           nvp * Kp, nk, nk, h->C.p, nd, nd * h->blk, nd, nv, td, 1);
        // S0 += Wd_all DWd_all' over the long rows of all local scenarios in local order: partial sums over chunks of
        // GRAM_S0_CHUNK k-tiles (blockIdx.y = chunk), added to S0 in chunk order
        const int nk_all = (int)(h->ns * Kp / GRAM_BK), nk_last = nk_all - (int)(as.nchunk - 1) * GRAM_S0_CHUNK;
        const int64_t cstride = (int64_t)GRAM_S0_CHUNK * GRAM_BK * ndp;
        hipLaunchKernelGGL(mnk::schur_gram_kernel, dim3((unsigned)(td * td), (unsigned)as.nchunk), blkdim, 0, s, Wd, ndp, cstride, DWd, ndp,
                           cstride, GRAM_S0_CHUNK, nk_last, as.P.p, nd, nd * nd, nd, nd, td, 0);
        hipLaunchKernelGGL(mnk::schur_gram_reduce_kernel, dim3((unsigned)((nd * nd + 255) / 256)), dim3(256), 0, s, as.S0.p, as.P.p, as.nchunk,
                           nd * nd);
    }
    MNK_HIP(hipGetLastError());
    h->built = false;
    return 0;
}

void* mnk_schur_s0_buffer(mnk_schur* h) { return (h && h->as.have) ? (void*)h->as.S0.p : nullptr; }

int mnk_schur_get_block(mnk_schur* h, int64_t k, double* A_kk, double* C_dk, double* S0) {
    MNK_REQUIRE(h && ((k >= 0 && k < h->ns) || (!A_kk && !C_dk)) && (!S0 || h->as.have), "mnk_schur_get_block: bad argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (A_kk) MNK_HIP(mnk::d2h_copy(A_kk, h->A.p + k * h->blk * h->blk, (size_t)h->blk * h->blk * sizeof(double), s));
    if (C_dk) MNK_HIP(mnk::d2h_copy(C_dk, h->C.p + k * h->nd * h->blk, (size_t)h->nd * h->blk * sizeof(double), s));
    if (S0) MNK_HIP(mnk::d2h_copy(S0, h->as.S0.p, (size_t)h->nd * h->nd * sizeof(double), s));
    MNK_HIP(mnk::stream_wait(s));
    return 0;
}

// A device buffer of nd x nd doubles owned by the handle: `S_out` of mnk_schur_build_local and `S` of mnk_schur_factorize_s for
// callers that keep no device memory themselves (the Julia glue's host-driven KKT system, julia/MadNLPHIP.jl).
void* mnk_schur_s_buffer(mnk_schur* h) {
    if (!h) return nullptr;
    (void)hipSetDevice(h->ctx->device);
    if (!h->Sown.p && h->Sown.alloc((size_t)h->nd * h->nd + 8)) { (void)hipGetLastError(); return nullptr; }
    return h->Sown.p;
}

// Steps 3-5 of solve_kkt! in one call on ONE rank (reference :1078-1092): rhs_k (ns x blk, scenario k's vector at k * blk) and
// rhs_d (nd) are overwritten with the solution; host or device vectors.  (Several ranks: forward / all-reduce / solve_s /
// backward separately, as above.)
int mnk_schur_solve(mnk_schur* h, double* rhs_k, double* rhs_d, int loc) {
    MNK_REQUIRE(h && rhs_d && (rhs_k || h->ns == 0), "mnk_schur_solve: NULL argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const size_t nk = (size_t)h->ns * h->blk;
    if (!h->hostrd.p && h->hostrd.alloc(2 * (size_t)h->nd + 8)) return -2;
    double* rk = rhs_k;
    double* rd = rhs_d;
    double* contrib = h->hostrd.p + h->nd;
    if (loc != MNK_DEVICE) {
        if (nk > 0 && !h->hostrk.p && h->hostrk.alloc(nk + 8)) return -2;
        rk = h->hostrk.p;
        rd = h->hostrd.p;
        if (nk > 0) MNK_HIP(mnk::h2d_copy(rk, rhs_k, nk * sizeof(double), s));
        MNK_HIP(mnk::h2d_copy(rd, rhs_d, (size_t)h->nd * sizeof(double), s));
    }
    int rc = mnk_schur_forward(h, rk, contrib);
    if (rc) return rc;
    hipLaunchKernelGGL(schur_axpy_kernel, dim3((unsigned)((h->nd + 255) / 256)), dim3(256), 0, s, rd, contrib, h->nd);
    MNK_HIP(hipGetLastError());
    rc = mnk_schur_solve_s(h, rd);
    if (!rc) rc = mnk_schur_backward(h, rk, rd);
    if (rc) return rc;
    if (loc != MNK_DEVICE) {
        if (nk > 0) MNK_HIP(mnk::d2h_copy(rhs_k, rk, nk * sizeof(double), s));
        MNK_HIP(mnk::d2h_copy(rhs_d, rd, (size_t)h->nd * sizeof(double), s));
    }
    return 0;
}

// ---- the KKT-handle contract on the Schur handle (single rank): bound / barrier state, feeders, solve_kkt!, mul!, jtprod!,
// mul_hess_blk! on host or device vectors.  State and frames are kkt_vec.h's; the matrix parts are the row-list products above.
int mnk_schur_set_spmv_threshold(mnk_schur* h, int64_t row_entries) {
    MNK_REQUIRE(h, "mnk_schur_set_spmv_threshold: NULL handle");
    h->spmv_T = row_entries < 0 ? -1 : row_entries;
    return 0;
}

static int schur_kkt_enter(mnk_schur* h, bool args_ok, const char* who) {
    KKT_REQUIRE(h && args_ok, "%s: NULL argument", who);
    KKT_REQUIRE(h->as.have, "%s: call mnk_schur_set_structure first", who);
    KKT_REQUIRE(h->kv.have, "%s: single rank only: this handle is sharded (scenarios on other ranks or a design block it does not own)", who);
    MNK_HIP(hipSetDevice(h->ctx->device));
    return 0;
}

// compress_jacobian! / compress_hessian! (reference schur.jl:917-923: the transfer of the callbacks' COO values to jt_csc / hess_csc):
// the kept values of one operator as of NOW, without an assemble -- the interior-point loop calls jtprod! on a fresh Jacobian
// before it builds the next KKT system.
static int schur_keep_values(mnk_schur* h, double* dst, const double* src, int64_t cnt, int loc, const char* who) {
    int rc = schur_kkt_enter(h, src != nullptr || cnt == 0, who);
    if (rc) return rc;
    hipStream_t s = h->ctx->stream;
    if (cnt > 0 && loc == MNK_DEVICE) MNK_HIP(hipMemcpyAsync(dst, src, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
    else if (cnt > 0) MNK_HIP(mnk::h2d_copy(dst, src, (size_t)cnt * sizeof(double), s));
    return 0;
}

int mnk_schur_compress_jacobian(mnk_schur* h, const double* jac, int loc) {
    int rc = schur_keep_values(h, h ? h->jac_v() : nullptr, jac, h ? h->as.nnzj : 0, loc, "mnk_schur_compress_jacobian");
    if (!rc) h->kv.have_jac = true;
    return rc;
}

int mnk_schur_compress_hessian(mnk_schur* h, const double* hess, int loc) {
    int rc = schur_keep_values(h, h ? h->hess_v() : nullptr, hess, h ? h->as.nnzh : 0, loc, "mnk_schur_compress_hessian");
    if (!rc) h->kv.have_hess = true;
    return rc;
}

int mnk_schur_set_bounds(mnk_schur* h, int64_t nlb, const int64_t* ind_lb, int64_t nub, const int64_t* ind_ub, int index_base) {
    int rc = schur_kkt_enter(h, nlb >= 0 && nub >= 0 && (nlb == 0 || ind_lb) && (nub == 0 || ind_ub), "mnk_schur_set_bounds");
    if (rc) return rc;
    const int64_t npr = h->as.n + h->as.n_ineq;
    return kkt_set_bounds(h->kv.st, h->ctx, "mnk_schur_set_bounds", npr, npr + h->as.m, nlb, ind_lb, nub, ind_ub, index_base);
}

int mnk_schur_set_barrier_terms(mnk_schur* h, const double* reg, const double* l_diag, const double* u_diag, const double* l_lower,
                                const double* u_lower, int loc) {
    int rc = schur_kkt_enter(h, true, "mnk_schur_set_barrier_terms");
    if (rc) return rc;
    return kkt_set_barrier_terms(h->kv.st, h->ctx, "mnk_schur_set_barrier_terms", h->as.n + h->as.n_ineq, reg, l_diag, u_diag, l_lower,
                                 u_lower, loc);
}

static int schur_diag_view(mnk_schur* h, AugDiagView& v, const char* who) {
    int rc = schur_kkt_enter(h, true, who);
    if (rc) return rc;
    return kkt_diag_view(v, h->kv.st, h->ctx, who, h->as.n + h->as.n_ineq, h->as.m, h->pr_diag(), h->du_diag());
}

int mnk_schur_set_aug_diagonal(mnk_schur* h, const double* x, const double* xl, const double* xu, const double* zl, const double* zu,
                               double primal_reg, double dual_reg, int loc) {
    AugDiagView v;
    int rc = schur_diag_view(h, v, "mnk_schur_set_aug_diagonal");
    return rc ? rc : kkt_set_aug_diagonal(v, "mnk_schur_set_aug_diagonal", x, xl, xu, zl, zu, primal_reg, dual_reg, loc);
}

int mnk_schur_regularize_diagonal(mnk_schur* h, double primal, double dual) {
    AugDiagView v;
    int rc = schur_diag_view(h, v, "mnk_schur_regularize_diagonal");
    return rc ? rc : kkt_regularize_diagonal(v, "mnk_schur_regularize_diagonal", primal, dual);
}

int mnk_schur_get_diagonals(mnk_schur* h, double* pr_diag, double* du_diag, double* reg, double* l_diag, double* u_diag, double* l_lower,
                            double* u_lower) {
    AugDiagView v;
    int rc = schur_diag_view(h, v, "mnk_schur_get_diagonals");
    return rc ? rc : kkt_get_diagonals(v, pr_diag, du_diag, reg, l_diag, u_diag, l_lower, u_lower);
}

// y = alpha Op x (+ beta y): the short rows, then the long ones (disjoint rows: the order of the two launches does not matter)
static int schur_spmv(mnk_schur* h, int which, const double* vals, double alpha, const double* x, double beta, double* y) {
    const auto& op = h->kv.op[which];
    hipStream_t s = h->ctx->stream;
    if (op.rows > 0)
        hipLaunchKernelGGL(schur_spmv_rows_kernel, MNK_GRID1(op.rows), op.rows, h->kv.T, op.ptr.p, op.idx.p, op.perm.p, vals, x, alpha, beta, y);
    if (op.nlong > 0)
        hipLaunchKernelGGL(schur_spmv_long_kernel, dim3((unsigned)((op.nlong + 3) / 4)), dim3(256), 0, s, op.nlong, op.long_rows.p, op.ptr.p,
                           op.idx.p, op.perm.p, vals, x, alpha, beta, y);
    MNK_HIP(hipGetLastError());
    return 0;
}

// solve_kkt! (reference schur.jl:1007-1109) on w = (x, s, y, z_l, z_u), host or device.  A scenario or design solve that gave up
// ends the call with its error, as mnk_schur_solve does (the solver has then switched to the stepwise solve: the caller repeats).
int mnk_schur_solve_kkt(mnk_schur* h, double* w, int loc) {
    const char* who = "mnk_schur_solve_kkt";
    int rc = schur_kkt_enter(h, w != nullptr, who);
    if (rc) return rc;
    auto& kv = h->kv;
    KKT_REQUIRE(kv.st.have_bounds, "%s: call mnk_schur_set_bounds first", who);
    KKT_REQUIRE(kv.st.have_terms, "%s: call mnk_schur_set_barrier_terms first", who);
    KKT_REQUIRE(kv.have_vals, "%s: call mnk_schur_assemble first", who);
    hipStream_t s = h->ctx->stream;
    const int64_t n = h->as.n, m = h->as.m, ni = h->as.n_ineq, ns = h->ns, nv = h->as.nv, nd = h->nd, blk = h->blk;
    return kkt_solve_kkt(kv.st, h->ctx, who, h->ls_s, n + ni + m, w, loc, [&](double* d) -> int {
        double *wx = d, *ws = d + n, *wy = d + n + ni;
        const double* Ss = h->pr_diag() + n;
        if (ni > 0) {   // step 1: condense the inequality rows into wx
            MNK_HIP(hipMemsetAsync(kv.buffer.p, 0, (size_t)m * sizeof(double), s));
            hipLaunchKernelGGL(schur_condense_rhs_kernel, MNK_GRID1(ni), kv.buffer.p, h->as.D.p, ws, wy, Ss, h->as.ind_ineq.p, ni);
            int rc = schur_spmv(h, SCHUR_OP_JT, h->jac_v(), 1.0, kv.buffer.p, 1.0, wx);
            if (rc) return rc;
        }
        const int64_t nt = ns * blk + nd;
        hipLaunchKernelGGL(schur_rhs_blocks_kernel, MNK_GRID1(nt), wx, wy, kv.rk.p, kv.rd.p, kv.eq_rows.p, ns, nv, blk, nd, 0);
        MNK_HIP(hipGetLastError());
        int rc = mnk_schur_solve(h, kv.rk.p, kv.rd.p, MNK_DEVICE);   // steps 3-5
        if (rc) return rc;
        hipLaunchKernelGGL(schur_rhs_blocks_kernel, MNK_GRID1(nt), wx, wy, kv.rk.p, kv.rd.p, kv.eq_rows.p, ns, nv, blk, nd, 1);
        if (ni > 0) {   // step 7: inequality duals and slacks from J wx
            rc = schur_spmv(h, SCHUR_OP_J, h->jac_v(), 1.0, wx, 0.0, kv.buffer2.p);
            if (rc) return rc;
            hipLaunchKernelGGL(schur_expand_kernel, MNK_GRID1(ni), ws, wy, kv.buffer2.p, kv.buffer.p, h->as.D.p, Ss, h->as.ind_ineq.p, ni);
        }
        MNK_HIP(hipGetLastError());
        return 0;
    });
}

// mul!(w, kkt, x, alpha, beta) (reference :1112-1139): the slack coupling goes through ind_ineq
int mnk_schur_mul(mnk_schur* h, double* w, const double* x, double alpha, double beta, int loc) {
    const char* who = "mnk_schur_mul";
    int rc = schur_kkt_enter(h, w && x, who);
    if (rc) return rc;
    auto& kv = h->kv;
    KKT_REQUIRE(kv.st.have_bounds, "%s: call mnk_schur_set_bounds first", who);
    KKT_REQUIRE(kv.st.have_terms, "%s: call mnk_schur_set_barrier_terms first", who);
    KKT_REQUIRE(kv.have_vals, "%s: call mnk_schur_assemble first", who);
    hipStream_t s = h->ctx->stream;
    const int64_t n = h->as.n, m = h->as.m, ni = h->as.n_ineq;
    return kkt_mul(kv.st, h->ctx, who, n + ni + m, w, x, alpha, beta, loc, [&](double* dw, const double* dx) -> int {
        // wx = alpha Sym(H) xx + beta wx ; wx += alpha J' xy ; wy = alpha J xx + beta wy
        int rc = schur_spmv(h, SCHUR_OP_H, h->hess_v(), alpha, dx, beta, dw);
        if (rc) return rc;
        if (m > 0) {
            rc = schur_spmv(h, SCHUR_OP_JT, h->jac_v(), alpha, dx + n + ni, 1.0, dw);
            if (rc) return rc;
            rc = schur_spmv(h, SCHUR_OP_J, h->jac_v(), alpha, dx, beta, dw + n + ni);
            if (rc) return rc;
        }
        if (ni > 0)
            hipLaunchKernelGGL(schur_mul_slack_kernel, MNK_GRID1(ni), dw + n, dw + n + ni, dx + n, dx + n + ni, h->as.ind_ineq.p, alpha, beta, ni);
        hipLaunchKernelGGL(schur_mul_diag_kernel, MNK_GRID1(n + ni + m), dw, dx, kv.st.reg.p, h->du_diag(), alpha, n + ni, n + ni + m);
        MNK_HIP(hipGetLastError());
        return 0;
    });
}

// jtprod!(y, kkt, x) (reference :907-915): y (n + n_ineq) = [J' x ; -x[ind_ineq]], x (m)
int mnk_schur_jtprod(mnk_schur* h, double* y, const double* x, int loc) {
    int rc = schur_kkt_enter(h, y && x, "mnk_schur_jtprod");
    if (rc) return rc;
    auto& kv = h->kv;
    KKT_REQUIRE(kv.have_jac, "%s: call mnk_schur_assemble first (or mnk_schur_compress_jacobian: the Jacobian's values alone)", "mnk_schur_jtprod");
    hipStream_t s = h->ctx->stream;
    const int64_t n = h->as.n, m = h->as.m, ni = h->as.n_ineq;
    double* dy = y;
    const double* dx = x;
    if (loc != MNK_DEVICE) {
        dy = kv.va.p;
        dx = kv.vb.p;
        MNK_HIP(mnk::h2d_copy(kv.vb.p, x, (size_t)m * sizeof(double), s));
    }
    rc = schur_spmv(h, SCHUR_OP_JT, h->jac_v(), 1.0, dx, 0.0, dy);
    if (rc) return rc;
    if (ni > 0) hipLaunchKernelGGL(schur_jtprod_slack_kernel, MNK_GRID1(ni), dy + n, dx, h->as.ind_ineq.p, ni);
    MNK_HIP(hipGetLastError());
    if (loc != MNK_DEVICE) MNK_HIP(mnk::d2h_copy(y, dy, (size_t)(n + ni) * sizeof(double), s));
    return 0;
}

// mul_hess_blk!(wx, kkt, t) (reference :1141-1146): wx, t of length n + n_ineq; pr_diag: the handle's (the last assemble's)
int mnk_schur_mul_hess_blk(mnk_schur* h, double* wx, const double* t, int loc) {
    int rc = schur_kkt_enter(h, wx && t, "mnk_schur_mul_hess_blk");
    if (rc) return rc;
    auto& kv = h->kv;
    KKT_REQUIRE(kv.have_vals && kv.have_hess, "%s: call mnk_schur_assemble first", "mnk_schur_mul_hess_blk");
    hipStream_t s = h->ctx->stream;
    const int64_t n = h->as.n, npr = h->as.n + h->as.n_ineq;
    double* dw = wx;
    const double* dt = t;
    if (loc != MNK_DEVICE) {
        dw = kv.va.p;
        dt = kv.vb.p;
        MNK_HIP(mnk::h2d_copy(kv.vb.p, t, (size_t)npr * sizeof(double), s));
    }
    rc = schur_spmv(h, SCHUR_OP_H, h->hess_v(), 1.0, dt, 0.0, dw);
    if (rc) return rc;
    hipLaunchKernelGGL(schur_hess_blk_diag_kernel, MNK_GRID1(npr), dw, dt, h->pr_diag(), n, npr);
    MNK_HIP(hipGetLastError());
    if (loc != MNK_DEVICE) MNK_HIP(mnk::d2h_copy(wx, dw, (size_t)npr * sizeof(double), s));
    return 0;
}

#undef MNK_GRID1

}  // extern "C"

// EVD linear solver: lapack_algorithm = EVD of LapackCPUSolver / LapackROCmSolver (reference src/LinearSolvers/lapack.jl:211-234,
// lib/MadNLPGPU/ext/MadNLPGPUAMDGPUExt/rocsolver.jl: syevd): factorize! computes A = Q diag(lambda) Q^T of the transferred lower
// triangle (dsyevd('V', 'L') semantics: eigenvectors in the columns of Q, lambda ascending), the inertia is the count of the
// signs of lambda, solve! is t = Q^T x, t ./= lambda, x = Q t.
//
// Algorithm: two-sided cyclic BLOCK JACOBI with 32-column blocks.  The padded order Np holds nb = Np / 32 blocks (even); a
// sweep is nb - 1 rounds of a round-robin schedule, nb / 2 disjoint block pairs per round, every unordered pair once per
// sweep.  One round is three launches on the context's stream:
//   1. evd_pair_kernel, one workgroup per pair (I, J): the symmetric 64 x 64 pivot block [A_II A_IJ; A_JI A_JJ] is diagonalized
//      in LDS by a scalar Jacobi in parallel order (32 disjoint rotations per step, 63 steps per inner sweep, inner sweeps until
//      off(S) <= eps |S|_F).  The accumulated R is polished by one Newton-Schulz step (orthogonal to rounding) and has its
//      real columns ordered by the row of their largest entry (ties by column index), padding columns fixed: R stays close to
//      the identity.  A rotation whose off-diagonal entry is exactly 0, or that touches a padding index, is skipped altogether
//      (no arithmetic); a pair without any rotation is marked "identity" and the updates skip it.  R is written transposed
//      (the operand layout of the updates).
//   2. evd_update_kernel<true>: A <- Q^T A Q for the round's Q = diag-of-pairs(R).  One workgroup per pair of pairs (p >= q):
//      the 64 x 64 tile A[IJ_p, IJ_q] is gathered into LDS, multiplied by R_q from the right and R_p^T from the left on the fp64
//      matrix cores (v_mfma_f64_16x16x4) and written back in place together with its transpose -- A stays exactly symmetric,
//      and every entry is read and written by exactly one workgroup.
//   3. evd_update_kernel<false>: V[:, IJ_q] <- V[:, IJ_q] R_q, one workgroup per 64 rows and pair.
// After each sweep off(A)^2 and |A|_F^2 are reduced in a fixed order and stored to the solver's pinned host words; the host
// reads them (one synchronization per sweep) and stops one sweep after off <= N eps |A|_F first held (at once if off <= eps
// |A|_F), or with info = 1 at the sweep cap or at a norm that is not finite (NaN / Inf input: every comparison with a NaN is
// false, nothing waits for convergence).  Then lambda = diag(A) is ranked ascending (ties by index), Q = V's
// columns in that order go to the factor buffer, lambda to dvec, and the counts of the signs to the pinned inertia words.
//
// Padding: rows / columns N .. Np - 1 of the work matrix are zero and of V the identity; they are excluded BY INDEX from the
// rotations, the norms, lambda, the inertia, the ranking and the solves.  Both work matrices are rebuilt by every factorize!.
// Nothing depends on timing or on atomics: two factorizations of the same matrix are bit-identical.
#include <atomic>
#include <cfloat>
#include <climits>
#include <cmath>

#include "gemm_tile.h"
#include "ls.h"

namespace mnk {

constexpr int EB = 32;            // block width: columns per block of the block Jacobi (a pivot block is 64 x 64: twice in LDS)
constexpr int EP = 2 * EB;         // order of a pivot block
static_assert(EB == 32, "the kernels of evd.hip are written for 32-column blocks");
constexpr int ELD = EP + 1;        // leading dimension of the pair kernel's LDS matrices
constexpr int EVD_INNER_CAP = 16;  // inner sweeps of the pair kernel
constexpr int TLD = 80;            // leading dimension of the update kernel's LDS tile (= 16 mod 32: gemm_f64.hip)
constexpr int WLD = 68;            // ... of a wave's 64 x 16 intermediate
constexpr size_t EVD_PAIR_LDS = (size_t)2 * EP * ELD * sizeof(double);

// Round-robin schedule on n players (n even): player 0 stays in slot 0, the others move one slot per round; the pairs of a
// round are the slots (i, n - 1 - i).  n - 1 rounds hold every unordered pair exactly once.
__host__ __device__ __forceinline__ int evd_player(int n, int round, int slot) {
    if (slot == 0) return 0;
    int v = (slot - 1 - round) % (n - 1);
    if (v < 0) v += n - 1;
    return v + 1;
}
__host__ __device__ __forceinline__ void evd_pair(int n, int round, int i, int& lo, int& hi) {
    const int a = evd_player(n, round, i), b = evd_player(n, round, n - 1 - i);
    lo = a < b ? a : b;
    hi = a < b ? b : a;
}
// global index of local index l (0 .. 63) of the block pair (I, J)
__device__ __forceinline__ int64_t evd_gidx(int I, int J, int l) { return l < EB ? (int64_t)I * EB + l : (int64_t)J * EB + (l - EB); }

// sum over the workgroup (256 threads) in a fixed order: butterfly inside the waves, the four waves in order
__device__ __forceinline__ double evd_block_sum(double v, double* red4) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_xor(v, h);
    __syncthreads();   // (red4 may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// work matrix W (Np x Np, full) from the lower triangle of the transferred matrix F; V = identity
__global__ __launch_bounds__(256) void evd_init_kernel(const double* __restrict__ F, int64_t ld, int64_t N, int64_t Np,
                                                       double* __restrict__ W, double* __restrict__ V) {
    const int64_t j = blockIdx.x;
    for (int64_t i = threadIdx.x; i < Np; i += 256) {
        double a = 0.0;
        if (i < N && j < N) a = i >= j ? F[i + j * ld] : F[j + i * ld];
        W[i + j * Np] = a;
        V[i + j * Np] = i == j ? 1.0 : 0.0;
    }
}

// 1. of a round: R^T of every pair (RT: 4096 doubles per pair, RT[n + 64 k] = R[k][n]) and its "identity" mark
__global__ __launch_bounds__(256) void evd_pair_kernel(const double* __restrict__ A, int64_t ld, int64_t N, int nb, int round,
                                                       double* __restrict__ RT, int* __restrict__ ident) {
    extern __shared__ __attribute__((aligned(16))) char evd_smem[];
    double* S = reinterpret_cast<double*>(evd_smem);   // [64][ELD] column-major
    double* R = S + EP * ELD;
    __shared__ double cs[EB], sn[EB], tn[EB], red4[4];
    __shared__ int pp[EB], qq[EB], amx[EP], src[EP], rotated;
    const int tid = threadIdx.x;
    int I, J;
    evd_pair(nb, round, blockIdx.x, I, J);
    for (int e = tid; e < EP * EP; e += 256) {
        const int r = e & 63, c = e >> 6;
        S[r + ELD * c] = A[evd_gidx(I, J, r) + ld * evd_gidx(I, J, c)];
        R[r + ELD * c] = r == c ? 1.0 : 0.0;
    }
    if (tid == 0) rotated = 0;
    __syncthreads();
    for (int isweep = 0; isweep < EVD_INNER_CAP; ++isweep) {
        double off2 = 0.0, all2 = 0.0;
        for (int e = tid; e < EP * EP; e += 256) {
            const int r = e & 63, c = e >> 6;
            const double v = S[r + ELD * c];
            all2 += v * v;
            if (r != c) off2 += v * v;
        }
        off2 = evd_block_sum(off2, red4);
        all2 = evd_block_sum(all2, red4);
        if (!(off2 > (DBL_EPSILON * DBL_EPSILON) * all2)) break;   // (converged, or NaN: the sweep cap of the host ends that)
        for (int step = 0; step < EP - 1; ++step) {
            if (tid < EB) {
                int p, q;
                evd_pair(EP, step, tid, p, q);
                const double apq = S[p + ELD * q];
                double c = 1.0, s = 0.0, t = 0.0;
                if (apq != 0.0 && evd_gidx(I, J, p) < N && evd_gidx(I, J, q) < N) {
                    const double theta = (S[q + ELD * q] - S[p + ELD * p]) / (2.0 * apq);
                    t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    if (s != 0.0) rotated = 1;
                }
                pp[tid] = p;
                qq[tid] = q;
                cs[tid] = c;
                sn[tid] = s;
                tn[tid] = t;
            }
            __syncthreads();
            // S <- J^T S J by 2 x 2 quads (row pair a, column pair b): each quad belongs to one thread
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int id = tid + 256 * k, a = id >> 5, b = id & 31;
                const double sa = sn[a], sb = sn[b];
                if (sa == 0.0 && sb == 0.0) continue;   // (identity on both sides: untouched)
                const int pa = pp[a], qa = qq[a], pb = pp[b], qb = qq[b];
                double xpp = S[pa + ELD * pb], xpq = S[pa + ELD * qb], xqp = S[qa + ELD * pb], xqq = S[qa + ELD * qb];
                if (a == b) {   // the pivot itself: annihilated exactly
                    const double tt = tn[a];
                    S[pa + ELD * pa] = xpp - tt * xpq;
                    S[qa + ELD * qa] = xqq + tt * xpq;
                    S[pa + ELD * qa] = 0.0;
                    S[qa + ELD * pa] = 0.0;
                    continue;
                }
                if (sb != 0.0) {   // columns
                    const double c = cs[b];
                    const double ypp = c * xpp - sb * xpq, ypq = sb * xpp + c * xpq;
                    const double yqp = c * xqp - sb * xqq, yqq = sb * xqp + c * xqq;
                    xpp = ypp; xpq = ypq; xqp = yqp; xqq = yqq;
                }
                if (sa != 0.0) {   // rows
                    const double c = cs[a];
                    const double ypp = c * xpp - sa * xqp, yqp = sa * xpp + c * xqp;
                    const double ypq = c * xpq - sa * xqq, yqq = sa * xpq + c * xqq;
                    xpp = ypp; xpq = ypq; xqp = yqp; xqq = yqq;
                }
                S[pa + ELD * pb] = xpp;
                S[pa + ELD * qb] = xpq;
                S[qa + ELD * pb] = xqp;
                S[qa + ELD * qb] = xqq;
            }
            // R <- R J
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int id = tid + 256 * k, r = id >> 5, b = id & 31;
                const double sb = sn[b];
                if (sb == 0.0) continue;
                const double c = cs[b];
                const int pb = pp[b], qb = qq[b];
                const double xp = R[r + ELD * pb], xq = R[r + ELD * qb];
                R[r + ELD * pb] = c * xp - sb * xq;
                R[r + ELD * qb] = sb * xp + c * xq;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (rotated) {
        // One Newton-Schulz step R <- R (3 I - R^T R) / 2.  The product of the several hundred rotations above is orthogonal to
        // some tens of eps only, and every round multiplies V by such a factor; the step brings R^T R - I down to the rounding
        // of the two 64 x 64 products (measured on the test matrices: the scaled residual and orthogonality of the
        // decomposition fall from 10-25 to below 1).  An identity column (padding) stays one: its products are x * 1 and x * 0.
        const int bi = tid >> 4, bj = tid & 15;
        double g[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) g[i][j] = 0.0;
        for (int k = 0; k < EP; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = R[k + ELD * (4 * bi + i)]; b[i] = R[k + ELD * (4 * bj + i)]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) g[i][j] += a[i] * b[j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) S[4 * bi + i + ELD * (4 * bj + j)] = (4 * bi + i == 4 * bj + j ? 1.5 : 0.0) - 0.5 * g[i][j];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) g[i][j] = 0.0;
        for (int k = 0; k < EP; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = R[4 * bi + i + ELD * k]; b[i] = S[k + ELD * (4 * bj + i)]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) g[i][j] += a[i] * b[j];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) R[4 * bi + i + ELD * (4 * bj + j)] = g[i][j];
        __syncthreads();
    }
    // order the columns: the real columns, sorted by the row of their largest entry (stable: ties by column index), take the
    // real positions in ascending order; a padding column stays where it is (an eigenvalue must never move to a padding index,
    // where nothing rotates)
    const int64_t nvi = N - (int64_t)I * EB, nvj = N - (int64_t)J * EB;
    const int nvI = (int)(nvi < 0 ? 0 : (nvi > EB ? EB : nvi)), nvJ = (int)(nvj < 0 ? 0 : (nvj > EB ? EB : nvj));
    const bool real = tid < EP && (tid < EB ? tid < nvI : tid - EB < nvJ);
    if (tid < EP) {
        int am = 0;
        double best = fabs(R[ELD * tid]);
        for (int r = 1; r < EP; ++r) {
            const double v = fabs(R[r + ELD * tid]);
            if (v > best) { best = v; am = r; }
        }
        amx[tid] = real ? am * EP + tid : INT_MAX;
        src[tid] = tid;
    }
    __syncthreads();
    if (real) {
        const int key = amx[tid];
        int rank = 0;
        for (int j = 0; j < EP; ++j) rank += amx[j] < key ? 1 : 0;
        src[rank < nvI ? rank : EB + (rank - nvI)] = tid;
    }
    __syncthreads();
    double* out = RT + (size_t)blockIdx.x * (EP * EP);
    for (int e = tid; e < EP * EP; e += 256) {
        const int n = e & 63, k = e >> 6;
        out[e] = R[k + ELD * src[n]];
    }
    if (tid == 0) ident[blockIdx.x] = rotated ? 0 : 1;
}

// 2. / 3. of a round (see the top).  TWO: tile (p, q), p >= q, of the work matrix, both sides; otherwise rows
// 64 blockIdx.x .. of V times R_q (q = blockIdx.y).
template <bool TWO>
__global__ __launch_bounds__(256) void evd_update_kernel(double* M, int64_t ld, int nb, int round, const double* __restrict__ RT,
                                                         const int* __restrict__ ident) {
    __shared__ __attribute__((aligned(16))) double T[EP * TLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    int p = 0, q;
    if (TWO) {
        const int t = blockIdx.x;
        p = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (p > 0 && p * (p + 1) / 2 > t) --p;
        while ((p + 1) * (p + 2) / 2 <= t) ++p;
        q = t - p * (p + 1) / 2;
    } else {
        q = blockIdx.y;
    }
    const bool idq = ident[q] != 0, idp = TWO && ident[p] != 0;
    if (idq && (!TWO || idp)) return;
    int Ip = 0, Jp = 0, Iq, Jq;
    evd_pair(nb, round, q, Iq, Jq);
    if (TWO) evd_pair(nb, round, p, Ip, Jp);
    auto grow = [&](int m) -> int64_t { return TWO ? evd_gidx(Ip, Jp, m) : (int64_t)blockIdx.x * EP + m; };
    for (int e = tid; e < EP * EP; e += 256) {
        const int m = e & 63, k = e >> 6;
        T[m + TLD * k] = M[grow(m) + ld * evd_gidx(Iq, Jq, k)];
    }
    __syncthreads();
    // W = T R_q: wave w owns the columns 16 w .. 16 w + 15; acc[mi][r] = W[16 mi + l15][16 w + l4 + 4 r]
    v4f64 acc[4];
    if (idq) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mi][r] = T[16 * mi + l15 + TLD * (16 * w + l4 + 4 * r)];
    } else {
        const double* rq = RT + (size_t)q * (EP * EP) + 16 * w + l15;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[mi] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int kk = 0; kk < EP / 4; ++kk) {
            const int k = 4 * kk + l4;
            const double x = rq[EP * k];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[mi] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, T[16 * mi + l15 + TLD * k], acc[mi], 0, 0, 0);
        }
    }
    const int64_t gc0 = 16 * w + l4;
    if (!TWO) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* cp = M + ld * evd_gidx(Iq, Jq, (int)gc0 + 4 * r);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) cp[grow(16 * mi + l15)] = acc[mi][r];
        }
        return;
    }
    __syncthreads();   // (every wave has read T: its space now holds the waves' intermediates)
    double* Ww = T + w * (16 * WLD);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ww[16 * mi + l15 + WLD * (l4 + 4 * r)] = acc[mi][r];
    __syncthreads();
    if (!idp) {   // out = R_p^T W
        const double* rp = RT + (size_t)p * (EP * EP) + l15;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[mi] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int kk = 0; kk < EP / 4; ++kk) {
            const int k = 4 * kk + l4;
            const double x = Ww[k + WLD * l15];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[mi] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, rp[16 * mi + EP * k], acc[mi], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = (int)gc0 + 4 * r;
        const int64_t gj = evd_gidx(Iq, Jq, n);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = 16 * mi + l15;
            const int64_t gi = evd_gidx(Ip, Jp, m);
            if (p != q || m >= n) {
                M[gi + ld * gj] = acc[mi][r];
                if (gi != gj) M[gj + ld * gi] = acc[mi][r];
            }
        }
    }
}

// per column j < N of the work matrix: sum of a_ij^2 over i < N, i != j, and a_jj^2
__global__ __launch_bounds__(256) void evd_colnorm_kernel(const double* __restrict__ A, int64_t ld, int64_t N,
                                                          double* __restrict__ colsum) {
    __shared__ double red4[4];
    const int64_t j = blockIdx.x;
    double off2 = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256)
        if (i != j) {
            const double v = A[i + ld * j];
            off2 += v * v;
        }
    off2 = evd_block_sum(off2, red4);
    if (threadIdx.x == 0) {
        const double d = A[j + ld * j];
        colsum[2 * j] = off2;
        colsum[2 * j + 1] = d * d;
    }
}
// off(A)^2 and |A|_F^2 (bit patterns) -> pinned words 4 and 5
__global__ __launch_bounds__(256) void evd_norm_kernel(const double* __restrict__ colsum, int64_t N,
                                                       unsigned long long* __restrict__ host_words) {
    __shared__ double red4[4];
    double off2 = 0.0, d2 = 0.0;
    for (int64_t j = threadIdx.x; j < N; j += 256) {
        off2 += colsum[2 * j];
        d2 += colsum[2 * j + 1];
    }
    off2 = evd_block_sum(off2, red4);
    d2 = evd_block_sum(d2, red4);
    if (threadIdx.x == 0) {
        __hip_atomic_store(host_words + 4, (unsigned long long)__double_as_longlong(off2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_words + 5, (unsigned long long)__double_as_longlong(off2 + d2), __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// a key that orders the doubles totally (-0 counts as +0; every NaN lands at one of the two ends)
__device__ __forceinline__ long long evd_key(double v) {
    const long long b = __double_as_longlong(v + 0.0);
    return b < 0 ? (long long)(0x8000000000000000ull - (unsigned long long)b) : b;
}
__global__ __launch_bounds__(256) void evd_diag_kernel(const double* __restrict__ A, int64_t ld, int64_t N, double* __restrict__ lam) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) lam[i] = A[i + ld * i] + 0.0;
}
// rank[i]: position of lam[i] in ascending order, ties by index
__global__ __launch_bounds__(256) void evd_rank_kernel(const double* __restrict__ lam, int64_t N, int* __restrict__ rank) {
    __shared__ long long keys[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const long long ki = i < N ? evd_key(lam[i]) : 0;
    int r = 0;
    for (int64_t j0 = 0; j0 < N; j0 += 256) {
        __syncthreads();
        if (j0 + threadIdx.x < N) keys[threadIdx.x] = evd_key(lam[j0 + threadIdx.x]);
        __syncthreads();
        const int cnt = (int)(N - j0 < 256 ? N - j0 : 256);
        for (int j = 0; j < cnt; ++j) {
            const long long kj = keys[j];
            r += (kj < ki || (kj == ki && j0 + j < i)) ? 1 : 0;
        }
    }
    if (i < N) rank[i] = r;
}
// Q[:, rank[j]] = V[:, j] (N rows), dvec[rank[j]] = lam[j]
__global__ __launch_bounds__(256) void evd_permute_kernel(const double* __restrict__ V, int64_t ldv, int64_t N,
                                                          const int* __restrict__ rank, const double* __restrict__ lam,
                                                          double* __restrict__ Q, int64_t ldq, double* __restrict__ dvec) {
    const int64_t j = blockIdx.x, d = rank[j];
    for (int64_t i = threadIdx.x; i < N; i += 256) Q[i + ldq * d] = V[i + ldv * j];
    if (threadIdx.x == 0) dvec[d] = lam[j];
}
// inertia (count(lambda > 0), the rest, count(lambda < 0)) and info -> pinned words 0 .. 3
__global__ __launch_bounds__(256) void evd_inertia_kernel(const double* __restrict__ lam, int64_t N, int info,
                                                          unsigned long long* __restrict__ host_words) {
    __shared__ int red[4][2];
    int pos = 0, neg = 0;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const double v = lam[i];
        pos += v > 0.0 ? 1 : 0;
        neg += v < 0.0 ? 1 : 0;
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        pos += __shfl_xor(pos, h);
        neg += __shfl_xor(neg, h);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = pos; red[threadIdx.x >> 6][1] = neg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long P = red[0][0] + red[1][0] + red[2][0] + red[3][0], Ng = red[0][1] + red[1][1] + red[2][1] + red[3][1];
        __hip_atomic_store(host_words + 0, (unsigned long long)P, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_words + 1, (unsigned long long)(N - P - Ng), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_words + 2, (unsigned long long)Ng, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_words + 3, (unsigned long long)(long long)info, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- solve: t = Q^T x (one wave per column, rows in a fixed order), t ./= lambda, x = Q t (64-column chunks, then their sum) ----
__global__ __launch_bounds__(256) void evd_qtx_kernel(const double* __restrict__ Q, int64_t ld, int64_t N,
                                                      const double* __restrict__ lam, const double* __restrict__ x,
                                                      double* __restrict__ t) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N) return;
    const double* q = Q + ld * j;
    double acc = 0.0;
    for (int64_t i = lane; i < N; i += 64) acc += q[i] * x[i];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) acc += __shfl_xor(acc, h);
    if (lane == 0) t[j] = acc / lam[j];
}
__global__ __launch_bounds__(256) void evd_qt_kernel(const double* __restrict__ Q, int64_t ld, int64_t N, int64_t Np,
                                                     const double* __restrict__ t, double* __restrict__ part) {
    __shared__ double ts[64];
    const int64_t j0 = (int64_t)blockIdx.y * 64, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cnt = (int)(N - j0 < 64 ? N - j0 : 64);
    if ((int)threadIdx.x < cnt) ts[threadIdx.x] = t[j0 + threadIdx.x];
    __syncthreads();
    if (i >= N) return;
    const double* q = Q + i + ld * j0;
    double acc = 0.0;
    for (int j = 0; j < cnt; ++j) acc += q[ld * j] * ts[j];
    part[(int64_t)blockIdx.y * Np + i] = acc;
}
__global__ __launch_bounds__(256) void evd_sum_kernel(const double* __restrict__ part, int64_t N, int64_t Np, int nchunk,
                                                      double* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += part[(int64_t)c * Np + i];
    x[i] = acc;
}

struct EvdSolver final : mnk_ls_alt {
    // the work matrix (full, Np x Np) that the block Jacobi sweeps diagonalize and the accumulated eigenvectors, the transposed
    // 64 x 64 rotations of a round's block pairs and their "identity" marks, per-column sums of squares of the stop test, the
    // unsorted eigenvalues and their ranks, the 64-column partial sums of x = Q t
    DevBuf<double> evd_a, evd_v, evd_rt, evd_colsum, evd_lam, evd_part;
    DevBuf<int> evd_ident, evd_rank;
    int evd_sweep_cap = 60;      // sweeps after which factorize! gives up (info = 1).  Measured: 5-13 on random matrices, 17 and 23 on
                                 // the bench's matrices, whose off-norm falls 2-4 x per sweep through a long linear phase before the
                                 // quadratic end; 60 still serves a rate of 1.7 x per sweep
    int evd_sweeps = 0;          // sweeps of the last factorization (get_stat "evd_sweeps")

    int alloc(mnk_ls* ls) override {
        const size_t Np = (size_t)ls->Np;
        int rc = evd_a.alloc(Np * Np + SLACK);
        rc |= evd_v.alloc(Np * Np + SLACK);
        rc |= evd_rt.alloc((Np / EP) * (EP * EP));
        rc |= evd_ident.alloc(Np / EP);
        rc |= evd_colsum.alloc(2 * Np);
        rc |= evd_lam.alloc(Np);
        rc |= evd_rank.alloc(Np);
        rc |= evd_part.alloc((Np / 64) * Np);
        return rc;
    }

    // off(A)^2 and |A|_F^2 of the work matrix, through the pinned words (waits for the stream)
    int norms(mnk_ls* ls, double* off2, double* all2) {
        hipStream_t s = ls->ctx->stream;
        hipLaunchKernelGGL(evd_colnorm_kernel, dim3((unsigned)ls->N), dim3(256), 0, s, evd_a.p, ls->Np, ls->N, evd_colsum.p);
        hipLaunchKernelGGL(evd_norm_kernel, dim3(1), dim3(256), 0, s, evd_colsum.p, ls->N, ls->pin_dev);
        MNK_HIP(hipGetLastError());
        MNK_HIP(stream_wait(s));
        volatile unsigned long long* pw = ls->pin;
        const unsigned long long wo = pw[4], wa = pw[5];
        memcpy(off2, &wo, sizeof wo);
        memcpy(all2, &wa, sizeof wa);
        return 0;
    }

    // factorize! of an EVD solver: the matrix has been transferred (lower triangle); see the top.  Runs to its end before it
    // returns (one host synchronization per sweep), so the *_async entry points are synchronous for EVD.
    int factor(mnk_ls* ls) override {
        hipStream_t s = ls->ctx->stream;
        const int64_t N = ls->N, Np = ls->Np;
        const int nb = (int)(Np / EB), npairs = nb / 2;
        double *A = evd_a.p, *V = evd_v.p;
        {   // the pair kernel's LDS is above the static limit: once per (kernel, device) pair of this process
            static DynLdsAttr attr;
            if (int rc_a = attr.set((int)EVD_PAIR_LDS, evd_pair_kernel)) return rc_a;
        }
        hipLaunchKernelGGL(evd_init_kernel, dim3((unsigned)Np), dim3(256), 0, s, ls->fact.p, ls->ld, N, Np, A, V);
        MNK_HIP(hipGetLastError());
        int info = 0, sweeps = 0;
        // Stop rule: off(A) <= N eps |A|_F, the Frobenius test, leaves a residual |A Q - Q L|_1 of up to sqrt(N) times that
        // (measured at N = 2100: scaled residuals of 5 .. 95 where the other ratios are below 1).  Convergence is quadratic, so
        // one sweep more takes off(A) to rounding level: the sweeps end when off <= eps |A|_F, or when the Frobenius test had
        // already held before the last sweep.
        bool near = false;
        for (;;) {
            double off2 = 0.0, all2 = 0.0;
            int rc = norms(ls, &off2, &all2);
            if (rc) return rc;
            // (a NaN / Inf entry, or one above 1e154, makes the norm non-finite for good: no sweep can help)
            if (!std::isfinite(all2)) { info = 1; break; }
            const double off = std::sqrt(off2), nrm = std::sqrt(all2);
            if (off <= DBL_EPSILON * nrm) break;
            if (off <= (double)N * DBL_EPSILON * nrm) {
                if (near) break;
                near = true;
            }
            if (sweeps >= evd_sweep_cap) { info = near ? 0 : 1; break; }
            for (int round = 0; round < nb - 1; ++round) {
                hipLaunchKernelGGL(evd_pair_kernel, dim3(npairs), dim3(256), EVD_PAIR_LDS, s, A, Np, N, nb, round, evd_rt.p,
                                   evd_ident.p);
                hipLaunchKernelGGL(evd_update_kernel<true>, dim3((unsigned)(npairs * (npairs + 1) / 2)), dim3(256), 0, s, A, Np,
                                   nb, round, evd_rt.p, evd_ident.p);
                hipLaunchKernelGGL(evd_update_kernel<false>, dim3((unsigned)(Np / EP), (unsigned)npairs), dim3(256), 0, s, V, Np,
                                   nb, round, evd_rt.p, evd_ident.p);
            }
            MNK_HIP(hipGetLastError());
            ++sweeps;
        }
        evd_sweeps = sweeps;
        const unsigned g = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(evd_diag_kernel, dim3(g), dim3(256), 0, s, A, Np, N, evd_lam.p);
        hipLaunchKernelGGL(evd_rank_kernel, dim3(g), dim3(256), 0, s, evd_lam.p, N, evd_rank.p);
        hipLaunchKernelGGL(evd_permute_kernel, dim3((unsigned)N), dim3(256), 0, s, V, Np, N, evd_rank.p, evd_lam.p, ls->fact.p,
                           ls->ld, ls->dvec.p);
        hipLaunchKernelGGL(evd_inertia_kernel, dim3(1), dim3(256), 0, s, evd_lam.p, N, info, ls->pin_dev);
        MNK_HIP(hipGetLastError());
        return 0;
    }

    // info (0, or 1 at the sweep cap) and the inertia (the signs of lambda) of the factorization queued last, from the pinned
    // words (waits for it)
    int fetch_info(mnk_ls* ls) override {
        MNK_HIP(stream_wait(ls->ctx->stream));
        volatile unsigned long long* pw = ls->pin;
        ls->verdict.accept((int)(long long)pw[3], (int64_t)pw[0], (int64_t)pw[1], (int64_t)pw[2]);
        return 0;
    }

    // solve_linear_system! of an EVD solver (reference src/LinearSolvers/lapack.jl:229-234).  The division is IEEE's: a zero
    // eigenvalue gives Inf / NaN.
    int solve_vec(mnk_ls* ls, const double* b, double* x) override {
        hipStream_t s = ls->ctx->stream;
        const int64_t N = ls->N, Np = ls->Np, ld = ls->ld;
        const double* Q = ls->fact.p;
        double* t = ls->xwork.p + Np;
        const int nchunk = (int)((N + 63) / 64);
        const unsigned g = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(evd_qtx_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, Q, ld, N, ls->dvec.p, b, t);
        hipLaunchKernelGGL(evd_qt_kernel, dim3(g, (unsigned)nchunk), dim3(256), 0, s, Q, ld, N, Np, t, evd_part.p);
        hipLaunchKernelGGL(evd_sum_kernel, dim3(g), dim3(256), 0, s, evd_part.p, N, Np, nchunk, x);
        MNK_HIP(hipGetLastError());
        return 0;
    }

    double stat(const char* key) override { return !strcmp(key, "evd_sweeps") ? (double)evd_sweeps : 0.0; }
};

}  // namespace mnk

using namespace mnk;

std::unique_ptr<mnk_ls_alt> mnk_evd_new() { return std::make_unique<EvdSolver>(); }

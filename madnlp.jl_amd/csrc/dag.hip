// Task-DAG schedule of the blocked factorization (panel_algo = 5): the bulk of `factorize!` (reference
// src/LinearSolvers/lapack_common.jl:54-66 -> dsytrf / dpotrf, src/LinearSolvers/lapack.jl:145-148,164-167) as ONE
// persistent, LEFT-LOOKING tile kernel that runs beside the pivot chain instead of one trailing-update launch per outer
// panel.
//
// Units: block = 64 columns, tile = 128 x 128, strip-column = 256 columns (one persistent panel launch of factor.hip).
//   * chain (factor.hip, ppanel_kernel, panel stream, a few CUs): for every strip-column Js the eight 64-row strips of the
//     BAND -- its four diagonal strips and the four below them, which are the diagonal strips of Js + 1.  A strip applies
//     the previous strip-column itself (left-looking prologue, K = 256) and then runs the right-looking pivot chain.
//   * bulk (this file, update stream, all other CUs): every 128 x 128 tile (I, J) below the band receives
//     C(I, J) -= sum_{k < 128 J} L(I, k) d_k L(J, k)^T  left-looking, in CHUNKS of tile columns of k: one task = one chunk
//     accumulated in registers (the k-loop of the MFMA tile kernel) and applied to the tile in memory; the task of the
//     last tile column also finalizes the tile in place, X = C L_JJ^-T (D^-1) against the two diagonal blocks of tile
//     column J, and publishes the rows.  The band's own tiles are accumulated the same way up to the columns the chain's
//     prologue covers (BANDACC tasks).  (One task per tile over the whole depth -- the tile written once -- was built
//     first: a task that has caught up with the pivot chain then holds its workgroup slot while it advances one tile
//     column per chain step, and the slots doing catch-up work were too few: 63 % of the slot-time computing.)
//   * order: tasks are drawn from ONE queue sorted by the chain position at which they become ready (the last tile
//     column they read), band tiles and rows next to the band first: a drawn task can start at once or nearly so, and a
//     workgroup that holds a task only ever waits for tasks drawn before it, so any number of resident workgroups makes
//     progress.  (A single factorization deals that list into one queue per XCD, each a subsequence of it popped from its head:
//     dag_plan.h: dag_deal_list, and dag_pop below.  The planner that builds and deals the lists is dag_plan.hip; the batches that
//     merge them are dag_batch.hip.)
//   * progress: front[t] = number of leading 128-column tile columns for which the 64-row strip t of L is final
//     (monotone; zeroed per factorization); af[] = "band tile accumulated"; tprog[I, J] = chunks applied to tile (I, J).
//     Producer: stores -> barrier -> one lane's
//     agent-scope release -> drained relaxed store; consumer: relaxed polls by one wave, one agent-scope acquire, barrier.
//     Every wait is bounded (info = -7 -> the host redoes the factorization with the launch-per-piece schedule).
// There is no trailing-update launch per outer panel any more and no barrier between the updates of different panels: the
// look-ahead is as deep as the queue -- the pivot chain never waits for a bulk update of an older panel.
// LDL^T: V = L D is kept in a second N x N array (written once per element, next to L): scaling the B operand's k-columns
// by d_k inside the k-loop instead was built first and cost 16 % of the loop (fp64 VALU work between the fp64 MFMAs).
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <climits>
#include <vector>

#include "gemm_tile.h"
#include "ls.h"

namespace mnk {

// Diagonal tiles are accumulated in SUBTRACT order (gemm_tile.h: gemm_nt_load_neg_lower): C - t_1 - t_2 ... with the tile in
// the accumulators from the first chunk on, instead of a sum of products that grows from zero and is subtracted at the end.
// Both are backward stable; the difference shows on condensed KKT matrices whose pivots are the difference of numbers of
// size 1e13 that agree to 15 digits (AC-OPF case1354): the pivot chain saw -0.031 where the exact
// value is +0.0195, the interior-point run needed 10 Richardson steps per solve and left LAPACK's trajectory at iteration 9;
// with the subtract order it follows it to three digits through all 20 iterations (47 -> 30 back-solves).  Cost: a tile's
// chunks run one after the other (+0.5 % at N = 11 192 against the old order: profiles/r05_diag_subtract_order_ab.txt).

// (the instance record of a task, DagInst: ls.h.  It is read through the constant address space: the fields are uniform and
// never written while a bulk kernel runs, so every use is a scalar load that can be repeated instead of a value that must stay
// live -- a by-value copy of the record in the task loop cost 88 spilled registers and a scratch access inside the K-loop)
typedef const DagInst __attribute__((address_space(4))) * DagInstP;

struct DagArgs {       // (the batch kernel's; a single factorization: DagArgs1 / dag_bulk_kernel1 below)
    const DagInst* insts; // the instance records in device memory (written by dag_reset_kernel), indexed by the task's instance field
    const int4* tasks;    // a merged list of DagTask (dag_plan.h)
    int ntasks;
    int ntile;
    int* qctr;
    long spin_limit;
    unsigned long long* trace;  // diagnostics (option dag_trace): 8 time stamps per task
    unsigned long long* wgstat; // diagnostics: per workgroup {first grab, exit, ticks waited, tasks, ticks in finalize}
    int fake_share;             // DIAGNOSTIC (env MNK_DAG_FAKE_SHARE, wrong results): every chunk reads the operand rows of tile rows 0..n-1
};

// The bulk kernels decode a task's words with literal masks and shifts (readfirstlane per word: the text the tuned register
// allocation was measured with); these tie the literals to the field widths of DagTask.
static_assert(sizeof(int4) == sizeof(DagTask), "a task is one int4");
static_assert(DagTask::FLAG_BITS == 8, "tk.x & 255: flags, tk.x >> 8: chunk index");
static_assert(DagTask::ROW_BITS == 16, "tk.y & 0xffff: I, tk.y >> 16: instance (dag_bulk_kernel1: no instance, tk.y is I)");
static_assert(DagTask::COL_BITS == 12, "tk.z & 0xfff: J, tk.z >> 12: list position (dag_bulk_kernel: no position, tk.z is J)");
static_assert(DagTask::KBEG_BITS == 16, "tk.w & 0xffff: kbeg, tk.w >> 16: kend");

// Wave 0 waits until min(front[s0..s3]) > c and returns that minimum (clamped to kend): tile columns [c, ret) are final
// for all four strips.  -1: the factorization failed elsewhere or the wait expired.  Ends with an acquire + barrier.
template <class IP>
__device__ __forceinline__ int dag_wait_front(IP a, long spin_limit, int s0, int s1, int s2, int s3, int c, int kend, int* s_val) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const int idx = lane == 0 ? s0 : (lane == 1 ? s1 : (lane == 2 ? s2 : s3));
        long spins = 0;
        int r;
        for (;;) {
            int f = lane < 4 ? __hip_atomic_load(a->front + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : INT_MAX;
            f = min(f, __shfl_xor(f, 1));
            f = min(f, __shfl_xor(f, 2));
            r = __builtin_amdgcn_readfirstlane(f);
            if (r > c) break;
            __builtin_amdgcn_s_sleep(4);
            if ((++spins & 255) == 0) {
                if (__hip_atomic_load(a->info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                    r = -1;
                    break;
                }
                if (spins > spin_limit) {
                    if (lane == 0 && atomicCAS(a->info, 0, -7) == 0) a->info[1] = 1;   // (site 1: a bulk task waiting for operand rows)
                    r = -1;
                    break;
                }
            }
        }
        if (r > kend) r = kend;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (lane == 0) *s_val = r;
    }
    __syncthreads();
    const int r = *s_val;
    __syncthreads();
    return r;
}

// Wave 0 waits until *w0 >= t0 and *w1 >= t1 (progress words of the pivot chain); false: failed / expired.  Acquire + barrier.
template <class IP>
__device__ __forceinline__ bool dag_wait_words(IP a, long spin_limit, const int* w0, int t0, const int* w1, int t1, int* s_val) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        long spins = 0;
        int ok = 1;
        for (;;) {
            const int v = lane < 2 ? __hip_atomic_load(lane == 0 ? w0 : w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : INT_MAX;
            if (__all(v >= (lane == 0 ? t0 : (lane == 1 ? t1 : INT_MIN)))) break;
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 255) == 0) {
                if (__hip_atomic_load(a->info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                    ok = 0;
                    break;
                }
                if (spins > spin_limit) {
                    if (lane == 0 && atomicCAS(a->info, 0, -7) == 0) a->info[1] = 2;   // (site 2: chunk order of a tile)
                    ok = 0;
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (lane == 0) *s_val = ok;
    }
    __syncthreads();
    const int ok = *s_val;
    __syncthreads();
    return ok != 0;
}

// In-place finalization of a bulk tile against the two factored diagonal blocks (ja, jb = ja + 1) of its tile column:
// the block substitution of trsm64_mfma_kernel (factor.hip) for the 64 columns of block ja, the K = 64 update of the
// columns of block jb with L(jb, ja), the substitution for block jb.  Wave w owns the 16-row strips 2w, 2w + 1 of the
// tile (C^T layout: register r of column block cb at lane (l15, l4) is C[row + l15][16 cb + l4 + 4 r]) and runs their two
// independent MFMA chains interleaved.  The operands every wave needs -- the strictly lower 16x16 blocks and the 16x16
// inverses of a diagonal block, then L(jb, ja) -- are staged ONCE per workgroup through the k-loop's LDS tiles in MFMA
// A-operand order (one v4 per lane and block: M[l15][l4 + 4 s], s = 0..3): fed straight from global memory the chains
// waited for one L2 round trip per MFMA (90 us per tile measured, on the critical path of every row of tiles; ~30 us
// staged).  (Starting the block-ja part before D_jb is published, with all operands prefetched into registers, was built
// and measured slower: the 168-register budget of the k-loop forces the strips to run one after the other.)
// X: the tile in that layout, X[cb][ns] = column block cb (0..7) of strip ns -- the accumulators of gemm_nt_mainloop3<2, 8>.
template <bool LDL, class IP>
__device__ __forceinline__ void dag_finalize_tile(IP a, int64_t row0, int64_t col0, int ja, char* smem_raw, int tid,
                                                  v4f64 (&X)[8][2], unsigned long long* tr) {
    // trace: six 16-bit stage times (ticks of 10 ns since entry) packed into tr[6] (stages 1..4) and tr[7] (5, 6)
    const unsigned long long t_in = tr ? wall_clock64() : 0;
    auto stamp = [&](int stage) {
        if (tr) {
            const unsigned long long d = (wall_clock64() - t_in) & 0xffff;
            if (stage < 4) tr[6] = (stage == 0 ? 0 : tr[6]) | d << (16 * stage);
            else tr[7] = (stage == 4 ? 0 : tr[7]) | d << (16 * (stage - 4));
        }
    };
    v4f64* S = reinterpret_cast<v4f64*>(smem_raw);  // up to 16 blocks x 64 lanes (32 KB of the 36 KB)
    double* F = a->F;
    const int64_t ld = a->ld;
    const int lane = tid & 63, w = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    double* Fs = F + (row0 + 32 * w + l15) + (col0 + l4) * ld;  // this lane's element (row of strip 0, column l4)
    double* Vs = LDL ? a->V + (row0 + 32 * w + l15) + (col0 + l4) * ld : nullptr;
    double vm = 0.0;  // max|V| of this wave's strips (growth monitor)

    // blocks 0..5: -L_kk[cb, ib] for (cb, ib) = (1,0) (2,0) (2,1) (3,0) (3,1) (3,2); blocks 6..9: inv(L_kk[cb, cb])
    auto fill_diag = [&](int jk) {
        const double* __restrict__ Dk = a->dblk + (int64_t)jk * 4096;
        const double* __restrict__ Iv = a->inv16 + (int64_t)jk * 1024;
        for (int slot = tid; slot < 640; slot += 256) {
            const int q = slot >> 6, i = slot & 15, k4 = (slot >> 4) & 3;
            v4f64 v;
            if (q < 6) {
                const int cb = q == 0 ? 1 : (q < 3 ? 2 : 3), ib = q == 0 ? 0 : (q < 3 ? q - 1 : q - 3);
                const double* src = Dk + (16 * cb + i) + 64 * (16 * ib + k4);
#pragma unroll
                for (int sx = 0; sx < 4; ++sx) v[sx] = -src[64 * 4 * sx];
            } else {
                const double* src = Iv + (q - 6) * 256 + i + 16 * k4;
#pragma unroll
                for (int sx = 0; sx < 4; ++sx) v[sx] = src[16 * 4 * sx];
            }
            S[slot] = v;
        }
        // D^-1 of the block's 64 columns rides along (LDL^T): read back four at a time in front of the stores -- a global
        // load behind a possibly aliasing store would wait for it, and 16 preloaded values do not fit the registers
        if (LDL && tid < 64) reinterpret_cast<double*>(S + 640)[tid] = a->dinv[(int64_t)64 * jk + tid];
    };
    // X <- X L_kk^-T for both strips; stores L (LDL^T: V D^-1, and V next to it), keeps V in X
    auto trsm = [&](auto half, int coff) {
        constexpr int h4 = 4 * decltype(half)::value;
        const double* Sd = reinterpret_cast<const double*>(S + 640) + l4;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            v4f64 t0 = X[h4 + cb][0], t1 = X[h4 + cb][1];
#pragma unroll
            for (int ib = 0; ib < cb; ++ib) {
                const v4f64 aop = S[(cb * (cb - 1) / 2 + ib) * 64 + lane];
#pragma unroll
                for (int sx = 0; sx < 4; ++sx) {
                    t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], X[h4 + ib][0][sx], t0, 0, 0, 0);
                    t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], X[h4 + ib][1][sx], t1, 0, 0, 0);
                }
            }
            const v4f64 iv = S[(6 + cb) * 64 + lane];
            v4f64 x0 = {0.0, 0.0, 0.0, 0.0}, x1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) {
                x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(iv[sx], t0[sx], x0, 0, 0, 0);
                x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(iv[sx], t1[sx], x1, 0, 0, 0);
            }
            X[h4 + cb][0] = x0;
            X[h4 + cb][1] = x1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (LDL) vm = fmax(vm, fmax(fabs(x0[r]), fabs(x1[r])));
                const int64_t cc = (int64_t)(coff + 16 * cb + 4 * r) * ld;
                const double di = LDL ? Sd[16 * cb + 4 * r] : 1.0;
                Fs[cc] = LDL ? x0[r] * di : x0[r];
                Fs[cc + 16] = LDL ? x1[r] * di : x1[r];
                if (LDL) {
                    Vs[cc] = x0[r];
                    Vs[cc + 16] = x1[r];
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // (the whole tile is live in registers: nothing of the next block may be hoisted)
        }
    };
    fill_diag(ja);
    __syncthreads();
    stamp(0);
    trsm(std::integral_constant<int, 0>(), 0);
    __syncthreads();
    stamp(1);
    {   // blocks (cb2, ib): -L(jb, ja)[16 cb2 + i][16 ib + k]
        const double* __restrict__ Lba = F + (int64_t)64 * (ja + 1) + (int64_t)64 * ja * ld;
        for (int slot = tid; slot < 1024; slot += 256) {
            const int q = slot >> 6, i = slot & 15, k4 = (slot >> 4) & 3;
            const double* src = Lba + (16 * (q >> 2) + i) + (int64_t)(16 * (q & 3) + k4) * ld;
            v4f64 v;
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) v[sx] = -src[(int64_t)(4 * sx) * ld];
            S[slot] = v;
        }
    }
    __syncthreads();
    stamp(2);
#pragma unroll
    for (int cb2 = 0; cb2 < 4; ++cb2)
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            const v4f64 aop = S[(cb2 * 4 + ib) * 64 + lane];
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) {
                X[4 + cb2][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], X[ib][0][sx], X[4 + cb2][0], 0, 0, 0);
                X[4 + cb2][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[sx], X[ib][1][sx], X[4 + cb2][1], 0, 0, 0);
            }
            if (ib == 3) __builtin_amdgcn_sched_barrier(0);
        }
    __syncthreads();
    stamp(3);
    fill_diag(ja + 1);
    __syncthreads();
    stamp(4);
    trsm(std::integral_constant<int, 1>(), 64);
    stamp(5);
    if (LDL && a->vmax != nullptr) {
        if (!(vm <= DBL_MAX)) vm = __longlong_as_double(0x7ff0000000000000LL);
        for (int off = 32; off > 0; off >>= 1) vm = fmax(vm, __shfl_xor(vm, off));
        if (lane == 0 && vm > 0.0) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(vm);
            if (bits > __hip_atomic_load(a->vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a->vmax, bits);
        }
    }
}

// (`envw`: the solver's mnk_ls::env_word -- the verdict of the transfer on its finiteness becomes this factorization's, and the word
// the next transfer marks is cleared)
__global__ __launch_bounds__(256) void dag_reset_kernel(int* __restrict__ flags, int64_t n, int* __restrict__ info, DagInst rec,
                                                        DagInst* __restrict__ rec_dst, const SmallSysRec* __restrict__ recs = nullptr,
                                                        int* __restrict__ envw = nullptr, int* __restrict__ qheads = nullptr, int nqh = 0) {
    if (recs != nullptr) {   // (a batch of small systems: blockIdx.y = system; the instance records are uploaded by the host)
        const SmallSysRec r = recs[blockIdx.y];
        flags = r.flags; n = r.nflags; info = r.info;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && rec_dst != nullptr) *rec_dst = rec;   // the instance record the bulk kernel reads
    if (blockIdx.x == 0 && threadIdx.x == 0 && envw != nullptr) { envw[1] = envw[0]; envw[0] = 0; }
    int4* f4 = reinterpret_cast<int4*>(flags);   // (hipMalloc alignment; the tail is done word by word)
    const int64_t n4 = n / 4, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) f4[i] = make_int4(0, 0, 0, 0);
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < nqh; i += blockDim.x) qheads[i] = 0;   // (the heads of the per-XCD queues and the count of stolen tasks)
        if (threadIdx.x < (unsigned)(n - 4 * n4)) flags[4 * n4 + threadIdx.x] = 0;
        if (threadIdx.x == 0) { info[0] = 0; info[1] = 0; }
    }
}

// Zero one 128 x 128 tile (I >= J) of the buffer that the NEXT factorization scatters its sparse matrix into, with the unit
// diagonal of the padding rows: the background zero-fill of ls.hip (fill_lower_kernel on a side stream, where it ran beside
// the solves and cost the first of them ~60 us of HBM contention) as tasks of the bulk queue -- 128 KB of stores per task,
// a few microseconds of a slot, absorbed where the matrix cores are the bound.
template <class IP>
__device__ __forceinline__ void dag_fill_tile(IP in, int I, int J, int tid) {
    double* Z = in->zfill;
    const int64_t ld = in->ld;
    // thread: two consecutive rows (a double2) of 4 columns per pass; 64 threads cover 128 rows, 4 groups x 8 passes the 128 columns... 
    const int r2 = (tid & 63) * 2, cg = tid >> 6;
#pragma unroll 4
    for (int c = cg; c < 128; c += 4) {
        const int64_t col = (int64_t)128 * J + c, row = (int64_t)128 * I + r2;
        double2 v = make_double2(0.0, 0.0);
        if (I == J && col >= in->N) {
            if (row == col) v.x = 1.0;
            if (row + 1 == col) v.y = 1.0;
        }
        *reinterpret_cast<double2*>(Z + row + col * ld) = v;
    }
}

// Zero the 128 x 128 tile at (row0, col0) of V: the tile-closing task of a structurally zero tile.  F holds the zeros of the fill
// there, V is never refilled and may hold anything the previous factorization of this solver (any source) left.
__device__ __forceinline__ void dag_zero_tile(double* Z, int64_t ld, int64_t row0, int64_t col0, int tid) {
    const int r2 = (tid & 63) * 2, cg = tid >> 6;
#pragma unroll 4
    for (int c = cg; c < 128; c += 4) *reinterpret_cast<double2*>(Z + row0 + r2 + (col0 + c) * ld) = make_double2(0.0, 0.0);
}

template <bool LDL>
__global__ __launch_bounds__(256, 3) void dag_bulk_kernel(DagArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int s_val;
    // per-workgroup statistics of the trace option live in LDS (thread 0 only): no registers across the task loop
    __shared__ unsigned long long s_stat[4];  // first grab, ticks waited, tasks, ticks in the finalization
    if (threadIdx.x < 4) s_stat[threadIdx.x] = 0;
    __syncthreads();
    for (;;) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // (keeps the thread-id arithmetic out of the task loop's live ranges, as in gemm_nt_tile)
        if (tid == 0) s_val = atomicAdd(a.qctr, 1);
        __syncthreads();
        const int t = s_val;
        __syncthreads();
        if (t >= a.ntasks) {
            if (a.wgstat != nullptr && tid == 0) {
                unsigned long long* w = a.wgstat + (int64_t)blockIdx.x * 8;
                w[0] = s_stat[0]; w[1] = wall_clock64(); w[2] = s_stat[1]; w[3] = s_stat[2]; w[4] = s_stat[3];
            }
            return;
        }
        if (a.wgstat != nullptr && tid == 0) { if (s_stat[0] == 0) s_stat[0] = wall_clock64(); ++s_stat[2]; }
        const int4 tk = a.tasks[t];
        const int flags = __builtin_amdgcn_readfirstlane(tk.x) & 255, q = __builtin_amdgcn_readfirstlane(tk.x) >> 8;
        const int I = __builtin_amdgcn_readfirstlane(tk.y) & 0xffff, inst = __builtin_amdgcn_readfirstlane(tk.y) >> 16;
        const int J = __builtin_amdgcn_readfirstlane(tk.z);
        const int kbeg = __builtin_amdgcn_readfirstlane(tk.w) & 0xffff, kend = __builtin_amdgcn_readfirstlane(tk.w) >> 16;
        const int64_t row0 = (int64_t)128 * I, col0 = (int64_t)128 * J;
        unsigned long long* tr = a.trace != nullptr && tid == 0 ? a.trace + (int64_t)t * 8 : nullptr;
        if (tr) { tr[0] = wall_clock64(); tr[6] = 0; tr[7] = 0; }
        // `in`: the factorization this task belongs to -- the task's instance record, read through the constant address space
        // (uniform: scalar loads)
        auto do_task = [&](auto in) __attribute__((always_inline)) {
        if (flags & DAG_FILL) {   // (no dependence on anything: not even on the instance's factorization being alive)
            if (in->zfill != nullptr) dag_fill_tile(in, I, J, tid);
            return;
        }

        // One task; false: the instance's factorization has failed (a non-positive Cholesky pivot, an expired wait) -- the
        // task is dropped, nothing is published, and every other task of that instance will be dropped the same way (their
        // waits see `info`); tasks of OTHER instances of a batch are not affected.
        // (`dead` must be the same for every wave of the workgroup: ONE thread looks and the answer goes through LDS.  Round 4
        // let every thread look for itself -- a member of a batch that died between two waves' looks sent some waves of the
        // workgroup into the task and the others on to the next one, sharing the LDS tiles and s_val: wrong tiles in OTHER
        // members, spurious breakdowns, once a memory fault; found in round 5, tools/dbg_batch_reject.py.)
        if (tid == 0) s_val = __hip_atomic_load(in->info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ? 1 : 0;
        __syncthreads();
        const bool dead = s_val != 0;
        __syncthreads();
        auto run_task = [&]() __attribute__((always_inline)) -> bool {
        if (dead) return false;
        // the envelope of this instance's factorization (as in dag_bulk_kernel1)
        int eI = 0, k0 = kbeg;
        if (in->env != nullptr && __builtin_amdgcn_readfirstlane(*in->envgate) == 0) {
            eI = __builtin_amdgcn_readfirstlane(in->env[I]);
            k0 = min(kend, max(kbeg, max(eI, __builtin_amdgcn_readfirstlane(in->env[J]))));
        }
        // k-tiles [0, limit) of this chunk have final operands; the gate blocks at the first k-tile of a tile column that is
        // not final yet (a rare event: the queue is sorted by readiness)
        int limit = 0;
        auto gate_at = [&](int kc) -> int {
            const unsigned long long w0 = tr ? wall_clock64() : 0;
            const int r = dag_wait_front(in, a.spin_limit, 2 * I, 2 * I + 1, 2 * J, 2 * J + 1, kc, kend, &s_val);
            if (tr) { const unsigned long long w1 = wall_clock64(); tr[2] = w1; tr[6] += 1; tr[7] += w1 - w0; s_stat[1] += w1 - w0; }
            return r;
        };
        auto gate = [&](int kt) -> bool {
            if (kt < limit) return true;
            const int r = gate_at(k0 + (kt >> 4));
            if (r < 0) return false;
            limit = (__builtin_amdgcn_readfirstlane(r) - k0) * 16;
            return true;
        };
        const double* Ak = in->F + (a.fake_share > 0 ? (int64_t)128 * (kend + I % a.fake_share) : row0) + (int64_t)128 * k0 * in->ld;
        const double* Bk = (LDL ? in->V : in->F) + (a.fake_share > 0 ? (int64_t)128 * (kend + J % a.fake_share) : col0) + (int64_t)128 * k0 * in->ld;
        auto wait_chunk_order = [&]() -> bool {   // the chunks of one tile are applied in order
            if (flags & DAG_FIRST) return true;
            const int* word = in->tprog + (int64_t)I * a.ntile + J;
            const unsigned long long w0 = tr ? wall_clock64() : 0;
            if (!dag_wait_words(in, a.spin_limit, word, q, word, q, &s_val)) return false;
            if (tr) s_stat[1] += wall_clock64() - w0;
            return true;
        };
        if ((flags & DAG_FINAL) && !(flags & DAG_BANDACC)) {
            // Tile-closing task: on the critical path of its row of tiles (and through it of the band the row enters).  The
            // last tile column is multiplied with every wave owning 32 full rows -- the register layout of the
            // finalization -- so the tile goes from the accumulators through the two substitutions to memory ONCE:
            // X = C - acc without a store, no reload (the round trip through memory was 14 + ~5 us of the task's ~78).
            __builtin_amdgcn_s_setprio(3);
            // the tile as the earlier chunks left it goes into the accumulators BEFORE the wait for the row's previous tile
            // column: its load is off the critical path; the K-loop then subtracts (NEG)
            if (!wait_chunk_order()) return false;
            if (J < eI) {   // structurally zero tile (as in dag_bulk_kernel1)
                if (kend > kbeg && gate_at(kbeg) < 0) return false;
                if (LDL) dag_zero_tile(in->V, in->ld, row0, col0, tid);
                return true;
            }
            v4f64 X[8][2];
            {
                const int lane = tid & 63, w = tid >> 6;
                const double* Cs = in->F + (row0 + 32 * w + (lane & 15)) + (col0 + (lane >> 4)) * in->ld;
#pragma unroll
                for (int cb = 0; cb < 8; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double* cp = Cs + (int64_t)(16 * cb + 4 * r) * in->ld;
                        X[cb][0][r] = cp[0];
                        X[cb][1][r] = cp[16];
                    }
            }
            if (kend > kbeg && gate_at(kbeg) < 0) return false;   // one tile column: its operands are final at once
            if (kend > k0) (void)gemm_nt_mainloop3<2, 8, true>(X, Ak, in->ld, Bk, in->ld, (kend - k0) * 16, smem_raw, tid);
            // (new live ranges: the register pressure of the finalization below must not push the accumulators of the
            // K-loop above into scratch)
#pragma unroll
            for (int i = 0; i < 8; ++i) { asm volatile("" : "+v"(X[i][0])); asm volatile("" : "+v"(X[i][1])); }
            if (tr) tr[1] = tr[3] = wall_clock64();  // K-loop done = tile applied
            // the diagonal blocks of tile column J and L(2J + 1, 2J)
            if (dag_wait_front(in, a.spin_limit, 2 * J, 2 * J + 1, 2 * J, 2 * J + 1, J, J + 1, &s_val) < 0) return false;
            if (tr) { tr[4] = wall_clock64(); s_stat[1] += tr[4] - tr[3]; }
            dag_finalize_tile<LDL>(in, row0, col0, 2 * J, smem_raw, tid, X, tr);
            if (tr) s_stat[3] += wall_clock64() - tr[4];
        } else if (!(I == J && kend > k0)) {
            v4f64 acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0.0, 0.0, 0.0, 0.0};
            // the last chunk of a band tile is on the critical path of the chain: it issues first
            if (flags & DAG_FINAL) __builtin_amdgcn_s_setprio(3);
            // (the two-buffer loop: the three-buffer one is ~10 % slower at three workgroups per CU -- tools/hip/time_kstep.hip)
            if (!gemm_nt_mainloop<2, 2, 4, 8>(acc, Ak, in->ld, Bk, in->ld, (kend - k0) * 16, smem_raw, tid, gate)) return false;
            if (tr) tr[1] = wall_clock64();  // K-loop done
            if (!wait_chunk_order()) return false;
            // C(I, J) -= acc
            if (kend > k0)
                gemm_nt_epilogue<2, 2, 4, 2, false, true>(acc, row0, col0, (int64_t)1 << 40, (int64_t)1 << 40, in->F, in->ld, nullptr, nullptr, 0, tid);
            if (tr) tr[3] = wall_clock64();
        } else {
            // A chunk of a DIAGONAL tile, accumulated in subtract order (gemm_nt_load_neg_lower; its chunks run one after the
            // other).  A branch of its own: the body chunks' K-loop below must keep the registers it was tuned with.
            v4f64 acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0.0, 0.0, 0.0, 0.0};
            __builtin_amdgcn_s_setprio(3);   // (every chunk: the next one of the tile -- in the end the chain -- waits for it)
            if (!wait_chunk_order()) return false;
            gemm_nt_load_neg_lower<2, 2, 4>(acc, row0, col0, in->F, in->ld, tid);
            if (!gemm_nt_mainloop<2, 2, 4, 8>(acc, Ak, in->ld, Bk, in->ld, (kend - k0) * 16, smem_raw, tid, gate)) return false;
            if (tr) tr[1] = wall_clock64();  // K-loop done
            gemm_nt_store_neg_lower<2, 2, 4>(acc, row0, col0, in->F, in->ld, tid);
            if (tr) tr[3] = wall_clock64();
        }
        return true;
        };
        const bool done = run_task();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (done && tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (!(flags & DAG_FINAL)) {
                __hip_atomic_store(in->tprog + (int64_t)I * a.ntile + J, q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (!(flags & DAG_BANDACC)) {
                __hip_atomic_store(in->front + 2 * I, J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(in->front + 2 * I + 1, J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                __hip_atomic_store(in->af + (int64_t)I * a.ntile + J, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tr) tr[5] = wall_clock64();
        }
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();  // (s_val and the LDS tiles are reused by the next task)
        };
        do_task((DagInstP)(uintptr_t)(a.insts + inst));
    }
}

// The bulk kernel of a SINGLE factorization: the arguments of the one instance travel in the kernel's argument block (flat,
// as in round 3) and the task loop below is round 3's, statement for statement, plus the DAG_FILL branch.  Not folded into
// the batch kernel above on purpose: with the identical K-loop instructions (compared block by block in the assembly) the
// generic body compiled to a different VGPR assignment of the MFMA operands and ran the k-steps 7 % slower (44.8 -> 48.1 us,
// 9.20 -> 9.45 ms per factorize! at C3, same box, alternating runs) -- this loop is the one the headline number rests on.
struct DagArgs1 {
    double* F;
    int64_t ld;
    double* V;            // LDL^T: V = L D, same layout as F (the B operand of the updates); Cholesky: nullptr (V = L)
    const double* dinv;   // 1 / d_k
    const double* dblk;   // factored 64x64 diagonal blocks
    const double* inv16;  // inverses of their 16x16 diagonal sub-blocks
    const int4* tasks;    // the list of DagTask (dag_plan.h), as built or dealt (below)
    int ntasks;
    int* front;
    int* af;
    int* tprog;           // [I * ntile + J]: chunks of tile (I, J) that are in memory
    int ntile;
    int* qctr;
    int* info;
    long spin_limit;
    unsigned long long* trace;  // diagnostics (option dag_trace): 8 time stamps per task
    unsigned long long* wgstat; // diagnostics: per workgroup {first grab, exit, ticks waited, tasks, ticks in finalize}
    unsigned long long* vmax;   // growth monitor of the static-pivot LDL^T (factor.hip growth_fold): receives max|V|, or NULL
    int fake_share;             // DIAGNOSTIC (env MNK_DAG_FAKE_SHARE, wrong results): every chunk reads the operand rows of tile rows 0..n-1
    double* zfill;              // DAG_FILL tasks: the buffer of the next factorization (or NULL)
    int64_t N;
    const int* env;             // (as in DagInst)
    const int* envgate;
    const int* envh;
    // per-XCD queues (dag_plan.h: dag_deal_list): nq > 0: `tasks` is the dealt copy of the list, queue x = tasks [qoff[x], qoff[x + 1]), its head
    // qheads[x * DAG_QHEAD_STRIDE]; a task's position in the LIST (the index of its trace record) rides in the third word above
    // the tile column.  nq == 0: one queue, the list as built, popped through `qctr`.
    const int* qoff;
    int* qheads;
    int nq;
};

// The next task of a workgroup (one thread) with per-XCD queues: the head of the queue of its own XCD (sq[0] >= 0: that queue;
// -1 - queue once it was found empty), and only when that one is exhausted the head of the queue with the most tasks left.  Own
// pops and steals both advance a head by one atomic add -- what has been taken of a queue is always a prefix of it, nothing comes
// from the middle: the premise of the progress argument.  An index past a queue's end is a miss (another
// workgroup was faster), not the end of the work: the heads are scanned again.  INT_MAX: every head is past its end.
// sq[1] counts this workgroup's stolen tasks, the word behind the heads those of the launch (statistic dag_steals).
__device__ __forceinline__ int dag_pop(const int* __restrict__ qoff, int* __restrict__ qheads, int nq, int* sq) {
    const int h = sq[0];
    if (h >= 0) {
        const int beg = qoff[h], n = qoff[h + 1] - beg;
        const int i = atomicAdd(qheads + h * DAG_QHEAD_STRIDE, 1);
        if (i < n) return beg + i;
        sq[0] = -1 - h;
    }
    for (;;) {
        int best = -1, most = 0;
        for (int x = 0; x < nq; ++x) {
            const int left = qoff[x + 1] - qoff[x] - __hip_atomic_load(qheads + x * DAG_QHEAD_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (left > most) { most = left; best = x; }
        }
        if (best < 0) return INT_MAX;
        const int i = atomicAdd(qheads + best * DAG_QHEAD_STRIDE, 1);
        if (i < qoff[best + 1] - qoff[best]) {
            sq[1] += 1;
            atomicAdd(qheads + nq * DAG_QHEAD_STRIDE, 1);
            return qoff[best] + i;
        }
    }
}

template <bool LDL>
__global__ __launch_bounds__(256, 3) void dag_bulk_kernel1(DagArgs1 a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int s_val;
    __shared__ int s_q[2];   // per-XCD queues: {own queue (dag_pop), tasks stolen}
    if (threadIdx.x == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        s_q[0] = a.nq > 0 ? (int)(xcc & 15u) % a.nq : 0;
        s_q[1] = 0;
    }
    // per-workgroup statistics of the trace option live in LDS (thread 0 only): no registers across the task loop
    __shared__ unsigned long long s_stat[4];  // first grab, ticks waited, tasks, ticks in the finalization
    if (threadIdx.x < 4) s_stat[threadIdx.x] = 0;
    // the envelope of this factorization (NULL: dense -- no envelope, or a NaN / Inf entry)
    const int* __restrict__ env = a.env != nullptr && __builtin_amdgcn_readfirstlane(*a.envgate) == 0 ? a.env : nullptr;
    const int* __restrict__ envh = env != nullptr ? a.envh : nullptr;   // (the same gate)
    __syncthreads();
    for (;;) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // (keeps the thread-id arithmetic out of the task loop's live ranges, as in gemm_nt_tile)
        if (tid == 0)
            s_val = __hip_atomic_load(a.info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0
                        ? INT_MAX
                        : (a.nq > 0 ? dag_pop(a.qoff, a.qheads, a.nq, s_q) : atomicAdd(a.qctr, 1));
        __syncthreads();
        const int t = s_val;
        __syncthreads();
        if (t >= a.ntasks) {
            if (a.wgstat != nullptr && tid == 0) {
                unsigned long long* w = a.wgstat + (int64_t)blockIdx.x * 8;
                w[0] = s_stat[0]; w[1] = wall_clock64(); w[2] = s_stat[1]; w[3] = s_stat[2]; w[4] = s_stat[3];
                // (per-XCD queues: 1 + the workgroup's own queue, the tasks it took from other queues)
                w[5] = a.nq > 0 ? (unsigned long long)(1 + (s_q[0] >= 0 ? s_q[0] : -1 - s_q[0])) : 0; w[6] = (unsigned long long)s_q[1];
            }
            return;
        }
        if (a.wgstat != nullptr && tid == 0) { if (s_stat[0] == 0) s_stat[0] = wall_clock64(); ++s_stat[2]; }
        const int4 tk = a.tasks[t];
        const int flags = __builtin_amdgcn_readfirstlane(tk.x) & 255, q = __builtin_amdgcn_readfirstlane(tk.x) >> 8;
        const int I = __builtin_amdgcn_readfirstlane(tk.y), J = __builtin_amdgcn_readfirstlane(tk.z) & 0xfff;
        const int kbeg = __builtin_amdgcn_readfirstlane(tk.w) & 0xffff, kend = __builtin_amdgcn_readfirstlane(tk.w) >> 16;
        const int64_t row0 = (int64_t)128 * I, col0 = (int64_t)128 * J;
        // (the trace is indexed by the task's position in the list, whichever queue it came from)
        unsigned long long* tr = a.trace != nullptr && tid == 0
                                     ? a.trace + (int64_t)(a.nq > 0 ? (int)((unsigned)__builtin_amdgcn_readfirstlane(tk.z) >> 12) : t) * 8
                                     : nullptr;
        if (tr) { tr[0] = wall_clock64(); tr[6] = 0; tr[7] = 0; }
        if (flags & DAG_FILL) {   // zero-fill of the next factorization's buffer (see dag_fill_tile)
            if (a.zfill != nullptr) dag_fill_tile(&a, I, J, tid);
            continue;
        }

        // Envelope: the tile columns k < max(env[I], env[J]) of L(I, k) or of V(J, k) are exact zeros -- the K-loop starts
        // behind them (k0; an empty chunk still keeps its place in the tile's chunk order), and a tile-closing task of a tile
        // with J < env[I] has nothing to compute
        int eI = 0, k0 = kbeg;
        if (env != nullptr) {
            eI = __builtin_amdgcn_readfirstlane(env[I]);
            k0 = min(kend, max(kbeg, max(eI, __builtin_amdgcn_readfirstlane(env[J]))));
        }
        // Half-tile envelope (chunks): wave w of the chunks' K-loop owns the quadrant (rows 64 (w & 1) ..,
        // columns 64 (w >> 1) ..) of the tile, its operands are the 64-row halves 2I + (w & 1) of L and 2J + (w >> 1) of V.  Left
        // of the later of the two halves' envelopes one factor of every product is an exact zero: the wave multiplies from
        // k-tile kf on (k-tiles of 8 columns, counted from k0; <= 0: all).  The upper quadrant of a diagonal tile (w == 2) is
        // neither stored nor read by anybody: never multiplied.  The k-tiles in front of EVERY wave's first one (ks: 0 or 8 --
        // the tile envelope is the earlier half's, in whole tiles) are not even staged: the chunk's K-loop starts behind them.
        int kf = 0, ks = 0;
        if (envh != nullptr && (!(flags & DAG_FINAL) || (flags & DAG_BANDACC))) {
            const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int hI0 = __builtin_amdgcn_readfirstlane(envh[2 * I]), hI1 = __builtin_amdgcn_readfirstlane(envh[2 * I + 1]);
            const int hJ0 = __builtin_amdgcn_readfirstlane(envh[2 * J]), hJ1 = __builtin_amdgcn_readfirstlane(envh[2 * J + 1]);
            ks = min(max(8 * max(min(hI0, hI1), min(hJ0, hJ1)) - 16 * k0, 0), 16 * (kend - k0));
            kf = (I == J && w == 2) ? INT_MAX : 8 * max((w & 1) ? hI1 : hI0, (w >> 1) ? hJ1 : hJ0) - 16 * k0 - ks;
        }
        const int nk = 16 * (kend - k0) - ks;   // k-tiles of a chunk's K-loop
        // k-tiles [0, limit) of this chunk have final operands; the gate blocks at the first k-tile of a tile column that is
        // not final yet (a rare event: the queue is sorted by readiness)
        int limit = 0;
        auto gate_at = [&](int kc) -> int {   // tile columns [kc, return value) final for all four strips
            const unsigned long long w0 = tr ? wall_clock64() : 0;
            const int r = dag_wait_front(&a, a.spin_limit, 2 * I, 2 * I + 1, 2 * J, 2 * J + 1, kc, kend, &s_val);
            if (tr) { const unsigned long long w1 = wall_clock64(); tr[2] = w1; tr[6] += 1; tr[7] += w1 - w0; s_stat[1] += w1 - w0; }
            return r;
        };
        auto gate = [&](int kt) -> bool {
            if (kt < limit) return true;
            const int r = gate_at(k0 + ((kt + ks) >> 4));
            if (r < 0) return false;
            limit = (__builtin_amdgcn_readfirstlane(r) - k0) * 16 - ks;
            return true;
        };
        const double* Ak = a.F + (a.fake_share > 0 ? (int64_t)128 * (kend + I % a.fake_share) : row0) + (int64_t)(128 * k0 + 8 * ks) * a.ld;
        const double* Bk = (LDL ? a.V : a.F) + (a.fake_share > 0 ? (int64_t)128 * (kend + J % a.fake_share) : col0) + (int64_t)(128 * k0 + 8 * ks) * a.ld;
        auto wait_chunk_order = [&]() -> bool {   // the chunks of one tile are applied in order
            if (flags & DAG_FIRST) return true;
            const int* word = a.tprog + (int64_t)I * a.ntile + J;
            const unsigned long long w0 = tr ? wall_clock64() : 0;
            if (!dag_wait_words(&a, a.spin_limit, word, q, word, q, &s_val)) return false;
            if (tr) s_stat[1] += wall_clock64() - w0;
            return true;
        };
        if ((flags & DAG_FINAL) && !(flags & DAG_BANDACC)) {
            // Tile-closing task: on the critical path of its row of tiles (and through it of the band the row enters).  The
            // last tile column is multiplied with every wave owning 32 full rows -- the register layout of the
            // finalization -- so the tile goes from the accumulators through the two substitutions to memory ONCE:
            // X = C - acc without a store, no reload (the round trip through memory was 14 + ~5 us of the task's ~78).
            __builtin_amdgcn_s_setprio(3);
            // the tile as the earlier chunks left it goes into the accumulators BEFORE the wait for the row's previous tile
            // column: its load is off the critical path; the K-loop then subtracts (NEG)
            if (!wait_chunk_order()) return;
            if (J < eI) {
                // structurally zero tile: only V needs its zeros.  (The wait of the K-step all the same: the row's closing tasks
                // publish front[2I] in column order.)
                if (kend > kbeg && gate_at(kbeg) < 0) return;
                if (LDL) dag_zero_tile(a.V, a.ld, row0, col0, tid);
                goto publish;
            }
            v4f64 X[8][2];
            {
                const int lane = tid & 63, w = tid >> 6;
                const double* Cs = a.F + (row0 + 32 * w + (lane & 15)) + (col0 + (lane >> 4)) * a.ld;
#pragma unroll
                for (int cb = 0; cb < 8; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double* cp = Cs + (int64_t)(16 * cb + 4 * r) * a.ld;
                        X[cb][0][r] = cp[0];
                        X[cb][1][r] = cp[16];
                    }
            }
            if (kend > kbeg && gate_at(kbeg) < 0) return;   // one tile column: its operands are final at once
            if (kend > k0) (void)gemm_nt_mainloop3<2, 8, true>(X, Ak, a.ld, Bk, a.ld, (kend - k0) * 16, smem_raw, tid);
            // (new live ranges: the register pressure of the finalization below must not push the accumulators of the
            // K-loop above into scratch)
#pragma unroll
            for (int i = 0; i < 8; ++i) { asm volatile("" : "+v"(X[i][0])); asm volatile("" : "+v"(X[i][1])); }
            if (tr) tr[1] = tr[3] = wall_clock64();  // K-loop done = tile applied
            // the diagonal blocks of tile column J and L(2J + 1, 2J)
            if (dag_wait_front(&a, a.spin_limit, 2 * J, 2 * J + 1, 2 * J, 2 * J + 1, J, J + 1, &s_val) < 0) return;
            if (tr) { tr[4] = wall_clock64(); s_stat[1] += tr[4] - tr[3]; }
            dag_finalize_tile<LDL>(&a, row0, col0, 2 * J, smem_raw, tid, X, tr);
            if (tr) s_stat[3] += wall_clock64() - tr[4];
        } else if (!(I == J && kend > k0)) {
            v4f64 acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0.0, 0.0, 0.0, 0.0};
            // the last chunk of a band tile is on the critical path of the chain: it issues first
            if (flags & DAG_FINAL) __builtin_amdgcn_s_setprio(3);
            // (the two-buffer loop: the three-buffer one is ~10 % slower at three workgroups per CU -- tools/hip/time_kstep.hip)
            if (!gemm_nt_mainloop<2, 2, 4, 8>(acc, Ak, a.ld, Bk, a.ld, nk, smem_raw, tid, gate, kf)) return;
            if (tr) tr[1] = wall_clock64();  // K-loop done
            if (!wait_chunk_order()) return;
            // C(I, J) -= acc (a wave that multiplied nothing has nothing to subtract)
            if (kend > k0 && kf < nk)
                gemm_nt_epilogue<2, 2, 4, 2, false, true>(acc, row0, col0, (int64_t)1 << 40, (int64_t)1 << 40, a.F, a.ld, nullptr, nullptr, 0, tid);
            if (tr) tr[3] = wall_clock64();
        } else {
            // A chunk of a DIAGONAL tile, accumulated in subtract order (gemm_nt_load_neg_lower; its chunks run one after the
            // other).  A branch of its own: the body chunks' K-loop below must keep the registers it was tuned with.
            v4f64 acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = v4f64{0.0, 0.0, 0.0, 0.0};
            __builtin_amdgcn_s_setprio(3);   // (every chunk: the next one of the tile -- in the end the chain -- waits for it)
            if (!wait_chunk_order()) return;
            gemm_nt_load_neg_lower<2, 2, 4>(acc, row0, col0, a.F, a.ld, tid);
            if (!gemm_nt_mainloop<2, 2, 4, 8>(acc, Ak, a.ld, Bk, a.ld, nk, smem_raw, tid, gate, kf)) return;
            if (tr) tr[1] = wall_clock64();  // K-loop done
            gemm_nt_store_neg_lower<2, 2, 4>(acc, row0, col0, a.F, a.ld, tid);
            if (tr) tr[3] = wall_clock64();
        }
    publish:
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (!(flags & DAG_FINAL)) {
                __hip_atomic_store(a.tprog + (int64_t)I * a.ntile + J, q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (!(flags & DAG_BANDACC)) {
                __hip_atomic_store(a.front + 2 * I, J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.front + 2 * I + 1, J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                __hip_atomic_store(a.af + (int64_t)I * a.ntile + J, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tr) tr[5] = wall_clock64();
        }
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();  // (s_val and the LDS tiles are reused by the next task)
    }
}

// One launcher for the four bulk kernels (template on the kernel, hence one DynLdsAttr per kernel): the dynamic LDS attribute is
// set once per device, the grid is `nwg` persistent workgroups.
template <class Args, void (*Kern)(Args)>
static int launch_bulk(hipStream_t s, const Args& a, int nwg) {
    const size_t smem = TILE3_LDS_BYTES;  // three k-tile buffers of the tile-closing tasks (gemm_nt_mainloop3); chunks use two, the finalization 32 KB
    static DynLdsAttr attr;
    if (int rc = attr.set((int)smem, Kern)) return rc;
    hipLaunchKernelGGL(Kern, dim3(nwg), dim3(256), smem, s, a);
    MNK_HIP(hipGetLastError());
    return 0;
}
static int launch_bulk1(hipStream_t s, bool ldl, const DagArgs1& a, int nwg) {
    return ldl ? launch_bulk<DagArgs1, dag_bulk_kernel1<true>>(s, a, nwg) : launch_bulk<DagArgs1, dag_bulk_kernel1<false>>(s, a, nwg);
}
static int launch_bulk_batch(hipStream_t s, bool ldl, const DagArgs& a, int nwg) {
    return ldl ? launch_bulk<DagArgs, dag_bulk_kernel<true>>(s, a, nwg) : launch_bulk<DagArgs, dag_bulk_kernel<false>>(s, a, nwg);
}

static int dag_fake_share() {
    static const int fake = getenv("MNK_DAG_FAKE_SHARE") ? atoi(getenv("MNK_DAG_FAKE_SHARE")) : 0;
    return fake;
}

// one factorization: dag_bulk_kernel1, the record `one` flattened into its argument block
static int launch_dag_bulk_single(hipStream_t s, bool ldl, const DagInst& one, const int* tasks, int ntasks, int ntile, int* qctr,
                                  long spin_limit, int nwg, unsigned long long* trace, unsigned long long* wgstat, const int* qoff,
                                  int* qheads, int nq) {
    if (ntasks <= 0) return 0;
    DagArgs1 a{one.F, one.ld, one.V, one.dinv, one.dblk, one.inv16, reinterpret_cast<const int4*>(tasks), ntasks, one.front, one.af,
               one.tprog, ntile, qctr, one.info, spin_limit, trace, wgstat, one.vmax, dag_fake_share(), one.zfill, one.N, one.env, one.envgate,
               one.envh, qoff, qheads, nq};
    return launch_bulk1(s, ldl, a, nwg);
}

int launch_dag_bulk_merged(hipStream_t s, bool ldl, const DagInst* insts, const int* tasks, int ntasks, int ntile, int* qctr,
                           long spin_limit, int nwg) {
    if (ntasks <= 0) return 0;
    DagArgs a{insts, reinterpret_cast<const int4*>(tasks), ntasks, ntile, qctr, spin_limit, nullptr, nullptr, dag_fake_share()};
    return launch_bulk_batch(s, ldl, a, nwg);
}

// dag_reset_kernel in its three uses.  (progress words and `info` in ONE launch: two memsets are two fill kernels, ~8 us each in
// front of the pivot chain)
static dim3 dag_reset_grid(int64_t Np, int systems) {
    return dim3((unsigned)std::min<size_t>((DagPlan::progress_words(Np) + 1023) / 1024, 64), (unsigned)systems);
}
// one factorization: also the heads of its per-XCD queues; consumes the envelope word
static void dag_reset_single(hipStream_t s, mnk_ls* ls, const DagInst& rec) {
    hipLaunchKernelGGL(dag_reset_kernel, dag_reset_grid(ls->Np, 1), dim3(256), 0, s, ls->plan.flags.p, (int64_t)DagPlan::progress_words(ls->Np),
                       ls->info_dev.p, rec, (DagInst*)nullptr, (const SmallSysRec*)nullptr, ls->env_word.p, ls->plan.qheads.p,
                       ls->plan.qheads.p ? 2 * DAG_QHEAD_WORDS : 0);
    ls->src.env_armed = false;
}
// (the instance's record for the bulk kernel rides along with the reset of its progress words)
void dag_reset_member(hipStream_t s, mnk_ls* ls, const DagInst& rec, DagInst* rec_dst) {
    hipLaunchKernelGGL(dag_reset_kernel, dag_reset_grid(ls->Np, 1), dim3(256), 0, s, ls->plan.flags.p, (int64_t)DagPlan::progress_words(ls->Np),
                       ls->info_dev.p, rec, rec_dst, (const SmallSysRec*)nullptr, ls->env_word.p);
    ls->src.env_armed = false;
}
// (blockIdx.y = system; the instance records are uploaded by the host, no envelope word is consumed: the round runs dense)
void dag_reset_round(hipStream_t s, int64_t Np, const SmallSysRec* recs_dev, int k) {
    hipLaunchKernelGGL(dag_reset_kernel, dag_reset_grid(Np, k), dim3(256), 0, s, (int*)nullptr, (int64_t)0, (int*)nullptr, DagInst{},
                       (DagInst*)nullptr, recs_dev);
}

}  // namespace mnk

using namespace mnk;

// First launch of the bulk kernels on a stream, with an EMPTY queue (every workgroup leaves at once): the code objects are
// loaded and the stream's hardware queue gets its scratch memory (these kernels spill a few registers) while nothing is
// resident that could wait for them.  Without it the first real factorization of a process launches a pivot chain that
// spins for a bulk kernel the runtime is still setting up -- normally microseconds, but seen to exceed the bound of the
// device-side waits (info = -7, schedule 1 for the next 16 factorizations: round 3 met it in 2 of ~150 bench processes, this
// round in 1 of 8 runs of tools/dag_time.py).  Called once per device when its task-DAG streams are created (ctx.hip).
int mnk_dag_warmup(hipStream_t* streams, int n, int nwg) {
    static mnk::DevBuf<int> ctr;   // (process lifetime)
    if (!ctr.p) {
        if (ctr.alloc(4)) return -2;
        MNK_HIP(hipMemset(ctr.p, 0, 4 * sizeof(int)));
    }
    for (int i = 0; i < n; ++i) {
        if (streams[i] == nullptr) continue;
        mnk::DagArgs1 a1{};
        a1.qctr = ctr.p;
        a1.info = ctr.p + 1;
        mnk::DagArgs a{};
        a.qctr = ctr.p;
        // (a FULL-size grid: the runtime sizes a queue's scratch by the dispatch that asks for it)
        int rc = mnk::launch_bulk1(streams[i], true, a1, nwg);
        if (!rc) rc = mnk::launch_bulk1(streams[i], false, a1, nwg);
        if (!rc) rc = mnk::launch_bulk_batch(streams[i], true, a, nwg);
        if (!rc) rc = mnk::launch_bulk_batch(streams[i], false, a, nwg);
        if (rc) return rc;
    }
    for (int i = 0; i < n; ++i)
        if (streams[i] != nullptr) MNK_HIP(mnk::stream_wait(streams[i]));
    return 0;
}

// Bound of the schedule's device-side waits, in polls of ~0.17 us.  Every wait is on work that is queued or resident, so a
// bound only ever expires when something outside the schedule keeps a kernel of the group from running: another process'
// kernels on the CUs, a copy between pageable host memory and the device by OTHER code of this process, a device-synchronizing
// runtime call between the group's launches.  The recovery is cheap (the factorization is redone
// with one launch per piece, the schedule is tried again 16 factorizations later), a long bound is not: whatever stops the
// group costs the bound.  History: 2^24 polls (~3 s) in round 3; ~100 x the factorization's time, at least 1 s, in round 4 --
// a bound of 0.3 s then expired about once in 1000 factorizations on transient stalls, which turned out to be the workgroups of
// an oversized bulk grid that the hardware placed in mid-kernel (grid 720 -> 672).  With that
// grid, round 5 ran 3 x 10 240 factorizations of the C3 system at bounds of 0.05 / 0.1 / 0.3 s without a single expiry
// (profiles/r05_spin_bound_sweep.txt): the default is now ~10 x the time the factorization should take, at least 0.1 s -- the
// longest legitimate wait is a fraction of one factorization (a chain strip waiting for its band tiles: ~0.3 ms at N = 11 192).
long mnk_ls_dag_spin_limit(const mnk_ls* ls) {
    if (ls->dag_spin_limit > 0) return ls->dag_spin_limit;
    const double n = (double)ls->Np;
    const double t_est = n * n * n / 3.0 / 50e12;   // seconds at ~0.64 of the fp64 peak
    const double polls = 10.0 * t_est / 0.17e-6;
    //  several contexts alive on the device: the soak runs behind the 0.1 s floor were single-context; beside other
    // contexts' persistent groups (the case mnk_release_idle_streams exists for) short stalls are legitimate, and an expiry costs a
    // whole redo plus 16 / 64 / 256 factorizations on the slow schedule -- the floor is the old 1 s there
    const double floor_polls = mnk_live_contexts(ls->ctx->device) > 1 ? 5880000.0 : 588000.0;
    return (long)std::min(16777216.0, std::max(floor_polls, polls));
}

// ---- DagPlan (ls.h): the sizes of its device words ----
size_t DagPlan::progress_words(int64_t Np) {   // two queue counters | front | af | tprog
    const int64_t ntile = Np / 128;
    return (size_t)2 + (size_t)(Np / NBI) + 2 * (size_t)ntile * ntile;
}

size_t DagPlan::trace_words() const { return (size_t)list.size() * 8 + 4096 * 8 + 1024 * 8; }

mnk::DagInst mnk::dag_prepare_instance(mnk_ls* ls, bool dense) {
    const int ntile = (int)(ls->Np / 128), nblk = (int)(ls->Np / NBI);
    int* front = ls->plan.flags.p + 2;   // (the layout DagPlan::progress_words sizes)
    int* af = front + nblk;
    int* tprog = af + (size_t)ntile * ntile;
    // the spare factor buffer is zeroed by the queue's DAG_FILL tasks when the NEXT transfer will want it (a sparse source was
    // transferred for this factorization) and no background fill of it is in flight
    double* zfill = ls->dag_fill && ls->plan.key.has_fill ? ls->spare.dag_target() : nullptr;
    // the envelope of a sparse source (ls.hip: set_envelope); the bulk kernel reads the verdict on its finiteness (env_word[1])
    const bool env = !dense && ls->envelope && ls->src.env_dev != nullptr && ls->env_word.p != nullptr;
    const mnk::DagInst inst{ls->fact.p, ls->ld, ls->algo == MNK_LDL ? ls->vfull.p : nullptr, ls->dinv.p, ls->dblk.p, ls->inv16.p,
                            front, af, tprog, ls->info_dev.p, ls->bk.growth_word(ls), zfill, ls->N, env ? ls->src.env_dev : nullptr,
                            env ? ls->env_word.p + 1 : nullptr, env && ls->envelope_half ? ls->src.envh_dev : nullptr};
    // what the solver remembers about this launch: the spare buffer is being zeroed by it, the statistics count its envelope
    ls->spare.dag_fills(inst.zfill != nullptr);
    ls->env_used = inst.env != nullptr;
    ls->envh_used = inst.envh != nullptr;
    return inst;
}

// Buffers of the task-DAG schedule: the task list (built once per matrix order and option set), the progress words and,
// for LDL^T, V = L D of every column (a second N x N array).  Returns 0 when everything is there; non-zero when the device
// cannot hold it -- the caller keeps schedule 4 then (round 3 returned -2 from factorize! instead).  The spare factor buffer
// of the background zero-fill is given up first: with many solvers per GPU it can be the allocation that took V's memory.
int mnk_ls_dag_prepare(mnk_ls* ls) {
    mnk_ctx* ctx = ls->ctx;
    hipStream_t s = ctx->stream;
    const int64_t Np = ls->Np, ld = ls->ld;
    const bool ldl = ls->algo == MNK_LDL;
    const int ntile = (int)(Np / 128);
    auto give_up = [&]() {
        (void)hipGetLastError();
        ls->plan.invalidate();
        ls->plan.flags.release();
        ls->plan.qoff.release();
        ls->plan.qheads.release();
        ls->vfull.release();
        return 1;
    };
    if (!ls->plan.valid()) {
        // Two band shapes.  Large systems (more than dag_cus2 strips of 64 rows): a shallow band on a handful of CUs, the
        // rows below it closed by the bulk kernel's own tasks -- the factorization is bound by the bulk work for most of its
        // columns.  Small systems: EVERY row is a strip of the chain's band (one CU each, on a larger partition) and the
        // bulk kernel only accumulates: they are bound by the pivot chain from the first column on, and a row of tiles that
        // the bulk kernel closes advances one tile column per {K = 128 step + finalization} ~ 80 us against the chain's
        // ~50 us.  (Switching from the first shape to the second in mid-factorization, once dag_cus2 strips remain, is
        // supported by the task list -- dag_js2 -- and was measured: the deep band needs one CU per strip, the remaining bulk
        // work of a C3-size system then no longer fits the smaller bulk partition, 10.7 vs 10.3 ms.)
        // (round 6: the deep band pays up to ~5300 rows -- all rows in the band against band + bulk kernel throughout, LDL^T, one box:
        // N = 4096 1.61 vs 1.73 ms, 4608 1.86 vs 1.99, 5120 2.20 vs 2.27, 5632 2.70 vs 2.59, 6144 3.24 vs 2.93 (Cholesky 5632: 2.75 vs 2.46) --
        // above that every strip's left-looking prologue on its one CU costs more than the bulk kernel's closing tasks; the limit
        // was the partition's 96 strips = 6144 rows: dag_deep_rows)
        // (the rule, with the bound on an override that would leave the deep band more strips than it has CUs: dag_plan.h)
        ls->plan.key.js2 = mnk::dag_choose_js2(Np, ctx->dag_cus2, ls->dag_deep_rows, ls->dag_js2_override);
        mnk::DagTaskList& h = ls->plan.list;
        ls->plan.key.chunk = ls->dag_chunk; ls->plan.key.taper0 = ls->dag_taper0; ls->plan.key.band = ls->dag_band;
        h = mnk::dag_build_tasks(ntile, ls->dag_chunk, ls->dag_band / 2, ls->plan.key.js2, ls->dag_taper0);
        // zero-fill of the next factorization's buffer as tasks of the queue (sparse sources; see dag_fill_tile)
        ls->plan.key.has_fill = ls->dag_fill && ls->spare.wanted(Np);
        if (ls->plan.key.has_fill && h.tasks.empty()) ls->plan.key.has_fill = false;   // (a system of a few hundred rows has no bulk task: nothing to ride on)
        if (ls->plan.key.has_fill) mnk::dag_add_fill_tasks(ntile, h);
        // Per-XCD queues: the device list is the host list dealt per phase (dag_plan.h: dag_deal_list).  A phase keeps ONE queue
        // when its bulk grid might leave an XCD without a workgroup -- a queue nobody owns is only served by thieves, which come
        // when their own queues are empty, and the progress argument needs an owner -- or when the list does not fit the task's
        // fields (a list position beside the tile column: 20 | 12 bits).
        const bool queues = ls->dag_xcd_queues && mnk::DagTask::fits(ntile, 1, h.size());
        const int part[3] = {0, h.n1, h.size()}, chain_cus[2] = {ctx->dag_cus, ctx->dag_cus2};
        bool may_queue[2];
        for (int ph = 0; ph < 2; ++ph)
            may_queue[ph] = queues && part[ph + 1] - part[ph] >= mnk::grid_at_launch(0, ctx->num_cu, chain_cus[ph], 3) && mnk::bulk_xcds(0, ctx->num_cu, chain_cus[ph]) == mnk::DAG_NQ;
        const mnk::DagDealtList dev_list = mnk::dag_deal_list(h, mnk::DAG_NQ, ls->dag_gang, may_queue);
        std::vector<int> qoff(32, 0);   // (16 per phase)
        for (int ph = 0; ph < 2; ++ph) {
            std::copy_n(dev_list.qoff.begin() + ph * (mnk::DAG_NQ + 1), mnk::DAG_NQ + 1, qoff.begin() + 16 * ph);
            ls->plan.nq[ph] = dev_list.nq[ph];
        }
        if (ls->plan.tasks.alloc(4 * h.tasks.size() + 4)) return give_up();
        if (!ls->plan.qoff.p && ls->plan.qoff.alloc(qoff.size())) return give_up();
        if (!ls->plan.qheads.p && ls->plan.qheads.alloc(2 * (size_t)mnk::DAG_QHEAD_WORDS)) return give_up();
        {
            mnk::H2DGuard h2d;   // (a pageable upload beside another context's persistent group would stop that group: common.h)
            if (!h.tasks.empty() && hipMemcpyAsync(ls->plan.tasks.p, dev_list.tasks.data(), dev_list.tasks.size() * sizeof(mnk::DagTask), hipMemcpyHostToDevice, s) != hipSuccess) return give_up();
            if (hipMemcpyAsync(ls->plan.qoff.p, qoff.data(), qoff.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return give_up();
            if (mnk::stream_wait(s) != hipSuccess) return give_up();
        }
        if (ls->plan.flags.alloc(DagPlan::progress_words(Np))) return give_up();
    }
    if (ldl && !ls->vfull.p && ls->vfull.alloc((size_t)ld * Np + SLACK)) {   // V = L D of every column (LDL^T)
        (void)hipGetLastError();
        if (!ls->spare.give_up() || ls->vfull.alloc((size_t)ld * Np + SLACK) != 0) return give_up();
    }
    if (ls->dag_trace_on) {
        if (ls->dag_trace.n < ls->plan.trace_words() && ls->dag_trace.alloc(ls->plan.trace_words())) return give_up();   // (the task list may have been rebuilt with more tasks)
    }
    return 0;
}

// Host driver of the task-DAG schedule (panel_algo = 5): ONE persistent pivot-chain launch (factor.hip: pchain_kernel, one
// workgroup per 64-row strip of the band, on the chain's CU partition) beside ONE persistent bulk launch on all the other
// CUs; the two sides meet through progress words in device memory, no event is recorded or awaited between the fork and
// the join.  The buffers come from mnk_ls_dag_prepare (called by mnk_ls_run_factorization before it settles on this schedule).
int mnk_ls_run_factorization_dag(mnk_ls* ls) {
    mnk_ctx* ctx = ls->ctx;
    hipStream_t s = ctx->stream;
    const int64_t Np = ls->Np;
    const bool ldl = ls->algo == MNK_LDL;
    const int ntile = (int)(Np / 128), nsc = (int)((Np + 255) / 256);
    MNK_REQUIRE(ls->plan.tasks.p && ls->plan.flags.p && (!ldl || ls->vfull.p), "task-DAG schedule: mnk_ls_dag_prepare was not called");
    const mnk::DagInst inst = mnk::dag_prepare_instance(ls, false);
    mnk::dag_reset_single(s, ls, inst);
    int* qctr = ls->plan.flags.p;
    int* front = inst.front;
    const long spin_limit = mnk_ls_dag_spin_limit(ls);
    unsigned long long* trace = nullptr;
    if (ls->dag_trace_on && ls->dag_trace.p) {
        MNK_HIP(hipMemsetAsync(ls->dag_trace.p, 0, ls->plan.trace_words() * sizeof(unsigned long long), s));
        trace = ls->dag_trace.p;
    }
    const int js2 = ls->plan.key.js2, ntasks = ls->plan.list.size(), ntasks1 = ls->plan.list.n1;
    // one phase = one persistent bulk launch (update stream) beside one persistent chain launch (panel stream)
    auto phase = [&](hipStream_t sp, hipStream_t su, int chain_cus, int task0, int ntask, int* counter, int js_begin, int js_end,
                     unsigned strips) -> int {
        // A small system (every row a strip of the chain, one phase) runs its chain on the CALLER's stream: no fork in front
        // of the first diagonal block, no join behind the last one, and the inverses simply follow the chain.  Its workgroups
        // are dispatched before the bulk kernel's (which waits for the event) and need a CU each to themselves (registers);
        // the CUs outside the bulk stream's mask -- at least as many as there are strips -- cannot be taken from them.
        const bool small = js_begin == 0 && js_end == nsc && js2 == 0;
        if (small) sp = s;
        MNK_HIP(hipEventRecord(ctx->ev_a, s));
        if (!small) MNK_HIP(hipStreamWaitEvent(sp, ctx->ev_a, 0));
        MNK_HIP(hipStreamWaitEvent(su, ctx->ev_a, 0));
        mnk::PpDag dag{front, inst.af, ntile, 0, 0, -1, spin_limit, trace ? trace + (size_t)ntasks * 8 + (size_t)js_begin * 8 * 16 : nullptr,
                  ls->bk.growth_word(ls), ls->dag_debug ? ls->dag_dbg.p : nullptr};
        // (the chain first: its first diagonal block is the start of the critical path, the bulk kernel has nothing to do before it)
        int rc = mnk_launch_pchain(ls, sp, dag, js_begin, js_end, strips);
        if (rc) return rc;
        // (more than three workgroups per CU -- to fill slots a shader-engine-imbalanced mask might leave empty -- measured
        // no difference: 4 / 5 / 6 per CU 9.63-9.67 vs 9.64-9.68 ms)
        const int ph = (int)(counter - qctr), nq = ls->plan.nq[ph];
        // (per-XCD queues: every queue needs workgroups of its own XCD -- the grid the list was dealt for, see mnk_ls_dag_prepare)
        const int bulk_wgs = mnk::grid_at_launch(0, ctx->num_cu, chain_cus, 3);
        MNK_REQUIRE(nq == 0 || (ntask >= bulk_wgs && mnk::bulk_xcds(0, ctx->num_cu, chain_cus) == nq),
                    "task-DAG schedule: the bulk grid does not cover the XCDs the task list was dealt for");
        rc = mnk::launch_dag_bulk_single(su, ldl, inst, ls->plan.tasks.p + 4 * (size_t)task0, ntask, ntile, counter, spin_limit,
                                  std::min(ntask, bulk_wgs), trace ? trace + 8 * (size_t)task0 : nullptr,
                                  trace ? trace + (size_t)ntasks * 8 + 4096 * 8 + (task0 > 0 ? 512 * 8 : 0) : nullptr,
                                  ls->plan.qoff.p + 16 * ph, ls->plan.qheads.p + ph * mnk::DAG_QHEAD_WORDS, nq);
        if (rc) return rc;
        // Once the bulk kernel has run out of tasks every tile-closing task is done, hence every strip-column that still
        // had rows below the band is final: its diagonal blocks are inverted for the solves here, behind the bulk kernel
        // on its stream, while the chain works on the last strip-columns (all rows in the band: no bulk task left).
        // (Measured and dropped in round 4: the inverses of the LAST strip-columns one by one on this stream behind device-side
        // gates on the chain's progress.  The bulk kernel leaves only ~130 us before the chain's end -- its last tile-closing
        // tasks -- and every gated launch pair costs ~170 us whatever its size: C3 factorize! 9.66 -> 10.78 ms.)
        if (js_begin == 0 && js_end > 0) {
            const int64_t safe = std::min<int64_t>(js_end, std::max<int64_t>(0, (ntile - ls->dag_band / 2 - 1) / 2)) & ~(int64_t)1;  // (even: 512-row triangles)
            if (strips == (unsigned)ls->dag_band && safe > 0) {
                rc = mnk_ls_invert_blocks(ls, su, 0, safe);
                if (rc) return rc;
                ls->inv_done = safe;
            }
        }
        if (small) {
            rc = mnk_ls_invert_blocks(ls, s, 0, nsc);
            if (rc) return rc;
            ls->inv_done = nsc;
        }
        if (!small) MNK_HIP(hipEventRecord(ctx->ev_a, sp));
        MNK_HIP(hipEventRecord(ctx->ev_b, su));
        if (!small) MNK_HIP(hipStreamWaitEvent(s, ctx->ev_a, 0));
        MNK_HIP(hipStreamWaitEvent(s, ctx->ev_b, 0));
        return 0;
    };
    // (the pairs are there: mnk_ls_run_factorization asked for them when it settled on this schedule)
    hipStream_t sp = nullptr, su = nullptr;
    if (js2 > 0) {
        int rc = mnk_ctx_stream_pair(ctx, mnk::PAIR_DAG, 0, &sp, &su);
        if (rc) return rc;
        MNK_REQUIRE(sp != nullptr, "task-DAG schedule: the chain and bulk streams are missing");
        rc = phase(sp, su, ctx->dag_cus, 0, ntasks1, qctr, 0, std::min(js2, nsc), (unsigned)std::min<int64_t>(ls->dag_band, Np / NBI));
        if (rc) return rc;
    }
    if (js2 < nsc) {
        const int64_t rows2 = Np - 256 * (int64_t)js2;
        int rc = mnk_ctx_stream_pair(ctx, mnk::PAIR_DEEP, 0, &sp, &su);
        if (rc) return rc;
        MNK_REQUIRE(sp != nullptr, "task-DAG schedule: the deep-band streams are missing");
        rc = phase(sp, su, ctx->dag_cus2, ntasks1, ntasks - ntasks1, qctr + 1, js2, nsc, (unsigned)(rows2 / NBI));
        if (rc) return rc;
    }
    return 0;
}


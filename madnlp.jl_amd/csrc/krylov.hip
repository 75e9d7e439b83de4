// Vector kernels of the restarted GMRES refinement (the `iterator = "krylov"` option of both IPM drivers; capability of the
// reference's lib/MadNLPKrylov, algorithm in DESIGN.md section 17; host mirror madnlp.jl_amd/backsolve.py `KrylovIterator`).
// The basis V is a device buffer of restart + 1 columns with leading dimension ldv >= n, u the vector being orthogonalized.
// One Arnoldi step is  dots -> project -> dots -> project -> normalize,  enqueued back to back: the coefficients and the norm
// pass from launch to launch in device memory (mnk_ipm::kry_res / kry_part) and reach the host together, at the one
// synchronization of the step.  The Givens rotations, the triangular solve and every decision stay on the host.
//
// Ordinary grid launches on the context's stream, IPM_BLOCKS x IPM_THREADS lanes with a grid stride: element i belongs to lane
// i mod 65536, a lane adds its terms in increasing i, the block and the block partials are added by the halving trees of
// map_reduce_kernel / final_reduce_kernel (ipm_vec.hip) -- every sum has the bits of `ordered_sum` (ipm.py) over the same
// terms, and every product, sum and difference is rounded on its own (no FMA contraction), so the host mirror reproduces
// each kernel bit for bit.  HBM-bound: 8 (k + 1) n bytes read per dots, 8 (k + 2) n moved per project / axpy, 16 n per
// normalize.
#pragma clang fp contract(off)
#include <cmath>

#include "common.h"
#include "ipm_handle.h"

using namespace mnk;

namespace {

constexpr int KRY_MAX = 8;   // columns per call: the largest restart length

struct KryCoef { double v[KRY_MAX]; };

// the block's sum of v (fixed tree, as block_reduce_store of ipm_vec.hip); may be called more than once per kernel
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double sh[IPM_THREADS];
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = IPM_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// a result word in pinned, device-mapped host memory (the store of final_reduce_kernel)
__device__ __forceinline__ void store_result(double* res, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(res), (unsigned long long)__double_as_longlong(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// part[j][block] = the block's share of V_j . u (j < k), part[k][block] of u . u: one pass over u and the k columns
__global__ __launch_bounds__(IPM_THREADS) void kry_dots_kernel(const double* __restrict__ V, int64_t ldv, int k,
                                                                const double* __restrict__ u, int64_t n,
                                                                double* __restrict__ part) {
    double acc[KRY_MAX], uu = 0.0;
#pragma unroll
    for (int j = 0; j < KRY_MAX; ++j) acc[j] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS) {
        const double ui = u[i];
#pragma unroll
        for (int j = 0; j < KRY_MAX; ++j)
            if (j < k) acc[j] += V[j * ldv + i] * ui;
        uu += ui * ui;
    }
#pragma unroll
    for (int j = 0; j < KRY_MAX; ++j) {
        if (j < k) {   // (k is uniform: every thread of the block takes the same branches)
            const double r = block_sum(acc[j]);
            if (threadIdx.x == 0) part[j * IPM_BLOCKS + blockIdx.x] = r;
        }
    }
    const double r = block_sum(uu);
    if (threadIdx.x == 0) part[k * IPM_BLOCKS + blockIdx.x] = r;
}

// block j: the sum of the partials of slot j, to the pinned slot and to the device-side copy
__global__ __launch_bounds__(IPM_THREADS) void kry_final_kernel(const double* __restrict__ part, double* __restrict__ res,
                                                                 double* __restrict__ dev) {
    double v = 0.0;
    for (int i = threadIdx.x; i < IPM_BLOCKS; i += IPM_THREADS) v += part[blockIdx.x * IPM_BLOCKS + i];
    v = block_sum(v);
    if (threadIdx.x == 0) {
        dev[blockIdx.x] = v;
        store_result(res + blockIdx.x, v);
    }
}

// u -= sum_j coef[j] V_j in the order j = 0 .. k-1, one multiply and one subtract each; part_uu[block] = the block's share
// of the new u . u
__global__ __launch_bounds__(IPM_THREADS) void kry_project_kernel(double* __restrict__ u, const double* __restrict__ V,
                                                                   int64_t ldv, int k, int64_t n,
                                                                   const double* __restrict__ coef,
                                                                   double* __restrict__ part_uu) {
    double c[KRY_MAX], uu = 0.0;
#pragma unroll
    for (int j = 0; j < KRY_MAX; ++j) c[j] = j < k ? coef[j] : 0.0;
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS) {
        double t = u[i];
#pragma unroll
        for (int j = 0; j < KRY_MAX; ++j)
            if (j < k) t = t - c[j] * V[j * ldv + i];
        u[i] = t;
        uu += t * t;
    }
    const double r = block_sum(uu);
    if (threadIdx.x == 0) part_uu[blockIdx.x] = r;
}

// x += sum_j y[j] V_j in the order j = 0 .. k-1, one multiply and one add each
__global__ __launch_bounds__(IPM_THREADS) void kry_axpy_kernel(double* __restrict__ x, const double* __restrict__ V,
                                                                int64_t ldv, int k, KryCoef y, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS) {
        double t = x[i];
#pragma unroll
        for (int j = 0; j < KRY_MAX; ++j)
            if (j < k) t = t + y.v[j] * V[j * ldv + i];
        x[i] = t;
    }
}

// part_uu[block] = the block's share of u . u (what kry_project_kernel leaves, for a vector that was not projected)
__global__ __launch_bounds__(IPM_THREADS) void kry_uu_kernel(const double* __restrict__ u, int64_t n,
                                                              double* __restrict__ part_uu) {
    double uu = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS)
        uu += u[i] * u[i];
    const double r = block_sum(uu);
    if (threadIdx.x == 0) part_uu[blockIdx.x] = r;
}

// v = u / |u|: every block adds the IPM_BLOCKS partials of u . u itself (2 KiB from L2, the tree of kry_final_kernel), so the
// norm needs no launch of its own; block 0 reports it
__global__ __launch_bounds__(IPM_THREADS) void kry_normalize_kernel(double* __restrict__ v, const double* __restrict__ u,
                                                                     int64_t n, const double* __restrict__ part_uu,
                                                                     double* __restrict__ res, double* __restrict__ dev) {
    double s = 0.0;
    for (int i = threadIdx.x; i < IPM_BLOCKS; i += IPM_THREADS) s += part_uu[i];
    const double nrm = sqrt(block_sum(s));
    for (int64_t i = blockIdx.x * (int64_t)IPM_THREADS + threadIdx.x; i < n; i += (int64_t)IPM_BLOCKS * IPM_THREADS)
        v[i] = u[i] / nrm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *dev = nrm;
        store_result(res, nrm);
    }
}

}  // namespace

extern "C" {

#define KRY_ENTER(ptrs, who)                                                                    \
    MNK_REQUIRE(h != nullptr && (ptrs), who ": NULL argument");                                 \
    MNK_REQUIRE(k >= 1 && k <= KRY_MAX, who ": k must be 1 to 8");                              \
    MNK_REQUIRE(n >= 0 && ldv >= n, who ": n must not be negative and ldv not smaller than n"); \
    MNK_HIP(hipSetDevice(h->ctx->device))
#define KRY_GRID dim3(IPM_BLOCKS), dim3(IPM_THREADS), 0, h->ctx->stream

int mnk_ipm_krylov_dots(mnk_ipm* h, const double* V, int64_t ldv, int k, const double* u, int64_t n, double* out) {
    KRY_ENTER(V && u && out, "mnk_ipm_krylov_dots");
    const int cnt = k + 1;
    const int b = ipm_slot_base(h, cnt);
    if (b < 0) return -1;
    double* part = h->part.p + b * IPM_BLOCKS;
    hipLaunchKernelGGL(kry_dots_kernel, KRY_GRID, V, ldv, k, u, n, part);
    hipLaunchKernelGGL(kry_final_kernel, dim3((unsigned)cnt), dim3(IPM_THREADS), 0, h->ctx->stream, part, h->pin_dev + b,
                       h->kry_res.p + b);
    MNK_HIP(hipGetLastError());
    h->kry_last = h->kry_res.p + b;
    return ipm_finish(h, b, cnt, [=](const double* r) { for (int i = 0; i < cnt; ++i) out[i] = r[i]; });
}

int mnk_ipm_krylov_last_dots(mnk_ipm* h, const double** coef) {
    MNK_REQUIRE(h != nullptr && coef != nullptr, "mnk_ipm_krylov_last_dots: NULL argument");
    MNK_REQUIRE(h->kry_last != nullptr, "mnk_ipm_krylov_last_dots: no mnk_ipm_krylov_dots call yet");
    *coef = h->kry_last;
    return 0;
}

int mnk_ipm_krylov_project(mnk_ipm* h, double* u, const double* V, int64_t ldv, int k, int64_t n, const double* coef) {
    KRY_ENTER(u && V && coef, "mnk_ipm_krylov_project");
    hipLaunchKernelGGL(kry_project_kernel, KRY_GRID, u, V, ldv, k, n, coef, h->kry_part.p);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_ipm_krylov_axpy(mnk_ipm* h, double* x, const double* V, int64_t ldv, int k, const double* y_host, int64_t n) {
    KRY_ENTER(x && V && y_host, "mnk_ipm_krylov_axpy");
    KryCoef y{};
    for (int j = 0; j < k; ++j) y.v[j] = y_host[j];
    hipLaunchKernelGGL(kry_axpy_kernel, KRY_GRID, x, V, ldv, k, y, n);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_ipm_krylov_normalize(mnk_ipm* h, double* v, const double* u, int64_t n, int after_project, double* out) {
    MNK_REQUIRE(h != nullptr && v && u && out, "mnk_ipm_krylov_normalize: NULL argument");
    MNK_REQUIRE(n >= 0 && (after_project == 0 || after_project == 1), "mnk_ipm_krylov_normalize: bad argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    const int b = ipm_slot_base(h, 1);
    if (b < 0) return -1;
    if (!after_project) hipLaunchKernelGGL(kry_uu_kernel, KRY_GRID, u, n, h->kry_part.p);
    hipLaunchKernelGGL(kry_normalize_kernel, KRY_GRID, v, u, n, h->kry_part.p, h->pin_dev + b, h->kry_res.p + b);
    MNK_HIP(hipGetLastError());
    return ipm_finish(h, b, 1, [=](const double* r) { *out = r[0]; });
}

}  // extern "C"

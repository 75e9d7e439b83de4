// NLP scaling and objective sense on device vectors: what the reference's callback wrappers apply around a model's raw
// values (src/Callbacks/nlpmodels.jl:771-906 `c .*= con_scale`, `grad .*= obj_scale`, `jac .*= jac_scale`,
// `con_buffer .= y .* con_scale`; src/IPM/callbacks.jl:28-30,48-49 the sign, the slack and rhs).  Plain streaming kernels:
// 8 bytes per element read / written, coalesced, grid-stride above SCALE_MAX_BLOCKS workgroups.  No FMA contraction: every
// product and difference is rounded on its own, as the numpy mirror (`madnlp_jl_amd.ipm`) and Julia's broadcast do.
#pragma clang fp contract(off)
#include "common.h"
#include "ipm_handle.h"

using namespace mnk;

namespace {

constexpr int SCALE_THREADS = 256;
constexpr int64_t SCALE_MAX_BLOCKS = 2048;

inline dim3 scale_grid(int64_t n) {
    const int64_t b = (n + SCALE_THREADS - 1) / SCALE_THREADS;
    return dim3((unsigned)(b < SCALE_MAX_BLOCKS ? b : SCALE_MAX_BLOCKS));
}

// out = a .* b (out may alias a or b: every element is read before it is written, by the same thread)
__global__ __launch_bounds__(SCALE_THREADS) void vec_mul_kernel(double* out, const double* a, const double* b, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * SCALE_THREADS;
    for (int64_t i = blockIdx.x * (int64_t)SCALE_THREADS + threadIdx.x; i < n; i += stride) out[i] = a[i] * b[i];
}

// c[i] = c[i] * con_scale[i] - slack[pos(i)] - rhs[i], in this order; pos(i) = i (identity), slack_pos[i] (< 0: row i is an
// equality and has no slack), or none at all (ns == 0)
__global__ __launch_bounds__(SCALE_THREADS) void scale_cons_kernel(double* __restrict__ c, const double* __restrict__ con_scale,
                                                                    const double* __restrict__ slack,
                                                                    const int64_t* __restrict__ slack_pos, int64_t ns,
                                                                    const double* __restrict__ rhs, int64_t m) {
    const int64_t stride = (int64_t)gridDim.x * SCALE_THREADS;
    for (int64_t i = blockIdx.x * (int64_t)SCALE_THREADS + threadIdx.x; i < m; i += stride) {
        double v = c[i];
        if (con_scale != nullptr) v = v * con_scale[i];
        const int64_t p = ns == 0 ? -1 : (slack_pos != nullptr ? slack_pos[i] : i);
        if (p >= 0 && p < ns) v = v - slack[p];
        c[i] = v - rhs[i];
    }
}

// f[:n] *= factor, f[n:ntot] = 0
__global__ __launch_bounds__(SCALE_THREADS) void scale_grad_kernel(double* __restrict__ f, int64_t n, int64_t ntot, double factor) {
    const int64_t stride = (int64_t)gridDim.x * SCALE_THREADS;
    for (int64_t i = blockIdx.x * (int64_t)SCALE_THREADS + threadIdx.x; i < ntot; i += stride) f[i] = i < n ? f[i] * factor : 0.0;
}

}  // namespace

extern "C" {

int mnk_ipm_vec_mul(mnk_ipm* h, double* out, const double* a, const double* b, int64_t n) {
    MNK_REQUIRE(h != nullptr && n >= 0 && (n == 0 || (out && a && b)), "mnk_ipm_vec_mul: bad argument");
    if (n == 0) return 0;
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(vec_mul_kernel, scale_grid(n), dim3(SCALE_THREADS), 0, h->ctx->stream, out, a, b, n);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_ipm_scale_cons(mnk_ipm* h, double* c, const double* con_scale, const double* slack, const int64_t* slack_pos,
                       int64_t ns, const double* rhs, int64_t m) {
    MNK_REQUIRE(h != nullptr && m >= 0 && ns >= 0 && ns <= m, "mnk_ipm_scale_cons: bad size");
    MNK_REQUIRE(m == 0 || (c && rhs), "mnk_ipm_scale_cons: NULL c or rhs");
    MNK_REQUIRE(ns == 0 || slack, "mnk_ipm_scale_cons: NULL slack");
    MNK_REQUIRE(ns == 0 || ns == m || slack_pos, "mnk_ipm_scale_cons: 0 < ns < m needs the rows' slack positions");
    if (m == 0) return 0;
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(scale_cons_kernel, scale_grid(m), dim3(SCALE_THREADS), 0, h->ctx->stream, c, con_scale, slack, slack_pos,
                       ns, rhs, m);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_ipm_scale_grad(mnk_ipm* h, double* f, int64_t n, int64_t ntot, double factor) {
    MNK_REQUIRE(h != nullptr && n >= 0 && ntot >= n && (ntot == 0 || f), "mnk_ipm_scale_grad: bad argument");
    if (ntot == 0) return 0;
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(scale_grad_kernel, scale_grid(ntot), dim3(SCALE_THREADS), 0, h->ctx->stream, f, n, ntot, factor);
    MNK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// Fixed variables made parameters on device vectors: the reference's `MakeParameter` callback wrappers
// (src/Callbacks/nlpmodels.jl:912-1033: `_update_x!`, `grad .= g_full[free]`, `jac .= jac_full[ind_jac_free]`,
// `hess .= hess_full[ind_hess_free]`, the dense `grad[fixed] = x[fixed] - lvar[fixed]`) around a model that is evaluated at
// its FULL length.  The handle owns the index sets and x_full; the fixed entries of x_full are written at create and by
// no kernel afterwards.  Plain grid-stride kernels: the compact side (index loads, reduced-vector loads / stores) is
// coalesced, the full-length side is a gather / scatter through the index.  Everything is asynchronous on the context's
// stream; nothing is allocated after create, there are no atomics and no host round trips (mnk_fix_get_x_full, a download
// for tests and reporting, aside).  No FMA contraction: (src * scale) * factor is two rounded products, as in the host layer.
#pragma clang fp contract(off)
#include "common.h"

using namespace mnk;

namespace {

constexpr int FIX_THREADS = 256;
constexpr int64_t FIX_MAX_BLOCKS = 2048;

inline dim3 fix_grid(int64_t n) {
    const int64_t b = (n + FIX_THREADS - 1) / FIX_THREADS;
    return dim3((unsigned)(b < FIX_MAX_BLOCKS ? b : FIX_MAX_BLOCKS));
}

// x_full[idx[i]] = x[i]
__global__ __launch_bounds__(FIX_THREADS) void fix_expand_kernel(double* __restrict__ x_full, const int64_t* __restrict__ idx,
                                                                  const double* __restrict__ x, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * FIX_THREADS;
    for (int64_t i = blockIdx.x * (int64_t)FIX_THREADS + threadIdx.x; i < n; i += stride) x_full[idx[i]] = x[i];
}

// dst[i] = (src[idx[i]] * scale[i]) * factor; scale == nullptr: ones
__global__ __launch_bounds__(FIX_THREADS) void fix_gather_kernel(double* __restrict__ dst, const double* __restrict__ src,
                                                                  const int64_t* __restrict__ idx,
                                                                  const double* __restrict__ scale, double factor, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * FIX_THREADS;
    for (int64_t i = blockIdx.x * (int64_t)FIX_THREADS + threadIdx.x; i < n; i += stride) {
        double v = src[idx[i]];
        if (scale != nullptr) v = v * scale[i];
        dst[i] = v * factor;
    }
}

// g[idx[i]] = x[idx[i]] - value[i]
__global__ __launch_bounds__(FIX_THREADS) void fix_dense_grad_kernel(double* __restrict__ g, const double* __restrict__ x,
                                                                      const int64_t* __restrict__ idx,
                                                                      const double* __restrict__ value, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * FIX_THREADS;
    for (int64_t i = blockIdx.x * (int64_t)FIX_THREADS + threadIdx.x; i < n; i += stride) g[idx[i]] = x[idx[i]] - value[i];
}

// every entry in [0, bound), and (for the sets a kernel scatters through) strictly increasing: no two threads share a target
bool indices_ok(const int64_t* idx, int64_t count, int64_t bound, bool increasing) {
    for (int64_t i = 0; i < count; ++i) {
        if (idx[i] < 0 || idx[i] >= bound) return false;
        if (increasing && i > 0 && idx[i] <= idx[i - 1]) return false;
    }
    return true;
}

}  // namespace

struct mnk_fix {
    mnk_ctx* ctx = nullptr;
    int64_t n = 0, nfree = 0, nfixed = 0, nnzj_full = 0, njac = 0, nnzh_full = 0, nhess = 0;
    DevBuf<int64_t> free_idx, fixed_idx, ind_jac, ind_hess;
    DevBuf<double> value, x_full;
};

extern "C" {

int mnk_fix_create(mnk_ctx* ctx, int64_t n, int64_t nfree, const int64_t* free_idx, int64_t nfixed, const int64_t* fixed_idx,
                   const double* fixed_val, int64_t nnzj_full, int64_t njac, const int64_t* ind_jac_free, int64_t nnzh_full,
                   int64_t nhess, const int64_t* ind_hess_free, void* out_) {
    mnk_fix** out = static_cast<mnk_fix**>(out_);
    MNK_REQUIRE(ctx && out, "mnk_fix_create: NULL argument");
    MNK_REQUIRE(n > 0 && nfree > 0 && nfixed > 0 && nfree + nfixed == n, "mnk_fix_create: need n = nfree + nfixed with both positive");
    MNK_REQUIRE(free_idx && fixed_idx && fixed_val, "mnk_fix_create: NULL index set");
    MNK_REQUIRE(nnzj_full >= 0 && njac >= 0 && njac <= nnzj_full && (njac == 0 || ind_jac_free),
                "mnk_fix_create: bad Jacobian entry set");
    MNK_REQUIRE(nnzh_full >= 0 && nhess >= 0 && nhess <= nnzh_full && (nhess == 0 || ind_hess_free),
                "mnk_fix_create: bad Hessian entry set");
    MNK_REQUIRE(indices_ok(free_idx, nfree, n, true) && indices_ok(fixed_idx, nfixed, n, true),
                "mnk_fix_create: free / fixed must be strictly increasing indices in [0, n)");
    {
        std::vector<char> seen((size_t)n, 0);
        for (int64_t i = 0; i < nfree; ++i) seen[(size_t)free_idx[i]] = 1;
        for (int64_t i = 0; i < nfixed; ++i) MNK_REQUIRE(!seen[(size_t)fixed_idx[i]], "mnk_fix_create: a variable is both free and fixed");
    }
    MNK_REQUIRE(indices_ok(ind_jac_free, njac, nnzj_full, false), "mnk_fix_create: ind_jac_free out of range");
    MNK_REQUIRE(indices_ok(ind_hess_free, nhess, nnzh_full, false), "mnk_fix_create: ind_hess_free out of range");
    MNK_HIP(hipSetDevice(ctx->device));
    auto* h = new mnk_fix();
    h->ctx = ctx;
    h->n = n, h->nfree = nfree, h->nfixed = nfixed;
    h->nnzj_full = nnzj_full, h->njac = njac, h->nnzh_full = nnzh_full, h->nhess = nhess;
    std::vector<double> xf((size_t)n, 0.0);
    for (int64_t i = 0; i < nfixed; ++i) xf[(size_t)fixed_idx[i]] = fixed_val[i];
    const hipStream_t s = ctx->stream;
    if (h->free_idx.upload(std::vector<int64_t>(free_idx, free_idx + nfree), s) ||
        h->fixed_idx.upload(std::vector<int64_t>(fixed_idx, fixed_idx + nfixed), s) ||
        h->value.upload(std::vector<double>(fixed_val, fixed_val + nfixed), s) ||
        h->ind_jac.upload(std::vector<int64_t>(ind_jac_free, ind_jac_free + njac), s) ||
        h->ind_hess.upload(std::vector<int64_t>(ind_hess_free, ind_hess_free + nhess), s) || h->x_full.upload(xf, s)) {
        delete h;
        return -2;
    }
    mnk_ctx_child_added(ctx);
    *out = h;
    return 0;
}

int mnk_fix_destroy(void* fix) {
    mnk_fix* h = static_cast<mnk_fix*>(fix);
    if (!h) return 0;
    mnk_ctx* ctx = h->ctx;
    (void)hipSetDevice(ctx->device);
    (void)mnk::stream_wait(ctx->stream);
    delete h;
    mnk_ctx_child_gone(ctx);
    return 0;
}

void* mnk_fix_x_full(void* fix) {
    mnk_fix* h = static_cast<mnk_fix*>(fix);
    return h ? (void*)h->x_full.p : nullptr;
}

int mnk_fix_get_x_full(void* fix, double* out) {
    mnk_fix* h = static_cast<mnk_fix*>(fix);
    MNK_REQUIRE(h && out, "mnk_fix_get_x_full: NULL argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    MNK_HIP(d2h_copy(out, h->x_full.p, (size_t)h->n * sizeof(double), h->ctx->stream));
    return 0;
}

int mnk_fix_expand(void* fix, const double* x) {
    mnk_fix* h = static_cast<mnk_fix*>(fix);
    MNK_REQUIRE(h && x, "mnk_fix_expand: NULL argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(fix_expand_kernel, fix_grid(h->nfree), dim3(FIX_THREADS), 0, h->ctx->stream, h->x_full.p, h->free_idx.p, x,
                       h->nfree);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_fix_gather(void* fix, int which, const double* src_full, const double* scale, double factor, double* dst) {
    mnk_fix* h = static_cast<mnk_fix*>(fix);
    MNK_REQUIRE(h != nullptr, "mnk_fix_gather: NULL handle");
    MNK_REQUIRE(which == MNK_FIX_FREE || which == MNK_FIX_JAC || which == MNK_FIX_HESS,
                "mnk_fix_gather: which must be MNK_FIX_FREE, MNK_FIX_JAC or MNK_FIX_HESS");
    const int64_t count = which == MNK_FIX_FREE ? h->nfree : which == MNK_FIX_JAC ? h->njac : h->nhess;
    const int64_t* idx = which == MNK_FIX_FREE ? h->free_idx.p : which == MNK_FIX_JAC ? h->ind_jac.p : h->ind_hess.p;
    if (count == 0) return 0;
    MNK_REQUIRE(src_full && dst, "mnk_fix_gather: NULL vector");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(fix_gather_kernel, fix_grid(count), dim3(FIX_THREADS), 0, h->ctx->stream, dst, src_full, idx, scale, factor,
                       count);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_fix_dense_grad(void* fix, double* g, const double* x) {
    mnk_fix* h = static_cast<mnk_fix*>(fix);
    MNK_REQUIRE(h && g && x, "mnk_fix_dense_grad: NULL argument");
    MNK_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(fix_dense_grad_kernel, fix_grid(h->nfixed), dim3(FIX_THREADS), 0, h->ctx->stream, g, x, h->fixed_idx.p,
                       h->value.p, h->nfixed);
    MNK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

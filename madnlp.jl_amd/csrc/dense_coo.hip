// COO callbacks into the dense KKT handle (mnk_dc_coo_*, mnk_dc_compress_*): the reference's SparseCallback on a dense KKT
// system, src/Callbacks/nlpmodels.jl:829-842 (_eval_jac_wrapper!) and :863-881 (_eval_lag_hess_wrapper!): the dense matrix is
// zeroed and the values of jac_coord! / hess_coord! are added entry by entry, in COO order.  Here the order is kept without
// atomics: mnk_dc_coo_attach sorts, once and on the host, the DISTINCT destinations column-major and lists per destination
// the COO positions that feed it, ascending; one thread per destination then adds its list in that order, which is the order
// the sequential loop reaches that destination in.  A Hessian destination is the unordered pair {i, j}: the thread stores its
// sum to (i, j) and (j, i), as the reference writes both.  J'y for the quasi-Newton secant pair and for jtprod! is the same
// idea by Jacobian column, on the COO values the handle keeps (current) or has been told to keep (mnk_dc_keep_jacobian).
//
// These launches are a few thousand threads: they sit at the floor of a small launch whatever the block size; 256 threads per
// block as everywhere in this library.  Consecutive threads store to ascending addresses of one column (the mirrored store of
// a Hessian pair is strided by n, by nature), the gathers v[idx[k]] are element-granular and stay in L2.
#pragma clang fp contract(off)

#include "ls.h"

#include <algorithm>
#include <numeric>

namespace mnk {

// out[dst[d]] = sum of v[idx[k]], k in ptr[d] .. ptr[d+1]-1, in that order, from 0.0; keep[idx[k]] = v[idx[k]] (every COO
// position feeds exactly one destination, so the copy the handle keeps costs no launch of its own; keep == v: nothing to copy)
__global__ __launch_bounds__(256) void coo_scatter_jac_kernel(double* __restrict__ jac, int64_t m, const int32_t* __restrict__ row,
                                                              const int32_t* __restrict__ col, const int32_t* __restrict__ ptr,
                                                              const int32_t* __restrict__ idx, const double* v, double* keep,
                                                              int32_t nd) {
    const int32_t d = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (d >= nd) return;
    double acc = 0.0;
    for (int32_t k = ptr[d]; k < ptr[d + 1]; ++k) {
        const int32_t p = idx[k];
        const double t = v[p];
        if (keep != v) keep[p] = t;
        acc += t;
    }
    jac[row[d] + (int64_t)col[d] * m] = acc;
}

// the same for the pair {i, j}, i >= j: hess[i + j n] and hess[j + i n]
__global__ __launch_bounds__(256) void coo_scatter_hess_kernel(double* __restrict__ hess, int64_t n, const int32_t* __restrict__ row,
                                                               const int32_t* __restrict__ col, const int32_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ idx, const double* __restrict__ v,
                                                               int32_t nd) {
    const int32_t d = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (d >= nd) return;
    double acc = 0.0;
    for (int32_t k = ptr[d]; k < ptr[d + 1]; ++k) acc += v[idx[k]];
    const int64_t i = row[d], j = col[d];
    hess[i + j * n] = acc;
    if (i != j) hess[j + i * n] = acc;
}

// out[j] = sum over the entries of column j, in COO order, of v[k] * y[I[k]], from 0.0
__global__ __launch_bounds__(256) void coo_jtprod_kernel(double* __restrict__ out, int64_t n, const int32_t* __restrict__ cptr,
                                                         const int32_t* __restrict__ cidx, const int32_t* __restrict__ I,
                                                         const double* __restrict__ v, const double* __restrict__ y) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double acc = 0.0;
    for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k) {
        const int32_t p = cidx[k];
        acc += v[p] * y[I[p]];
    }
    out[j] = acc;
}

struct CooMap {   // distinct destinations, column-major, and the CSR of the COO positions feeding each
    int32_t nd = 0;
    DevBuf<int32_t> row, col, ptr, idx;
};

struct DcCoo {
    int64_t nnzj = 0, nnzh = 0;
    CooMap jac, hess;
    DevBuf<int32_t> cptr, cidx, I;      // the Jacobian by column (J'y)
    DevBuf<double> jv, jv_kept, stage;  // current / kept COO values of the Jacobian; staging of host-resident values
    bool kept = false;
};

// (r[k], c[k]) -> CooMap; a stable sort by (c, r) leaves the positions of one destination ascending
static int build_map(CooMap& mp, const std::vector<int32_t>& r, const std::vector<int32_t>& c, hipStream_t s) {
    const size_t nnz = r.size();
    std::vector<int32_t> order(nnz);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return c[a] != c[b] ? c[a] < c[b] : r[a] < r[b]; });
    std::vector<int32_t> row, col, ptr;
    for (size_t k = 0; k < nnz; ++k) {
        const int32_t p = order[k];
        if (k == 0 || r[p] != row.back() || c[p] != col.back()) {
            row.push_back(r[p]);
            col.push_back(c[p]);
            ptr.push_back((int32_t)k);
        }
    }
    ptr.push_back((int32_t)nnz);
    mp.nd = (int32_t)row.size();
    return mp.row.upload(row, s) | mp.col.upload(col, s) | mp.ptr.upload(ptr, s) | mp.idx.upload(order, s);
}

}  // namespace mnk

using namespace mnk;

static DcCoo* coo_of(mnk_dc* dc) { return static_cast<DcCoo*>(dc->coo); }

void mnk_dc_coo_release(mnk_dc* dc) {
    delete coo_of(dc);
    dc->coo = nullptr;
}

#define COO_REQUIRE(cond, ...) do { if (!(cond)) { mnk::set_error(__VA_ARGS__); return -1; } } while (0)
#define COO_GRID(cnt) dim3((unsigned)(((cnt) + 255) / 256)), dim3(256), 0, s

extern "C" {

int mnk_dc_coo_attach(mnk_dc* dc, int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t nnzh, const int32_t* hess_I,
                      const int32_t* hess_J, int base) {
    COO_REQUIRE(dc && dc->ctx, "mnk_dc_coo_attach: NULL handle");
    COO_REQUIRE(dc->coo == nullptr, "mnk_dc_coo_attach: a COO structure is attached to this handle already");
    COO_REQUIRE(nnzj >= 0 && nnzh >= 0 && nnzj < INT32_MAX && nnzh < INT32_MAX,
                "mnk_dc_coo_attach: nnzj = %lld, nnzh = %lld: a count is negative or does not fit int32", (long long)nnzj,
                (long long)nnzh);
    COO_REQUIRE(dc->n < INT32_MAX && dc->m < INT32_MAX, "mnk_dc_coo_attach: n or m does not fit int32");
    COO_REQUIRE((nnzj == 0 || (jac_I && jac_J)) && (nnzh == 0 || (hess_I && hess_J)), "mnk_dc_coo_attach: NULL index array");
    std::vector<int32_t> jr(nnzj), jc(nnzj), hr(nnzh), hc(nnzh);
    for (int64_t k = 0; k < nnzj; ++k) {
        const int64_t i = (int64_t)jac_I[k] - base, j = (int64_t)jac_J[k] - base;
        COO_REQUIRE(i >= 0 && i < dc->m && j >= 0 && j < dc->n,
                    "mnk_dc_coo_attach: Jacobian entry %lld = (%d, %d) is out of range (m = %lld, n = %lld, base %d)", (long long)k,
                    jac_I[k], jac_J[k], (long long)dc->m, (long long)dc->n, base);
        jr[k] = (int32_t)i;
        jc[k] = (int32_t)j;
    }
    for (int64_t k = 0; k < nnzh; ++k) {
        const int64_t i = (int64_t)hess_I[k] - base, j = (int64_t)hess_J[k] - base;
        COO_REQUIRE(i >= 0 && i < dc->n && j >= 0 && j < dc->n,
                    "mnk_dc_coo_attach: Hessian entry %lld = (%d, %d) is out of range (n = %lld, base %d)", (long long)k, hess_I[k],
                    hess_J[k], (long long)dc->n, base);
        hr[k] = (int32_t)std::max(i, j);   // the unordered pair, as a lower-triangular destination
        hc[k] = (int32_t)std::min(i, j);
    }
    MNK_HIP(hipSetDevice(dc->ctx->device));
    hipStream_t s = dc->ctx->stream;
    DcCoo* co = new DcCoo();
    co->nnzj = nnzj;
    co->nnzh = nnzh;
    // the Jacobian by column: a stable sort by column leaves the entries of one column in COO order
    std::vector<int32_t> cidx(nnzj), cptr(dc->n + 1, 0);
    std::iota(cidx.begin(), cidx.end(), 0);
    std::stable_sort(cidx.begin(), cidx.end(), [&](int32_t a, int32_t b) { return jc[a] < jc[b]; });
    for (int64_t k = 0; k < nnzj; ++k) ++cptr[jc[k] + 1];
    for (int64_t j = 0; j < dc->n; ++j) cptr[j + 1] += cptr[j];
    int rc = build_map(co->jac, jr, jc, s) | build_map(co->hess, hr, hc, s);
    rc |= co->cptr.upload(cptr, s) | co->cidx.upload(cidx, s) | co->I.upload(jr, s);
    rc |= co->jv.alloc(nnzj) | co->jv_kept.alloc(nnzj) | co->stage.alloc(std::max(nnzj, nnzh));
    if (rc) { delete co; return -2; }
    MNK_HIP(hipMemsetAsync(co->jv.p, 0, co->jv.n * sizeof(double), s));
    dc->coo = co;
    return 0;
}

// `src` on the device: the caller's device values, or host values staged (the copy waits: the caller's array is only valid for
// the duration of the call)
static int coo_values(mnk_dc* dc, DcCoo* co, const double* v, int64_t nnz, int loc, const double** src) {
    *src = v;
    if (loc != MNK_DEVICE && nnz > 0) {
        MNK_HIP(mnk::h2d_copy(co->stage.p, v, nnz * sizeof(double), dc->ctx->stream));
        *src = co->stage.p;
    }
    return 0;
}

int mnk_dc_compress_jacobian(mnk_dc* dc, const double* jac_coo, int loc) {
    COO_REQUIRE(dc && dc->ctx, "mnk_dc_compress_jacobian: NULL handle");
    DcCoo* co = coo_of(dc);
    COO_REQUIRE(co != nullptr, "mnk_dc_compress_jacobian: call mnk_dc_coo_attach first");
    COO_REQUIRE(jac_coo || co->nnzj == 0, "mnk_dc_compress_jacobian: the value pointer is NULL and nnzj = %lld", (long long)co->nnzj);
    MNK_HIP(hipSetDevice(dc->ctx->device));
    hipStream_t s = dc->ctx->stream;
    if (dc->jac_dirty) {   // something else than this scatter has written the buffer: entries outside the structure may be nonzero
        MNK_HIP(hipMemsetAsync(dc->jac.p, 0, dc->jac.n * sizeof(double), s));
        dc->jac_dirty = false;
    }
    if (co->jac.nd == 0) return 0;
    const double* src;
    int rc = coo_values(dc, co, jac_coo, co->nnzj, loc, &src);
    if (rc) return rc;
    hipLaunchKernelGGL(coo_scatter_jac_kernel, COO_GRID(co->jac.nd), dc->jac.p, dc->m, co->jac.row.p, co->jac.col.p, co->jac.ptr.p,
                       co->jac.idx.p, src, co->jv.p, co->jac.nd);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_dc_compress_hessian(mnk_dc* dc, const double* hess_coo, int loc) {
    COO_REQUIRE(dc && dc->ctx, "mnk_dc_compress_hessian: NULL handle");
    DcCoo* co = coo_of(dc);
    COO_REQUIRE(co != nullptr, "mnk_dc_compress_hessian: call mnk_dc_coo_attach first");
    COO_REQUIRE(hess_coo || co->nnzh == 0, "mnk_dc_compress_hessian: the value pointer is NULL and nnzh = %lld", (long long)co->nnzh);
    MNK_HIP(hipSetDevice(dc->ctx->device));
    hipStream_t s = dc->ctx->stream;
    if (dc->hess_dirty) {
        MNK_HIP(hipMemsetAsync(dc->hess.p, 0, dc->hess.n * sizeof(double), s));
        dc->hess_dirty = false;
    }
    if (co->hess.nd == 0) return 0;
    const double* src;
    int rc = coo_values(dc, co, hess_coo, co->nnzh, loc, &src);
    if (rc) return rc;
    hipLaunchKernelGGL(coo_scatter_hess_kernel, COO_GRID(co->hess.nd), dc->hess.p, dc->n, co->hess.row.p, co->hess.col.p,
                       co->hess.ptr.p, co->hess.idx.p, src, co->hess.nd);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_dc_keep_jacobian(mnk_dc* dc) {
    COO_REQUIRE(dc && dc->ctx, "mnk_dc_keep_jacobian: NULL handle");
    DcCoo* co = coo_of(dc);
    COO_REQUIRE(co != nullptr, "mnk_dc_keep_jacobian: call mnk_dc_coo_attach first");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    if (co->nnzj > 0)
        MNK_HIP(hipMemcpyAsync(co->jv_kept.p, co->jv.p, co->nnzj * sizeof(double), hipMemcpyDeviceToDevice, dc->ctx->stream));
    co->kept = true;
    return 0;
}

int mnk_dc_coo_jtprod(mnk_dc* dc, int which, const double* y, double* out) {
    COO_REQUIRE(dc && dc->ctx && out, "mnk_dc_coo_jtprod: NULL argument");
    DcCoo* co = coo_of(dc);
    COO_REQUIRE(co != nullptr, "mnk_dc_coo_jtprod: call mnk_dc_coo_attach first");
    COO_REQUIRE(which == MNK_DC_JAC_CURRENT || which == MNK_DC_JAC_KEPT, "mnk_dc_coo_jtprod: which must be MNK_DC_JAC_CURRENT or MNK_DC_JAC_KEPT");
    COO_REQUIRE(which == MNK_DC_JAC_CURRENT || co->kept, "mnk_dc_coo_jtprod: MNK_DC_JAC_KEPT before mnk_dc_keep_jacobian");
    COO_REQUIRE(y || co->nnzj == 0, "mnk_dc_coo_jtprod: y is NULL");
    MNK_HIP(hipSetDevice(dc->ctx->device));
    hipStream_t s = dc->ctx->stream;
    hipLaunchKernelGGL(coo_jtprod_kernel, COO_GRID(dc->n), out, dc->n, co->cptr.p, co->cidx.p, co->I.p,
                       which == MNK_DC_JAC_KEPT ? co->jv_kept.p : co->jv.p, y);
    MNK_HIP(hipGetLastError());
    return 0;
}

int mnk_dc_get_jac(mnk_dc* dc, double* out, int64_t ld, int loc) {
    COO_REQUIRE(dc && dc->ctx && (out || dc->m == 0), "mnk_dc_get_jac: NULL argument");
    COO_REQUIRE(ld >= dc->m, "mnk_dc_get_jac: leading dimension smaller than m");
    if (dc->m == 0) return 0;
    MNK_HIP(hipSetDevice(dc->ctx->device));
    const size_t w = dc->m * sizeof(double);
    if (loc == MNK_DEVICE)
        MNK_HIP(hipMemcpy2DAsync(out, ld * sizeof(double), dc->jac.p, w, w, dc->n, hipMemcpyDeviceToDevice, dc->ctx->stream));
    else
        MNK_HIP(mnk::d2h_copy_2d(out, ld * sizeof(double), dc->jac.p, w, w, dc->n, dc->ctx->stream));
    return 0;
}

}  // extern "C"

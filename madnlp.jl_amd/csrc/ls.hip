// C-ABI of the linear solver handle (mnk_ls_*): allocation, `transfer_matrix!`
// (reference src/LinearSolvers/lapack_common.jl:28 and its device twin
// lib/MadNLPGPU/src/utils.jl:12-23 / kernels_sparse.jl:27-33), factorize / inertia /
// solve entry points.  See include/madnlp_hip.h for the per-function citations.
#include <cstdarg>
#include <cstdlib>
#include <mutex>

#include <cfloat>
#include "ls.h"

namespace mnk {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// Zero the (padded) factor buffer and put a unit diagonal on the padding rows.
// Only column blocks on/below the diagonal tile row are touched: nothing in the
// factorization or the solves ever reads above the 128-row tile containing the diagonal.
__global__ __launch_bounds__(256) void fill_lower_kernel(double* __restrict__ F, int64_t ld, int64_t N, int64_t Np) {
    const int64_t col = blockIdx.x;
    const int64_t first = (col / PAD) * PAD;  // first row of the diagonal tile of this column
    const int64_t r = first + ((int64_t)blockIdx.y * 256 + threadIdx.x) * 2;
    if (r >= Np) return;
    double2 v = make_double2(0.0, 0.0);
    if (col >= N) {
        if (r == col) v.x = 1.0;
        if (r + 1 == col) v.y = 1.0;
    }
    *reinterpret_cast<double2*>(F + r + col * ld) = v;
}

// aug_com (lower CSC) -> dense: one thread per stored entry (coordinates precomputed).
// max |v| over the wave -> one atomicMax on the bit pattern (non-negative doubles order like unsigned integers; NaN -> +Inf)
__device__ __forceinline__ void wave_absmax_to(unsigned long long* word, double v) {
    double a = fabs(v);
    if (!(a <= DBL_MAX)) a = __longlong_as_double(0x7ff0000000000000LL);
    for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off));
    // (a relaxed look first: once the word holds a large value almost every wave skips the atomic -- 80 000 atomics on
    // one address took 390 us of a 2112-row transfer)
    if ((threadIdx.x & 63) == 0 && a > 0.0) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
        if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
    }
}

// (`amax`: optional, max|a_ij| of what is transferred -- the growth guard of BUNCHKAUFMAN's static-pivot tier)
// (`lim`: only the leading principal block of that order is transferred -- a solver of order lim on a larger KKT handle, the
// leading-block probe of mnk_ls_factorize_sc_async)
__global__ void scatter_csc_kernel(double* __restrict__ F, int64_t ld, const int32_t* __restrict__ row,
                                   const int32_t* __restrict__ col, const double* __restrict__ nz, int64_t nnz,
                                   unsigned long long* __restrict__ amax, int32_t lim = INT32_MAX, int* __restrict__ nonfinite = nullptr) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double v = 0.0;
    if (k < nnz && row[k] < lim && col[k] < lim) {
        v = nz[k];
        F[row[k] + (int64_t)col[k] * ld] = v;
        if (nonfinite != nullptr && !(fabs(v) <= DBL_MAX)) *nonfinite = 1;   // (mnk_ls::env_word: the envelope is off for this matrix)
    }
    if (amax != nullptr) wave_absmax_to(amax + AMAX_SLOT0 + AMAX_STRIDE * (blockIdx.x & (AMAX_SLOTS - 1)), v);
}

// dense source -> factor buffer, rows >= first row of the diagonal tile of each column.
__global__ __launch_bounds__(256) void copy_lower_kernel(double* __restrict__ F, int64_t ld,
                                                         const double* __restrict__ A, int64_t lda, int64_t N,
                                                         int64_t Np, unsigned long long* __restrict__ amax) {
    const int64_t col = blockIdx.x;
    const int64_t first = (col / PAD) * PAD;
    // four rows per thread, 256 apart (coalesced, four loads in flight; a quarter of the workgroups and of the wave
    // reductions of one row per thread: 50-70 -> ~25 us for the 2112 x 2112 matrix of config C2)
    const int64_t r0 = first + (int64_t)blockIdx.y * 1024 + threadIdx.x;
    if (r0 - threadIdx.x >= Np) return;   // (uniform)
    double v[4], vl = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + 256 * i;
        v[i] = 0.0;
        if (r < Np) {
            if (col < N && r < N) {
                v[i] = A[r + col * lda];
                if (r >= col) vl = fmax(vl, fabs(v[i]));  // the lower triangle is the matrix ('L' storage: the rest may hold anything)
                if (r >= col && !(fabs(v[i]) <= DBL_MAX)) vl = __longlong_as_double(0x7ff0000000000000LL);
            } else if (r == col) {
                v[i] = 1.0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + 256 * i;
        if (r < Np) F[r + col * ld] = v[i];
    }
    if (amax != nullptr) {
        // one fold per workgroup, spread over AMAX_SLOTS words (publish_info_kernel takes their maximum): 25 000 waves
        // looking at ONE word cost 40 us of the 2112-row transfer
        __shared__ double wmax[4];
        for (int off = 32; off > 0; off >>= 1) vl = fmax(vl, __shfl_xor(vl, off));
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = vl;
        __syncthreads();
        if (threadIdx.x < 64)
            wave_absmax_to(amax + AMAX_SLOT0 + AMAX_STRIDE * ((blockIdx.x + 5 * blockIdx.y) & (AMAX_SLOTS - 1)),
                           fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])));
    }
}

}  // namespace mnk

using namespace mnk;

extern "C" {

int mnk_version(void) { return MNK_VERSION; }
const char* mnk_last_error_string(void) { return g_err.c_str(); }

int mnk_ls_create(mnk_ctx* ctx, int64_t N, int algo, mnk_ls** out) {
    MNK_REQUIRE(ctx && out, "mnk_ls_create: NULL argument");
    mnk::LaunchLock lock;   // (pinned host allocations, buffers)
    MNK_REQUIRE(N > 0, "mnk_ls_create: N must be positive");
    const bool bk_requested = algo == MNK_BUNCHKAUFMAN;
    if (bk_requested) algo = MNK_LDL;  // tier 1: static-pivot blocked LDL^T; tier 2 on breakdown: bk.hip
    MNK_REQUIRE(algo == MNK_CHOLESKY || algo == MNK_LDL || algo == MNK_QR || algo == MNK_LU || algo == MNK_EVD,
                "mnk_ls_create: unknown algorithm (BUNCHKAUFMAN, LU, QR, CHOLESKY, LDL and EVD are implemented on device)");
    MNK_HIP(hipSetDevice(ctx->device));
    mnk_ls* ls = new mnk_ls();
    ls->ctx = ctx;
    ls->N = N;
    ls->algo = algo;
    ls->bk.requested = bk_requested;
    // Tuning overrides from the environment, for runs of unmodified callers: MNK_OPTIONS="key=value,key=value" with the keys
    // of mnk_ls_set_option (plus MNK_PANEL_ALGO / MNK_PERSISTENT_SOLVE, the two a deployment may need: INTEGRATION.md).  An
    // option set this way is not changed by later mnk_ls_set_option calls.
    {
        auto from_env = [&](const std::string& key, double v) {
            if (mnk_ls_set_option(ls, key.c_str(), v) == 0) ls->env_keys.push_back(key);
            else fprintf(stderr, "madnlp_hip: ignoring environment override '%s': %s\n", key.c_str(), mnk_last_error_string());
        };
        if (const char* e = getenv("MNK_PANEL_ALGO")) from_env("panel_algo", atof(e));
        if (const char* e = getenv("MNK_PERSISTENT_SOLVE")) from_env("persistent_solve", atof(e));
        if (const char* e = getenv("MNK_OPTIONS")) {
            std::string all(e);
            size_t pos = 0;
            while (pos < all.size()) {
                size_t end = all.find(',', pos);
                if (end == std::string::npos) end = all.size();
                const std::string item = all.substr(pos, end - pos);
                const size_t eq = item.find('=');
                if (eq != std::string::npos && eq > 0) from_env(item.substr(0, eq), atof(item.c_str() + eq + 1));
                pos = end + 1;
            }
        }
    }
    ls->Np = round_up(N, PAD);
    ls->ld = ls->Np;
    ls->ldw = ls->Np;
    int rc = 0;
    rc |= ls->fact.alloc((size_t)ls->ld * ls->Np + SLACK);
    rc |= ls->linv.alloc((size_t)(ls->Np / NBI) * NBI * NBI);
    rc |= ls->dblk.alloc((size_t)(ls->Np / NBI) * NBI * NBI);
    rc |= ls->inv16.alloc((size_t)(ls->Np / NBI) * 1024);
    rc |= ls->linv256.alloc((size_t)((ls->Np + 255) / 256) * 65536);
    rc |= ls->linv256t.alloc((size_t)((ls->Np + 255) / 256) * 65536);
    rc |= ls->dvec.alloc(ls->Np);
    rc |= ls->dinv.alloc(ls->Np);
    rc |= ls->xwork.alloc(10 * ls->Np);
    rc |= ls->solves.create();
    if (hipHostMalloc((void**)&ls->pin, 8 * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&ls->pin_dev, ls->pin, 0) != hipSuccess) {
        (void)hipGetLastError();
        rc |= -2;
    }
    rc |= ls->info_dev.alloc(4);   // info | which bounded device-side wait expired (info = -7) / last valid pivot (info = -9) | early-rejection switch | -
    rc |= ls->inertia_dev.alloc(3);
    ls->alt = mnk_ls_alt_new(algo);
    if (ls->alt) {
        rc |= ls->alt->alloc(ls);
        ls->spare.prefill = 0;   // (they write the whole factor buffer, the upper triangle included: no background zero-fill)
    }
    if (rc) { delete ls; return -2; }
    MNK_HIP(hipMemsetAsync(ls->fact.p, 0, ((size_t)ls->ld * ls->Np + SLACK) * sizeof(double), ctx->stream));
    mnk_ctx_child_added(ctx);
    *out = ls;
    return 0;
}

int mnk_ls_destroy(mnk_ls* ls) {
    if (!ls) return 0;
    (void)hipSetDevice(ls->ctx->device);
    if (mnk_ls_pending_elsewhere(ls)) {
        // the other thread's batch still holds this pointer and will launch on it at its end: deleting now would leave it dangling
        set_error("mnk_ls_destroy: a factorize! call of this solver is pending in a batch that another thread opened "
                  "(that thread's mnk_factorize_batch_end must come first); the solver was NOT destroyed");
        return -1;
    }
    (void)mnk_ls_sync_deferred(ls);
    (void)mnk::stream_wait(ls->ctx->stream);
    ls->probe.destroy();
    mnk::LaunchLock lock;   // (host-memory frees and event destruction below; the device buffers lock for themselves)
    mnk::quiesce_persistent();
    ls->solves.destroy();
    if (ls->pin) (void)hipHostFree(ls->pin);
    ls->spare.destroy(ls->ctx);
    if (ls->ev_defer) (void)hipEventDestroy(ls->ev_defer);
    ls->verdict.destroy();
    mnk_ctx* ctx = ls->ctx;
    delete ls;
    mnk_ctx_child_gone(ctx);
    return 0;
}

int mnk_ls_set_option(mnk_ls* ls, const char* key, double value) {
    MNK_REQUIRE(ls && key, "mnk_ls_set_option: NULL argument");
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    for (const std::string& k : ls->env_keys)
        if (k == key) {   // fixed by the environment for this process (MNK_OPTIONS): the call is ignored, once per key out loud
            static std::mutex warn_mutex;
            static std::vector<std::string> warned;
            std::lock_guard<std::mutex> lock(warn_mutex);
            if (std::find(warned.begin(), warned.end(), k) == warned.end()) {
                warned.push_back(k);
                fprintf(stderr, "madnlp_hip: set_option('%s', %g) ignored: the option is pinned by MNK_OPTIONS / MNK_PANEL_ALGO / "
                                "MNK_PERSISTENT_SOLVE for this process (query: get_stat(\"pinned:%s\"))\n", key, value, key);
            }
            return 0;
        }
    if (!strcmp(key, "pivot_tol")) { ls->pivot_tol = value; return 0; }
    if (!strcmp(key, "envelope_half")) { ls->envelope_half = value != 0.0; return 0; }   // 0: the waves of a bulk chunk multiply the k-tiles left of their own 64-row halves' envelopes and the upper quadrant of a diagonal tile too (ignored with envelope = 0)
    if (!strcmp(key, "envelope")) { ls->envelope = value != 0.0; return 0; }   // 0: the task-DAG bulk kernel multiplies the structurally zero tiles of sparse sources too
    if (!strcmp(key, "dag_js2")) { ls->dag_js2_override = (int)value; ls->plan.invalidate(); return 0; }   // experiments: strip-column at which every row joins the band (-1: by size; raised where the deep band would get more strips than CUs: dag_plan.h); the task list is rebuilt
    if (!strcmp(key, "outer_block")) {
        int64_t v = (int64_t)value;
        MNK_REQUIRE(v == 0 || (v >= NBI && v % NBI == 0), "outer_block must be 0 (by size) or a positive multiple of 64");
        ls->nbo_auto = v == 0;
        if (v > 0) ls->nbo = v;
        ls->wbuf[0].release();
        ls->wbuf[1].release();
        return 0;
    }
    if (!strcmp(key, "solve512")) { ls->solves.solve512 = value != 0; return 0; }   // 512-column steps of the one-launch solve
    if (!strcmp(key, "linv_mfma")) { ls->solves.linv_mfma = value != 0.0; return 0; }
    if (!strcmp(key, "multi_rhs_min")) {   // solves of this many right-hand sides or more run blocked on the matrix cores (static-pivot tier); 0: never
        MNK_REQUIRE(value >= 0.0, "multi_rhs_min must be 0 (never) or a positive count of right-hand sides");
        ls->solves.multi_rhs_min = (int64_t)value;
        return 0;
    }
    if (!strcmp(key, "prefill")) { ls->spare.prefill = value != 0; return 0; }   // background zero-fill into a second factor buffer
    if (!strcmp(key, "single_rows")) {  // systems up to this order: one outer panel, no look-ahead (0: never)
        ls->single_rows = (int64_t)value;
        ls->wbuf[0].release();
        ls->wbuf[1].release();
        return 0;
    }
    if (!strcmp(key, "lookahead")) { ls->lookahead = value != 0.0; return 0; }
    // 0: no work sharing, 1: the panel stream joins the trailing update when that is the longer leg,
    // 2: always (used by the schedule tests)
    if (!strcmp(key, "share")) { ls->share = (int)value; return 0; }
    if (!strcmp(key, "small_tiles")) { ls->small_tiles = (int)value; return 0; }
    // 5: task-DAG schedule (persistent left-looking bulk kernel beside the pivot chain, dag.hip); 4: persistent panel
    // kernel per 256 columns + one trailing update per outer panel; 1: one launch per piece (the fallback of 4 and 5)
    if (!strcmp(key, "panel_algo")) {
        MNK_REQUIRE((int)value == 1 || (int)value == 4 || (int)value == 5, "panel_algo must be 1, 4 or 5");
        ls->panel_algo = (int)value;
        return 0;
    }
    if (!strcmp(key, "pp_fuse_rows")) { ls->pp_fuse_rows = (int64_t)value; return 0; }
    if (!strcmp(key, "dag_min_rows")) { ls->dag_min_rows = (int64_t)value; return 0; }
    if (!strcmp(key, "dag_taper0")) {
        MNK_REQUIRE(value >= 1.0 && value <= 16.0, "dag_taper0 must be in 1..16");
        ls->dag_taper0 = (int)value;
        ls->plan.invalidate();
        return 0;
    }
    if (!strcmp(key, "dag_chunk")) {   // tile columns per bulk task of the task-DAG schedule (the task list is rebuilt)
        MNK_REQUIRE(value >= 1.0 && value <= 64.0, "dag_chunk must be in 1..64");
        ls->dag_chunk = (int)value;
        ls->plan.invalidate();
        return 0;
    }
    if (!strcmp(key, "dag_band")) {    // 64-row strips of the pivot chain's band
        MNK_REQUIRE(value >= 8.0 && value <= 64.0 && (int)value % 4 == 0 && (double)(int)value == value, "dag_band must be a multiple of 4 in 8..64");
        ls->dag_band = (int)value;
        ls->plan.invalidate();
        return 0;
    }
    if (!strcmp(key, "dag_spin_limit")) {  // polls a wait of the task-DAG schedule's kernels may take before it gives up
        MNK_REQUIRE(value >= 1024.0, "dag_spin_limit must be at least 1024");
        ls->dag_spin_limit = (long)value;
        return 0;
    }
    if (!strcmp(key, "dag_fill")) { ls->dag_fill = value != 0.0; ls->plan.invalidate(); return 0; }   // zero-fill of the spare buffer as tasks of the bulk queue
    // per-XCD queues of the bulk kernel (dag_plan.hip: dag_deal_list); the task list is dealt again
    if (!strcmp(key, "dag_xcd_queues")) { ls->dag_xcd_queues = value != 0.0; ls->plan.invalidate(); return 0; }   // 0: one queue, popped by every workgroup
    if (!strcmp(key, "dag_gang")) {   // tasks of one group that go to one queue together; negative: every task to queue 0 (tests of the steal path)
        MNK_REQUIRE(value <= 64.0 && value != 0.0 && (double)(int)value == value, "dag_gang must be an integer in 1..64 (or negative)");
        ls->dag_gang = (int)value;
        ls->plan.invalidate();
        return 0;
    }
    if (!strcmp(key, "dag_trace")) { ls->dag_trace_on = value != 0.0; return 0; }  // diagnostics: tools/dag_timeline.py
    if (!strcmp(key, "dag_max_rows")) { ls->dag_max_rows = (int64_t)value; return 0; }
    if (!strcmp(key, "dag_deep_rows")) { ls->dag_deep_rows = (int64_t)value; ls->plan.invalidate(); return 0; }   // largest order with every row in the chain's band
    // BUNCHKAUFMAN only: 1 (default) = refactor with the pivoted Bunch-Kaufman tier when the static-pivot
    // factorization breaks down; 0 = report the breakdown as num_zero and let the IPM regularize
    if (!strcmp(key, "bk_fallback")) { ls->bk.bk_fallback = (int)value; return 0; }
    if (!strcmp(key, "bk_panel_wgs")) {   // pivoted tier: 0 = a workgroup per 256 rows of a panel, 1 = one workgroup per panel
        MNK_REQUIRE(value == 0.0 || value == 1.0, "bk_panel_wgs must be 0 or 1");
        ls->bk.bk_panel_wgs = (int)value;
        return 0;
    }
    if (!strcmp(key, "accept_only_pd")) { ls->accept_only_pd = value != 0; return 0; }  // see mnk_ls_fetch_info
    if (!strcmp(key, "probe")) { ls->probe.on = value != 0; return 0; }   // leading-block probe in front of a factorization that is likely to be rejected early (ls.h)
    if (!strcmp(key, "early_reject")) { ls->early_reject = value != 0; return 0; }      // with accept_only_pd: stop at the first non-positive pivot (leaf64.h)
    // BUNCHKAUFMAN only: element growth max|d_k| / max|a_ij| of the static-pivot tier above which the pivoted tier takes over
    if (!strcmp(key, "dag_debug")) {
        ls->dag_debug = value != 0.0;
        if (ls->dag_debug && !ls->dag_dbg.p) {
            // (8 words per chain strip; the 16 words per bulk workgroup behind them were a removed diagnostic build's and stay zero)
            if (ls->dag_dbg.alloc(8 * 128 + 16 * 1024)) return -2;
            MNK_HIP(hipMemset(ls->dag_dbg.p, 0, (8 * 128 + 16 * 1024) * sizeof(int)));
        }
        return 0;
    }
    if (!strcmp(key, "bk_max_wgs")) {
        MNK_REQUIRE(value >= 0.0 && value <= 256.0, "bk_max_wgs must be in 0..256");
        ls->bk.bk_max_wgs = (int)value;
        return 0;
    }
    if (!strcmp(key, "bk_spin_limit")) {
        MNK_REQUIRE(value >= 1024.0, "bk_spin_limit must be at least 1024");
        ls->bk.bk_spin_limit = (long)value;
        return 0;
    }
    if (!strcmp(key, "debug_bk_missing")) { ls->bk.debug_bk_missing = (int)value; return 0; }
    if (!strcmp(key, "bk_growth_tol")) {
        MNK_REQUIRE(value > 1.0, "bk_growth_tol must be > 1");
        ls->bk.bk_growth_tol = value;
        return 0;
    }
    if (!strcmp(key, "bk_growth_tol_qd")) {  // the same for pivot sequences "all positive, then all negative"
        MNK_REQUIRE(value > 1.0, "bk_growth_tol_qd must be > 1");
        ls->bk.bk_growth_tol_qd = value;
        return 0;
    }
    if (!strcmp(key, "persistent_solve")) { ls->solves.persistent_solve = value != 0.0; return 0; }
    if (!strcmp(key, "ps_spin_limit")) {  // polls a persistent-solve wait may take before it gives up
        MNK_REQUIRE(value >= 1024.0, "ps_spin_limit must be at least 1024");
        ls->solves.ps_spin_limit = (long)value;
        return 0;
    }
    // tests only: workgroup `value` of every persistent solve leaves at once, as a peer that never became
    // resident would (< 0: off); the others must give up after ps_spin_limit polls instead of hanging
    if (!strcmp(key, "debug_pp_missing")) { ls->debug_pp_missing = (int)value; return 0; }
    if (!strcmp(key, "debug_ps_missing")) { ls->solves.debug_ps_missing = (int)value; return 0; }
    if (!strcmp(key, "solve_trace")) {  // diagnostics: time stamps of the forward sweep's critical path
        if (value != 0.0) {
            int rc = ls->solves.trace.alloc((size_t)(ls->Np / 64) * 8);
            if (rc) return rc;
            MNK_HIP(hipMemset(ls->solves.trace.p, 0, (size_t)(ls->Np / 64) * 8 * sizeof(unsigned long long)));
        } else {
            ls->solves.trace.release();
        }
        return 0;
    }
    set_error("mnk_ls_set_option: unknown option '%s'", key);
    return -1;
}

static int ensure_wbuf(mnk_ls* ls) {
    if (ls->algo != MNK_LDL || ls->wbuf[0].p) return 0;
    const size_t cnt = (size_t)ls->ldw * std::min<int64_t>(mnk_ls_effective_nbo(ls), ls->Np) + SLACK;
    int rc = ls->wbuf[0].alloc(cnt);
    // double buffered for the look-ahead: panel k+1 is factored while panel k is applied
    if (!rc && mnk_ls_effective_nbo(ls) < ls->Np) rc = ls->wbuf[1].alloc(cnt);
    return rc;
}

// The word that receives max|a_ij| of the matrix being transferred (zeroed here), or NULL when nobody will ask for it.
static unsigned long long* amax_word(mnk_ls* ls) {
    if (!ls->bk.wanted(ls)) return nullptr;
    if (!ls->bk.amax_dev.p && ls->bk.amax_dev.alloc(AMAX_WORDS)) return nullptr;
    (void)hipMemsetAsync(ls->bk.amax_dev.p, 0, AMAX_WORDS * sizeof(unsigned long long), ls->ctx->stream);
    return ls->bk.amax_dev.p;
}

}  // extern "C"
// ---- SpareFill (ls.h): the only code that touches the spare factor buffer, its events and its state ----
int SpareFill::acquire(mnk_ls* ls) {
    mnk_ctx* ctx = ls->ctx;
    hipStream_t s = ctx->stream;
    bool pre = wanted(ls->Np);
    if (pre && !buf.p) {
        // second factor buffer, events, side stream; if any of it cannot be had the fill stays in line
        if (buf.alloc(ls->fact.n) != 0) { (void)hipGetLastError(); prefill = 0; pre = false; }
        if (pre && mnk_ctx_fill_stream(ctx) == nullptr) { prefill = 0; pre = false; }
        if (pre && (hipEventCreateWithFlags(&ev_zeroed, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&ev_free, hipEventDisableTiming) != hipSuccess)) { prefill = 0; pre = false; }
        if (pre) MNK_HIP(hipMemsetAsync(buf.p, 0, buf.n * sizeof(double), s));  // (slack behind the matrix)
    }
    // (the fill was left to the task queue of the previous factorization, and nobody has looked at its `info` yet)
    if (pre && state == State::ZeroedByDag && !ls->verdict.known()) state = State::Dirty;
    if (pre && zeroed()) {
        std::swap(ls->fact.p, buf.p);          // the buffer zeroed in the background becomes the factor buffer
        MNK_HIP(hipStreamWaitEvent(s, ev_zeroed, 0));
    } else {
        hipLaunchKernelGGL(fill_lower_kernel, dim3((unsigned)ls->Np, (unsigned)((ls->Np / 2 + 255) / 256)), dim3(256), 0, s, ls->fact.p, ls->ld, ls->N, ls->Np);
    }
    if (pre) state = State::Pending;           // (after a swap the other buffer holds the previous factor)
    else if (!zeroed()) state = State::Dirty;
    MNK_HIP(hipGetLastError());
    return 0;
}

// The other factor buffer (the previous factor, or fresh memory) is free once everything queued so far has run: from then
// on it is zeroed on the side stream, behind the factorization that was just queued (whose persistent kernels want the
// whole chip from their first microsecond) and concurrently with the inertia fetch and the solves that follow.
int SpareFill::queued(mnk_ls* ls) {
    if (!pending()) return 0;
    const bool by_dag = state == State::PendingDagFills;
    state = State::Dirty;   // (until the fill is queued)
    mnk_ctx* ctx = ls->ctx;
    if (by_dag) {   // the bulk queue of the factorization that was just queued zeroes the buffer (DAG_FILL tasks): stream order does the rest
        MNK_HIP(hipEventRecord(ev_zeroed, ctx->stream));
        state = State::ZeroedByDag;
        return 0;
    }
    MNK_HIP(hipEventRecord(ev_free, ctx->stream));
    MNK_HIP(hipStreamWaitEvent(ctx->s_fill, ev_free, 0));
    hipLaunchKernelGGL(fill_lower_kernel, dim3((unsigned)ls->Np, (unsigned)((ls->Np / 2 + 255) / 256)), dim3(256), 0, ctx->s_fill, buf.p, ls->ld, ls->N, ls->Np);
    MNK_HIP(hipGetLastError());
    MNK_HIP(hipEventRecord(ev_zeroed, ctx->s_fill));
    state = State::ZeroedBySide;
    return 0;
}

bool SpareFill::give_up() {
    if (!buf.p || zeroed()) return false;   // (zeroed: a fill of the buffer has been queued and the next transfer will swap it in)
    buf.release();
    prefill = 0;
    state = State::Dirty;
    return true;
}

void SpareFill::destroy(mnk_ctx* ctx) {
    if (ctx->s_fill) (void)mnk::stream_wait(ctx->s_fill);   // a background fill of this solver's buffer
    if (ev_zeroed) (void)hipEventDestroy(ev_zeroed);
    if (ev_free) (void)hipEventDestroy(ev_free);
}
extern "C" {

// The envelope of a sparse source for the factorization that follows (MatrixSource::env_dev; nullptr: none), and the word its
// transfer marks when it meets a NaN / Inf entry.  `env_host`: the envelope of the source's order, truncated to this solver's
// tiles (a leading principal block of the source has the leading part of its envelope).
static int* set_envelope(mnk_ls* ls, const int32_t* env_dev, const std::vector<int32_t>& env_host, const int32_t* envh_dev,
                         const std::vector<int32_t>& envh_host) {
    ls->src.env_dev = nullptr;
    ls->src.envh_dev = nullptr;
    if (!ls->envelope || env_dev == nullptr || ls->alt) return nullptr;
    if (!ls->env_word.p) {
        if (ls->env_word.alloc(2) || hipMemsetAsync(ls->env_word.p, 0, 2 * sizeof(int), ls->ctx->stream) != hipSuccess) {
            (void)hipGetLastError();   // (no envelope then)
            ls->env_word.release();
            return nullptr;
        }
    }
    // (a transfer whose mark no task-DAG factorization consumed -- another schedule ran, or the pivoted tier transferred the
    // matrix again -- must not close the envelope of this one)
    if (ls->src.env_armed && hipMemsetAsync(ls->env_word.p, 0, sizeof(int), ls->ctx->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ls->src.env_armed = true;
    ls->src.env_dev = env_dev;
    ls->src.env_host.assign(env_host.begin(), env_host.begin() + std::min<size_t>(env_host.size(), (size_t)(ls->Np / 128)));
    // the half-tile envelope rides on the tile envelope: the same source, the same gate
    if (ls->envelope_half && envh_dev != nullptr && envh_host.size() == 2 * env_host.size()) {
        ls->src.envh_dev = envh_dev;
        ls->src.envh_host.assign(envh_host.begin(), envh_host.begin() + 2 * ls->src.env_host.size());
    }
    return ls->env_word.p;
}

// The way back to a matrix that lives in a KKT handle: the handle's buffers may be reallocated and the handle may be destroyed
// before the inertia of an asynchronous call is fetched, so the transfer goes through the handle and refuses once it is gone.
static std::function<int()> handle_retransfer(std::weak_ptr<int> alive, std::function<int()> transfer) {
    return [alive, transfer]() {
        if (alive.expired()) {
            set_error("factorize!: the KKT handle of the last factorize! call was destroyed before its inertia was fetched; the "
                      "matrix cannot be transferred again for the fall-back tier");
            return -5;
        }
        return transfer();
    };
}

// A source that is only guaranteed for the duration of the call (the caller's arrays, staging buffers): no way back behind it.
struct SourceEndsWithCall { mnk_ls* ls; ~SourceEndsWithCall() { ls->src.retransfer = nullptr; } };

static int transfer_sc(mnk_ls* ls, mnk_sc* sc) {
    int rc = ls->spare.acquire(ls);
    if (rc) return rc;
    const int64_t nnz = sc->nnz_aug;
    int* nonfinite = set_envelope(ls, sc->d_tile_env.p, sc->tile_env, sc->d_tile_envh.p, sc->tile_envh);
    hipLaunchKernelGGL(scatter_csc_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ls->ctx->stream,
                       ls->fact.p, ls->ld, sc->aug_row.p, sc->aug_col.p, sc->aug_nz.p, nnz, amax_word(ls),
                       ls->N < sc->n ? (int32_t)ls->N : INT32_MAX, nonfinite);
    MNK_HIP(hipGetLastError());
    return 0;
}

// The leading-block probe (ls.h).  On the AC-OPF run of the bench line 13 of 17 rejected trials stop in the same 64 columns
// (3072-3135 of 11 192): the static-pivot elimination has done 1 - (1 - 0.28)^3 = 63 % of a factorization's flops by then (4.4 ms),
// the leading principal block of order 3328 alone is 2.6 % of them (1.8 ms as a factorization of its own).  A matrix whose leading
// block is not positive definite is not positive definite, and the pivots of the block do not depend on the rest of the matrix: a
// probe that fails gives the verdict of the full factorization.  When: early rejection armed, the previous verdict of this solver
// was an acceptance (in inertia_correction! the matrix after a rejection is the regularized one), and a rejection that stopped in
// the first half of the columns is at most three verdicts old -- solvers that never reject never probe.
// Returns 0 and *rejected; on a rejection the solver's state is that of an early-rejected factorization (inertia: the block's
// positive pivots, everything else negative; a solve that comes all the same completes the factorization from the handle).
static int probe_leading_block(mnk_ls* ls, mnk_sc* sc, bool* rejected) {
    *rejected = false;
    if (!(ls->probe.on && ls->early_reject && ls->accept_only_pd && ls->algo == MNK_LDL && ls->N == sc->n && !mnk_batch_active())) return 0;
    const int64_t m = ls->probe.order_due(ls->N);
    mnk_ls* c = m > 0 ? ls->probe.child(ls, m) : nullptr;
    if (c == nullptr) return 0;
    int rc = mnk_ls_factorize_sc_async(c, sc);
    if (!rc) rc = mnk_ls_fetch_info(c);
    if (rc) return rc;
    const FactorVerdict& cv = c->verdict;
    if (cv.npos == m && cv.nzero == 0 && cv.nneg == 0) { ++ls->probe.misses; return 0; }
    // not positive definite: the verdict, without the full factorization (the factor buffer still holds the PREVIOUS matrix's
    // factor: a solve that comes all the same goes through ensure_complete_factor)
    ++ls->probe.hits;
    ls->verdict.reject_early(cv.npos, cv.nzero, ls->N, cv.usable() ? m - 1 : cv.early_reject_col);
    ls->probe.note_verdict(true, ls->verdict.early_reject_col, ls->N);
    *rejected = true;
    return 0;
}

// ---- LeadingBlockProbe (ls.h): the child solver ----
mnk_ls* LeadingBlockProbe::child(mnk_ls* ls, int64_t m) {
    if (ls_child == nullptr || order != m) {
        destroy();
        if (mnk_ls_create(ls->ctx, m, ls->algo, &ls_child) != 0) { (void)hipGetLastError(); ls_child = nullptr; return nullptr; }   // (no memory for it: no probe)
        ls_child->probe.on = 0;
        ls_child->accept_only_pd = 1;
        ls_child->early_reject = 1;
        order = m;
    }
    mnk_ls* c = ls_child;
    // (the options that decide a verdict follow the parent's at every probe, not at the child's creation: a pivot_tol lowered
    // since then would otherwise count a small positive pivot of the block as zero and reject what the parent accepts)
    c->pivot_tol = ls->pivot_tol;
    c->envelope = ls->envelope;
    c->envelope_half = ls->envelope_half;
    if (c->dag_xcd_queues != ls->dag_xcd_queues || c->dag_gang != ls->dag_gang) {
        c->dag_xcd_queues = ls->dag_xcd_queues;
        c->dag_gang = ls->dag_gang;
        c->plan.invalidate();
    }
    return c;
}

int mnk_ls_factorize_sc_async(mnk_ls* ls, mnk_sc* sc) {
    MNK_REQUIRE(ls && sc && sc->ctx, "mnk_ls_factorize_sc: NULL argument or host-only handle");
    // A solver of SMALLER order factors the leading principal block of the handle's matrix (round 6: the probe of
    // madnlp_jl_amd.ipm_dev -- a matrix whose leading block is not positive definite is not positive definite, and a static-pivot
    // elimination that stops at column c has done 1 - (1 - c/N)^3 of the full factorization's work where the block alone costs (c/N)^3)
    MNK_REQUIRE(sc->n >= ls->N, "mnk_ls_factorize_sc: the solver's order exceeds the KKT system's");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }   // (a factorize! of this solver pending in an open batch runs first)
    ls->src_lowrank = sc->lbfgs != nullptr;
    int rc = ensure_wbuf(ls);
    if (rc) return rc;
    bool probe_rejected = false;
    rc = probe_leading_block(ls, sc, &probe_rejected);
    if (rc) return rc;
    if (!probe_rejected) {
        rc = transfer_sc(ls, sc);
        if (rc) return rc;
    }
    // (the KKT handle keeps aug_com until the next build_kkt!, so the pivoted tier can fetch the matrix again when
    // the inertia is asked for)
    ls->src.persistent = true;
    ls->src.retransfer = handle_retransfer(sc->alive, [ls, sc]() { return transfer_sc(ls, sc); });
    if (probe_rejected) return 0;   // (the verdict is in; ensure_complete_factor knows the way back to the matrix)
    return mnk_ls_run_factorization(ls);
}

static int transfer_dense(mnk_ls* ls, const double* Adev, int64_t lda) {
    ls->src.env_dev = nullptr;   // (no envelope: the dense order)
    dim3 grid((unsigned)ls->Np, (unsigned)((ls->Np + 1023) / 1024));
    hipLaunchKernelGGL(copy_lower_kernel, grid, dim3(256), 0, ls->ctx->stream, ls->fact.p, ls->ld, Adev, lda,
                       ls->N, ls->Np, amax_word(ls));
    MNK_HIP(hipGetLastError());
    return 0;
}

static int factorize_dense_dev(mnk_ls* ls, const double* Adev, int64_t lda, bool src_persistent = false) {
    int rc = ensure_wbuf(ls);
    if (rc) return rc;
    rc = transfer_dense(ls, Adev, lda);
    if (rc) return rc;
    ls->src.persistent = src_persistent;   // (early rejection needs a source that outlives the call: ensure_complete_factor)
    ls->src.retransfer = [ls, Adev, lda]() { return transfer_dense(ls, Adev, lda); };  // (SourceEndsWithCall where Adev's life ends with the call)
    return mnk_ls_run_factorization(ls);
}

}  // extern "C"
// (internal: the dense device source of the Schur stage's scenario blocks; asynchronous -- the caller keeps `Adev` alive and
// fetches the info itself)
int mnk_ls_factorize_dense_dev_async(mnk_ls* ls, const double* Adev, int64_t lda) {
    MNK_REQUIRE(ls && Adev && lda >= ls->N, "mnk_ls_factorize_dense_dev_async: bad argument");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    return factorize_dense_dev(ls, Adev, lda);
}
extern "C" {

int mnk_ls_factorize_dc_async(mnk_ls* ls, mnk_dc* dc) {
    MNK_REQUIRE(ls && dc, "mnk_ls_factorize_dc: NULL argument");
    MNK_REQUIRE(dc->order == ls->N, "mnk_ls_factorize_dc: order mismatch");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }   // (a factorize! of this solver pending in an open batch runs first)
    int rc = factorize_dense_dev(ls, dc->aug.p, round_up(dc->order, PAD), true);
    // (behind the run, as ever: until here the way back was factorize_dense_dev's, through the buffer's address)
    ls->src.retransfer = handle_retransfer(dc->alive, [ls, dc]() { return transfer_dense(ls, dc->aug.p, round_up(dc->order, PAD)); });
    return rc;
}

static int finish_info(mnk_ls* ls, int* info) {
    int rc = mnk_ls_fetch_info(ls);
    if (rc) return rc;
    if (info) *info = ls->verdict.info;
    return 0;
}

int mnk_ls_factorize_sc(mnk_ls* ls, mnk_sc* sc, int* info) {
    int rc = mnk_ls_factorize_sc_async(ls, sc);
    return rc ? rc : finish_info(ls, info);
}

int mnk_ls_factorize_dc(mnk_ls* ls, mnk_dc* dc, int* info) {
    int rc = mnk_ls_factorize_dc_async(ls, dc);
    return rc ? rc : finish_info(ls, info);
}

int mnk_ls_factorize_dense(mnk_ls* ls, const double* A, int64_t lda, int loc, int* info) {
    MNK_REQUIRE(ls && A, "mnk_ls_factorize_dense: NULL argument");
    MNK_REQUIRE(lda >= ls->N, "mnk_ls_factorize_dense: lda < N");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }   // (a factorize! of this solver pending in an open batch runs first)
    DevBuf<double> tmp;   // staging of a host matrix
    if (loc != MNK_DEVICE) {
        int rc_t = tmp.alloc((size_t)ls->N * ls->N);
        if (rc_t) return rc_t;
        MNK_HIP(mnk::h2d_copy_2d(tmp.p, ls->N * sizeof(double), A, lda * sizeof(double), ls->N * sizeof(double), ls->N,
                                 ls->ctx->stream));
        A = tmp.p;
        lda = ls->N;
    }
    SourceEndsWithCall ends{ls};   // (a breakdown is handled below, while the caller's buffer / the staging buffer is alive)
    const int rc = factorize_dense_dev(ls, A, lda);
    if (loc != MNK_DEVICE) MNK_HIP(mnk::stream_wait(ls->ctx->stream));
    return rc ? rc : finish_info(ls, info);
}

int mnk_ls_factorize_csc(mnk_ls* ls, const int32_t* colptr, const int32_t* rowval, const double* nzval,
                         int index_base, int* info) {
    MNK_REQUIRE(ls && colptr && rowval && nzval, "mnk_ls_factorize_csc: NULL argument");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }   // (a factorize! of this solver pending in an open batch runs first)
    const int64_t N = ls->N;
    const int64_t nnz = colptr[N] - index_base;
    std::vector<int32_t> row(nnz), col(nnz);
    for (int64_t c = 0; c < N; ++c)
        for (int64_t k = colptr[c] - index_base; k < colptr[c + 1] - index_base; ++k) {
            row[k] = rowval[k] - index_base;
            col[k] = (int32_t)c;
            MNK_REQUIRE(row[k] >= c && row[k] < N, "mnk_ls_factorize_csc: matrix must be lower triangular");
        }
    DevBuf<int32_t> drow, dcol;
    DevBuf<double> dnz;
    std::vector<double> nzv(nzval, nzval + nnz);
    int rc = drow.upload(row, ls->ctx->stream);
    rc |= dcol.upload(col, ls->ctx->stream);
    rc |= dnz.upload(nzv, ls->ctx->stream);
    // the envelope of this pattern (only the task-DAG schedule reads it)
    const std::vector<int32_t> env = ls->envelope ? mnk_tile_envelope(N, row.data(), col.data(), nnz, 128) : std::vector<int32_t>();
    const std::vector<int32_t> envh = ls->envelope && ls->envelope_half ? mnk_tile_envelope(N, row.data(), col.data(), nnz, 64) : std::vector<int32_t>();
    if (ls->envelope) rc |= ls->env_own.upload(env, ls->ctx->stream);
    if (!envh.empty()) rc |= ls->envh_own.upload(envh, ls->ctx->stream);
    if (rc) return -2;
    rc = ensure_wbuf(ls);
    if (rc) return rc;
    auto transfer = [ls, nnz, &drow, &dcol, &dnz, &env, &envh]() -> int {
        int r = ls->spare.acquire(ls);
        if (r) return r;
        int* nonfinite = set_envelope(ls, env.empty() ? nullptr : ls->env_own.p, env, envh.empty() ? nullptr : ls->envh_own.p, envh);
        if (nnz > 0)
            hipLaunchKernelGGL(scatter_csc_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ls->ctx->stream,
                               ls->fact.p, ls->ld, drow.p, dcol.p, dnz.p, nnz, amax_word(ls), INT32_MAX, nonfinite);
        MNK_HIP(hipGetLastError());
        return 0;
    };
    rc = transfer();
    if (rc) return rc;
    SourceEndsWithCall ends{ls};   // (the staging buffers die with this call)
    ls->src.persistent = false;
    ls->src.retransfer = transfer;
    rc = mnk_ls_run_factorization(ls);
    if (rc) return rc;
    MNK_HIP(mnk::stream_wait(ls->ctx->stream));
    return finish_info(ls, info);
}

static int debug_envelope_csc(int64_t n, const int32_t* colptr, const int32_t* rowval, int index_base, int32_t* out, int cap, int64_t block) {
    if (n <= 0 || colptr == nullptr || rowval == nullptr || cap < 0) return -1;
    const int64_t nnz = colptr[n] - index_base;
    std::vector<int32_t> row(nnz), col(nnz);
    for (int64_t c = 0; c < n; ++c)
        for (int64_t k = colptr[c] - index_base; k < colptr[c + 1] - index_base; ++k) { row[k] = rowval[k] - index_base; col[k] = (int32_t)c; }
    const std::vector<int32_t> env = mnk_tile_envelope(n, row.data(), col.data(), nnz, block);
    if (out != nullptr)
        for (int I = 0; I < std::min((int)env.size(), cap); ++I) out[I] = env[I];
    return (int)env.size();
}

int mnk_debug_tile_env_csc(int64_t n, const int32_t* colptr, const int32_t* rowval, int index_base, int32_t* out, int cap) {
    return debug_envelope_csc(n, colptr, rowval, index_base, out, cap, 128);
}

int mnk_debug_tile_envh_csc(int64_t n, const int32_t* colptr, const int32_t* rowval, int index_base, int32_t* out, int cap) {
    return debug_envelope_csc(n, colptr, rowval, index_base, out, cap, 64);
}

int mnk_debug_probe_schedule(int64_t N, int n, const int64_t* cols, int64_t* orders) {
    if (N <= 0 || n < 0 || (n > 0 && (cols == nullptr || orders == nullptr))) return -1;
    LeadingBlockProbe probe;
    for (int i = 0; i < n; ++i) {
        orders[i] = probe.order_due(N);
        probe.note_verdict(cols[i] >= 0, cols[i], N);
    }
    return 0;
}

int mnk_ls_inertia(mnk_ls* ls, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg) {
    MNK_REQUIRE(ls, "mnk_ls_inertia: NULL argument");
    if (ls->alt) { const char* refusal = ls->alt->no_inertia_message(); MNK_REQUIRE(refusal == nullptr, refusal); }
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    MNK_REQUIRE(ls->verdict.has_factorization(), "mnk_ls_inertia: factorize first");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    int rc = mnk_ls_fetch_info(ls);
    if (rc) return rc;
    if (num_pos) *num_pos = ls->verdict.npos;
    if (num_zero) *num_zero = ls->verdict.nzero;
    if (num_neg) *num_neg = ls->verdict.nneg;
    return 0;
}

int mnk_ls_check_solve(mnk_ls* ls) {
    MNK_REQUIRE(ls, "mnk_ls_check_solve: NULL argument");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_q = mnk_solve_sync_deferred(ls); if (rc_q) return rc_q; }
    MNK_HIP(mnk::stream_wait(ls->ctx->stream));
    if (mnk_ls_take_solve_abort(ls)) {
        set_error("mnk_ls_check_solve: a persistent solve on device-resident data gave up waiting for a peer workgroup "
                  "(device oversubscribed by another process?); its result is invalid -- solve again "
                  "(persistent_solve is now off for this solver)");
        return -3;
    }
    return 0;
}

// A factorization that was stopped at its first non-positive pivot (early_reject) left no factor.  A caller that solves all the
// same did not ask for the inertia, or overrules its own test: MadNLP does where it initializes the multipliers by least
// squares and in the restoration phases' first steps (reference src/IPM/solver.jl:147-190, src/IPM/restoration.jl: factorize_wrapper!
// followed by solve_refine_wrapper! without inertia_correction!).  The matrix is then factored again, to the end: early
// rejection is an optimization of the rejected trials, never a change of what the solver can do.
static int ensure_complete_factor(mnk_ls* ls, const char* who) {
    if (ls->verdict.reject_armed()) { int rc_i = mnk_ls_fetch_info(ls); if (rc_i) return rc_i; }   // (known when the pivots are)
    if (ls->verdict.usable()) return 0;
    { static const bool peek = getenv("MNK_DBG_NO_REDO") != nullptr; if (peek) return 0; }   // (diagnostics: look at what a rejected factorization left)
    if (!ls->src.retransfer) {
        set_error("%s: the last factorization was stopped at its first non-positive pivot (early_reject) and its source is gone: "
                  "there is no factor", who);
        return -1;
    }
    const int keep = ls->early_reject;
    ls->early_reject = 0;
    int rc = ls->src.retransfer();
    if (!rc) rc = mnk_ls_run_factorization(ls);
    if (!rc) rc = mnk_ls_fetch_info(ls);
    ls->early_reject = keep;
    ls->verdict.completed_after_all();
    return rc;
}

int mnk_ls_solve(mnk_ls* ls, double* x, int64_t nrhs, int64_t ldx, int loc) {
    MNK_REQUIRE(ls && x, "mnk_ls_solve: NULL argument");
    { int rc_d = mnk_ls_sync_deferred_fact(ls); if (rc_d) return rc_d; }
    MNK_REQUIRE(ls->verdict.has_factorization(), "mnk_ls_solve: factorize first");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_f = ensure_complete_factor(ls, "mnk_ls_solve"); if (rc_f) return rc_f; }
    MNK_REQUIRE(nrhs >= 1 && ldx >= ls->N, "mnk_ls_solve: bad nrhs/ldx");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    if (ls->alt) return mnk_ls_alt_solve(ls, x, nrhs, ldx, loc);   // (never queued in a solve batch: runs at once)
    if (ls->solves.take_abort()) {
        // a previous solve on device-resident vectors gave up (its result is invalid): fail loudly now and use
        // the stepwise solve from here on
        set_error("mnk_ls_solve: an earlier persistent solve on device-resident data gave up waiting for a peer "
                  "workgroup (device oversubscribed by another process?); its result is invalid -- refactorize/solve "
                  "again (persistent_solve is now off for this solver)");
        return -3;
    }
    // from option multi_rhs_min right-hand sides on, a static-pivot factor solves them blocked (never queued in a solve batch)
    const mnk::SolveMultiPlan mp = mnk_ls_plan_multi(ls, nrhs);
    if (mp.path == mnk::SOLVE_BLOCKED) return mnk_ls_run_solve_multi(ls, x, nrhs, ldx, loc, mp);
    hipStream_t s = ls->ctx->stream;
    const int64_t N = ls->N, Np = ls->Np;
    double* w = ls->xwork.p;
    for (int64_t k = 0; k < nrhs; ++k) {
        double* xk = x + k * ldx;
        if (loc == MNK_DEVICE) {   // (the one-launch solve works on the caller's vector itself)
            if (nrhs == 1 && mnk_solve_defer(ls, xk)) continue;   // an open solve batch of this thread took it
            int rc = mnk_solve_sync_deferred(ls);                   // (earlier queued solves of this solver keep their place)
            if (rc) return rc;
            rc = mnk_ls_run_solve(ls, w, xk);
            if (rc) return rc;
            continue;
        }
        { int rc_q = mnk_solve_sync_deferred(ls); if (rc_q) return rc_q; }
        auto solve_staged = [&]() -> int {   // the host's right-hand side, zero padded, through the work vector
            MNK_HIP(hipMemsetAsync(w, 0, Np * sizeof(double), s));
            MNK_HIP(mnk::h2d_copy(w, xk, N * sizeof(double), s));
            return mnk_ls_run_solve(ls, w);
        };
        int rc = solve_staged();
        if (rc) return rc;
        if (ls->solves.persistent_solve) {
            // The one-launch solve gives up (instead of hanging the device) if its workgroups cannot all become
            // resident, e.g. another process saturates the GPU with its own persistent kernels.  The host still
            // owns the right-hand side here: redo this and all later solves with one launch per step.
            MNK_HIP(mnk::stream_wait(s));
            if (mnk_ls_take_solve_abort(ls) && (rc = solve_staged()) != 0) return rc;
        }
        MNK_HIP(mnk::d2h_copy(xk, w, N * sizeof(double), s));
    }
    return 0;
}

// ---- array entry points for batches of independent instances (one call per phase of an iteration instead of four to six
// calls per instance: from an interpreted host the per-call overhead of 16 instances was 4.6 ms of a 150 ms step) ----
int mnk_sc_step_batch(int n, mnk_sc* const* sc, mnk_ls* const* ls, const double* const* jac_coo, const double* const* hess_coo,
                      const double* const* pr_diag, const double* const* du_diag, int loc) {
    MNK_REQUIRE(n >= 0 && (n == 0 || (sc && ls && jac_coo && hess_coo && pr_diag && du_diag)), "mnk_sc_step_batch: NULL argument");
    for (int i = 0; i < n; ++i)
        MNK_REQUIRE(sc[i] == nullptr || sc[i]->lbfgs == nullptr, "mnk_sc_step_batch: a system with a compact L-BFGS handle attached is not batched");
    int rc = mnk_factorize_batch_begin();
    if (rc) return rc;
    for (int i = 0; i < n && !rc; ++i) {
        rc = mnk_sc_compress_jacobian(sc[i], jac_coo[i], loc);
        if (!rc) rc = mnk_sc_compress_hessian(sc[i], hess_coo[i], loc);
        if (!rc) rc = mnk_sc_build(sc[i], pr_diag[i], du_diag[i], loc);
        if (!rc) rc = mnk_ls_factorize_sc_async(ls[i], sc[i]);
    }
    const int rc_end = mnk_factorize_batch_end();
    return rc ? rc : rc_end;
}

int mnk_ls_inertia_batch(int n, mnk_ls* const* ls, int64_t* num_pos, int64_t* num_zero, int64_t* num_neg) {
    MNK_REQUIRE(n >= 0 && (n == 0 || (ls && num_pos && num_zero && num_neg)), "mnk_ls_inertia_batch: NULL argument");
    for (int i = 0; i < n; ++i) {
        int rc = mnk_ls_inertia(ls[i], num_pos + i, num_zero + i, num_neg + i);
        if (rc) return rc;
    }
    return 0;
}

int mnk_ls_solve_batch(int n, mnk_ls* const* ls, double* const* x, int loc) {
    MNK_REQUIRE(n >= 0 && (n == 0 || (ls && x)), "mnk_ls_solve_batch: NULL argument");
    for (int i = 0; i < n; ++i)
        MNK_REQUIRE(ls[i] == nullptr || !ls[i]->src_lowrank, "mnk_ls_solve_batch: the system factored last has a compact L-BFGS handle attached (its solves go through mnk_sc_solve_kkt)");
    int rc = mnk_solve_batch_begin();
    if (rc) return rc;
    for (int i = 0; i < n && !rc; ++i) rc = mnk_ls_solve(ls[i], x[i], 1, ls[i]->N, loc);
    const int rc_end = mnk_solve_batch_end();
    return rc ? rc : rc_end;
}

int mnk_ls_debug_dag_state(mnk_ls* ls, int* flags, int64_t nflags, int* chain, int64_t nchain, int* have) {
    MNK_REQUIRE(ls && have, "mnk_ls_debug_dag_state: NULL argument");
    *have = ls->dbg_flags.empty() ? 0 : 1;
    if (flags) memcpy(flags, ls->dbg_flags.data(), sizeof(int) * (size_t)std::min<int64_t>(nflags, (int64_t)ls->dbg_flags.size()));
    if (chain) memcpy(chain, ls->dbg_chain.data(), sizeof(int) * (size_t)std::min<int64_t>(nchain, (int64_t)ls->dbg_chain.size()));
    return 0;
}

int mnk_ls_debug_solve_trace(mnk_ls* ls, unsigned long long* out, int64_t n) {
    if (ls && out && ls->dag_trace.p && ls->dag_trace_on) {  // the task-DAG schedule's trace (option dag_trace) shares this read-out
        MNK_HIP(hipSetDevice(ls->ctx->device));
        MNK_HIP(mnk::stream_wait(ls->ctx->stream));
        const int64_t cnt = std::min<int64_t>(n, (int64_t)ls->dag_trace.n);
        MNK_HIP(mnk::d2h_copy(out, ls->dag_trace.p, cnt * sizeof(unsigned long long), ls->ctx->stream));
        return 0;
    }
    MNK_REQUIRE(ls && out && ls->solves.trace.p, "mnk_ls_debug_solve_trace: tracing is off (option solve_trace)");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    MNK_HIP(mnk::stream_wait(ls->ctx->stream));
    const int64_t cnt = std::min<int64_t>(n, (ls->Np / 64) * 8);
    MNK_HIP(mnk::d2h_copy(out, ls->solves.trace.p, cnt * sizeof(unsigned long long), ls->ctx->stream));
    return 0;
}

int mnk_ls_get_factor(mnk_ls* ls, double* L, double* D, int loc) {
    MNK_REQUIRE(ls && L, "mnk_ls_get_factor: NULL argument");
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    MNK_REQUIRE(ls->verdict.has_factorization(), "mnk_ls_get_factor: factorize first");
    { int rc_f = ensure_complete_factor(ls, "mnk_ls_get_factor"); if (rc_f) return rc_f; }
    MNK_HIP(hipSetDevice(ls->ctx->device));
    hipStream_t s = ls->ctx->stream;
    if (loc == MNK_DEVICE) {
        MNK_HIP(hipMemcpy2DAsync(L, ls->N * sizeof(double), ls->fact.p, ls->ld * sizeof(double), ls->N * sizeof(double), ls->N,
                                 hipMemcpyDeviceToDevice, s));
        if (D) MNK_HIP(hipMemcpyAsync(D, ls->dvec.p, ls->N * sizeof(double), hipMemcpyDeviceToDevice, s));
        MNK_HIP(mnk::stream_wait(s));
    } else {
        MNK_HIP(mnk::d2h_copy_2d(L, ls->N * sizeof(double), ls->fact.p, ls->ld * sizeof(double), ls->N * sizeof(double), ls->N, s));
        if (D) MNK_HIP(mnk::d2h_copy(D, ls->dvec.p, ls->N * sizeof(double), s));
    }
    return 0;
}

int mnk_ls_get_stat(mnk_ls* ls, const char* key, double* value) {
    MNK_REQUIRE(ls && key && value, "mnk_ls_get_stat: NULL argument");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    if (ls->verdict.has_factorization()) {
        int rc = mnk_ls_fetch_info(ls);
        if (rc) return rc;
    }
    if (!strncmp(key, "pinned:", 7)) {   // 1 if MNK_OPTIONS & co. fixed this option for the process (set_option calls on it are ignored)
        *value = std::find(ls->env_keys.begin(), ls->env_keys.end(), std::string(key + 7)) != ls->env_keys.end() ? 1.0 : 0.0;
        return 0;
    }
    if (!strcmp(key, "panel_algo")) { *value = ls->algo_now; return 0; }
    if (!strcmp(key, "pp_fallbacks")) { *value = ls->pp.fallbacks; return 0; }
    if (!strcmp(key, "solve_path")) { *value = ls->solves.last_path; return 0; }   // how the last solve ran (solve_plan.h: SolvePath; 0: none yet)
    if (!strcmp(key, "solve_rhs_chunks")) { *value = ls->solves.last_rhs_chunks; return 0; }   // passes over the factor per sweep of the last blocked solve (solve_path 5; 0: none yet)
    // which bounded device-side wait expired last (info = -7): 1 bulk task / operand rows, 2 bulk task / chunk order, 4 chain strip / diagonal block, 5 chain strip / bulk kernel's rows or band tiles; 0: none
    if (!strcmp(key, "timeout_site")) { *value = ls->pp.last_site; return 0; }
    if (!strcmp(key, "probe_hits")) { *value = (double)ls->probe.hits; return 0; }       // matrices rejected by the leading-block probe alone
    if (!strcmp(key, "probe_misses")) { *value = (double)ls->probe.misses; return 0; }   // probes that passed (the full factorization followed)
    if (!strcmp(key, "early_rejects")) { *value = (double)ls->verdict.early_rejects; return 0; }       // factorizations stopped at their first non-positive pivot
    if (!strcmp(key, "early_reject_redone")) { *value = (double)ls->verdict.early_reject_redone; return 0; }   // ... rejected factorizations completed after all because the caller solved
    if (!strcmp(key, "early_reject_col")) { *value = (double)ls->verdict.early_reject_col; return 0; } // ... the last valid pivot of the latest one
    if (!strcmp(key, "stall_ms_total")) { *value = ls->stall_ms_total; return 0; }      // what this solver's expired waits (fall-backs) have cost, host ms
    if (!strcmp(key, "stall_ms_process")) { *value = mnk_process_stall_ms(); return 0; }  // ... all solvers of the process
    if (!strcmp(key, "growth")) { *value = ls->bk.last_growth; return 0; }  // BUNCHKAUFMAN: max|d_k| / max|a_ij| of the static-pivot tier
    if (!strcmp(key, "sign_changes")) { *value = (double)ls->bk.last_sign_changes; return 0; }  // ... and sign changes along its pivots
    if (!strcmp(key, "bk_count")) { *value = ls->bk.count; return 0; }
    if (!strcmp(key, "evd_sweeps")) { *value = ls->alt ? ls->alt->stat(key) : 0.0; return 0; }   // EVD: block Jacobi sweeps of the last factorization
    if (!strcmp(key, "bk_panel_multi")) { *value = ls->bk.multi_last() ? 1.0 : 0.0; return 0; }
    if (!strcmp(key, "bk_mw_fallbacks")) { *value = ls->bk.mw_fallbacks(); return 0; }
    if (!strcmp(key, "dag_bulk_wgs")) { *value = ls->ctx->dag_cus > 0 ? mnk::grid_at_launch(0, ls->ctx->num_cu, ls->ctx->dag_cus, 3) : 0; return 0; }   // grid of the bulk kernel beside the 16-CU chain
    if (!strcmp(key, "dag_ntasks")) { *value = ls->plan.list.size(); return 0; }    // task-DAG schedule: bulk tasks, ...
    if (!strcmp(key, "dag_ntasks1")) { *value = ls->plan.list.n1; return 0; }  // ... of them in the first phase, ...
    if (!strcmp(key, "dag_js2")) { *value = ls->plan.key.js2; return 0; }          // ... first strip-column of the second phase
    if (!strcmp(key, "dag_nq")) { *value = std::max(ls->plan.nq[0], ls->plan.nq[1]); return 0; }   // ... queues the device list is dealt into (0: one)
    if (!strcmp(key, "dag_steals")) {   // ... tasks the last factorization's workgroups took from another XCD's queue
        int st[2] = {0, 0};
        if (ls->plan.qheads.p != nullptr)
            for (int ph = 0; ph < 2; ++ph)
                MNK_HIP(mnk::d2h_copy(&st[ph], ls->plan.qheads.p + ph * mnk::DAG_QHEAD_WORDS + mnk::DAG_NQ * mnk::DAG_QHEAD_STRIDE, sizeof(int), ls->ctx->stream));
        *value = (double)st[0] + (double)st[1];
        return 0;
    }
    if (!strcmp(key, "env_ksteps") || !strcmp(key, "env_ksteps_skipped")) {
        // task-DAG schedule: 128-column k-steps of the bulk tasks (tile columns of the chunks' K-loops, one per closing task) in
        // the task list / of them skipped by the last factorization as structurally zero (0 without an envelope, with the
        // envelope off, or when a NaN / Inf entry closed it)
        int gate = 1;
        if (ls->env_used && ls->env_word.p) MNK_HIP(mnk::d2h_copy(&gate, ls->env_word.p + 1, sizeof(int), ls->ctx->stream));
        int64_t cnt[2] = {0, 0};
        mnk::dag_env_count(ls->plan.list, ls->env_used && gate == 0 ? ls->src.env_host.data() : nullptr, (int)ls->src.env_host.size(), cnt);
        *value = (double)(!strcmp(key, "env_ksteps") ? cnt[0] : cnt[1]);
        return 0;
    }
    if (!strcmp(key, "envh_ksteps") || !strcmp(key, "envh_ksteps_skipped")) {
        // the same in HALF-tile k-steps (one 64 x 64 quadrant of a tile over 64 columns: 1 / 8 of a k-step): what the tile envelope
        // leaves of the bulk tasks / of that, what the waves of the last factorization skipped by the envelopes of their 64-row
        // halves and as upper quadrants of diagonal tiles (0 with envelope_half = 0, without an envelope or when the gate closed it)
        int gate = 1;
        if (ls->env_used && ls->env_word.p) MNK_HIP(mnk::d2h_copy(&gate, ls->env_word.p + 1, sizeof(int), ls->ctx->stream));
        const bool on = ls->env_used && gate == 0;
        int64_t cnt[2] = {0, 0};
        mnk::dag_envh_count(ls->plan.list, on ? ls->src.env_host.data() : nullptr, on && ls->envh_used ? ls->src.envh_host.data() : nullptr,
                            (int)ls->src.env_host.size(), cnt);
        *value = (double)(!strcmp(key, "envh_ksteps") ? cnt[0] : cnt[1]);
        return 0;
    }
    set_error("mnk_ls_get_stat: unknown key '%s'", key);
    return -1;
}

int mnk_ls_bk_info(mnk_ls* ls, int* active, int* count, int32_t* perm, double* doff) {
    MNK_REQUIRE(ls, "mnk_ls_bk_info: NULL argument");
    MNK_HIP(hipSetDevice(ls->ctx->device));
    { int rc_d = mnk_ls_sync_deferred(ls); if (rc_d) return rc_d; }
    if (ls->verdict.has_factorization()) {
        int rc = mnk_ls_fetch_info(ls);  // the tier is decided when the static factorization's pivots are known
        if (rc) return rc;
    }
    if (active) *active = ls->verdict.is_pivoted() ? 1 : 0;
    if (count) *count = ls->bk.count;
    return ls->verdict.is_pivoted() ? ls->bk.read_pivots(ls, perm, doff) : 0;
}

int mnk_gemm_nt(mnk_ctx* ctx, int mode, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda,
                const double* B, int64_t ldb, double* C, int64_t ldc) {
    MNK_REQUIRE(ctx && A && B && C, "mnk_gemm_nt: NULL argument");
    MNK_HIP(hipSetDevice(ctx->device));
    return launch_gemm_nt(ctx->stream, mode, M, N, K, A, lda, B, ldb, C, ldc, nullptr, nullptr, 0, nullptr);
}

}  // extern "C"

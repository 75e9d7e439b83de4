// Everything a context owns (mnk_ctx, common.h): the live-context list, the launch lock and the arbiter of the persistent
// kernels, context creation and destruction, and EVERY stream of a context -- no other unit creates or destroys one.  Which mask
// bits a CU-masked stream gets is decided in stream_plan.h (host only); here the streams are made, warmed up, kept and destroyed.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>

#include "common.h"
#include "stream_plan.h"

using namespace mnk;

static std::mutex g_ctx_mutex;
static std::atomic<int> g_live_ctx[64];
static std::vector<mnk_ctx*> g_ctx_list[64];   // live contexts per device that use the shared pairs (g_ctx_mutex): release_shared_streams_locked

int mnk_live_contexts(int device) { return g_live_ctx[device & 63].load(std::memory_order_relaxed); }

std::recursive_mutex& mnk::launch_mutex() {
    static std::recursive_mutex m;
    return m;
}

// ---- device arbiter of the persistent kernels (common.h) ----
namespace {
struct PersistSlot {   // (guarded by mnk::launch_mutex(): recursive -- a factorization that is redone inside mnk_ls_fetch_info re-enters on the same thread)
    hipEvent_t last = nullptr;
    bool recorded = false;
};
PersistSlot g_persist[64];
}  // namespace

void mnk::quiesce_persistent() {
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (int d = 0; d < 64; ++d) {
        PersistSlot& ps = g_persist[d];
        if (ps.last == nullptr || !ps.recorded) continue;
        (void)hipSetDevice(d);
        (void)hipEventSynchronize(ps.last);
    }
    if (have_cur) (void)hipSetDevice(cur);
    (void)hipGetLastError();
}

int mnk_persist_begin(mnk_ctx* ctx, hipStream_t s) {
    PersistSlot& ps = g_persist[ctx->device & 63];
    mnk::launch_mutex().lock();
    if (ps.last == nullptr && hipEventCreateWithFlags(&ps.last, hipEventDisableTiming) != hipSuccess) {
        ps.last = nullptr;
        mnk::launch_mutex().unlock();
        mnk::set_error("mnk_persist_begin: hipEventCreate failed");
        return -2;
    }
    if (ps.recorded && hipStreamWaitEvent(s, ps.last, 0) != hipSuccess) {
        mnk::launch_mutex().unlock();
        mnk::set_error("mnk_persist_begin: hipStreamWaitEvent failed");
        return -2;
    }
    return 0;
}

int mnk_persist_end(mnk_ctx* ctx, hipStream_t s, int rc) {
    PersistSlot& ps = g_persist[ctx->device & 63];
    if (hipEventRecord(ps.last, s) == hipSuccess) ps.recorded = true;
    else if (rc == 0) { mnk::set_error("mnk_persist_end: hipEventRecord failed"); rc = -2; }
    mnk::launch_mutex().unlock();
    return rc;
}

// ---- the owner of the CU-masked pairs that the contexts of a process share per device ----
// Every CU-masked stream is a hardware queue of its own, and the hardware runs only so many queues of a device side by side --
// ALL PROCESSES TOGETHER: with four idle contexts in a PARENT process, each holding its masked pair, a child's chain and bulk
// kernels were no longer scheduled together and every run of tools/parent_child_probe.py lost factorizations to their bounded
// waits; without the pairs, none.  So the contexts of a device SHARE one pair per kind (the persistent operations
// of a process take turns on the device anyway: mnk_persist_begin -- and two streams whose kernels must run side by side, chain
// and bulk, must not end up multiplexed behind a third one), a pair is made when a caller first needs it, and all of them go with
// mnk_release_idle_streams or the device's last context.
namespace {
struct MaskedPair { hipStream_t sp = nullptr, su = nullptr; int chain_cus = 0; };   // (sp == nullptr: masks were not to be had)
std::map<std::pair<int, int>, MaskedPair> g_pairs[64];   // per device: (kind, c of PAIR_SMALL) -> pair (g_ctx_mutex)

// First launches on a new pair: the bulk kernels (mnk_dag_warmup: kernels that need scratch, on the grid 3 * num_cu) and the
// inverse kernel of the solves (mnk_solve_warmup: where a factorization launches its inverses), in this order.  Best effort.
struct PairWarmups { bool dag_su, solve_su, solve_sp; };
constexpr PairWarmups PAIR_WARMUPS[PAIR_KINDS] = {
    {true, true, true},     // PAIR_DAG
    {true, true, false},    // PAIR_DEEP
    {true, true, true},     // PAIR_BATCH
    {true, false, false},   // PAIR_SMALL (its `su` may not exist)
    {false, false, false},  // PAIR_PANEL
};

// A stream restricted to the mask bits [first, first + count) of the device
bool make_masked_stream(int num_cu, int first, int count, hipStream_t& out) {
    const std::vector<uint32_t> m = cu_mask_words(num_cu, first, count);
    if (hipExtStreamCreateWithCUMask(&out, (uint32_t)m.size(), m.data()) == hipSuccess) return true;
    (void)hipGetLastError();
    out = nullptr;
    return false;
}

void kill_stream(hipStream_t& st) {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
}

// The two streams of a split, or neither; then the kind's warm-ups.
bool make_pair(int kind, int num_cu, const StreamSplit& sl, MaskedPair& p) {
    if (!sl.exists || !make_masked_stream(num_cu, sl.chain_first, sl.chain_count, p.sp)) return false;
    if (sl.rest_count > 0 && !make_masked_stream(num_cu, sl.rest_first, sl.rest_count, p.su)) { kill_stream(p.sp); return false; }
    p.chain_cus = sl.chain_count;
    const PairWarmups& w = PAIR_WARMUPS[kind];
    if (w.dag_su && p.su != nullptr && mnk_dag_warmup(&p.su, 1, 3 * num_cu) != 0) (void)hipGetLastError();
    for (hipStream_t s : {w.solve_su ? p.su : nullptr, w.solve_sp ? p.sp : nullptr})
        if (s != nullptr && mnk_solve_warmup(s) != 0) (void)hipGetLastError();
    return true;
}
}  // namespace

// The shared pair of this kind on the context's device, made now if the device has none (launch lock, then the context mutex:
// stream creation may synchronize the device).  *sp == nullptr with rc 0: no such pair (stream_plan.h) -- the caller keeps its
// fallback; rc -2: CU-masked streams are not available.
int mnk_ctx_stream_pair(mnk_ctx* c, int kind, int arg, hipStream_t* sp, hipStream_t* su) {
    *sp = *su = nullptr;
    const StreamSplit sl = stream_split(kind, c->num_cu, c->dag_cus, c->dag_cus2, arg);
    if (!sl.exists) return 0;
    const std::pair<int, int> key{kind, kind == PAIR_SMALL ? arg : 0};
    auto& pairs = g_pairs[c->device & 63];
    {
        std::lock_guard<std::mutex> lk(g_ctx_mutex);
        const auto it = pairs.find(key);
        if (it != pairs.end() && it->second.sp != nullptr) { *sp = it->second.sp; *su = it->second.su; return 0; }
    }
    mnk::LaunchLock lock;
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    MaskedPair& p = pairs[key];
    if (p.sp == nullptr) {
        mnk::quiesce_persistent();
        MNK_HIP(hipSetDevice(c->device));
        if (!make_pair(kind, c->num_cu, sl, p)) { set_error("CU-masked streams are not available on this device"); return -2; }
    }
    *sp = p.sp; *su = p.su;
    return 0;
}

// Destroys every shared pair of `device` and the look-ahead pairs of its live contexts: each is made again by the first
// operation that needs it.  Caller holds the launch mutex; nothing persistent is in flight afterwards.
static void release_shared_streams_locked(int device) {
    mnk::quiesce_persistent();
    (void)hipSetDevice(device);
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    for (auto& kv : g_pairs[device & 63]) { kill_stream(kv.second.sp); kill_stream(kv.second.su); }
    g_pairs[device & 63].clear();
    for (mnk_ctx* c : g_ctx_list[device & 63]) { kill_stream(c->sp); kill_stream(c->su); }
    (void)hipGetLastError();
}

extern "C" int mnk_release_idle_streams(int device) {
    MNK_REQUIRE(device >= 0 && device < 64, "mnk_release_idle_streams: bad device");
    mnk::LaunchLock lock;   // (no persistent group is being launched; the ones in flight are waited for)
    release_shared_streams_locked(device);
    return 0;
}

// the look-ahead streams of the launch-per-panel schedules (1, 4), per context: a quarter of the CUs for the panel stream, the
// rest for the update stream (measured, profiles/; MNK_PANEL_CUS overrides); stream priorities where masks are not to be had
int mnk_ctx_ensure_panel_streams(mnk_ctx* c) {
    if (c->sp != nullptr) return 0;
    mnk::LaunchLock lock;
    mnk::quiesce_persistent();
    MNK_HIP(hipSetDevice(c->device));
    const char* e = getenv("MNK_PANEL_CUS");
    const int want = e ? atoi(e) : panel_default_cus(c->num_cu);
    MaskedPair p;
    if (make_pair(PAIR_PANEL, c->num_cu, stream_split(PAIR_PANEL, c->num_cu, 0, 0, want), p)) {
        c->sp = p.sp; c->su = p.su; c->panel_cus = want;
    } else {
        int prio_lo = 0, prio_hi = 0;  // numerically lower = higher priority
        MNK_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        MNK_HIP(hipStreamCreateWithPriority(&c->sp, hipStreamNonBlocking, prio_hi));
        MNK_HIP(hipStreamCreateWithPriority(&c->su, hipStreamNonBlocking, prio_lo));
    }
    return 0;
}

// the side stream of the background zero-fill (SpareFill, ls.h), created on first use; nullptr: not to be had
hipStream_t mnk_ctx_fill_stream(mnk_ctx* c) {
    if (!c->s_fill && hipStreamCreateWithFlags(&c->s_fill, hipStreamNonBlocking) != hipSuccess) c->s_fill = nullptr;
    return c->s_fill;
}

static void ctx_free(mnk_ctx* c) {
    mnk::LaunchLock lock;   // (stream / event destruction may synchronize)
    mnk::quiesce_persistent();
    (void)hipSetDevice(c->device);
    const int live_left = g_live_ctx[c->device & 63].fetch_sub(1, std::memory_order_relaxed) - 1;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mutex);
        auto& v = g_ctx_list[c->device & 63];
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    // the last context of a device: the process keeps no CU-masked stream (= hardware queue) of that device behind
    if (live_left <= 0) release_shared_streams_locked(c->device);
    if (c->ev_a) (void)hipEventDestroy(c->ev_a);
    if (c->ev_b) (void)hipEventDestroy(c->ev_b);
    for (hipEvent_t e : c->ev_panel) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_next) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_next2) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_bdone) (void)hipEventDestroy(e);
    if (c->sp) (void)hipStreamDestroy(c->sp);
    if (c->su) (void)hipStreamDestroy(c->su);
    if (c->s_fill) (void)hipStreamDestroy(c->s_fill);
    mnk_batch_stream_gone(c->device, c->stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void mnk_ctx_child_added(mnk_ctx* ctx) {
    if (!ctx) return;
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    ++ctx->children;
}

void mnk_ctx_child_gone(mnk_ctx* ctx) {
    if (!ctx) return;
    bool free_now = false;
    {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        --ctx->children;
        free_now = ctx->released && ctx->children <= 0;
    }
    if (free_now) ctx_free(ctx);
}

extern "C" {

// A context always has the whole device.  (Contexts confined to a contiguous range of mask bits were tried and are gone:
// partitions run MFMA-bound kernels side by side at full rate, but the latency-bound panel chain of one instance slows ~2x next
// to the updates of the others -- every partition has CUs on every XCD and shares all L2s -- so 16 instances per GPU run faster
// time-sharing the whole chip, bench.py --batch, than on 2/4/8 partitions: 72 vs 58/45/26 it/s; tools/partition_probe.py.)
int mnk_ctx_create(int device, void* stream, mnk_ctx** out) {
    MNK_REQUIRE(out != nullptr, "mnk_ctx_create: out is NULL");
    mnk::LaunchLock lock;   // (stream / event creation: not between two launches of another thread's persistent group)
    int ndev = 0;
    MNK_HIP(hipGetDeviceCount(&ndev));
    MNK_REQUIRE(device >= 0 && device < ndev, "mnk_ctx_create: no such device");
    MNK_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MNK_HIP(hipGetDeviceProperties(&prop, device));
    mnk_ctx* c = new mnk_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        MNK_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    // The pair of the task-DAG schedule -- a handful of CUs for the pivot chain (two per XCD), the rest for the bulk kernel -- is
    // made with the first context of a device (and again on demand after a release: mnk_ctx_stream_pair); the others when a
    // caller first needs them (PAIR_DEEP, PAIR_BATCH, PAIR_SMALL; the look-ahead pair: mnk_ctx_ensure_panel_streams).
    if (c->num_cu >= DAG_MIN_CUS) {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        auto& pairs = g_pairs[device & 63];
        if (pairs.find({PAIR_DAG, 0}) == pairs.end()) {   // (a pair that could not be made is not tried again with every context)
            const int want = getenv("MNK_DAG_CUS") ? atoi(getenv("MNK_DAG_CUS")) : DAG_CUS_DEFAULT;
            (void)make_pair(PAIR_DAG, c->num_cu, stream_split(PAIR_DAG, c->num_cu, want, 0, 0), pairs[{PAIR_DAG, 0}]);
        }
        g_ctx_list[device & 63].push_back(c);
        c->dag_cus = pairs[{PAIR_DAG, 0}].chain_cus;
        const int want2 = getenv("MNK_DAG_CUS2") ? atoi(getenv("MNK_DAG_CUS2")) : DAG_CUS2_DEFAULT;
        c->dag_cus2 = stream_split(PAIR_DEEP, c->num_cu, c->dag_cus, want2, 0).exists ? want2 : 0;
    }
    MNK_HIP(hipEventCreateWithFlags(&c->ev_a, hipEventDisableTiming));
    MNK_HIP(hipEventCreateWithFlags(&c->ev_b, hipEventDisableTiming));
    if (mnk_solve_warmup(c->stream) != 0) (void)hipGetLastError();   // (the context's own stream runs the last inverses of every factorization)
    g_live_ctx[device & 63].fetch_add(1, std::memory_order_relaxed);
    *out = c;
    return 0;
}

int mnk_ctx_destroy(mnk_ctx* c) {
    if (!c) return 0;
    {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        if (c->children > 0) {  // a solver / KKT handle still points here: the last of them frees the context
            c->released = true;
            return 0;
        }
    }
    ctx_free(c);
    return 0;
}

int mnk_ctx_synchronize(mnk_ctx* c) {
    MNK_REQUIRE(c != nullptr, "ctx is NULL");
    MNK_HIP(mnk::stream_wait(c->stream));
    return 0;
}

void* mnk_ctx_stream(mnk_ctx* c) { return c ? (void*)c->stream : nullptr; }

}  // extern "C"

// Batches of independent factorizations (mnk_factorize_batch_begin / _end; BASELINE config C5: scenario batches per GPU).
// A single factorization of N ~ 1e4 leaves the bulk CUs nearly idle at both ends -- 0.5 ms of start-up and ~2.6 ms of a
// tail that is bound by the pivot chain -- which no schedule of ONE matrix can fill.  Between begin and end the
// factorize! calls of the calling thread only transfer their matrices; `end` launches them together: ONE bulk kernel
// drains the merged task queue of all instances (dag_plan.h: dag_merge_tasks) beside TWO pivot chains on two CU partitions (even
// instances on one, odd ones on the other), so that instance i + 1's saturated middle runs under instance i's tail.  The
// arithmetic per instance is exactly that of a single factorization (same task list, same order per tile): bit-identical
// factors.  Reference behaviour: distinct solver instances are driven concurrently (src/KKT/Schur/schur.jl:953).
// The kernels and their launchers are dag.hip's (declared in ls.h).
#include <algorithm>
#include <vector>

#include "ls.h"

using namespace mnk;

namespace {
struct BatchState {
    int depth = 0;             // (begin / end pairs nest: the outermost end launches)
    bool active = false;
    std::vector<mnk_ls*> pend;
};
thread_local BatchState t_batch;

struct BatchBuffers {   // per device, reused from batch to batch (guarded by the arbiter's mutex while in use)
    mnk::DevBuf<int> tasks;
    mnk::DevBuf<int> qctr;
    mnk::DevBuf<char> insts, pcsys, aux;
    char* stage = nullptr;        // pinned host memory: the records of one batch (instances | chain table | small-system records)
    size_t stage_bytes = 0;
    hipEvent_t stage_ev = nullptr;   // recorded behind the last upload from `stage` ...
    hipStream_t stage_on = nullptr;  // ... on this stream, which it must not outlive (mnk_batch_stream_gone)
    int ntile = 0, ninst = 0, period = 0, ntasks = 0;   // what `tasks` was merged for: ntile, the instances, their shift ...
    DagPlan::Key key;                                   // ... and the plan of the group's first solver
    bool holds(int ntile_, int ninst_, int period_, const DagPlan::Key& k) const {
        return tasks.p && ntile == ntile_ && ninst == ninst_ && period == period_ && key == k;
    }
    // `tasks` holds the merged queue of `ninst_` instances of `list`, shifted by `period_`: kept from batch to batch, merged and
    // uploaded when the last batch wanted another one.  The limits of the task's fields cannot be exceeded by an order the schedule
    // accepts (dag_max_rows: 240 tiles) or by solvers that fit a device; the single-factorization path falls back to one queue
    // instead, a merged queue has no such fallback.
    int hold_merged(const mnk::DagTaskList& list, int ntile_, int ninst_, int period_, const DagPlan::Key& k) {
        if (holds(ntile_, ninst_, period_, k)) return 0;
        MNK_REQUIRE(mnk::DagTask::fits(ntile_, ninst_, 0), "factorize batch: the merged queue does not fit the fields of a task");
        const mnk::DagTaskList merged = mnk::dag_merge_tasks(list, ninst_, period_);
        if (tasks.alloc(4 * merged.tasks.size() + 4)) return -2;
        { mnk::H2DGuard h2d; MNK_HIP(hipMemcpy(tasks.p, merged.tasks.data(), merged.tasks.size() * sizeof(mnk::DagTask), hipMemcpyHostToDevice)); }
        ntile = ntile_; ninst = ninst_; period = period_; key = k; ntasks = merged.size();
        return 0;
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int ensure_counter_and_events() {
        if (!qctr.p && qctr.alloc(4)) return -2;
        for (hipEvent_t& e : ev)
            if (!e) MNK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return 0;
    }
};
BatchBuffers g_batch[64];
}  // namespace

bool mnk_batch_active() { return t_batch.active; }

// ctx.hip calls this (launch mutex held) before it gives up a context's stream: the per-device staging event must not outlive the
// stream it was recorded on -- in a process whose contexts come and go hipEventSynchronize(stage_ev) answered "operation not permitted
// when stream is capturing" (nothing captures here; supposedly the destroyed stream behind the event) in every later round.
void mnk_batch_stream_gone(int device, hipStream_t s) {
    BatchBuffers& B = g_batch[device & 63];
    if (B.stage_ev == nullptr || B.stage_on != s) return;
    (void)hipEventSynchronize(B.stage_ev);
    (void)hipEventDestroy(B.stage_ev);
    B.stage_ev = nullptr;
}

bool mnk_batch_defer(mnk_ls* ls) {
    if (!t_batch.active) return false;
    const int nsc = (int)((ls->Np + 255) / 256);
    // (two merged launches: the large-system mode of the schedule -- band + bulk + two alternating chains -- and the small
    // one, every row in the chain's band, many chains side by side; a second phase in mid-factorization is simply run now)
    if (ls->algo_now != 5 || (ls->plan.key.js2 != nsc && ls->plan.key.js2 != 0) || ls->dag_trace_on) return false;
    hipStream_t spB = nullptr, suB = nullptr;
    if (mnk_ctx_stream_pair(ls->ctx, mnk::PAIR_BATCH, 0, &spB, &suB) != 0) (void)hipGetLastError();   // (made with the first batch of a process)
    if (!spB) return false;
    if (!ls->ev_defer && hipEventCreateWithFlags(&ls->ev_defer, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipEventRecord(ls->ev_defer, ls->ctx->stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    ls->deferred = true;
    t_batch.pend.push_back(ls);
    return true;
}

// the group's launches are queued on `h`: everybody's stream continues behind them, and every member is a queued factorization
static int batch_finish(std::vector<mnk_ls*>& g, hipStream_t h) {
    MNK_HIP(hipEventRecord(g[0]->ev_defer, h));
    for (mnk_ls* ls : g) {
        if (ls->ctx->stream != h) MNK_HIP(hipStreamWaitEvent(ls->ctx->stream, g[0]->ev_defer, 0));
        ls->verdict.queued();
        ls->deferred = false;
        int r = ls->spare.queued(ls);
        if (r) return r;
    }
    return 0;
}

// the merged launch of g.size() >= 2 deferred factorizations of one order / algorithm / option set on one device
static int batch_run_group(std::vector<mnk_ls*>& g) {
    mnk_ls* l0 = g[0];
    mnk_ctx* c0 = l0->ctx;
    hipStream_t h = c0->stream;
    MNK_HIP(hipSetDevice(c0->device));
    const int64_t Np = l0->Np;
    const bool ldl = l0->algo == MNK_LDL;
    const int ntile = (int)(Np / 128), nsc = (int)((Np + 255) / 256), ninst = (int)g.size();
    for (mnk_ls* ls : g)
        if (ls->ctx->stream != h) MNK_HIP(hipStreamWaitEvent(h, ls->ev_defer, 0));
    int rc = mnk_persist_begin(c0, h);
    if (rc) return rc;
    auto body = [&]() -> int {
        BatchBuffers& B = g_batch[c0->device & 63];
        const int period = (ntile + 1) / 2;   // shift between consecutive instances in the merged queue, in tile columns of chain position: half the matrix, the minimum
        // (a new queue comes with new instance records, allocated first: a failure leaves nothing that `holds`)
        if (!B.holds(ntile, ninst, period, l0->plan.key) && B.insts.alloc(sizeof(mnk::DagInst) * (size_t)ninst)) return -2;
        int r = B.hold_merged(l0->plan.list, ntile, ninst, period, l0->plan.key);
        if (!r) r = B.ensure_counter_and_events();
        if (r) return r;
        std::vector<mnk::DagInst> hin;
        mnk::DagInst* insts_dev = reinterpret_cast<mnk::DagInst*>(B.insts.p);
        for (mnk_ls* ls : g) {
            hin.push_back(mnk::dag_prepare_instance(ls, false));
            ls->envh_used = false;   // (the merged kernel of a batch skips by tiles only)
            mnk::dag_reset_member(h, ls, hin.back(), insts_dev + (hin.size() - 1));
        }
        MNK_HIP(hipMemsetAsync(B.qctr.p, 0, 4 * sizeof(int), h));
        // two chain partitions (the chain stream of PAIR_DAG, whose bulk stream idles here, and PAIR_BATCH's) and the bulk stream outside both
        hipStream_t sp[2] = {nullptr, nullptr}, su_dag = nullptr, su = nullptr;
        r = mnk_ctx_stream_pair(c0, mnk::PAIR_DAG, 0, &sp[0], &su_dag);
        if (!r) r = mnk_ctx_stream_pair(c0, mnk::PAIR_BATCH, 0, &sp[1], &su);
        if (r) return r;
        MNK_REQUIRE(sp[0] && sp[1], "factorize batch: the chain and bulk streams are missing");   // (mnk_batch_defer saw them)
        MNK_HIP(hipEventRecord(B.ev[0], h));
        MNK_HIP(hipStreamWaitEvent(sp[0], B.ev[0], 0));
        MNK_HIP(hipStreamWaitEvent(sp[1], B.ev[0], 0));
        MNK_HIP(hipStreamWaitEvent(su, B.ev[0], 0));
        const unsigned strips = (unsigned)std::min<int64_t>(l0->dag_band, Np / NBI);
        const int bulk_wgs = mnk::grid_at_launch(0, c0->num_cu, 2 * c0->dag_cus, 3);   // (the grid that is resident at launch: stream_plan.hip)
        // Launch order: the first two chains, THEN the bulk kernel, then everything else -- the host needs ~3 ms for the
        // 4 x ninst launches of the chains' streams (measured: the bulk kernel used to start 3 ms after the first chain,
        // 2 % of a 16-instance step).  Per chain stream: chain i, its inverses for the solves and its inertia / info words
        // (the next chain of the stream starts behind them; the bulk kernel has work of the other instance meanwhile).
        auto launch_chain = [&](int i) -> int {
            mnk_ls* ls = g[i];
            mnk::PpDag dag{hin[i].front, hin[i].af, ntile, 0, 0, -1, mnk_ls_dag_spin_limit(ls), nullptr, ls->bk.growth_word(ls)};
            return mnk_launch_pchain(ls, sp[i & 1], dag, 0, nsc, strips);
        };
        auto launch_tail = [&](int i) -> int {
            mnk_ls* ls = g[i];
            int r = mnk_ls_invert_blocks(ls, sp[i & 1], 0, nsc);
            if (r) return r;
            ls->inv_done = nsc;
            return mnk_ls_launch_finish_info(ls, sp[i & 1]);
        };
        for (int i = 0; i < std::min(2, ninst); ++i) {
            r = launch_chain(i);
            if (r) return r;
        }
        r = mnk::launch_dag_bulk_merged(su, ldl, insts_dev, B.tasks.p, B.ntasks, ntile, B.qctr.p, mnk_ls_dag_spin_limit(l0),
                                        std::min(B.ntasks, bulk_wgs));
        if (r) return r;
        for (int i = 0; i < ninst; ++i) {
            r = launch_tail(i);
            if (r) return r;
            if (i + 2 < ninst) {
                r = launch_chain(i + 2);
                if (r) return r;
            }
        }
        MNK_HIP(hipEventRecord(B.ev[1], sp[0]));
        MNK_HIP(hipEventRecord(B.ev[2], sp[1]));
        MNK_HIP(hipEventRecord(B.ev[3], su));
        for (int e = 1; e < 4; ++e) MNK_HIP(hipStreamWaitEvent(h, B.ev[e], 0));
        return 0;
    };
    rc = body();
    rc = mnk_persist_end(c0, h, rc);
    if (rc) return rc;
    return batch_finish(g, h);
}

// Small systems (every row a strip of the chain, dag_js2 == 0): rounds of K systems whose chains run SIDE BY SIDE in one
// launch (factor.hip: pchain_multi_kernel) on K * strips CUs, the band tiles of all of them accumulated by one bulk
// launch on the other CUs (systems of up to 768 rows have no bulk task at all).  A system this small is bound by its own
// pivot chain from the first column on -- 0.9 ms for N = 2048 on the whole chip, of which it uses 32 CUs.
static int batch_run_group_small(std::vector<mnk_ls*>& g) {
    mnk_ls* l0 = g[0];
    mnk_ctx* c0 = l0->ctx;
    hipStream_t h = c0->stream;
    MNK_HIP(hipSetDevice(c0->device));
    const int64_t Np = l0->Np;
    const bool ldl = l0->algo == MNK_LDL;
    const int ntile = (int)(Np / 128), nsc = (int)((Np + 255) / 256), strips = (int)(Np / NBI);
    const int ntasks1 = l0->plan.list.size();   // (single phase: all tasks)
    // (chain partitions of a round and the most systems it takes beside the bulk kernel's CUs: stream_plan.hip)
    const int kmax = mnk::small_rounds(strips, c0->num_cu, ntasks1 > 0).kmax;
    if (kmax < 2) {   // (no room for two chains: one after the other, as without a batch)
        for (mnk_ls* ls : g) {
            ls->deferred = false;
            int rc = mnk_ls_run_factorization_now(ls);
            if (rc) return rc;
        }
        return 0;
    }
    for (mnk_ls* ls : g)
        if (ls->ctx->stream != h) MNK_HIP(hipStreamWaitEvent(h, ls->ev_defer, 0));
    BatchBuffers& B = g_batch[c0->device & 63];
    for (size_t r0 = 0; r0 < g.size(); r0 += (size_t)kmax) {
        const int k = (int)std::min<size_t>(kmax, g.size() - r0);
        hipStream_t sp = nullptr, su = nullptr;
        const int chain_cus = mnk::small_chain_cus(k, strips, c0->num_cu);
        int rc = mnk_ctx_stream_pair(c0, mnk::PAIR_SMALL, chain_cus, &sp, &su);
        if (rc) return rc;
        MNK_REQUIRE(sp != nullptr, "factorize batch: bad size of the chains' CU partition");
        if (ntasks1 > 0 && su == nullptr) { set_error("factorize batch: no CUs left for the bulk kernel"); return -1; }
        rc = mnk_persist_begin(c0, h);
        if (rc) return rc;
        auto body = [&]() -> int {
            int r = ntasks1 > 0 ? B.hold_merged(l0->plan.list, ntile, k, 0, l0->plan.key) : 0;
            if (!r) r = B.ensure_counter_and_events();
            if (r) return r;
            if (B.insts.n < sizeof(mnk::DagInst) * (size_t)k && B.insts.alloc(sizeof(mnk::DagInst) * (size_t)std::max(k, 32))) return -2;
            if (B.pcsys.n < mnk_pchain_sys_bytes() * (size_t)k && B.pcsys.alloc(mnk_pchain_sys_bytes() * (size_t)std::max(k, 32))) return -2;
            // The records of this round (instances for the bulk kernel, the chains' table, what the kernels around them
            // need) go through pinned host memory in ONE piece each: a kernel launch per record and per small kernel made the
            // host the bound of a batch of many small systems (~8 launches per system).
            std::vector<mnk::DagInst> hin;
            mnk::DagInst* insts_dev = reinterpret_cast<mnk::DagInst*>(B.insts.p);
            const size_t pc_bytes = mnk_pchain_sys_bytes();
            const size_t need = (size_t)k * (sizeof(mnk::DagInst) + pc_bytes + sizeof(mnk::SmallSysRec));
            if (B.aux.n < sizeof(mnk::SmallSysRec) * (size_t)k && B.aux.alloc(sizeof(mnk::SmallSysRec) * (size_t)std::max(k, 32))) return -2;
            if (B.stage_ev == nullptr) MNK_HIP(hipEventCreateWithFlags(&B.stage_ev, hipEventDisableTiming));
            else MNK_HIP(hipEventSynchronize(B.stage_ev));   // (the previous round's uploads have left the staging memory)
            if (B.stage_bytes < need) {
                mnk::LaunchLock lock;
                if (B.stage) { mnk::quiesce_persistent(); (void)hipHostFree(B.stage); B.stage = nullptr; }
                const size_t cap = (size_t)std::max(k, 32) * (sizeof(mnk::DagInst) + pc_bytes + sizeof(mnk::SmallSysRec));
                MNK_HIP(hipHostMalloc((void**)&B.stage, cap, hipHostMallocDefault));
                B.stage_bytes = cap;
            }
            mnk::DagInst* st_inst = reinterpret_cast<mnk::DagInst*>(B.stage);
            char* st_pc = B.stage + (size_t)k * sizeof(mnk::DagInst);
            mnk::SmallSysRec* st_aux = reinterpret_cast<mnk::SmallSysRec*>(st_pc + (size_t)k * pc_bytes);
            const bool batch_aux = mnk::solve_inverses_batchable(l0->solves.linv_mfma != 0, l0->solves.solve512 != 0);
            for (int i = 0; i < k; ++i) {
                mnk_ls* ls = g[r0 + i];
                hin.push_back(mnk::dag_prepare_instance(ls, true));   // (batches of small systems run dense: their bulk tasks only accumulate band tiles)
                st_inst[i] = hin.back();
                mnk_pchain_fill_sys(ls, st_pc + (size_t)i * pc_bytes, hin.back().front, hin.back().af);
                mnk_ls_fill_small_rec(ls, st_aux + i);
            }
            MNK_HIP(hipMemcpyAsync(B.insts.p, st_inst, (size_t)k * sizeof(mnk::DagInst), hipMemcpyHostToDevice, h));
            MNK_HIP(hipMemcpyAsync(B.pcsys.p, st_pc, (size_t)k * pc_bytes, hipMemcpyHostToDevice, h));
            MNK_HIP(hipMemcpyAsync(B.aux.p, st_aux, (size_t)k * sizeof(mnk::SmallSysRec), hipMemcpyHostToDevice, h));
            MNK_HIP(hipEventRecord(B.stage_ev, h));
            B.stage_on = h;
            const mnk::SmallSysRec* aux_dev = reinterpret_cast<const mnk::SmallSysRec*>(B.aux.p);
            mnk::dag_reset_round(h, Np, aux_dev, k);
            MNK_HIP(hipMemsetAsync(B.qctr.p, 0, 4 * sizeof(int), h));
            MNK_HIP(hipEventRecord(B.ev[0], h));
            MNK_HIP(hipStreamWaitEvent(sp, B.ev[0], 0));
            if (su != nullptr) MNK_HIP(hipStreamWaitEvent(su, B.ev[0], 0));
            // (the records of the chains' table are written on the home stream before the fork)
            r = mnk_launch_pchain_multi(g.data() + r0, k, sp, B.pcsys.p);
            if (r) return r;
            if (ntasks1 > 0) {
                const int bulk_wgs = mnk::grid_at_launch(0, c0->num_cu, chain_cus, 3);
                r = mnk::launch_dag_bulk_merged(su, ldl, insts_dev, B.tasks.p, B.ntasks, ntile, B.qctr.p, mnk_ls_dag_spin_limit(l0),
                                                std::min(B.ntasks, bulk_wgs));
                if (r) return r;
                MNK_HIP(hipEventRecord(B.ev[2], su));
                MNK_HIP(hipStreamWaitEvent(h, B.ev[2], 0));
            }
            MNK_HIP(hipEventRecord(B.ev[1], sp));
            MNK_HIP(hipStreamWaitEvent(h, B.ev[1], 0));
            if (su != nullptr) MNK_HIP(hipStreamWaitEvent(su, B.ev[1], 0));   // (all chains done: every system's factor is final)
            if (su != nullptr) MNK_HIP(hipStreamWaitEvent(sp, B.ev[2], 0));
            // inverses for the solves, inertia / info words: small latency-bound kernels, spread over the three streams
            if (batch_aux) {
                // ONE launch each for all systems of the round: 64 x 64 inverses, 256 x 256 inverses, inertia / info words
                r = mnk_ls_invert_blocks_batch(h, ldl, aux_dev, k, Np);
                if (r) return r;
                r = mnk_ls_finish_info_batch(h, aux_dev, k, ldl ? (l0->N >= 4096 ? 1024 : 256) : 64);
                if (r) return r;
                for (int i = 0; i < k; ++i) {
                    mnk_ls* ls = g[r0 + i];
                    ls->inv_done = nsc;
                    r = ls->verdict.record_info_event(h);
                    if (r) return r;
                }
                return 0;
            }
            hipStream_t inv_s[3] = {h, sp, su != nullptr ? su : sp};
            for (int i = 0; i < k; ++i) {
                mnk_ls* ls = g[r0 + i];
                hipStream_t si = inv_s[i % 3];
                r = mnk_ls_invert_blocks(ls, si, 0, nsc);
                if (r) return r;
                ls->inv_done = nsc;
                r = mnk_ls_launch_finish_info(ls, si);
                if (r) return r;
            }
            MNK_HIP(hipEventRecord(B.ev[1], sp));
            MNK_HIP(hipStreamWaitEvent(h, B.ev[1], 0));
            if (su != nullptr) {
                MNK_HIP(hipEventRecord(B.ev[2], su));
                MNK_HIP(hipStreamWaitEvent(h, B.ev[2], 0));
            }
            return 0;
        };
        rc = body();
        rc = mnk_persist_end(c0, h, rc);
        if (rc) return rc;
    }
    return batch_finish(g, h);
}

static int batch_flush() {
    std::vector<mnk_ls*> pend;
    pend.swap(t_batch.pend);
    int rc_all = 0;
    while (!pend.empty()) {
        // group: same device, order, algorithm and schedule options as the first one pending
        mnk_ls* l0 = pend.front();
        std::vector<mnk_ls*> g, rest;
        for (mnk_ls* ls : pend) {
            const bool same = ls->ctx->device == l0->ctx->device && ls->Np == l0->Np && ls->algo == l0->algo && ls->plan.key == l0->plan.key;
            (same && std::find(g.begin(), g.end(), ls) == g.end() ? g : rest).push_back(ls);
        }
        pend.swap(rest);
        int rc;
        if (g.size() >= 2) {
            rc = l0->plan.key.js2 == 0 ? batch_run_group_small(g) : batch_run_group(g);
            if (rc)   // (nothing of the group counts as factorized: the factor buffers already hold the NEW, unfactored matrices, so
                      // a solve or an inertia call that ignores this error must not find the previous factorization's flag)
                for (mnk_ls* ls : g) { ls->deferred = false; ls->verdict.launch_failed(); }
        } else {
            g[0]->deferred = false;
            if (g[0]->Np < g[0]->dag_min_rows) g[0]->algo_now = 4;   // (alone, a system below the schedule's window keeps its usual one)
            rc = mnk_ls_run_factorization_now(g[0]);
            if (rc) g[0]->verdict.launch_failed();
        }
        if (rc && !rc_all) rc_all = rc;
    }
    return rc_all;
}

int mnk_ls_sync_deferred(mnk_ls* ls) {
    {   // (queued solves of this solver run before anything else touches it)
        int rc_s = mnk_solve_sync_deferred(ls);
        if (rc_s) return rc_s;
    }
    return mnk_ls_sync_deferred_fact(ls);
}

// true: a factorize! call of this solver is queued in a batch that ANOTHER thread opened (its thread-local list holds the pointer)
bool mnk_ls_pending_elsewhere(const mnk_ls* ls) {
    return ls->deferred && std::find(t_batch.pend.begin(), t_batch.pend.end(), ls) == t_batch.pend.end();
}

int mnk_ls_sync_deferred_fact(mnk_ls* ls) {
    if (!ls->deferred) return 0;
    if (std::find(t_batch.pend.begin(), t_batch.pend.end(), ls) == t_batch.pend.end()) {
        set_error("a factorize! call of this solver is pending in a batch that another thread opened (mnk_factorize_batch_end must come first)");
        return -1;
    }
    return batch_flush();   // (the batch stays open: later factorize! calls form the next group)
}

extern "C" int mnk_factorize_batch_begin(void) {
    ++t_batch.depth;
    t_batch.active = true;
    return 0;
}

extern "C" int mnk_factorize_batch_end(void) {
    if (t_batch.depth <= 0) { set_error("mnk_factorize_batch_end: no batch is open on this thread"); return -1; }
    if (--t_batch.depth > 0) return 0;
    t_batch.active = false;
    return batch_flush();
}

// The planner of the task-DAG schedule (dag_plan.h): task lists, their merge for a batch, the deal into per-XCD queues, the
// statistics counted from a list, and the host-only entries through which the tests and tools read all of it.  Plain C++.
#include "dag_plan.h"

#include <algorithm>

#include "../../include/madnlp_hip.h"

namespace mnk {

int dag_choose_js2(int64_t Np, int cus2, int64_t deep_rows, int js2_override) {
    const int64_t nsc = (Np + 255) / 256;
    if (cus2 <= 0) return (int)nsc;
    int64_t js2 = Np <= std::min<int64_t>(64 * (int64_t)cus2, deep_rows) ? 0 : nsc;
    if (js2_override >= 0) js2 = std::min<int64_t>(nsc, js2_override);
    // (Np - 256 js2) / 64 strips of the deep band on cus2 CUs
    const int64_t over = Np - 64 * (int64_t)cus2;
    const int64_t least = over > 0 ? std::min(nsc, (over + 255) / 256) : 0;
    return (int)std::max(js2, least);
}

// The tasks come in the order of the queue: sorted by the chain position at which they become ready (the last tile column they
// read), band tiles and rows next to the band first.
DagTaskList dag_build_tasks(int ntile, int chunk, int band_tiles, int js2, int taper0) {
    struct T { int ready, cls, J, I, flags, q, kbeg, kend; };
    std::vector<T> ts;
    // Tile (I, J), tile columns [0, K) to accumulate.  A bulk tile's last tile column is a task of its own (paced by the pivot
    // chain: K = 128 step, then the finalization); the columns in front of it -- all columns of a band tile -- go in chunks:
    //   * STAGGERED from tile to tile (first chunk 1 .. chunk tile columns long, by a hash of the tile's coordinates): at
    //     every chain position about 1 / chunk of the tiles have a chunk that just became ready, so ready work arrives
    //     evenly.  (With boundaries at multiples of `chunk` the queue alternated between a big batch of ready chunks and a
    //     stretch of tile-closing tasks that are serialized along every row of tiles: 23 % of the slot-time waiting.)
    //   * TAPERED towards K (..., chunk, 4, 2, 1): a chunk [b, e) cannot start before the chain has passed tile column
    //     e - 1 and the tile is due when the chain reaches K, so a full-length chunk that becomes ready one chain step
    //     before the tile is due was 100-300 us late for the band, every time (measured).
    auto add_tile = [&](int I, int J, int K, bool band) {
        const int body = band ? K : std::max(0, K - 1);
        std::vector<int> cuts{body};  // chunk boundaries, back to front
        int e = body;
        for (int len = taper0; len < chunk && e > 0; len *= 2) { e = std::max(0, e - len); cuts.push_back(e); }   // (factors 3 / 4 instead of 2: +2 / +5 %)
        const int first = 1 + (I * 5 + J * 3) % chunk;
        while (e > first) { e = std::max(first, e - chunk); cuts.push_back(e); }
        if (e > 0) cuts.push_back(0);
        int q = 0;
        for (int c = (int)cuts.size() - 1; c > 0; --c, ++q) {
            const int kb = cuts[c], ke = cuts[c - 1];
            const bool last = band && ke == K;
            ts.push_back({ke, band ? 0 : 2, J, I, (band ? DAG_BANDACC : 0) | (last ? DAG_FINAL : 0) | (q == 0 ? DAG_FIRST : 0), q, kb, ke});
        }
        if (!band) ts.push_back({K, 1, J, I, DAG_FINAL | (q == 0 ? DAG_FIRST : 0), q, body, K});
    };
    for (int Jt = 0; Jt < ntile; ++Jt) {
        const int Js = Jt / 2;
        const int bt = Js >= js2 ? ntile : band_tiles;
        for (int I = 2 * Js + bt; I < ntile; ++I) add_tile(I, Jt, Jt, false);
        // band tiles of strip-column Js (tile rows 2Js .. 2Js + bt - 1, lower part): accumulated over the tile columns
        // k < 2Js - 2 (the chain's prologue applies strip-column Js - 1 itself)
        if (2 * Js - 2 > 0)
            for (int I = std::max(2 * Js, Jt); I < 2 * Js + bt && I < ntile; ++I) add_tile(I, Jt, 2 * Js - 2, true);
    }
    // by the chain position that makes a task ready (the last tile column it reads), then band tiles, then the tile-closing
    // tasks, then by column and row (rows next to the band first)
    std::stable_sort(ts.begin(), ts.end(), [](const T& x, const T& y) {
        if (x.ready != y.ready) return x.ready < y.ready;
        if (x.cls != y.cls) return x.cls < y.cls;
        if (x.J != y.J) return x.J < y.J;
        return x.I < y.I;
    });
    DagTaskList out;
    out.tasks.reserve(ts.size());
    out.ready.reserve(ts.size());
    for (const T& t : ts) {
        if (t.ready <= 2 * js2) ++out.n1;  // needs only tile columns the first phase's chain has passed (sorted by `ready`)
        out.ready.push_back(t.ready);
        out.tasks.push_back(DagTask::built(t.flags, t.q, t.I, t.J, t.kbeg, t.kend));
    }
    return out;
}

// Zero-fill tasks (DAG_FILL) for the lower tiles of the NEXT factorization's buffer, one after every few tasks of the first
// phase: 128 KB of stores each, absorbed by the queue while the matrix cores are the bound.  `ready` gets the value of the
// task in front (the merge of several instances keeps them where they are).
void dag_add_fill_tasks(int ntile, DagTaskList& list) {
    const int nt = list.size(), nfill = ntile * (ntile + 1) / 2;
    const int span = list.n1 > 0 ? list.n1 : nt;   // (spread over the first phase; a list without one: over everything)
    if (span <= 0) return;
    DagTaskList out;
    out.tasks.reserve((size_t)nt + nfill);
    out.ready.reserve((size_t)nt + nfill);
    int fi = 0, fj = 0, done = 0;
    for (int t = 0; t < nt; ++t) {
        out.tasks.push_back(list.tasks[t]);
        out.ready.push_back(list.ready[t]);
        // after task t of the span, (t + 1) * nfill / span fill tasks are out
        if (t < span)
            for (; done < (int)((int64_t)(t + 1) * nfill / span); ++done) {
                out.tasks.push_back(DagTask::built(DAG_FILL, 0, fi, fj, 0, 0));
                out.ready.push_back(list.ready[t]);
                if (++fi >= ntile) { ++fj; fi = fj; }
            }
    }
    out.n1 = list.n1 > 0 ? list.n1 + nfill : 0;
    list = std::move(out);
}

// One queue for `ninst` independent factorizations of the same order (mnk_factorize_batch_*): instance i's tasks keep their
// order and are shifted by i * period chain positions (tile columns) against instance 0's, so that an instance's
// saturated middle runs under the chain-bound ends of its neighbours.  Two pivot chains run at a time (instances i and
// i + 1; chain i + 2 follows chain i on its stream), hence period >= ntile / 2: every task of instance i then precedes
// every task of instance i + 2, and a workgroup that holds a task waits only for tasks in front of it or for a chain that
// is running or will run once tasks in front of it are done.
DagTaskList dag_merge_tasks(const DagTaskList& list, int ninst, int period) {
    const int nt = list.size();
    DagTaskList out;
    out.tasks.reserve((size_t)ninst * nt);
    out.ready.reserve((size_t)ninst * nt);
    std::vector<int> pos(ninst, 0);
    for (;;) {   // k-way merge by (i * period + ready, i); every list is sorted by `ready`
        int best = -1;
        long bkey = 0;
        for (int i = 0; i < ninst; ++i) {
            if (pos[i] >= nt) continue;
            const long key = (long)i * period + list.ready[pos[i]];
            if (best < 0 || key < bkey) { best = i; bkey = key; }
        }
        if (best < 0) break;
        out.tasks.push_back(list.tasks[pos[best]++].with_instance(best));
        out.ready.push_back((int)bkey);
    }
    out.n1 = out.size();
    return out;
}

// Per-XCD queues.  Neighbours in the list are chunks of one tile column with the same [kbeg, kend): they walk the same B rows
// V(J, kbeg..kend).  Popped from one counter by workgroups that the dispatcher deals round-robin over the eight XCDs, they land in
// eight different L2s; dealt to the queue of ONE XCD they can share that stream.  The list is only PARTITIONED: every queue is a
// subsequence of the list in list order and no task changes, so every tile still sees its chunks in the same order (same bits),
// and a queue popped from its head keeps the list's progress argument.
//   * group: a maximal run of consecutive chunk tasks (body chunks, band accumulation) with the same (ready, class, J, kbeg, kend);
//     it is cut into gangs of `gang` consecutive tasks.  Tile-closing tasks, zero-fill tasks and runs of one are gangs of one.
//   * a gang goes whole to the queue with the fewest k-steps dealt so far (ties: round-robin), so the queues carry equal work at
//     every position of the list: the heaviest and the lightest differ by at most one gang.
// The envelope is ignored (gang-mates whose K-loops start later join the shared stream later): one deal serves every matrix of an order.
// (Balancing the queues by the K-loop lengths under the envelope, kend - max(kbeg, env[I], env[J]), was measured on C3 and is not
// built: 9.101 against 9.080 ms per step)
void dag_deal_tasks(const DagTaskList& list, int t0, int t1, int nq, int gang, std::vector<int>& order, std::vector<int>& off) {
    nq = std::max(nq, 1);
    const std::vector<DagTask>& tk = list.tasks;
    std::vector<std::vector<int>> qs(nq);
    std::vector<int64_t> load(nq, 0);
    int rr = 0;
    auto cls = [&](int t) { return tk[t].fill() ? 3 : ((tk[t].flags() & DAG_BANDACC) ? 0 : ((tk[t].flags() & DAG_FINAL) ? 1 : 2)); };
    auto same = [&](int x, int y) {   // (the instance too: a merged list carries it)
        return list.ready[x] == list.ready[y] && cls(x) == cls(y) && tk[x].J() == tk[y].J() && tk[x].kbeg() == tk[y].kbeg() &&
               tk[x].kend() == tk[y].kend() && tk[x].instance() == tk[y].instance();
    };
    auto deal = [&](int b, int e) {   // the gang [b, e)
        int q = 0;
        if (gang >= 0) {
            q = rr % nq;
            for (int i = 1; i < nq; ++i)
                if (load[(rr + i) % nq] < load[q]) q = (rr + i) % nq;
            rr = q + 1;
        }
        for (int t = b; t < e; ++t) { qs[q].push_back(t); load[q] += tk[t].ksteps(); }
    };
    for (int i = t0; i < t1;) {
        int j = i + 1;
        const int c = cls(i);
        if (gang > 1 && (c == 0 || c == 2))
            while (j < t1 && same(i, j)) ++j;
        for (int b = i; b < j; b += std::max(gang, 1)) deal(b, std::min(j, b + std::max(gang, 1)));
        i = j;
    }
    order.clear();
    off.assign(1, 0);
    for (int q = 0; q < nq; ++q) {
        order.insert(order.end(), qs[q].begin(), qs[q].end());
        off.push_back((int)order.size());
    }
}

// The host list stays as built (the statistics and the merged queue of a batch read it); this is the copy for the device.
DagDealtList dag_deal_list(const DagTaskList& list, int nq, int gang, const bool may_queue[2]) {
    DagDealtList out;
    out.tasks = list.tasks;
    out.order.resize(list.tasks.size());
    for (int t = 0; t < list.size(); ++t) out.order[t] = t;
    out.qoff.assign(2 * ((size_t)std::max(nq, 1) + 1), 0);
    const int part[3] = {0, list.n1, list.size()};
    for (int ph = 0; ph < 2; ++ph) {
        if (!may_queue[ph]) continue;
        const int t0 = part[ph], t1 = part[ph + 1];
        std::vector<int> order, off;
        dag_deal_tasks(list, t0, t1, nq, gang, order, off);
        for (int p = 0; p < t1 - t0; ++p) out.tasks[(size_t)t0 + p] = list.tasks[order[p]].with_list_pos(order[p] - t0);
        std::copy(order.begin(), order.end(), out.order.begin() + t0);
        std::copy(off.begin(), off.end(), out.qoff.begin() + ph * (off.size()));
        out.nq[ph] = std::max(nq, 1);
    }
    return out;
}

void dag_env_count(const DagTaskList& list, const int* env, int nenv, int64_t* count) {
    count[0] = count[1] = 0;
    for (const DagTask& t : list.tasks) {
        if (t.fill()) continue;
        count[0] += t.ksteps();
        if (env == nullptr || t.I() >= nenv || t.J() >= nenv) continue;
        count[1] += std::min(t.kend(), std::max(t.kbeg(), std::max(env[t.I()], env[t.J()]))) - t.kbeg();
    }
}

// Half-tile k-steps: one 64 x 64 quadrant of a tile over 64 columns, 8 per 128-column k-step of a tile.  count[0]: what the tile
// envelope leaves (NULL: everything); count[1]: of that, what the waves of dag_bulk_kernel1 skip with the half-tile envelope -- in
// a chunk's K-loop the quadrant (r, c) of tile (I, J) starts at max(envh[2I + r], envh[2J + c]), and the upper quadrant of a
// diagonal tile is never multiplied.  Tile-closing tasks skip nothing by halves.
void dag_envh_count(const DagTaskList& list, const int* env, const int* envh, int nenv, int64_t* count) {
    count[0] = count[1] = 0;
    for (const DagTask& t : list.tasks) {
        const int I = t.I(), J = t.J(), kb = t.kbeg(), ke = t.kend();
        if (t.fill()) continue;
        const bool in = env != nullptr && I < nenv && J < nenv;
        const int k0 = in ? std::min(ke, std::max(kb, std::max(env[I], env[J]))) : kb;
        if (in && t.closes_tile() && J < env[I]) continue;   // (a structurally zero tile is closed without its K-step)
        count[0] += 8 * (int64_t)(ke - k0);
        if (!in || envh == nullptr || t.closes_tile()) continue;
        for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 2; ++c) {
                const int h0 = (I == J && r == 0 && c == 1) ? 2 * ke : std::max(envh[2 * I + r], envh[2 * J + c]);
                count[1] += std::min(2 * ke, std::max(2 * k0, h0)) - 2 * k0;
            }
    }
}

}  // namespace mnk

// ---- diagnostics / tests (include/madnlp_hip.h): host only, no device needed.  Tasks go out as the bulk kernels read them, four
// ints each; at most `cap` are written and the number of tasks is returned. ----
namespace {
bool plan_args_ok(int ntile, int chunk, int band_tiles, int taper0) { return ntile > 0 && chunk > 0 && band_tiles > 0 && taper0 > 0; }

mnk::DagTaskList plan_list(int ntile, int chunk, int band_tiles, int js2, int taper0, int fill, int ninst, int period) {
    mnk::DagTaskList list = mnk::dag_build_tasks(ntile, chunk, band_tiles, js2, taper0);
    if (fill) mnk::dag_add_fill_tasks(ntile, list);
    return ninst > 1 ? mnk::dag_merge_tasks(list, ninst, period) : list;
}

int plan_write(const mnk::DagTaskList& list, int* out, int cap) {
    if (out != nullptr)
        for (int t = 0; t < std::min(list.size(), cap); ++t) std::copy(list.tasks[t].word, list.tasks[t].word + 4, out + 4 * (size_t)t);
    return list.size();
}
}  // namespace

// js2 of a factorization of padded order Np (dag_choose_js2) on a context with `dag_cus2` deep-band CUs, under the options
// dag_deep_rows and dag_js2 (`js2_override`; negative: by size).
extern "C" int mnk_debug_dag_js2(int64_t Np, int dag_cus2, int64_t dag_deep_rows, int js2_override) {
    if (Np <= 0 || Np % 64 != 0 || dag_cus2 < 0 || dag_deep_rows < 0) return -1;
    return mnk::dag_choose_js2(Np, dag_cus2, dag_deep_rows, js2_override);
}

// The task list of one factorization; *first_phase receives the number of first-phase tasks.
extern "C" int mnk_debug_dag_tasks(int ntile, int chunk, int band_tiles, int js2, int taper0, int* out, int cap, int* first_phase) {
    if (!plan_args_ok(ntile, chunk, band_tiles, taper0)) return -1;
    const mnk::DagTaskList list = plan_list(ntile, chunk, band_tiles, js2, taper0, 0, 1, 0);
    if (first_phase != nullptr) *first_phase = list.n1;
    return plan_write(list, out, cap);
}

// The merged queue of `ninst` instances (with the zero-fill tasks if `fill`).
extern "C" int mnk_debug_dag_merged_tasks(int ntile, int chunk, int band_tiles, int js2, int taper0, int fill, int ninst, int period,
                                          int* out, int cap) {
    if (!plan_args_ok(ntile, chunk, band_tiles, taper0) || ninst <= 0 || period < 0) return -1;
    mnk::DagTaskList list = mnk::dag_build_tasks(ntile, chunk, band_tiles, js2, taper0);
    if (fill) mnk::dag_add_fill_tasks(ntile, list);
    return plan_write(mnk::dag_merge_tasks(list, ninst, period), out, cap);   // (merged also for one instance)
}

// The list above (merged over `ninst` > 1 instances with shift `period`: one phase) dealt into `nq` queues per phase as the
// single-factorization bulk kernel pops them (dag_deal_list; nq <= 1: the list itself).  order: the list positions, queue after
// queue -- the first phase's queues, then the second phase's; off: 2 x (nq + 1) offsets into `order`.  -2: the position packed
// into a dealt task is not the one it was dealt from (checked for every list that fits the task's fields).
extern "C" int mnk_debug_dag_deal(int ntile, int chunk, int band_tiles, int js2, int taper0, int fill, int ninst, int period, int nq,
                                  int gang, int* tasks_out, int* order, int cap, int* off, int* first_phase) {
    if (!plan_args_ok(ntile, chunk, band_tiles, taper0) || ninst <= 0 || period < 0 || nq <= 0 || nq > 64 || gang == 0) return -1;
    const mnk::DagTaskList list = plan_list(ntile, chunk, band_tiles, js2, taper0, fill, ninst, period);
    const int n = list.size();
    if (first_phase != nullptr) *first_phase = list.n1;
    const bool both[2] = {true, true};
    const mnk::DagDealtList dealt = mnk::dag_deal_list(list, nq, gang, both);
    const int part[3] = {0, list.n1, n};
    for (int ph = 0; ph < 2; ++ph) {
        for (int x = 0; x <= nq; ++x)
            if (off != nullptr) off[ph * (nq + 1) + x] = part[ph] + dealt.qoff[(size_t)ph * (nq + 1) + x];
        for (int t = part[ph]; t < part[ph + 1]; ++t) {
            if (mnk::DagTask::fits(ntile, ninst, n) && part[ph] + dealt.tasks[t].list_pos() != dealt.order[t]) return -2;
            if (order != nullptr && t < cap) order[t] = dealt.order[t];
        }
    }
    return plan_write(list, tasks_out, cap);
}

// The statistics envh_ksteps (count[0]) and envh_ksteps_skipped (count[1]) of the task list of `ntile` tiles under the tile
// envelope `env` (ntile entries) and the half-tile envelope `envh` (2 ntile entries; NULL: nothing skipped).
extern "C" int mnk_debug_envh_ksteps(int ntile, int chunk, int band_tiles, int js2, int taper0, const int* env, const int* envh, int64_t* count) {
    if (!plan_args_ok(ntile, chunk, band_tiles, taper0) || count == nullptr) return -1;
    const mnk::DagTaskList list = mnk::dag_build_tasks(ntile, chunk, band_tiles, js2, taper0);
    mnk::dag_envh_count(list, env, envh, ntile, count);
    return list.size();
}

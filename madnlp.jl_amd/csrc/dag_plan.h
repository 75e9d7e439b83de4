// The planner of the task-DAG schedule: the bulk task, the task list of one factorization, the merged list of a batch and
// the per-XCD queues a list is dealt into.  Host only and plain C++ -- no HIP header, no runtime call, no kernel -- so the unit
// (dag_plan.hip) also compiles with a host compiler and runs under its sanitizers (tools/dag_plan_check.cpp).  The kernels
// that execute the tasks are in dag.hip, the batches that merge lists in dag_batch.hip.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mnk {

constexpr int DAG_BANDACC = 1, DAG_FINAL = 2, DAG_FIRST = 4, DAG_FILL = 8;  // task flags

constexpr int DAG_NQ = 8;             // queues of the bulk kernel: one per XCD
constexpr int DAG_QHEAD_STRIDE = 32;  // ints between two queue heads (128 bytes)
constexpr int DAG_QHEAD_WORDS = (DAG_NQ + 1) * DAG_QHEAD_STRIDE;   // the heads of one launch and, behind them, its count of stolen tasks

// One bulk task: the four words the bulk kernels read as one int4 (dag.hip decodes them with the same widths).
//   word 0: flags (8 bits)       | chunk index of the task within its tile (24)
//   word 1: tile row I (16)      | instance of a merged list (16; 0 in the list of one factorization)
//   word 2: tile column J (12)   | position in the list (20; only in a list dealt into queues: the index of the trace record)
//   word 3: kbeg (16)            | kend (16): the tile columns [kbeg, kend) the task accumulates
// A task is BUILT with the lower fields, a merged list adds the instance, a dealt list the position.
struct DagTask {
    static constexpr int FLAG_BITS = 8, CHUNK_BITS = 24;
    static constexpr int ROW_BITS = 16, INST_BITS = 16;
    static constexpr int COL_BITS = 12, POS_BITS = 20;
    static constexpr int KBEG_BITS = 16, KEND_BITS = 16;
    int32_t word[4];

    static DagTask built(int flags, int chunk_index, int I, int J, int kbeg, int kend) {
        return DagTask{{flags | hi(chunk_index, FLAG_BITS), I, J, kbeg | hi(kend, KBEG_BITS)}};
    }
    DagTask with_instance(int i) const { DagTask t = *this; t.word[1] |= hi(i, ROW_BITS); return t; }
    DagTask with_list_pos(int p) const { DagTask t = *this; t.word[2] |= hi(p, COL_BITS); return t; }

    int flags() const { return lo(word[0], FLAG_BITS); }
    int chunk_index() const { return word[0] >> FLAG_BITS; }
    int I() const { return lo(word[1], ROW_BITS); }
    int instance() const { return word[1] >> ROW_BITS; }
    int J() const { return lo(word[2], COL_BITS); }
    int list_pos() const { return (int)((uint32_t)word[2] >> COL_BITS); }
    int kbeg() const { return lo(word[3], KBEG_BITS); }
    int kend() const { return word[3] >> KBEG_BITS; }
    bool fill() const { return (flags() & DAG_FILL) != 0; }
    bool closes_tile() const { return (flags() & DAG_FINAL) && !(flags() & DAG_BANDACC); }   // (the tile-closing task of a bulk tile)
    int ksteps() const { return fill() ? 0 : kend() - kbeg(); }

    // What the fields hold: `ntile` tile rows / columns (and with them every k and chunk index), `ninst` instances and
    // `npos` list positions.  The upper fields of words 0, 1 and 3 are read with an arithmetic shift: one bit less.
    static constexpr bool fits(int64_t ntile, int64_t ninst, int64_t npos) {
        return ntile < (1 << COL_BITS) && ninst <= (1 << (INST_BITS - 1)) && npos < (1 << POS_BITS);
    }

   private:
    static constexpr int32_t lo(int32_t w, int bits) { return w & (int32_t)((1u << bits) - 1); }
    static constexpr int32_t hi(int v, int shift) { return (int32_t)((uint32_t)v << shift); }
};
static_assert(sizeof(DagTask) == 16 && alignof(DagTask) == 4 && offsetof(DagTask, word) == 0, "a task is the int4 the bulk kernels read");
static_assert(DagTask::FLAG_BITS + DagTask::CHUNK_BITS == 32 && DagTask::ROW_BITS + DagTask::INST_BITS == 32 &&
                  DagTask::COL_BITS + DagTask::POS_BITS == 32 && DagTask::KBEG_BITS + DagTask::KEND_BITS == 32,
              "two fields per word");
static_assert(DagTask::COL_BITS < DagTask::ROW_BITS && DagTask::COL_BITS < DagTask::KEND_BITS && DagTask::COL_BITS < DagTask::CHUNK_BITS,
              "fits(): the tile column's field is the narrowest");

// A task list in the order of the queue: `ready[t]` is the chain position (tile column) that makes task t ready -- the list is
// sorted by it --, the first `n1` tasks are the first phase's (ready before the chain enters strip-column js2).
struct DagTaskList {
    std::vector<DagTask> tasks;
    std::vector<int> ready;
    int n1 = 0;
    int size() const { return (int)tasks.size(); }
};

// js2 of a factorization of padded order `Np` (a multiple of 64): the first strip-column (256 columns) of the second phase, from
// which every remaining row is a 64-row strip of the chain's deep band.  0: every row in the band from the first column on (orders
// up to `deep_rows` that fit the `cus2` CUs of the deep band's partition); nsc = ceil(Np / 256): band + bulk kernel throughout
// (also whenever cus2 == 0: there is no deep band); `js2_override` >= 0 (option dag_js2) asks for a strip-column in between.
// Every strip of the deep band needs a CU to itself and they wait on one another, so a request that would leave more than `cus2`
// strips to it is raised to the smallest admissible strip-column, ceil((Np - 64 cus2) / 256), capped at nsc.
int dag_choose_js2(int64_t Np, int cus2, int64_t deep_rows, int js2_override);

// The list of one factorization of `ntile` 128-row tiles: chunks of at most `chunk` tile columns, tapered from `taper0`; strip-
// columns Js < js2 have a band of `band_tiles` tile rows, the others a band that covers every remaining row.
DagTaskList dag_build_tasks(int ntile, int chunk, int band_tiles, int js2, int taper0);
// ... with the zero-fill tasks (DAG_FILL) of the next factorization's buffer spread over its first phase
void dag_add_fill_tasks(int ntile, DagTaskList& list);
// One list for `ninst` factorizations of the same order, instance i shifted by i * period chain positions: `ready` holds the
// keys of the merge (i * period + ready), everything is one phase.
DagTaskList dag_merge_tasks(const DagTaskList& list, int ninst, int period);
// The tasks [t0, t1) of a list dealt into `nq` queues, each a subsequence of the list in list order: `order` receives the list
// positions queue after queue, `off` the nq + 1 offsets of the queues in it.  `gang`: tasks of one group (same B rows, same k-range) that
// go to one queue together; 1: every task on its own; < 0: everything to queue 0 (tests of the steal path).
void dag_deal_tasks(const DagTaskList& list, int t0, int t1, int nq, int gang, std::vector<int>& order, std::vector<int>& off);

// The list as the single-factorization bulk kernel reads it: per phase either the list as built (nq[ph] == 0: one queue) or its
// tasks queue after queue, each with its position in the phase's part of the list riding in word 2.
struct DagDealtList {
    std::vector<DagTask> tasks;
    std::vector<int> order;  // the list position of every dealt task (tasks[t] is the list's task order[t])
    std::vector<int> qoff;   // 2 x (nq + 1): the queues' offsets in the phase's part (zeros for a phase with one queue)
    int nq[2] = {0, 0};
};
// `may_queue[ph]`: the phase's bulk grid has a workgroup on every one of `nq` XCDs, and the list fits the fields of a task
// (DagTask::fits with its length: a longer list is dealt all the same, but the positions in `tasks` are then cut short).
DagDealtList dag_deal_list(const DagTaskList& list, int nq, int gang, const bool may_queue[2]);

// Statistics of a list under the tile envelope `env` (`nenv` entries; NULL: none) ...
// ... env_ksteps / env_ksteps_skipped: count[0] 128-column k-steps of the bulk tasks, count[1] of them structurally zero
void dag_env_count(const DagTaskList& list, const int* env, int nenv, int64_t* count);
// ... envh_ksteps / envh_ksteps_skipped: count[0] half-tile k-steps the tile envelope leaves, count[1] of them skipped with the
// half-tile envelope `envh` (NULL: none)
void dag_envh_count(const DagTaskList& list, const int* env, const int* envh, int nenv, int64_t* count);

}  // namespace mnk

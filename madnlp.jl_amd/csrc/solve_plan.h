// The planner of solve!: which of its five ways a solve runs, the grid of a one-launch solve, whether a solver gets the 512-row
// inverses, and how the queued solves of a batch are grouped into launches.  Host only and plain C++ -- no HIP header, no runtime
// call, no kernel -- so the unit (solve_plan.hip) also compiles with a host compiler and runs under its sanitizers
// (tools/solve_plan_check.cpp), and a CPU test checks the rules (tests/test_solve_plan_cpu.py).  The executor that fills a
// SolveShape from a solver and launches what the plan says is in solve.hip (mnk_ls_run_solve, solve_batch_flush).
//
// The five ways (the statistic "solve_path" of mnk_ls_get_stat reports the one a solver's last solve took):
//   SOLVE_STEPWISE         one launch per 256-column step; always possible, and the only way for a pivoted (Bunch-Kaufman) factor
//   SOLVE_ONE_LAUNCH_256   both sweeps in one launch, 64-row blocks, 256-column steps
//   SOLVE_ONE_LAUNCH_512   ... 32-row blocks, 512-column steps (option solve512, needs the 512-row inverses)
//   SOLVE_MERGED           a system of a merged launch of a solve batch (the 256-column body, G workgroups per system)
//   SOLVE_BLOCKED          several right-hand sides at once, a chunk of SP_MULTI_W of them per pass over the factor (solve_multi.hip;
//                          static-pivot tier, from option multi_rhs_min right-hand sides on: solve_plan_multi)
//
// THE RESIDENCY AND OWNERSHIP RULE of the one-launch solves (solve_grid): the blocks of the right-hand side are owned round-robin
// by G = min(blocks, CUs available) workgroups, which wait for each other and so must all be resident (G <= CUs, one per CU);
// a workgroup keeps at most SP_MAXOWN blocks in LDS; and the blocks of one step belong to different workgroups (G >= blocks per
// step) unless every block has a workgroup of its own anyway.
#pragma once
#include <cstdint>
#include <vector>

namespace mnk {

constexpr int SP_MAXOWN = 12;                      // blocks a workgroup of a one-launch solve owns at most
constexpr int SP_RB256 = 64, SP_STEP256 = 256;     // one-launch solve over 256 columns: rows per block, columns per step
constexpr int SP_RB512 = 32, SP_STEP512 = 512;     // ... over 512 columns
constexpr int SP_NBS256 = SP_STEP256 / SP_RB256;   // blocks per step (4)
constexpr int SP_NBS512 = SP_STEP512 / SP_RB512;   // (16)
constexpr int SP_BATCH_MAXQ = 32;                  // systems of a merged launch at most (the size of its table of systems)
constexpr int SP_BATCH_LARGE_Q = 4;                // ... of large systems: four side by side share the chip's bandwidth best (see solve_batch_groups)
constexpr int64_t SOLVE512_MIN_ROWS = 4096;        // smaller systems never get the 512-row inverses

constexpr int SP_MULTI_W = 64;                     // blocked solve: right-hand sides per pass over the factor (four MFMA tiles of 16)
constexpr int SP_MULTI_TILE = 16;                  // ... the last chunk is padded to a multiple of this (the MFMA tile edge)

enum SolvePath : int32_t { SOLVE_NONE = 0, SOLVE_STEPWISE = 1, SOLVE_ONE_LAUNCH_256 = 2, SOLVE_ONE_LAUNCH_512 = 3, SOLVE_MERGED = 4, SOLVE_BLOCKED = 5 };

// What the rules read of a solver, and nothing else (solve.hip: mnk_ls_solve_shape fills it).
struct SolveShape {
    int64_t Np;            // padded order (a multiple of 64)
    int num_cu;            // CUs of the solver's context
    bool pivoted;          // the factor is the pivoted tier's
    bool persistent_opt;   // option persistent_solve (off, too, once a one-launch solve of this solver gave up)
    bool solve512_opt;     // option solve512
    bool have_linv512;     // the 512-row inverses exist
    bool partitioned;      // the context runs on a CU partition of the device (no entry point creates such a context today: always false)
    bool abort_raised;     // a one-launch solve gave up and nobody has answered it yet
    bool debug_missing;    // option debug_ps_missing is set (tests)
    bool tracing;          // option solve_trace
    bool ldl;              // LDL^T (the D^-1 scaling between the sweeps) or Cholesky
};

struct SolvePlan { int32_t path, G; };   // SolvePath and, for a one-launch path, its grid (0: stepwise)

// The rule above: the workgroups per system for `blocks` blocks, `nbs` of them per step, on `cus` CUs; 0: no one-launch solve.
int solve_grid(int64_t blocks, int cus, int nbs);
// How one solve of this solver runs outside a merged launch.
SolvePlan solve_plan_single(const SolveShape& s);
// How a solve of `nrhs` right-hand sides runs.  SOLVE_BLOCKED exactly when the factor is not pivoted, multi_rhs_min > 0 and
// nrhs >= multi_rhs_min: then W = SP_MULTI_W, `chunks` passes over the factor per sweep and `last_padded` = the width of the last
// chunk's working block (a multiple of SP_MULTI_TILE).  Otherwise the column loop: path and G are solve_plan_single's for every
// column, W = chunks = last_padded = 0.  (Nothing else of the shape matters: the blocked solve waits for no workgroup.)
struct SolveMultiPlan { int32_t path, G, W, chunks, last_padded; };
SolveMultiPlan solve_plan_multi(const SolveShape& s, int64_t nrhs, int64_t multi_rhs_min);
// A solver of this order gets the 512-row inverses (with option solve512): from SOLVE512_MIN_ROWS rows on, and not where the last
// 512-row triangle would end in a partial 256-row block (Np % 512 == 384: inv512_gemm_kernel multiplies whole 256-row blocks).
bool solve512_wanted(int64_t Np);
// The inverses of a batch round of small factorizations come from ONE launch for all systems: only the MFMA kernel of the 256-row
// inverses has that form (not the scalar one, and not the 512-row stage).
bool solve_inverses_batchable(bool linv_mfma, bool solve512_opt);
// A solve batch may queue this solver's single-right-hand-side solve on a device vector: it would run as SOLVE_ONE_LAUNCH_256 and
// nothing about the solver needs a launch of its own (abort pending, a test's missing workgroup, tracing, a CU partition).
bool solve_batchable(const SolveShape& s);

// ---- solve batches ----
// One queued solve.  Solvers are told apart by `solver_id` alone; device, Np, ldl and num_cu are its solver's.
struct SolveBatchReq { int64_t solver_id; int32_t device; int64_t Np; bool ldl; int32_t num_cu; };
// The launches of a batch, in the order they run: launch l is the requests idx[begin[l] .. begin[l + 1]) (indices into the queue,
// ascending) with G[l] workgroups per system.  A launch of one request means "run it as an ordinary solve" (G[l] = 0: its own plan
// decides).
struct SolveBatchGroups {
    std::vector<int32_t> begin, idx, G;
    int launches() const { return (int)G.size(); }
    std::vector<int32_t> rest, next;   // (scratch of solve_batch_groups, kept for its capacity)
};
// Groups the queue `req[0..n)`.  Pass after pass over what is left, the first request opens a launch and every later one joins it if
//   * the launch has room: at most min(SP_BATCH_MAXQ, num_cu / g4) systems, g4 = the workgroups of a system when SP_BATCH_LARGE_Q
//     share the chip -- four for large systems (measured at N = 11 192: 2 -> 104.0, 4 -> 107.4, 8 -> 106.2 it/s of the C5 step), as
//     many as the CUs hold for small ones (a 512-row system has 8 blocks of 64 rows: 32 of them per launch);
//   * it has the opener's device, order and algorithm;
//   * its solver has no right-hand side in this launch yet (the publication buffers of a solver serve one solve at a time) and none
//     that was passed over before it (a solver's right-hand sides keep their order; the other rules imply it while all requests of
//     a solver share device, order and algorithm, as they do in a real queue);
//   * solve_grid still holds with one system more: q systems of G = min(blocks, num_cu / q) workgroups each.
// The G of a launch is the one its last member was admitted with.  `out` is cleared first; its capacity is kept.
void solve_batch_groups(const SolveBatchReq* req, int n, SolveBatchGroups& out);

}  // namespace mnk

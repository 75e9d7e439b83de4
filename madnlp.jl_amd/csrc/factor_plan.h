// The planner of the launch-per-panel factorization schedules (panel_algo 1 and 4): one factorization as a flat list of typed
// steps -- what is launched or recorded on which stream, in the order the host enqueues it.  Host only and plain C++ -- no HIP
// header, no runtime call, no kernel -- so the unit (factor_plan.hip) also compiles with a host compiler and runs under its
// sanitizers (tools/factor_plan_check.cpp), and a CPU test replays the lists (tests/test_factor_plan_cpu.py).  The executor
// that turns the indices of a step into pointers and launches is in factor.hip (run_factor_steps).
//
// What every list must satisfy (the test's simulator checks all five over a grid of inputs; resources are the 64-column blocks
// of the factor and the two W buffers of LDL^T, order is stream order plus record -> wait edges):
//   (a) every block is factored exactly once and in order;
//   (b) when a block is factored, every earlier block's contribution has been applied to it exactly once (the fused prologue
//       of a persistent panel applies its K columns to the launch's own columns; the two launches of a shared queue are one update);
//   (c) every block an update reads as source is factored, and that happens-before the update;
//   (d) two steps that touch the same block or the same W buffer, one of them writing, are ordered -- except the two launches of
//       one shared queue, which share the work through a counter;
//   (e) all streams are joined into the caller's stream at the end.
#pragma once
#include <cstdint>
#include <vector>

namespace mnk {

enum FactorStepKind : int32_t {
    FS_LEAF = 1,    // schedule 1: the 64x64 diagonal block `col`
    FS_TRSM = 2,    // schedule 1: the rows below it (`n` 16-row strips per wave); LDL^T: writes W columns of `whalf`
    FS_PPANEL = 3,  // schedule 4: `n` blocks from `col` in one persistent launch; `K` > 0: its prologue first applies the K columns
                    // from `src` to the launch's own columns (LDL^T: read from `rhalf`)
    FS_UPDATE = 4,  // C[col.., col..col+ncols) -= L[.., src..src+K) (W or L)^T over `rows` rows (lower tiles); `variant`
    FS_RECORD = 5,  // record event (`event`, `index`) on `stream`
    FS_WAIT = 6,    // `stream` waits for event (`event`, `index`)
};
enum FactorStepStream : int32_t { FS_CALLER = 0, FS_PANEL = 1, FS_UPDATE_STREAM = 2 };
enum FactorStepVariant : int32_t { FS_SMALL = 0, FS_PLAIN = 1, FS_QUEUE = 2 };   // 64x64 tiles / 128x128 tiles / 128x128 tiles pulled from a counter
enum FactorStepEvent : int32_t { FS_EV_A = 0, FS_EV_B = 1, FS_EV_PANEL = 2, FS_EV_NEXT = 3, FS_EV_NEXT2 = 4, FS_EV_BDONE = 5 };

// One step.  Columns and rows are matrix indices (multiples of 64).  A W buffer holds W = L D of ONE outer panel: its column c is
// matrix column `wko` + c (the step's `wko` for the buffer it writes, `rko` for the one it reads).
struct FactorStep {
    int32_t kind, stream;
    int32_t col;           // leaf / trsm: the block's column; panel: first column; update: first column = first row of C
    int32_t n;             // trsm: strips per wave (1 or 2); panel: blocks; update: columns of C
    int32_t rows;          // update: rows of C
    int32_t src, K;        // update / panel prologue: first source column and their number (panel: K = 0: no prologue)
    int32_t variant;       // update: FactorStepVariant
    int32_t slot, cus;     // FS_QUEUE: counter slot (8 ints each) and the CUs whose workgroups pull from it
    int32_t whalf, wko;    // LDL^T: the W buffer the step writes (-1: none) and the matrix column of its column 0
    int32_t rhalf, rko;    // LDL^T: the W buffer the step reads (-1: none) and the matrix column of its column 0
    int32_t event, index;  // record / wait: FactorStepEvent and its index in the event array (0 for FS_EV_A / FS_EV_B)
};
constexpr int FACTOR_STEP_INTS = (int)(sizeof(FactorStep) / sizeof(int32_t));
static_assert(sizeof(FactorStep) == 16 * sizeof(int32_t), "a step is 16 ints (mnk_debug_factor_plan copies them out)");

struct FactorPlanIn {
    int64_t Np;            // padded order (a multiple of 64)
    bool ldl;              // LDL^T (W buffers) or Cholesky
    int algo_now;          // 1 or 4
    bool lookahead;
    int64_t nbo;           // effective width of the outer panels (mnk_ls_effective_nbo)
    int64_t pp_fuse_rows;  // schedule 4: rows from which persistent launches apply the columns in front of them themselves (0: never)
    int share;             // 0: no shared tile queue; 1: where the update is the longer leg; 2: always
    int small_tiles;       // (a)-updates with fewer 128x128 tiles than this use 64x64 workgroup tiles
    int num_cu, panel_cus; // CUs of the context / of its panel stream (0: no CU masks)
};

// lower 128x128 tiles of an M x N update (the tile count of launch_gemm_nt mode 2 and of the tile queue)
int gemm_nt_lower_tiles(int64_t M, int64_t N);

// What the executor must have ready before the first step: the outer panels (event arrays hold npanel + 1 events, the queue
// counters 8 ints per panel) and whether the list uses the panel and update streams at all.
struct FactorPlanShape { int npanel; bool lookahead; };
// The steps of one factorization into `steps` (cleared first; its capacity is kept).
FactorPlanShape factor_plan_build(const FactorPlanIn& in, std::vector<FactorStep>& steps);

}  // namespace mnk

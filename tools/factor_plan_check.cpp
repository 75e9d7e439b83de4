// The planner of the launch-per-panel factorization schedules (csrc/factor_plan.hip) as a host program under the host compiler's
// sanitizers: no HIP, no device, not loaded into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++
//       madnlp.jl_amd/csrc/factor_plan.hip tools/factor_plan_check.cpp -o /tmp/factor_plan_check && /tmp/factor_plan_check
//
// Builds the grid of tests/test_factor_plan_cpu.py (every combination, nothing thinned) through factor_plan_build and through the
// host-only entry mnk_debug_factor_plan with a short buffer, checks what needs no simulator -- the entry returns what the planner
// built and writes nothing behind `cap`, every index of a step lies inside the matrix, the event arrays and the counters the
// executor sizes from the plan's shape -- and prints the number of plans and one FNV-1a hash over all their steps, to compare two
// builds.  Any sanitizer report or failed check ends it with a non-zero status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madnlp.jl_amd/csrc/factor_plan.h"
#include "../include/madnlp_hip.h"

using namespace mnk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

int main() {
    const int NUM_CU = 256;
    long nplans = 0, nsteps = 0;
    uint64_t hash = 1469598103934665603ull;
    std::vector<FactorStep> steps;
    std::vector<int32_t> out;
    for (int64_t Np : {64, 128, 320, 640, 1152, 2560, 4672, 8192})
        for (int ldl = 0; ldl < 2; ++ldl)
            for (int algo : {1, 4})
                for (int la = 0; la < 2; ++la)
                    for (int64_t width : {(int64_t)128, (int64_t)192, (int64_t)256, (int64_t)512, (int64_t)1024, Np})
                        for (int64_t fuse : {0, 4096, 1000000})
                            for (int share = 0; share < 3; ++share)
                                for (int small_tiles : {0, 400, 100000})
                                    for (int pcus : {0, 64}) {
                                        const FactorPlanIn in{Np, ldl != 0, algo, la != 0, width, fuse, share, small_tiles, NUM_CU, pcus};
                                        const FactorPlanShape shape = factor_plan_build(in, steps);
                                        const int n = (int)steps.size();
                                        CHECK(n > 0 && shape.npanel >= 1 && shape.lookahead == (la && shape.npanel > 1));
                                        for (const FactorStep& t : steps) {
                                            CHECK(t.kind >= FS_LEAF && t.kind <= FS_WAIT && t.stream >= FS_CALLER && t.stream <= FS_UPDATE_STREAM);
                                            CHECK(shape.lookahead || t.stream == FS_CALLER);
                                            CHECK(t.whalf >= -1 && t.whalf <= 1 && t.rhalf >= -1 && t.rhalf <= 1 && (ldl || (t.whalf < 0 && t.rhalf < 0)));
                                            if (t.kind == FS_RECORD || t.kind == FS_WAIT) {
                                                CHECK(t.event >= FS_EV_A && t.event <= FS_EV_BDONE && t.index >= 0);
                                                CHECK(t.event <= FS_EV_B ? t.index == 0 : t.index <= shape.npanel);   // (arrays of npanel + 1 events)
                                                continue;
                                            }
                                            CHECK(t.col >= 0 && t.col % 64 == 0 && t.col < Np && t.wko >= 0 && t.wko <= t.col);
                                            if (t.kind == FS_TRSM) CHECK((t.n == 1 || t.n == 2) && t.col + 64 < Np);
                                            if (t.kind == FS_PPANEL) CHECK(t.n >= 1 && t.n <= 4 && t.col + 64 * t.n <= Np);
                                            if (t.kind == FS_PPANEL || t.kind == FS_UPDATE)
                                                CHECK(t.K >= 0 && t.K % 64 == 0 && t.src >= 0 && t.src + t.K <= t.col && (t.rhalf < 0 || (t.rko >= 0 && t.rko <= t.src)));
                                            if (t.kind == FS_UPDATE) {
                                                CHECK(t.K > 0 && t.n > 0 && t.n % 64 == 0 && t.col + t.n <= Np && t.rows == Np - t.col && (t.rhalf >= 0) == (ldl != 0));
                                                CHECK(t.variant >= FS_SMALL && t.variant <= FS_QUEUE);
                                                if (t.variant == FS_QUEUE) CHECK(share && pcus && t.slot >= 0 && t.slot <= shape.npanel && t.cus > 0 && t.cus < NUM_CU);
                                            }
                                        }
                                        // the entry the tests and tools call, with a short buffer: nothing is written behind `cap`
                                        const int cap = n > 7 ? n - 7 : n;
                                        out.assign((size_t)FACTOR_STEP_INTS * cap + 4, -77);
                                        int shp[2] = {-1, -1};
                                        CHECK(mnk_debug_factor_plan(Np, ldl, algo, la, width, fuse, share, small_tiles, NUM_CU, pcus, out.data(), cap, shp) == n);
                                        CHECK(shp[0] == shape.npanel && shp[1] == (shape.lookahead ? 1 : 0));
                                        for (int k = 0; k < 4; ++k) CHECK(out[(size_t)FACTOR_STEP_INTS * cap + k] == -77);
                                        for (int t = 0; t < n; ++t) {
                                            const int32_t* w = &steps[t].kind;
                                            for (int k = 0; k < FACTOR_STEP_INTS; ++k) {
                                                if (t < cap) CHECK(out[(size_t)FACTOR_STEP_INTS * t + k] == w[k]);
                                                hash = (hash ^ (uint32_t)w[k]) * 1099511628211ull;
                                            }
                                        }
                                        ++nplans;
                                        nsteps += n;
                                    }
    CHECK(mnk_debug_factor_plan(100, 0, 1, 0, 512, 0, 0, 400, NUM_CU, 0, nullptr, 0, nullptr) == -1);
    CHECK(mnk_debug_factor_plan(512, 0, 5, 0, 512, 0, 0, 400, NUM_CU, 0, nullptr, 0, nullptr) == -1);
    std::printf("factor_plan_check: %ld plans, %ld steps, hash %016llx, all checks passed\n", nplans, nsteps, (unsigned long long)hash);
    return 0;
}

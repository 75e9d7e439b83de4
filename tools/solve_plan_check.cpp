// The planner of solve! (csrc/solve_plan.hip) as a host program under the host compiler's sanitizers: no HIP, no device, not
// loaded into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++
//       madnlp.jl_amd/csrc/solve_plan.hip tools/solve_plan_check.cpp -o /tmp/solve_plan_check && /tmp/solve_plan_check
//
// Runs the grids of tests/test_solve_plan_cpu.py -- every single plan (orders x CUs x every combination of the flags) through
// solve_plan_single / solve_batchable and through the host-only entry mnk_debug_solve_plan, the rule of the blocked solve for several
// right-hand sides (solve_plan_multi / mnk_debug_solve_plan_multi) over counts and thresholds, and a few thousand random queues (up to 40
// requests of up to 8 solvers on 2 devices; a generator of its own, not the test's) through solve_batch_groups and
// mnk_debug_solve_batch_groups -- checks what the kernels need of every plan and every launch, that the entries return what the
// planner built and write nothing behind their arrays, and prints the counts and one FNV-1a hash over everything planned, to compare
// two builds.  Any sanitizer report or failed check ends it with a non-zero status.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madnlp.jl_amd/csrc/solve_plan.h"
#include "../include/madnlp_hip.h"

using namespace mnk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static uint64_t g_hash = 1469598103934665603ull;
static void mix(int64_t v) { g_hash = (g_hash ^ (uint64_t)v) * 1099511628211ull; }

static uint64_t g_rng = 88172645463325252ull;
static int rnd(int n) {   // xorshift64
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (int)((g_rng >> 11) % (uint64_t)n);
}

int main() {
    long nplans = 0, nqueues = 0, nlaunches = 0;
    std::vector<int64_t> orders;
    for (int64_t Np = 64; Np <= 8192; Np += 64) orders.push_back(Np);
    for (int64_t Np : {11200, 16384, 16448, 85568, 196608, 196672}) orders.push_back(Np);
    for (int64_t Np : orders)
        for (int cu : {1, 2, 3, 4, 16, 64, 240, 256})
            for (int bits = 0; bits < 512; ++bits) {
                auto bit = [&](int k) { return ((bits >> k) & 1) != 0; };
                const SolveShape s{Np, cu, bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8)};
                const SolvePlan p = solve_plan_single(s);
                CHECK(p.path >= SOLVE_STEPWISE && p.path <= SOLVE_ONE_LAUNCH_512);
                if (p.path == SOLVE_STEPWISE) CHECK(p.G == 0);
                else {
                    const int64_t blocks = Np / (p.path == SOLVE_ONE_LAUNCH_256 ? SP_RB256 : SP_RB512);
                    CHECK(p.G >= 1 && p.G <= cu && (blocks + p.G - 1) / p.G <= SP_MAXOWN && !s.pivoted && s.persistent_opt);
                }
                if (p.path == SOLVE_ONE_LAUNCH_512) CHECK(s.solve512_opt && s.have_linv512 && (p.G >= SP_NBS512 || p.G == Np / SP_RB512));
                const bool batchable = solve_batchable(s);
                if (batchable) CHECK(p.path == SOLVE_ONE_LAUNCH_256 && !s.partitioned && !s.abort_raised && !s.debug_missing && !s.tracing);
                int out[6] = {-77, -77, -77, -77, -77, -77};
                CHECK(mnk_debug_solve_plan(Np, cu, bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bits & 1, out) == 0);
                CHECK(out[0] == p.path && out[1] == p.G && out[2] == (batchable ? 1 : 0) && out[3] == (solve512_wanted(Np) ? 1 : 0));
                CHECK(out[4] == (solve_inverses_batchable(bit(0), bit(2)) ? 1 : 0) && out[5] == -77);
                mix(p.path); mix(p.G); mix(out[2]); mix(out[3]);
                // several right-hand sides: blocked exactly when not pivoted, multi_rhs_min > 0 and nrhs >= multi_rhs_min; the chunks
                // cover nrhs, the last one padded to the MFMA tile; otherwise every column as planned above
                if (bits % 8 <= 1)   // (only `pivoted` of the flags may matter: both values, one in four of the other combinations)
                    for (int64_t nrhs : {1, 3, 4, 15, 16, 17, 63, 64, 65, 130, 1000})
                        for (int64_t mn : {0, 2, 4, 16, 64, 65}) {
                            const SolveMultiPlan m = solve_plan_multi(s, nrhs, mn);
                            const bool blocked = !s.pivoted && mn > 0 && nrhs >= mn;
                            CHECK((m.path == SOLVE_BLOCKED) == blocked);
                            if (blocked) {
                                const int64_t last = nrhs - (int64_t)(m.chunks - 1) * m.W;
                                CHECK(m.W == SP_MULTI_W && m.G == 0 && m.chunks >= 1 && last >= 1 && last <= m.W);
                                CHECK(m.last_padded >= last && m.last_padded - last < SP_MULTI_TILE && m.last_padded % SP_MULTI_TILE == 0 && m.last_padded <= m.W);
                            } else CHECK(m.path == p.path && m.G == p.G && m.W == 0 && m.chunks == 0 && m.last_padded == 0);
                            int om[6] = {-77, -77, -77, -77, -77, -77};
                            CHECK(mnk_debug_solve_plan_multi(Np, cu, bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), nrhs, mn, om) == 0);
                            CHECK(om[0] == m.path && om[1] == m.W && om[2] == m.chunks && om[3] == m.last_padded && om[4] == m.G && om[5] == -77);
                            mix(m.path); mix(m.chunks); mix(m.last_padded);
                        }
                ++nplans;
            }

    const int64_t np_of[5] = {512, 2048, 6400, 11200, 131072};
    const int cu_of[3] = {16, 64, 256};
    std::vector<SolveBatchReq> solvers, req;
    SolveBatchGroups g;
    std::vector<int64_t> sid, Npv;
    std::vector<int32_t> dev, ldl, cus, begin, idx, G, where;
    for (int it = 0; it < 4000; ++it) {
        solvers.clear();
        const int nsolvers = 1 + rnd(8);
        for (int k = 0; k < nsolvers; ++k) solvers.push_back({1000 + 8 * k, rnd(2), np_of[rnd(5)], rnd(2) != 0, cu_of[rnd(3)]});
        const int kind = rnd(3);   // 0: solvers of one shape; 1: any shapes; 2: every field of every request on its own (no real queue)
        if (kind == 0)
            for (SolveBatchReq& s : solvers) { s.Np = solvers[0].Np; s.ldl = solvers[0].ldl; s.num_cu = solvers[0].num_cu; }
        const int n = rnd(41);
        req.clear();
        for (int i = 0; i < n; ++i) {
            req.push_back(solvers[rnd(nsolvers)]);
            if (kind == 2) req.back() = SolveBatchReq{req.back().solver_id, rnd(2), np_of[rnd(5)], rnd(2) != 0, cu_of[rnd(3)]};
        }
        solve_batch_groups(req.data(), n, g);
        const int nl = g.launches();
        CHECK((int)g.begin.size() == nl + 1 && g.begin[0] == 0 && g.begin[nl] == n && (int)g.idx.size() == n && nl <= n);
        where.assign(n, -1);
        for (int l = 0; l < nl; ++l) {
            const int q = g.begin[l + 1] - g.begin[l];
            CHECK(q >= 1);
            const SolveBatchReq& r0 = req[g.idx[g.begin[l]]];
            const int64_t nb = r0.Np / SP_RB256;
            if (q >= 2) CHECK(g.G[l] >= 1 && g.G[l] == (int)std::min<int64_t>(nb, r0.num_cu / q) && q * g.G[l] <= r0.num_cu && (nb + g.G[l] - 1) / g.G[l] <= SP_MAXOWN && q <= SP_BATCH_MAXQ);
            else CHECK(g.G[l] == 0);
            for (int k = g.begin[l]; k < g.begin[l + 1]; ++k) {
                const int i = g.idx[k];
                CHECK(i >= 0 && i < n && where[i] < 0 && (k == g.begin[l] || g.idx[k - 1] < i));
                where[i] = l;
                const SolveBatchReq& r = req[i];
                CHECK(r.device == r0.device && r.Np == r0.Np && r.ldl == r0.ldl);
                for (int j = 0; j < i; ++j)   // an earlier right-hand side of the same solver ran in an earlier launch
                    if (req[j].solver_id == r.solver_id) CHECK(where[j] >= 0 && where[j] < l);
                mix(i);
            }
            mix(g.G[l]);
        }
        // the entry the tests call: the same launches, nothing written behind n + 1 / n / n entries
        sid.clear(); Npv.clear(); dev.clear(); ldl.clear(); cus.clear();
        for (const SolveBatchReq& r : req) { sid.push_back(r.solver_id); Npv.push_back(r.Np); dev.push_back(r.device); ldl.push_back(r.ldl); cus.push_back(r.num_cu); }
        begin.assign(n + 2, -77); idx.assign(n + 1, -77); G.assign(n + 1, -77);
        CHECK(mnk_debug_solve_batch_groups(n, sid.data(), dev.data(), Npv.data(), ldl.data(), cus.data(), begin.data(), idx.data(), G.data()) == nl);
        CHECK(begin[n + 1] == -77 && idx[n] == -77 && G[n] == -77);
        for (int l = 0; l <= nl; ++l) CHECK(begin[l] == g.begin[l]);
        for (int k = 0; k < n; ++k) CHECK(idx[k] == g.idx[k]);
        for (int l = 0; l < nl; ++l) CHECK(G[l] == g.G[l]);
        ++nqueues;
        nlaunches += nl;
    }
    int out[5];
    CHECK(mnk_debug_solve_plan(100, 256, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, out) == -1);
    CHECK(mnk_debug_solve_plan(512, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, out) == -1);
    CHECK(mnk_debug_solve_plan_multi(512, 256, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 4, out) == -1);
    CHECK(mnk_debug_solve_plan_multi(500, 256, 0, 1, 0, 0, 0, 0, 0, 0, 0, 8, 4, out) == -1);
    CHECK(mnk_debug_solve_batch_groups(-1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    std::printf("solve_plan_check: %ld plans, %ld queues, %ld launches, hash %016llx, all checks passed\n", nplans, nqueues, nlaunches,
                (unsigned long long)g_hash);
    return 0;
}

// The planner of solve! (solve_plan.h): the residency and ownership rule of the one-launch solves, the path of a single solve,
// the 512-row inverses' condition and the grouping of a solve batch.  Plain C++: no HIP header, no runtime call, no kernel.
#include "solve_plan.h"

#include <algorithm>

namespace mnk {

int solve_grid(int64_t blocks, int cus, int nbs) {
    const int G = (int)std::min<int64_t>(blocks, cus);
    return G >= 1 && (blocks + G - 1) / G <= SP_MAXOWN && (G >= nbs || blocks <= G) ? G : 0;
}

bool solve512_wanted(int64_t Np) { return Np >= SOLVE512_MIN_ROWS && Np % SP_STEP512 != 384; }   // (384 = a 256-row block and half of one)

bool solve_inverses_batchable(bool linv_mfma, bool solve512_opt) { return linv_mfma && !solve512_opt; }

SolvePlan solve_plan_single(const SolveShape& s) {
    // (a 2x2 block of a pivoted factor may straddle two blocks, which the block ownership of the one-launch solves does not allow)
    const int G = s.pivoted || !s.persistent_opt ? 0 : solve_grid(s.Np / SP_RB256, s.num_cu, SP_NBS256);
    if (G == 0) return {SOLVE_STEPWISE, 0};
    const int G5 = s.solve512_opt && s.have_linv512 ? solve_grid(s.Np / SP_RB512, s.num_cu, SP_NBS512) : 0;
    return G5 != 0 ? SolvePlan{SOLVE_ONE_LAUNCH_512, G5} : SolvePlan{SOLVE_ONE_LAUNCH_256, G};
}

SolveMultiPlan solve_plan_multi(const SolveShape& s, int64_t nrhs, int64_t multi_rhs_min) {
    if (s.pivoted || multi_rhs_min <= 0 || nrhs < multi_rhs_min) {
        const SolvePlan p = solve_plan_single(s);
        return {p.path, p.G, 0, 0, 0};
    }
    const int64_t chunks = (nrhs + SP_MULTI_W - 1) / SP_MULTI_W, last = nrhs - (chunks - 1) * SP_MULTI_W;
    return {SOLVE_BLOCKED, 0, SP_MULTI_W, (int32_t)chunks, (int32_t)((last + SP_MULTI_TILE - 1) / SP_MULTI_TILE * SP_MULTI_TILE)};
}

bool solve_batchable(const SolveShape& s) {
    // (only the 256-column body has a multi-system kernel: a solver with the 512-row inverses keeps to launches of its own, whether
    // or not its own plan would take the 512-column path)
    return !(s.solve512_opt && s.have_linv512) && !s.partitioned && !s.abort_raised && !s.debug_missing && !s.tracing &&
           solve_plan_single(s).path == SOLVE_ONE_LAUNCH_256;
}

void solve_batch_groups(const SolveBatchReq* req, int n, SolveBatchGroups& out) {
    out.begin.clear(); out.idx.clear(); out.G.clear();
    std::vector<int32_t>&rest = out.rest, &next = out.next;
    rest.clear();
    for (int i = 0; i < n; ++i) rest.push_back(i);
    while (!rest.empty()) {
        const SolveBatchReq& r0 = req[rest.front()];
        const int64_t nb = r0.Np / SP_RB256;
        const int g4 = (int)std::max<int64_t>(1, std::min<int64_t>(nb, r0.num_cu / SP_BATCH_LARGE_Q));
        const int maxq = std::max(1, std::min(SP_BATCH_MAXQ, r0.num_cu / g4));
        const size_t first = out.idx.size();
        int G = 0;
        next.clear();
        for (const int32_t i : rest) {
            const SolveBatchReq& r = req[i];
            const int q = (int)(out.idx.size() - first);
            bool take = q < maxq && r.device == r0.device && r.Np == r0.Np && r.ldl == r0.ldl;
            for (size_t k = first; take && k < out.idx.size(); ++k) take = req[out.idx[k]].solver_id != r.solver_id;
            for (size_t k = 0; take && k < next.size(); ++k) take = req[next[k]].solver_id != r.solver_id;
            if (take && q > 0) {
                const int Gq = solve_grid(nb, r0.num_cu / (q + 1), SP_NBS256);
                take = Gq != 0;
                if (take) G = Gq;
            }
            if (take) out.idx.push_back(i);   // (the opener always goes: alone it is an ordinary solve)
            else next.push_back(i);
        }
        out.begin.push_back((int32_t)first);
        out.G.push_back(G);
        rest.swap(next);
    }
    out.begin.push_back((int32_t)out.idx.size());
}

}  // namespace mnk

// ---- host-only entries for tests and tools (include/madnlp_hip.h) ----
extern "C" int mnk_debug_solve_plan(int64_t Np, int num_cu, int pivoted, int persistent_opt, int solve512_opt, int have_linv512,
                                    int partitioned, int abort_raised, int debug_missing, int tracing, int ldl, int linv_mfma, int* out) {
    if (Np <= 0 || Np % 64 != 0 || num_cu <= 0 || out == nullptr) return -1;
    const mnk::SolveShape s{Np, num_cu, pivoted != 0, persistent_opt != 0, solve512_opt != 0, have_linv512 != 0, partitioned != 0,
                            abort_raised != 0, debug_missing != 0, tracing != 0, ldl != 0};
    const mnk::SolvePlan p = mnk::solve_plan_single(s);
    out[0] = p.path;
    out[1] = p.G;
    out[2] = mnk::solve_batchable(s) ? 1 : 0;
    out[3] = mnk::solve512_wanted(Np) ? 1 : 0;
    out[4] = mnk::solve_inverses_batchable(linv_mfma != 0, solve512_opt != 0) ? 1 : 0;
    return 0;
}

extern "C" int mnk_debug_solve_plan_multi(int64_t Np, int num_cu, int pivoted, int persistent_opt, int solve512_opt, int have_linv512,
                                          int partitioned, int abort_raised, int debug_missing, int tracing, int ldl, int64_t nrhs,
                                          int64_t multi_rhs_min, int* out) {
    if (Np <= 0 || Np % 64 != 0 || num_cu <= 0 || nrhs < 1 || nrhs > (int64_t)1 << 40 || out == nullptr) return -1;
    const mnk::SolveShape s{Np, num_cu, pivoted != 0, persistent_opt != 0, solve512_opt != 0, have_linv512 != 0, partitioned != 0,
                            abort_raised != 0, debug_missing != 0, tracing != 0, ldl != 0};
    const mnk::SolveMultiPlan p = mnk::solve_plan_multi(s, nrhs, multi_rhs_min);
    out[0] = p.path;
    out[1] = p.W;
    out[2] = p.chunks;
    out[3] = p.last_padded;
    out[4] = p.G;
    return 0;
}

extern "C" int mnk_debug_solve_batch_groups(int n, const int64_t* solver_id, const int32_t* device, const int64_t* Np, const int32_t* ldl,
                                            const int32_t* num_cu, int32_t* begin, int32_t* idx, int32_t* G) {
    if (n < 0 || !begin || (n > 0 && !(solver_id && device && Np && ldl && num_cu && idx && G))) return -1;
    std::vector<mnk::SolveBatchReq> req;
    for (int i = 0; i < n; ++i) {
        if (Np[i] <= 0 || Np[i] % 64 != 0 || num_cu[i] <= 0) return -1;
        req.push_back({solver_id[i], device[i], Np[i], ldl[i] != 0, num_cu[i]});
    }
    mnk::SolveBatchGroups g;
    mnk::solve_batch_groups(req.data(), n, g);
    std::copy(g.begin.begin(), g.begin.end(), begin);
    std::copy(g.idx.begin(), g.idx.end(), idx);
    std::copy(g.G.begin(), g.G.end(), G);
    return g.launches();
}

// The task-DAG planner (csrc/dag_plan.hip) as a host program under the host compiler's sanitizers: no HIP, no device, not loaded
// into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++
//       madnlp.jl_amd/csrc/dag_plan.hip tools/dag_plan_check.cpp -o /tmp/dag_plan_check && /tmp/dag_plan_check
//
// Runs the grid of tools/dag_plan_lists.py through the planner functions and the four host-only entries and checks what must hold
// for every list: a deal is a partition into subsequences, a dealt task carries the position it was dealt from, a merged list holds
// every instance's tasks in their order, the field accessors return what a task was built with; and the plan shape (dag_choose_js2)
// never leaves the deep band more strips than its partition has CUs.  Prints the number of lists; any
// sanitizer report or failed check ends it with a non-zero status.  `--quick`: orders up to 44 tiles.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../madnlp.jl_amd/csrc/dag_plan.h"
#include "../include/madnlp_hip.h"

using namespace mnk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static long g_lists = 0;

static void check_deal(const DagTaskList& list, int ntile, int ninst, int nq, int gang) {
    const bool both[2] = {true, true};
    const DagDealtList d = dag_deal_list(list, nq, gang, both);
    const int n = list.size(), part[3] = {0, list.n1, n};
    CHECK((int)d.tasks.size() == n && (int)d.order.size() == n && (int)d.qoff.size() == 2 * (nq + 1));
    std::vector<char> seen(n, 0);
    for (int ph = 0; ph < 2; ++ph) {
        const int* off = d.qoff.data() + ph * (nq + 1);
        CHECK(off[0] == 0 && off[nq] == part[ph + 1] - part[ph] && d.nq[ph] == nq);
        for (int x = 0; x < nq; ++x) {
            CHECK(off[x] <= off[x + 1]);
            for (int p = part[ph] + off[x]; p < part[ph] + off[x + 1]; ++p) {
                const int t = d.order[p];
                CHECK(t >= part[ph] && t < part[ph + 1] && !seen[t]);
                seen[t] = 1;
                if (p > part[ph] + off[x]) CHECK(d.order[p - 1] < t);   // a subsequence of the list in list order
                const DagTask &a = d.tasks[p], &b = list.tasks[t];
                CHECK(a.word[0] == b.word[0] && a.word[1] == b.word[1] && a.word[3] == b.word[3] && a.J() == b.J());
                if (DagTask::fits(ntile, ninst, n)) CHECK(a.list_pos() == t - part[ph]);
            }
        }
    }
    ++g_lists;
}

int main(int argc, char** argv) {
    const bool quick = argc > 1 && !std::strcmp(argv[1], "--quick");
    const int ntiles[] = {2, 3, 10, 11, 12, 43, 44, 88, 154, 240};
    std::vector<int> out, order;
    for (int ntile : ntiles) {
        if (quick && ntile > 44) continue;
        const int nsc = (ntile + 1) / 2, js2s[3] = {0, (ntile + 3) / 4, nsc};
        for (int js2 : js2s)
            for (int chunk : {4, 64})
                for (int taper0 : {1, 2})
                    for (int band : {4, 8}) {
                        const DagTaskList built = dag_build_tasks(ntile, chunk, band, js2, taper0);
                        CHECK(built.tasks.size() == built.ready.size() && built.n1 >= 0 && built.n1 <= built.size());
                        for (int t = 0; t < built.size(); ++t) {
                            const DagTask& k = built.tasks[t];
                            CHECK(k.I() < ntile && k.J() <= k.I() && k.kbeg() <= k.kend() && k.kend() <= k.J() && k.instance() == 0 && k.list_pos() == 0);
                            CHECK(built.ready[t] == k.kend() && (t == 0 || built.ready[t - 1] <= built.ready[t]));
                        }
                        // the statistics: a dense envelope skips nothing, a random monotone one (fixed seed) never more than there is
                        std::mt19937 rng(1000u * ntile + js2);
                        std::vector<int> env(ntile, 0), envh(2 * ntile, 0);
                        int64_t dense[2], cnt[2], cnth[2];
                        dag_env_count(built, env.data(), ntile, dense);
                        CHECK(dense[1] == 0);
                        for (int i = 1; i < ntile; ++i) env[i] = std::min<int>(i, env[i - 1] + (int)(rng() % 3));
                        for (int i = 0; i < 2 * ntile; ++i) envh[i] = std::min<int>(i, 2 * env[i / 2] + (i & 1) * (int)(rng() & 1));
                        dag_env_count(built, env.data(), ntile, cnt);
                        CHECK(cnt[0] == dense[0] && cnt[1] >= 0 && cnt[1] <= cnt[0]);
                        CHECK(mnk_debug_envh_ksteps(ntile, chunk, band, js2, taper0, env.data(), envh.data(), cnth) == built.size());
                        CHECK(cnth[0] >= 0 && cnth[0] <= 8 * dense[0] && cnth[1] >= 0 && cnth[1] <= cnth[0]);
                        for (int fill = 0; fill < 2; ++fill) {
                            DagTaskList list = built;
                            if (fill) dag_add_fill_tasks(ntile, list);
                            CHECK(list.size() == built.size() + (fill && built.size() > 0 ? ntile * (ntile + 1) / 2 : 0));
                            for (int ninst : {1, 2, 5})
                                for (int period : {0, nsc}) {
                                    if (ninst == 1 && period) continue;
                                    const DagTaskList m = ninst > 1 ? dag_merge_tasks(list, ninst, period) : list;
                                    CHECK(m.size() == ninst * list.size());
                                    if (ninst > 1) {   // every instance's tasks, in their order
                                        std::vector<int> pos(ninst, 0);
                                        for (int t = 0; t < m.size(); ++t) {
                                            const int i = m.tasks[t].instance();
                                            CHECK(i >= 0 && i < ninst && pos[i] < list.size() && (t == 0 || m.ready[t - 1] <= m.ready[t]));
                                            const DagTask& src = list.tasks[pos[i]++];
                                            CHECK(m.tasks[t].word[0] == src.word[0] && m.tasks[t].I() == src.I() && m.tasks[t].word[2] == src.word[2] && m.tasks[t].word[3] == src.word[3]);
                                        }
                                    }
                                    for (int nq : {1, 8})
                                        for (int gang : {-1, 1, 4}) check_deal(m, ntile, ninst, nq, gang);
                                }
                        }
                        // the entries the tests and tools call, with a short buffer: nothing is written behind `cap`
                        const int cap = 100;
                        out.assign(4 * cap + 4, -77);
                        order.assign(cap + 1, -77);
                        int off[18], n1 = -1;
                        CHECK(mnk_debug_dag_tasks(ntile, chunk, band, js2, taper0, out.data(), cap, &n1) == built.size() && n1 == built.n1);
                        CHECK(mnk_debug_dag_merged_tasks(ntile, chunk, band, js2, taper0, 1, 2, nsc, out.data(), cap) >= 2 * built.size());
                        CHECK(mnk_debug_dag_deal(ntile, chunk, band, js2, taper0, 1, 1, 0, 8, 4, out.data(), order.data(), cap, off, &n1) >= built.size());
                        CHECK(out[4 * cap] == -77 && order[cap] == -77);
                    }
    }
    // the plan shape (dag_choose_js2): within [0, nsc], never more strips in the deep band than its partition has CUs, the request
    // itself where that is admissible, and the entry the tests call returns the same
    for (int64_t Np = 128; Np <= 12288; Np += 128)
        for (int cus2 : {0, 42, 96})
            for (int64_t deep : {(int64_t)0, (int64_t)5376, (int64_t)1 << 40}) {
                const int nsc = (int)((Np + 255) / 256);
                for (int ovr = -1; ovr <= nsc + 1; ++ovr) {
                    const int js2 = dag_choose_js2(Np, cus2, deep, ovr);
                    CHECK(js2 >= 0 && js2 <= nsc && Np - 256 * (int64_t)js2 <= 64 * (int64_t)cus2);
                    if (cus2 == 0) CHECK(js2 == nsc);
                    if (cus2 > 0 && ovr >= 0 && Np - 256 * (int64_t)std::min(ovr, nsc) <= 64 * (int64_t)cus2) CHECK(js2 == std::min(ovr, nsc));
                    if (js2 > 0 && js2 < nsc && (ovr < 0 || js2 != ovr)) CHECK(Np - 256 * (int64_t)(js2 - 1) > 64 * (int64_t)cus2);   // (raised no further than needed)
                    CHECK(mnk_debug_dag_js2(Np, cus2, deep, ovr) == js2);
                }
            }
    CHECK(mnk_debug_dag_js2(100, 96, 5376, -1) == -1 && mnk_debug_dag_js2(128, -1, 5376, -1) == -1);
    std::printf("dag_plan_check: %ld dealt lists, all checks passed\n", g_lists);
    return 0;
}

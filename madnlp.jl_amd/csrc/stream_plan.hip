// The CU-mask rules (stream_plan.h): the split of every pair kind, mask words, grids that are resident at launch and the chain
// partitions of small-system rounds.  Plain C++: no HIP header, no runtime call, no kernel.
#include "stream_plan.h"

#include <algorithm>
#include <climits>

namespace mnk {

int panel_default_cus(int num_cu) { return num_cu >= 16 ? std::max(4, num_cu / 4) : 0; }

StreamSplit stream_split(int kind, int num_cu, int dag_cus, int dag_cus2, int arg) {
    const StreamSplit none{0, 0, 0, 0, false};
    auto head = [&](int chain) { return StreamSplit{0, chain, chain, num_cu - chain, true}; };   // [0, chain) | the rest
    const bool dag = num_cu >= DAG_MIN_CUS && dag_cus > 0 && dag_cus < num_cu;
    switch (kind) {
        case PAIR_DAG: return dag ? head(dag_cus) : none;
        case PAIR_DEEP: return dag && dag_cus2 > 0 && dag_cus2 < num_cu ? head(dag_cus2) : none;
        case PAIR_BATCH: return dag && 2 * dag_cus + 32 <= num_cu ? StreamSplit{dag_cus, dag_cus, 2 * dag_cus, num_cu - 2 * dag_cus, true} : none;
        case PAIR_SMALL: return arg > 0 && arg <= num_cu ? head(arg) : none;
        case PAIR_PANEL: return arg > 0 && arg < num_cu ? head(arg) : none;
    }
    return none;
}

std::vector<uint32_t> cu_mask_words(int total_cu, int first, int count) {
    std::vector<uint32_t> m((total_cu + 31) / 32, 0u);
    for (int bit = std::max(first, 0); bit < first + count && bit < total_cu; ++bit) m[bit / 32] |= 1u << (bit % 32);
    return m;
}

// The dispatcher deals the workgroups of a grid out evenly -- XCD by XCD, and inside an XCD shader engine by shader engine --
// whatever the mask left of an engine, so the engine with the fewest CUs bounds what is resident at once: 16 chain CUs take one CU
// from engines 0 and 1 of every XCD, which then hold 7 x 3 = 21 workgroups each, and of a grid of 3 x 240 = 720 exactly
// 32 x 21 = 672 start (seen in round 4 with a build whose bulk workgroups recorded their CU -- removed, record in
// profiles/r04_stall_captures.md: 21 / 21 / 22 / 21-22 workgroups per engine, 35 CUs of engines 2 and 3 holding two).  The others are placed LATER, in mid-kernel, when the hardware finds room -- and a workgroup
// placed in mid-kernel is what the one-in-~3000 time-out of the task-DAG schedule was: in both captured
// events 6 resp. 12 workgroups with block ids 672..686 had all just been started, within 0.2 ms of each other, took a task
// each, and then did nothing for the ~965 ms until the time-out sent the others home -- at which point each ran its whole
// task at the usual 13 us per tile column.  Tasks they held were ones the pivot chain needed.  (They were never in a wait of
// their own, and polling with a back-off changed nothing.  Why the hardware stalls them is not known; a persistent grid
// simply must not exceed what is co-resident at launch.)  Those workgroups did 0.9 % of the tasks.
int grid_at_launch(int cu_first, int num_cu, int first, int per_cu) {
    int per_engine[32] = {0};
    for (int b = std::max(first, 0); b < num_cu; ++b) ++per_engine[cu_xcd(cu_first + b) * 4 + cu_engine(cu_first + b)];
    int engines = 0, least = INT_MAX;
    for (int e = 0; e < 32; ++e)
        if (per_engine[e] > 0) { ++engines; least = std::min(least, per_engine[e]); }
    return engines > 0 ? per_cu * least * engines : per_cu;
}

int bulk_xcds(int cu_first, int num_cu, int first) {
    bool has[8] = {false, false, false, false, false, false, false, false};
    for (int b = std::max(first, 0); b < num_cu; ++b) has[cu_xcd(cu_first + b)] = true;
    int n = 0;
    for (bool x : has) n += x ? 1 : 0;
    return n;
}

// The chains' CU partition is a multiple of 32 CUs: every workgroup of the chain launch must be RESIDENT (one per CU), and
// the dispatcher places them all only when the mask gives every shader engine of every XCD the same number of CUs --
// 8 XCDs x 4 SEs = 32 (tools/hip/mask_resident.hip: masks of 32 / 64 / 96 / 192 / 256 bits hold as many 96-KB workgroups
// as they have bits; 40, 48, 56, 72, 104, 176 do not, e.g. 34 workgroups on a 40-bit mask: 32 resident -- five 34-strip
// systems on 176 CUs stalled into the schedule's time-out).
// (... and of 64, so that a process ends up with three such stream pairs at most: every masked stream is a hardware queue,
// and the device runs only so many of them side by side -- ctx.hip, mnk_ctx_create)
int small_chain_cus(int k, int strips, int num_cu) { return std::min(num_cu, (k * strips + 63) / 64 * 64); }

SmallRounds small_rounds(int strips, int num_cu, bool has_bulk) {
    const int bulk_min = has_bulk ? std::max(32, num_cu / 4) : 0;
    int kmax = std::min(32, (num_cu - bulk_min) / strips);
    while (kmax > 1 && small_chain_cus(kmax, strips, num_cu) > num_cu - bulk_min) --kmax;
    return {bulk_min, kmax};
}

}  // namespace mnk

// ---- host-only entries for tests and tools (include/madnlp_hip.h) ----
extern "C" int mnk_debug_grid_at_launch(int cu_first, int num_cu, int first, int per_cu) { return mnk::grid_at_launch(cu_first, num_cu, first, per_cu); }

extern "C" int mnk_debug_stream_split(int kind, int num_cu, int dag_cus, int dag_cus2, int arg, int* split, int32_t* chain_mask,
                                      int32_t* rest_mask) {
    if (kind < 0 || kind >= mnk::PAIR_KINDS || num_cu <= 0 || !split || !chain_mask || !rest_mask) return -1;
    if (kind == mnk::PAIR_PANEL && arg < 0) arg = mnk::panel_default_cus(num_cu);
    const mnk::StreamSplit s = mnk::stream_split(kind, num_cu, dag_cus, dag_cus2, arg);
    split[0] = s.chain_first; split[1] = s.chain_count; split[2] = s.rest_first; split[3] = s.rest_count;
    const std::vector<uint32_t> mc = mnk::cu_mask_words(num_cu, s.chain_first, s.chain_count), mr = mnk::cu_mask_words(num_cu, s.rest_first, s.rest_count);
    std::copy(mc.begin(), mc.end(), chain_mask);
    std::copy(mr.begin(), mr.end(), rest_mask);
    return s.exists ? 1 : 0;
}

extern "C" int mnk_debug_small_rounds(int strips, int num_cu, int has_bulk, int k, int* out) {
    if (strips <= 0 || num_cu <= 0 || k < 0 || !out) return -1;
    const mnk::SmallRounds r = mnk::small_rounds(strips, num_cu, has_bulk != 0);
    out[0] = r.bulk_min; out[1] = r.kmax; out[2] = mnk::small_chain_cus(k, strips, num_cu);
    return 0;
}

// The CU-mask rules of the hot path: which mask bits each stream of a CU-masked pair gets, the mask words of a bit range, the size
// of a persistent grid on a mask, and the chain partitions of a round of small factorizations.  Host only and plain C++ -- no HIP
// header, no runtime call, no kernel -- so the unit (stream_plan.hip) also compiles with a host compiler and runs under its
// sanitizers (tools/stream_plan_check.cpp), and a CPU test checks the rules (tests/test_stream_plan_cpu.py).  The executor that
// makes, keeps and destroys the streams is ctx.hip; the environment (MNK_DAG_CUS, MNK_DAG_CUS2, MNK_PANEL_CUS) is read there.
//
// Mask bit b is CU b / 8 of XCD b % 8, in shader engine (b / 8) % 4 of that XCD.  A contiguous range of bits therefore takes the
// same number of CUs from every XCD (masks that differ between XCDs are not honoured by the runtime: tools/cumask_probe.hip).
//
// A pair is a chain stream `sp` on the bits [chain_first, chain_first + chain_count) and a stream `su` on
// [rest_first, rest_first + rest_count) for the work beside it.  The kinds:
//   PAIR_DAG           pivot chain | bulk kernel of the task-DAG schedule: [0, dag_cus) | the rest; from DAG_MIN_CUS CUs on
//   PAIR_DEEP          its deep band (every row of a small system in the chain's band): [0, dag_cus2) | the rest, 0 < dag_cus2 < num_cu
//   PAIR_BATCH         batches: a second chain partition and a bulk stream outside both, [dag_cus, 2 dag_cus) | [2 dag_cus, num_cu);
//                      only where that leaves the bulk kernel 32 CUs
//   PAIR_SMALL(c)      rounds of small systems, chains side by side: [0, c) | the rest, which may be empty (no `su` then)
//   PAIR_PANEL(want)   look-ahead of the launch-per-panel schedules, per context: [0, want) | the rest, 0 < want < num_cu
// DEEP and BATCH exist only beside a DAG pair.
#pragma once
#include <cstdint>
#include <vector>

namespace mnk {

constexpr int DAG_MIN_CUS = 64;             // smaller devices have no task-DAG pair
constexpr int DAG_CUS_DEFAULT = 16;         // chain CUs of PAIR_DAG (two per XCD) ...
constexpr int DAG_CUS2_DEFAULT = 96;        // ... and of PAIR_DEEP, unless the environment says otherwise

inline int cu_xcd(int bit) { return bit % 8; }
inline int cu_engine(int bit) { return (bit / 8) % 4; }

enum StreamPairKind : int32_t { PAIR_DAG = 0, PAIR_DEEP = 1, PAIR_BATCH = 2, PAIR_SMALL = 3, PAIR_PANEL = 4, PAIR_KINDS = 5 };

struct StreamSplit {
    int chain_first, chain_count, rest_first, rest_count;
    bool exists;   // false: no such pair on this device with these sizes
};
// `dag_cus`, `dag_cus2`: the chain CUs of PAIR_DAG / PAIR_DEEP (0: none); `arg`: c of PAIR_SMALL, want of PAIR_PANEL.
StreamSplit stream_split(int kind, int num_cu, int dag_cus, int dag_cus2, int arg);
// want of PAIR_PANEL where nobody asks for another: a quarter of the CUs, at least 4, from 16 CUs on (0: no masked pair)
int panel_default_cus(int num_cu);

// The words of a CU mask of `total_cu` bits with the bits [first, first + count) set (those outside the device are dropped).
std::vector<uint32_t> cu_mask_words(int total_cu, int first, int count);

// Size of a persistent grid on the CUs [first, num_cu) of a device part that starts at mask bit `cu_first` (`per_cu` workgroups
// fit on a CU): the workgroups the hardware places AT LAUNCH; see stream_plan.hip.
int grid_at_launch(int cu_first, int num_cu, int first, int per_cu);
// XCDs that have a CU among those CUs
int bulk_xcds(int cu_first, int num_cu, int first);

// Rounds of small systems of `strips` 64-row strips each (dag_batch.hip): the chains of k systems run side by side on
// small_chain_cus(k, ..) CUs, at most `kmax` per round (< 2: no room for two chains), and the bulk kernel -- if the systems have
// bulk tasks at all -- keeps at least `bulk_min` CUs.
int small_chain_cus(int k, int strips, int num_cu);
struct SmallRounds { int bulk_min, kmax; };
SmallRounds small_rounds(int strips, int num_cu, bool has_bulk);

}  // namespace mnk

// The CU-mask rules (csrc/stream_plan.hip) as a host program under the host compiler's sanitizers: no HIP, no device, not loaded
// into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++
//       madnlp.jl_amd/csrc/stream_plan.hip tools/stream_plan_check.cpp -o /tmp/stream_plan_check && /tmp/stream_plan_check
//
// Runs the grid of tests/test_stream_plan_cpu.py -- every pair kind over the CU counts, chain sizes and arguments of the test,
// through stream_split / cu_mask_words and through the host-only entry mnk_debug_stream_split; the chain partitions of small-system
// rounds; grid_at_launch and bulk_xcds over every prefix of the masks -- checks that the two masks of a pair are disjoint, inside
// the device and as large as the split says, that the entries return what the planner built and write nothing behind their arrays,
// and prints the counts and one FNV-1a hash over everything planned, to compare two builds.  Any sanitizer report or failed check
// ends it with a non-zero status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madnlp.jl_amd/csrc/stream_plan.h"
#include "../include/madnlp_hip.h"

using namespace mnk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static uint64_t g_hash = 1469598103934665603ull;
static void mix(int64_t v) { g_hash = (g_hash ^ (uint64_t)v) * 1099511628211ull; }

static int popcount(const std::vector<uint32_t>& m) {
    int n = 0;
    for (uint32_t w : m) n += __builtin_popcount(w);
    return n;
}

int main() {
    long nsplits = 0, npairs = 0, nrounds = 0;
    for (int num_cu : {16, 32, 63, 64, 96, 128, 255, 256, 304})
        for (int dag_cus : {0, 8, 16, 32})
            for (int dag_cus2 : {0, 96, num_cu})
                for (int kind = 0; kind < PAIR_KINDS; ++kind) {
                    std::vector<int> args{0};
                    if (kind == PAIR_SMALL) { for (int c = 64; c <= num_cu + 64; c += 64) args.push_back(c); args.push_back(num_cu); }
                    if (kind == PAIR_PANEL) args = {-1, 0, 4, num_cu / 4, num_cu};
                    for (int arg : args) {
                        const int a = kind == PAIR_PANEL && arg < 0 ? panel_default_cus(num_cu) : arg;
                        const StreamSplit s = stream_split(kind, num_cu, dag_cus, dag_cus2, a);
                        const size_t words = (size_t)(num_cu + 31) / 32;
                        const std::vector<uint32_t> mc = cu_mask_words(num_cu, s.chain_first, s.chain_count), mr = cu_mask_words(num_cu, s.rest_first, s.rest_count);
                        CHECK(mc.size() == words && mr.size() == words);
                        if (s.exists) {
                            CHECK(s.chain_first >= 0 && s.chain_count > 0 && s.rest_count >= 0 && s.chain_first + s.chain_count <= s.rest_first && s.rest_first + s.rest_count == num_cu);
                            CHECK(popcount(mc) == s.chain_count && popcount(mr) == s.rest_count);
                            for (size_t w = 0; w < words; ++w) CHECK((mc[w] & mr[w]) == 0);
                            if (num_cu % 32) CHECK(((mc[words - 1] | mr[words - 1]) >> (num_cu % 32)) == 0);
                            CHECK(s.rest_count > 0 || kind == PAIR_SMALL);
                            ++npairs;
                        } else CHECK(s.chain_first == 0 && s.chain_count == 0 && s.rest_first == 0 && s.rest_count == 0 && popcount(mc) == 0 && popcount(mr) == 0);
                        // the entry the tests call: the same split and words, nothing written behind them
                        int split[5] = {-77, -77, -77, -77, -77};
                        std::vector<uint32_t> ec(words + 1, 0xdeadbeefu), er(words + 1, 0xdeadbeefu);
                        CHECK(mnk_debug_stream_split(kind, num_cu, dag_cus, dag_cus2, arg, split, (int32_t*)ec.data(), (int32_t*)er.data()) == (s.exists ? 1 : 0));
                        CHECK(split[0] == s.chain_first && split[1] == s.chain_count && split[2] == s.rest_first && split[3] == s.rest_count && split[4] == -77);
                        CHECK(ec[words] == 0xdeadbeefu && er[words] == 0xdeadbeefu);
                        for (size_t w = 0; w < words; ++w) { CHECK(ec[w] == mc[w] && er[w] == mr[w]); mix(mc[w]); mix(mr[w]); }
                        mix(s.exists); mix(s.chain_first); mix(s.chain_count); mix(s.rest_first); mix(s.rest_count);
                        ++nsplits;
                    }
                }
    // persistent grids: bounded by CUs x per_cu, never zero, and every XCD with a CU counted
    for (int num_cu : {16, 64, 128, 255, 256, 304})
        for (int cu_first : {0, 16, 128})
            for (int first = -1; first <= num_cu; ++first) {
                const int g = grid_at_launch(cu_first, num_cu, first, 3), x = bulk_xcds(cu_first, num_cu, first);
                const int cus = num_cu - (first < 0 ? 0 : first);
                CHECK(g >= 3 && g <= 3 * (cus > 0 ? cus : 1) && x >= 0 && x <= 8 && (x > 0) == (cus > 0) && x <= (cus > 0 ? cus : 0));
                CHECK(mnk_debug_grid_at_launch(cu_first, num_cu, first, 3) == g);
                mix(g); mix(x);
            }
    CHECK(grid_at_launch(0, 256, 16, 3) == 672 && bulk_xcds(0, 256, 16) == 8);
    // rounds of small systems
    for (int num_cu : {64, 128, 256, 304})
        for (int strips : {4, 8, 11, 20, 34, 40, 84})
            for (int has_bulk = 0; has_bulk < 2; ++has_bulk) {
                const SmallRounds r = small_rounds(strips, num_cu, has_bulk != 0);
                CHECK(r.kmax <= 32 && r.bulk_min == (has_bulk ? (num_cu / 4 > 32 ? num_cu / 4 : 32) : 0));
                for (int k = 1; k <= r.kmax; ++k) {
                    const int c = small_chain_cus(k, strips, num_cu);
                    CHECK((c % 64 == 0 || c == num_cu) && k * strips <= c && c <= num_cu);
                    if (r.kmax >= 2) CHECK(num_cu - c >= r.bulk_min);
                    int out[4] = {-77, -77, -77, -77};
                    CHECK(mnk_debug_small_rounds(strips, num_cu, has_bulk, k, out) == 0);
                    CHECK(out[0] == r.bulk_min && out[1] == r.kmax && out[2] == c && out[3] == -77);
                    mix(c);
                }
                mix(r.kmax);
                ++nrounds;
            }
    CHECK(small_chain_cus(5, 34, 256) == 192);
    int out[3];
    int32_t m[16];
    CHECK(mnk_debug_stream_split(PAIR_KINDS, 256, 16, 96, 0, out, m, m) == -1);
    CHECK(mnk_debug_stream_split(0, 0, 16, 96, 0, out, m, m) == -1);
    CHECK(mnk_debug_stream_split(0, 256, 16, 96, 0, nullptr, m, m) == -1);
    CHECK(mnk_debug_small_rounds(0, 256, 1, 1, out) == -1);
    std::printf("stream_plan_check: %ld splits, %ld pairs, %ld round plans, hash %016llx, all checks passed\n", nsplits, npairs, nrounds,
                (unsigned long long)g_hash);
    return 0;
}

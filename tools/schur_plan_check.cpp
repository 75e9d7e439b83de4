// The planner of the Schur stage's device-side assembly (csrc/schur_plan.hip) as a host program under the host compiler's
// sanitizers: no HIP, no device, not loaded into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++
//       madnlp.jl_amd/csrc/schur_plan.hip tools/schur_plan_check.cpp -o /tmp/schur_plan_check && /tmp/schur_plan_check
//
// The same structures go through schur_spmv_plan (the row lists of the device-side products of solve_kkt! / mul!): see the checks
// at the end of the loop.
//
// Random two-stage structures (one row mask for all scenarios, duplicated COO entries, every subset of the scenarios local, with
// and without the design block, thresholds from 0 to never) through schur_assembly_plan and mnk_debug_schur_assembly_plan: checks
// what the kernels of schur.hip need of a plan -- every segment inside [A | C | S0] and its sources inside the value arrays, every
// staging slot inside the operands, on an element no other slot writes and off the padding's rows, the long rows in ascending slack
// order -- and that rows are long exactly when they have more entries than the threshold, and prints the counts and one FNV-1a hash
// over everything planned, to compare two builds.  Any sanitizer report or failed check ends it with a non-zero status.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madnlp.jl_amd/csrc/schur_plan.h"
#include "../include/madnlp_hip.h"

namespace mnk {
void set_error(const char*, ...) {}   // (ls.hip in the library)
}
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
    long nplans = 0, nlong = 0, nslots = 0, nterms = 0;
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t ns = 1 + rnd(4), nv = 1 + rnd(70), nd = 1 + rnd(70), nc = 1 + rnd(24), nc_eq = rnd((int)nc + 1);
        const int64_t n = ns * nv + nd, m = ns * nc, off = ns * nv, base = rnd(2);
        const int dens = 1 + rnd(10);
        std::vector<int32_t> jI, jJ, hI, hJ;
        std::vector<std::vector<int>> cols(nc);
        for (int64_t i = 0; i < nc; ++i)
            for (int64_t c = 0; c < nv + nd; ++c)
                if (rnd(10) < dens) cols[i].push_back((int)c);
        for (int64_t k = 0; k < ns; ++k)
            for (int64_t i = 0; i < nc; ++i)
                for (int c : cols[i]) { jI.push_back((int32_t)(k * nc + i + base)); jJ.push_back((int32_t)((c < nv ? k * nv + c : off + c - nv) + base)); }
        for (int d = rnd(4); d > 0 && !jI.empty(); --d) { const int e = rnd((int)jI.size()); jI.push_back(jI[e]); jJ.push_back(jJ[e]); }
        for (int64_t i = 0; i < n; ++i) { hI.push_back((int32_t)(i + base)); hJ.push_back((int32_t)(i + base)); }
        hI.push_back((int32_t)(off + base)); hJ.push_back((int32_t)(base));   // a coupling entry
        std::vector<int64_t> ind_eq, ind_ineq;
        for (int64_t k = 0; k < ns; ++k)
            for (int64_t i = 0; i < nc; ++i) (i < nc_eq ? ind_eq : ind_ineq).push_back(k * nc + i + base);
        std::vector<int64_t> len(m, 0);
        for (int32_t r : jI) ++len[r - base];
        for (int mask = 1; mask < (1 << ns); ++mask) {
            std::vector<int64_t> local;
            for (int64_t k = 0; k < ns; ++k)
                if (mask >> k & 1) local.push_back(k);
            const int64_t nl = (int64_t)local.size(), blk = nv + nc_eq;
            const int64_t Ts[4] = {0, (int64_t)rnd(40), -1, INT64_MAX};
            for (int64_t Tin : Ts) {
                const int own = rnd(2);
                const SchurPatterns in{nl, blk, nd, n, m, nv, nc, (int64_t)hI.size(), hI.data(), hJ.data(), (int64_t)jI.size(), jI.data(), jJ.data(),
                                       (int64_t)ind_ineq.size(), ind_ineq.data(), (int64_t)ind_eq.size(), ind_eq.data(), (int)base, ns,
                                       local.data(), own, Tin};
                SchurAssemblyPlan p;
                const char* err = schur_assembly_plan(in, p);
                CHECK(err == nullptr);
                const int64_t T = Tin < 0 ? SCHUR_GRAM_DEFAULT_T : Tin;
                CHECK(p.T == T && p.nvp % 64 == 0 && p.nvp >= nv && p.nvp < nv + 64 && p.ndp % 64 == 0 && p.ndp >= nd && p.ndp < nd + 64);
                // long rows: exactly the local inequality rows with more than T entries, ascending slack order per scenario
                CHECK((int64_t)p.long_p.size() == nl);
                int64_t total = 0, R = 0;
                for (int64_t kl = 0; kl < nl; ++kl) {
                    std::vector<int32_t> want;
                    for (int64_t q = 0; q < (int64_t)ind_ineq.size(); ++q) {
                        const int64_t r = ind_ineq[q] - base;
                        if (r / nc == local[kl] && len[r] > T) want.push_back((int32_t)q);
                    }
                    CHECK(want == p.long_p[kl]);
                    total += (int64_t)want.size();
                    R = std::max<int64_t>(R, (int64_t)want.size());
                }
                CHECK(p.long_rows == total && p.R == R && p.Kp % 16 == 0 && p.Kp >= R && p.Kp < R + 16);
                // segments and sources
                const int64_t sizeAll = nl * blk * blk + nl * nd * blk + nd * nd;
                CHECK(p.seg_ptr.size() == p.seg_dst.size() + 1 && p.seg_ptr.front() == 0 && p.seg_ptr.back() == p.nsrc());
                for (size_t t = 0; t < p.seg_dst.size(); ++t) {
                    CHECK(p.seg_dst[t] >= 0 && p.seg_dst[t] < sizeAll && p.seg_ptr[t] < p.seg_ptr[t + 1] && (t == 0 || p.seg_dst[t - 1] < p.seg_dst[t]));
                }
                int64_t pairs = 0;
                for (int64_t q = 0; q < p.nsrc(); ++q) {
                    const int kind = p.kind[q];
                    CHECK(kind >= 0 && kind <= 4 && p.a[q] >= 0);
                    if (kind == 0) CHECK(p.a[q] < (int64_t)hI.size());
                    if (kind == 1) CHECK(p.a[q] < (int64_t)jI.size());
                    if (kind == 2) CHECK(p.a[q] < n);
                    if (kind == 3) CHECK(p.a[q] < m);
                    if (kind == 4) {
                        CHECK(p.a[q] < (int64_t)jI.size() && p.b[q] >= 0 && p.b[q] < (int64_t)jI.size() && p.w[q] >= 0 && p.w[q] < (int64_t)ind_ineq.size());
                        CHECK(jI[p.a[q]] == jI[p.b[q]] && jI[p.a[q]] - base == ind_ineq[p.w[q]] - base && len[jI[p.a[q]] - base] <= T);
                        ++pairs;
                    }
                }
                // staging slots
                const int64_t sizeW = p.size_wv() + p.size_wd();
                CHECK(p.slot_ptr.size() == p.slot_dst.size() + 1 && p.slot_p.size() == p.slot_dst.size() && p.slot_ptr.front() == 0 &&
                      p.slot_ptr.back() == (int32_t)p.slot_src.size());
                int64_t staged_entries = 0;
                for (size_t t = 0; t < p.slot_dst.size(); ++t) {
                    const int64_t d = p.slot_dst[t];
                    CHECK(d >= 0 && d < sizeW && (t == 0 || p.slot_dst[t - 1] < d) && p.slot_ptr[t] < p.slot_ptr[t + 1]);
                    const bool design = d >= p.size_wv();
                    const int64_t ld = design ? p.ndp : p.nvp, e = design ? d - p.size_wv() : d;
                    const int64_t kl = e / (ld * p.Kp), j = e % (ld * p.Kp) / ld, c = e % ld;
                    CHECK(kl < nl && j < (int64_t)p.long_p[kl].size() && c < (design ? nd : nv) && p.slot_p[t] == p.long_p[kl][j]);
                    for (int32_t q = p.slot_ptr[t]; q < p.slot_ptr[t + 1]; ++q) {
                        const int32_t s = p.slot_src[q];
                        CHECK(s >= 0 && s < (int32_t)jI.size() && (q == p.slot_ptr[t] || p.slot_src[q - 1] < s));   // COO order
                        CHECK(jI[s] - base == ind_ineq[p.slot_p[t]] - base);
                        const int64_t col = jJ[s] - base;
                        CHECK(design ? col - off == c : col - local[kl] * nv == c);
                        ++staged_entries;
                    }
                }
                int64_t want_entries = 0;
                for (int64_t kl = 0; kl < nl; ++kl)
                    for (int32_t q : p.long_p[kl]) want_entries += len[ind_ineq[q] - base];
                CHECK(staged_entries == want_entries);
                if (T == INT64_MAX) CHECK(p.long_rows == 0 && p.staged_doubles() == 0 && p.slot_dst.empty());
                // the host-only entry returns the same five numbers
                int64_t a[5], b[6] = {0, 0, 0, 0, 0, -77};
                p.stats(a);
                CHECK(mnk_debug_schur_assembly_plan(n, m, nv, nc, (int64_t)hI.size(), hI.data(), hJ.data(), (int64_t)jI.size(), jI.data(), jJ.data(),
                                                    (int64_t)ind_ineq.size(), ind_ineq.data(), (int64_t)ind_eq.size(), ind_eq.data(), (int)base, ns,
                                                    local.data(), own, nl, blk, nd, Tin, b, 5) == 0);
                CHECK(std::equal(a, a + 5, b) && b[5] == -77 && a[3] == 2 * nl * p.Kp * (p.nvp + p.ndp));
                CHECK(mnk_debug_schur_assembly_plan(n, m, nv, nc, (int64_t)hI.size(), hI.data(), hJ.data(), (int64_t)jI.size(), jI.data(), jJ.data(),
                                                    (int64_t)ind_ineq.size(), ind_ineq.data(), (int64_t)ind_eq.size(), ind_eq.data(), (int)base, ns,
                                                    local.data(), own, nl, blk + 1, nd, Tin, b, 5) < 0);
                for (int i = 0; i < 5; ++i) mix(a[i]);
                for (int64_t v : p.seg_dst) mix(v);
                for (int64_t v : p.slot_dst) mix(v);
                ++nplans; nlong += p.long_rows; nslots += (long)p.slot_dst.size(); nterms += (long)pairs;
                // the row lists of the device-side products (schur_spmv_plan): a single rank's only; what schur_spmv_rows_kernel and
                // schur_spmv_long_kernel need of them -- pointers ascending from 0 to the entry count, every column inside the
                // operand vector, every position inside the COO value array and ascending within a row (COO order), the long rows
                // exactly the rows above the threshold, ascending
                SchurPatterns whole = in;
                whole.local_scen = nullptr;
                whole.ns_local = ns;
                SchurSpmvPlan sp;
                if (nl < ns || !own) {
                    CHECK(schur_spmv_plan(in, Tin, sp) != nullptr);
                }
                whole.own_design = 1;
                CHECK(schur_spmv_plan(whole, Tin, sp) == nullptr && sp.T == T);
                const int64_t nnzj = (int64_t)jI.size(), nnzh = (int64_t)hI.size();
                const int64_t rows_of[3] = {m, n, n}, cols_of[3] = {n, m, n}, vals_of[3] = {nnzj, nnzj, nnzh};
                for (int w = 0; w < 3; ++w) {
                    const SchurSpmvOp& op = sp.op[w];
                    CHECK(op.rows == rows_of[w] && (int64_t)op.ptr.size() == op.rows + 1 && op.ptr.front() == 0 && op.ptr.back() == op.nnz() &&
                          op.perm.size() == op.idx.size());
                    CHECK(w == SCHUR_OP_H ? op.nnz() >= nnzh && op.nnz() <= 2 * nnzh : op.nnz() == nnzj);
                    std::vector<int32_t> lng;
                    for (int64_t r = 0; r < op.rows; ++r) {
                        CHECK(op.ptr[r] <= op.ptr[r + 1]);
                        if ((int64_t)op.ptr[r + 1] - op.ptr[r] > T) lng.push_back((int32_t)r);
                        for (int32_t q = op.ptr[r]; q < op.ptr[r + 1]; ++q) {
                            CHECK(op.idx[q] >= 0 && op.idx[q] < cols_of[w] && op.perm[q] >= 0 && op.perm[q] < vals_of[w]);
                            CHECK(q == op.ptr[r] || op.perm[q - 1] <= op.perm[q]);
                            const int32_t e = op.perm[q];
                            if (w == SCHUR_OP_J) CHECK(jI[e] - base == r && jJ[e] - base == op.idx[q]);
                            if (w == SCHUR_OP_JT) CHECK(jJ[e] - base == r && jI[e] - base == op.idx[q]);
                            if (w == SCHUR_OP_H)
                                CHECK((hI[e] - base == r && hJ[e] - base == op.idx[q]) || (hJ[e] - base == r && hI[e] - base == op.idx[q]));
                        }
                    }
                    CHECK(lng == op.long_rows);
                    mix(op.nnz());
                    for (int32_t v : op.long_rows) mix(v);
                }
                CHECK((int64_t)sp.eq_rows.size() == (int64_t)ind_eq.size() && std::is_sorted(sp.eq_rows.begin(), sp.eq_rows.end()));
            }
        }
    }
    std::printf("schur_plan_check: %ld plans, %ld long rows, %ld staging slots, %ld pair terms, hash %016llx\n", nplans, nlong, nslots, nterms,
                (unsigned long long)g_hash);
    return 0;
}

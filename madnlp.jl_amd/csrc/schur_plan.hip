// The planner of the Schur stage's device-side assembly (schur_plan.h): layout checks, source lists, long rows and staging slots.
// Plain C++: no HIP header, no runtime call, no kernel.
#include "schur_plan.h"

#include <algorithm>
#include <utility>

namespace mnk {

void set_error(const char* fmt, ...);   // (ls.hip; declared here to keep this unit free of the HIP headers of common.h)

namespace {
inline int64_t plan_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
}  // namespace

#define SCHUR_PLAN_REQUIRE(cond, msg) \
    do {                              \
        if (!(cond)) return msg;      \
    } while (0)

const char* schur_assembly_plan(const SchurPatterns& in, SchurAssemblyPlan& out) {
    const int64_t n = in.n, m = in.m, nv = in.nv, nc = in.nc, nnzh = in.nnzh, nnzj = in.nnzj, n_ineq = in.n_ineq, n_eq = in.n_eq;
    const int32_t *hess_I = in.hess_I, *hess_J = in.hess_J, *jac_I = in.jac_I, *jac_J = in.jac_J;
    const int64_t *ind_ineq = in.ind_ineq, *ind_eq = in.ind_eq, *local_scen = in.local_scen;
    const int index_base = in.index_base, own_design = in.own_design;
    const int64_t ns_local = in.ns_local;
    SCHUR_PLAN_REQUIRE(ns_local >= 0 && in.blk > 0 && in.nd > 0, "mnk_schur_set_structure: bad dimensions");
    SCHUR_PLAN_REQUIRE(index_base == 0 || index_base == 1, "mnk_schur_set_structure: index_base must be 0 or 1");
    SCHUR_PLAN_REQUIRE(nnzh >= 0 && nnzj >= 0 && n_ineq >= 0 && n_eq >= 0, "mnk_schur_set_structure: bad dimensions");
    SCHUR_PLAN_REQUIRE((nnzh == 0 || (hess_I && hess_J)) && (nnzj == 0 || (jac_I && jac_J)) && (n_ineq == 0 || ind_ineq) && (n_eq == 0 || ind_eq),
                       "mnk_schur_set_structure: NULL pattern");
    const int64_t ns = local_scen ? in.ns_global : ns_local, nd = in.nd, blk = in.blk;
    SCHUR_PLAN_REQUIRE(ns >= ns_local && nv > 0 && nc >= 0, "mnk_schur_set_structure: bad dimensions");
    SCHUR_PLAN_REQUIRE(n == ns * nv + nd && m == ns * nc, "mnk_schur_set_structure: n, m do not match ns * nv + nd, ns * nc");
    SCHUR_PLAN_REQUIRE(n_eq + n_ineq == m && n_eq % std::max<int64_t>(ns, 1) == 0 && n_ineq % std::max<int64_t>(ns, 1) == 0,
                       "mnk_schur_set_structure: the scenarios have different numbers of equality / inequality constraints");
    const int64_t nc_eq = ns > 0 ? n_eq / ns : 0;
    SCHUR_PLAN_REQUIRE(blk == nv + nc_eq, "mnk_schur_set_structure: the stage's block order is not nv + (equality rows per scenario)");
    SCHUR_PLAN_REQUIRE(nnzh < 2000000000 && nnzj < 2000000000 && n + n_ineq < 2000000000, "mnk_schur_set_structure: structure exceeds int32 range");
    const int64_t T = in.T < 0 ? SCHUR_GRAM_DEFAULT_T : in.T;
    const int64_t off = ns * nv;
    // global scenario -> local block (or -1)
    std::vector<int64_t> loc_of(ns, -1);
    for (int64_t i = 0; i < ns_local; ++i) {
        const int64_t g = local_scen ? local_scen[i] : i;
        SCHUR_PLAN_REQUIRE(g >= 0 && g < ns && loc_of[g] < 0, "mnk_schur_set_structure: bad local scenario list");
        loc_of[g] = i;
    }
    // equality rows: local index = rank among the scenario's equality rows (ascending); inequality rows: slack index
    std::vector<int64_t> eq_local(m, -1), slack_of(m, -1);
    {
        std::vector<int64_t> eq_sorted(ind_eq, ind_eq + n_eq);
        for (auto& r : eq_sorted) r -= index_base;
        std::sort(eq_sorted.begin(), eq_sorted.end());
        std::vector<int64_t> cnt(ns, 0);
        for (int64_t r : eq_sorted) {
            SCHUR_PLAN_REQUIRE(r >= 0 && r < m, "mnk_schur_set_structure: equality index out of range");
            const int64_t k = nc > 0 ? r / nc : 0;
            eq_local[r] = cnt[k]++;
        }
        for (int64_t k = 0; k < ns; ++k)
            SCHUR_PLAN_REQUIRE(cnt[k] == nc_eq, "mnk_schur_set_structure: the scenarios have different numbers of equality / inequality constraints");
        for (int64_t p = 0; p < n_ineq; ++p) {
            const int64_t r = ind_ineq[p] - index_base;
            SCHUR_PLAN_REQUIRE(r >= 0 && r < m && eq_local[r] < 0 && slack_of[r] < 0, "mnk_schur_set_structure: bad inequality index");
            slack_of[r] = p;
        }
    }
    auto scen = [&](int64_t var) -> int64_t { return var < off ? var / nv : -1; };
    struct Src { int64_t dst; int8_t kind; int32_t a, b, w; };
    std::vector<Src> src;
    const int64_t sizeA = ns_local * blk * blk, sizeC = ns_local * nd * blk;
    auto putA = [&](int64_t kl, int64_t r, int64_t c, int8_t kind, int64_t a, int64_t b = 0, int64_t w = 0) {
        src.push_back(Src{kl * blk * blk + r + c * blk, kind, (int32_t)a, (int32_t)b, (int32_t)w});
    };
    auto putC = [&](int64_t kl, int64_t d, int64_t c, int8_t kind, int64_t a, int64_t b = 0, int64_t w = 0) {
        src.push_back(Src{sizeA + kl * nd * blk + d + c * nd, kind, (int32_t)a, (int32_t)b, (int32_t)w});
    };
    auto putS = [&](int64_t r, int64_t c, int8_t kind, int64_t a, int64_t b = 0, int64_t w = 0) {
        src.push_back(Src{sizeA + sizeC + r + c * nd, kind, (int32_t)a, (int32_t)b, (int32_t)w});
    };
    // Hessian entries (forced to the lower triangle, matrixtools.jl:129-137): scenario block, coupling block, design block
    for (int64_t e = 0; e < nnzh; ++e) {
        int64_t i = hess_I[e] - index_base, j = hess_J[e] - index_base;
        SCHUR_PLAN_REQUIRE(i >= 0 && i < n && j >= 0 && j < n, "mnk_schur_set_structure: Hessian index out of range");
        if (j > i) std::swap(i, j);
        const int64_t si = scen(i), sj = scen(j);
        if (si >= 0 && sj >= 0) {
            SCHUR_PLAN_REQUIRE(si == sj, "mnk_schur_set_structure: a Hessian entry couples two scenarios");
            const int64_t kl = loc_of[si];
            if (kl < 0) continue;
            const int64_t li = i - si * nv, lj = j - sj * nv;
            putA(kl, li, lj, 0, e);
            if (li != lj) putA(kl, lj, li, 0, e);
        } else if (si < 0 && sj < 0) {
            if (!own_design) continue;
            putS(i - off, j - off, 0, e);
            if (i != j) putS(j - off, i - off, 0, e);
        } else {   // (lower triangle: the design variable is the row)
            const int64_t kl = loc_of[sj];
            if (kl >= 0) putC(kl, i - off, j - sj * nv, 0, e);
        }
    }
    // diagonal terms
    for (int64_t k = 0; k < ns; ++k) {
        const int64_t kl = loc_of[k];
        if (kl < 0) continue;
        for (int64_t j = 0; j < nv; ++j) putA(kl, j, j, 2, k * nv + j);
    }
    for (int64_t r = 0; r < m; ++r)
        if (eq_local[r] >= 0 && loc_of[r / nc] >= 0) putA(loc_of[r / nc], nv + eq_local[r], nv + eq_local[r], 3, r);
    if (own_design)
        for (int64_t j = 0; j < nd; ++j) putS(j, j, 2, off + j);
    // Jacobian entries of equality rows; the entries of every inequality row in COO order
    std::vector<std::vector<std::pair<int32_t, int64_t>>> row_entries(m);
    for (int64_t e = 0; e < nnzj; ++e) {
        const int64_t r = jac_I[e] - index_base, c = jac_J[e] - index_base;
        SCHUR_PLAN_REQUIRE(r >= 0 && r < m && c >= 0 && c < n, "mnk_schur_set_structure: Jacobian index out of range");
        const int64_t k = r / nc;
        SCHUR_PLAN_REQUIRE(c >= off || c / nv == k, "mnk_schur_set_structure: a constraint reaches the variables of another scenario");
        const int64_t kl = loc_of[k];
        if (kl < 0) continue;
        if (eq_local[r] >= 0) {
            const int64_t li = eq_local[r];
            if (c < off) { putA(kl, nv + li, c - k * nv, 1, e); putA(kl, c - k * nv, nv + li, 1, e); }
            else putC(kl, c - off, nv + li, 1, e);
        } else {
            row_entries[r].push_back({(int32_t)e, c});
        }
    }
    // the long rows of every local scenario, in ascending slack order; the pairs the short ones will add (counted before they are made:
    // a dense row of 400 entries in each of 16 000 rows is 2.6e9 of them)
    out.long_p.assign((size_t)ns_local, std::vector<int32_t>());
    out.long_rows = 0;
    uint64_t npairs = 0;
    for (int64_t p = 0; p < n_ineq; ++p) {
        const int64_t r = ind_ineq[p] - index_base, kl = loc_of[r / nc];
        if (kl < 0) continue;
        const uint64_t len = row_entries[r].size();
        if ((int64_t)len > T) { out.long_p[kl].push_back((int32_t)p); ++out.long_rows; }
        else {   // (a pair of a scenario column with a design column lands in C_dk once, not twice)
            uint64_t lv = 0;
            for (const auto& e1 : row_entries[r]) lv += e1.second < off ? 1 : 0;
            npairs += len * len - lv * (len - lv);
        }
    }
    SCHUR_PLAN_REQUIRE(src.size() + npairs < (uint64_t)2000000000,
                       "mnk_schur_set_structure: too many assembly terms: the pair lists of the inequality rows grow with the square of a row's "
                       "length -- lower the Gram row threshold (mnk_schur_set_gram_threshold, gram_row_threshold) so that long rows take the Gram path");
    out.R = 0;
    for (const auto& lp : out.long_p) out.R = std::max<int64_t>(out.R, (int64_t)lp.size());
    out.T = T;
    out.nvp = plan_round_up(nv, SCHUR_GRAM_TILE);
    out.ndp = plan_round_up(nd, SCHUR_GRAM_TILE);
    out.Kp = plan_round_up(out.R, SCHUR_GRAM_BK);
    SCHUR_PLAN_REQUIRE(ns_local * out.Kp < 2000000000, "mnk_schur_set_structure: structure exceeds int32 range");
    // inequality rows.  Short: J' D J over A_k, C_dk and S0, one pair of entries at a time (_scatter_quad_add!, schur.jl:966-972).
    // Long: one staging slot per distinct column, its entries in COO order.
    struct Slot { int64_t dst; int32_t e, p; };
    std::vector<Slot> slots;
    const int64_t sizeWv = out.size_wv();
    std::vector<int64_t> next_long((size_t)ns_local, 0);
    for (int64_t p = 0; p < n_ineq; ++p) {
        const int64_t r = ind_ineq[p] - index_base, k = r / nc, kl = loc_of[k];
        if (kl < 0) continue;
        const auto& ents = row_entries[r];
        if ((int64_t)ents.size() > T) {
            const int64_t j = next_long[kl]++;
            for (const auto& e1 : ents) {
                const int64_t c = e1.second;
                const int64_t dst = c < off ? kl * out.nvp * out.Kp + (c - k * nv) + j * out.nvp
                                            : sizeWv + kl * out.ndp * out.Kp + (c - off) + j * out.ndp;
                slots.push_back(Slot{dst, e1.first, (int32_t)p});
            }
            continue;
        }
        for (const auto& e1 : ents)
            for (const auto& e2 : ents) {
                const int64_t c1 = e1.second, c2 = e2.second;
                if (c1 < off && c2 < off) putA(kl, c1 - k * nv, c2 - k * nv, 4, e1.first, e2.first, p);
                else if (c1 >= off && c2 < off) putC(kl, c1 - off, c2 - k * nv, 4, e1.first, e2.first, p);
                else if (c1 >= off && c2 >= off) putS(c1 - off, c2 - off, 4, e1.first, e2.first, p);
            }
    }
    std::stable_sort(src.begin(), src.end(), [](const Src& x, const Src& y) { return x.dst < y.dst; });
    out.seg_dst.clear(); out.seg_ptr.clear();
    out.a.resize(src.size()); out.b.resize(src.size()); out.w.resize(src.size()); out.kind.resize(src.size());
    for (size_t q = 0; q < src.size(); ++q) {
        if (q == 0 || src[q].dst != src[q - 1].dst) { out.seg_dst.push_back(src[q].dst); out.seg_ptr.push_back((int32_t)q); }
        out.kind[q] = src[q].kind; out.a[q] = src[q].a; out.b[q] = src[q].b; out.w[q] = src[q].w;
    }
    out.seg_ptr.push_back((int32_t)src.size());
    std::stable_sort(slots.begin(), slots.end(), [](const Slot& x, const Slot& y) { return x.dst < y.dst; });
    out.slot_dst.clear(); out.slot_ptr.clear(); out.slot_p.clear();
    out.slot_src.resize(slots.size());
    for (size_t q = 0; q < slots.size(); ++q) {
        if (q == 0 || slots[q].dst != slots[q - 1].dst) {
            out.slot_dst.push_back(slots[q].dst); out.slot_ptr.push_back((int32_t)q); out.slot_p.push_back(slots[q].p);
        }
        out.slot_src[q] = slots[q].e;
    }
    out.slot_ptr.push_back((int32_t)slots.size());
    out.ineq0.resize((size_t)n_ineq);
    for (int64_t p = 0; p < n_ineq; ++p) out.ineq0[p] = ind_ineq[p] - index_base;
    return nullptr;
}

namespace {
// rows of `op` from (row, column, COO position) triples given in COO order: a counting sort keeps that order within a row
void spmv_rows(SchurSpmvOp& op, int64_t rows, const std::vector<int32_t>& r, const std::vector<int32_t>& c, const std::vector<int32_t>& e,
               int64_t T) {
    op.rows = rows;
    op.ptr.assign((size_t)rows + 1, 0);
    for (int32_t x : r) ++op.ptr[(size_t)x + 1];
    for (int64_t i = 0; i < rows; ++i) op.ptr[(size_t)i + 1] += op.ptr[(size_t)i];
    op.idx.resize(r.size());
    op.perm.resize(r.size());
    std::vector<int32_t> next(op.ptr.begin(), op.ptr.end() - 1);
    for (size_t q = 0; q < r.size(); ++q) {
        const int32_t at = next[(size_t)r[q]]++;
        op.idx[(size_t)at] = c[q];
        op.perm[(size_t)at] = e[q];
    }
    op.long_rows.clear();
    for (int64_t i = 0; i < rows; ++i)
        if ((int64_t)op.ptr[(size_t)i + 1] - op.ptr[(size_t)i] > T) op.long_rows.push_back((int32_t)i);
}
}  // namespace

const char* schur_spmv_plan(const SchurPatterns& in, int64_t T_in, SchurSpmvPlan& out) {
    const int64_t n = in.n, m = in.m, nnzh = in.nnzh, nnzj = in.nnzj;
    const int base = in.index_base;
    SCHUR_PLAN_REQUIRE(in.local_scen == nullptr && in.own_design,
                       "mnk_schur_set_structure: the device-side products need a single rank (a sharded handle -- scenarios on other ranks "
                       "or a design block it does not own -- has none)");
    SCHUR_PLAN_REQUIRE(base == 0 || base == 1, "mnk_schur_set_structure: index_base must be 0 or 1");
    SCHUR_PLAN_REQUIRE(n > 0 && m >= 0 && nnzh >= 0 && nnzj >= 0 && in.n_eq >= 0, "mnk_schur_set_structure: bad dimensions");
    SCHUR_PLAN_REQUIRE((nnzh == 0 || (in.hess_I && in.hess_J)) && (nnzj == 0 || (in.jac_I && in.jac_J)) && (in.n_eq == 0 || in.ind_eq),
                       "mnk_schur_set_structure: NULL pattern");
    SCHUR_PLAN_REQUIRE(2 * nnzh < 2000000000 && nnzj < 2000000000 && n < 2000000000 && m < 2000000000,
                       "mnk_schur_set_structure: structure exceeds int32 range");
    const int64_t T = T_in < 0 ? SCHUR_SPMV_DEFAULT_T : T_in;
    out.T = T;
    std::vector<int32_t> r, c, e;
    r.reserve((size_t)nnzj); c.reserve((size_t)nnzj); e.reserve((size_t)nnzj);
    for (int64_t q = 0; q < nnzj; ++q) {
        const int64_t i = in.jac_I[q] - base, j = in.jac_J[q] - base;
        SCHUR_PLAN_REQUIRE(i >= 0 && i < m && j >= 0 && j < n, "mnk_schur_set_structure: Jacobian index out of range");
        r.push_back((int32_t)i); c.push_back((int32_t)j); e.push_back((int32_t)q);
    }
    spmv_rows(out.op[SCHUR_OP_J], m, r, c, e, T);
    spmv_rows(out.op[SCHUR_OP_JT], n, c, r, e, T);
    r.clear(); c.clear(); e.clear();
    for (int64_t q = 0; q < nnzh; ++q) {   // Symmetric(H, :L): the entry and, off the diagonal, its mirror image, in COO order
        int64_t i = in.hess_I[q] - base, j = in.hess_J[q] - base;
        SCHUR_PLAN_REQUIRE(i >= 0 && i < n && j >= 0 && j < n, "mnk_schur_set_structure: Hessian index out of range");
        if (j > i) std::swap(i, j);
        r.push_back((int32_t)i); c.push_back((int32_t)j); e.push_back((int32_t)q);
        if (i != j) { r.push_back((int32_t)j); c.push_back((int32_t)i); e.push_back((int32_t)q); }
    }
    spmv_rows(out.op[SCHUR_OP_H], n, r, c, e, T);
    out.eq_rows.assign(in.ind_eq, in.ind_eq + in.n_eq);
    for (auto& x : out.eq_rows) {
        x -= base;
        SCHUR_PLAN_REQUIRE(x >= 0 && x < m, "mnk_schur_set_structure: equality index out of range");
    }
    std::sort(out.eq_rows.begin(), out.eq_rows.end());
    return nullptr;
}

}  // namespace mnk

// ---- host-only entry for tests and tools (include/madnlp_hip.h) ----
extern "C" int mnk_debug_schur_assembly_plan(int64_t n, int64_t m, int64_t nv, int64_t nc, int64_t nnzh, const int32_t* hess_I,
                                             const int32_t* hess_J, int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J,
                                             int64_t n_ineq, const int64_t* ind_ineq, int64_t n_eq, const int64_t* ind_eq, int index_base,
                                             int64_t ns_global, const int64_t* local_scen, int own_design, int64_t ns_local, int64_t blk,
                                             int64_t nd, int64_t T, int64_t* out, int cap) {
    if (!out || cap < 5) { mnk::set_error("mnk_debug_schur_assembly_plan: out needs room for five numbers"); return -1; }
    const mnk::SchurPatterns in{ns_local, blk, nd, n, m, nv, nc, nnzh, hess_I, hess_J, nnzj, jac_I, jac_J, n_ineq, ind_ineq,
                                n_eq, ind_eq, index_base, ns_global, local_scen, own_design, T};
    mnk::SchurAssemblyPlan plan;
    if (const char* err = mnk::schur_assembly_plan(in, plan)) { mnk::set_error("%s", err); return -1; }
    plan.stats(out);
    return 0;
}

// The row lists of one operator (which: 0 J, 1 J', 2 Symmetric(H, :L)) as mnk_schur_set_structure would build them with the
// product threshold T: counts = {rows, entries, long rows, T in force}; any of the four arrays may be NULL (a first call sizes them).
extern "C" int mnk_schur_spmv_plan(int64_t n, int64_t m, int64_t nv, int64_t nc, int64_t nnzh, const int32_t* hess_I, const int32_t* hess_J,
                                   int64_t nnzj, const int32_t* jac_I, const int32_t* jac_J, int64_t n_ineq, const int64_t* ind_ineq,
                                   int64_t n_eq, const int64_t* ind_eq, int index_base, int64_t ns_global, const int64_t* local_scen,
                                   int own_design, int64_t T, int which, int32_t* row_ptr, int32_t* col_idx, int32_t* perm,
                                   int32_t* long_rows, int64_t* counts) {
    if (which < 0 || which > 2 || !counts) { mnk::set_error("mnk_schur_spmv_plan: which must be 0 (J), 1 (J') or 2 (H), counts not NULL"); return -1; }
    const mnk::SchurPatterns in{ns_global, 0, 0, n, m, nv, nc, nnzh, hess_I, hess_J, nnzj, jac_I, jac_J, n_ineq, ind_ineq,
                                n_eq, ind_eq, index_base, ns_global, local_scen, own_design, -1};
    mnk::SchurSpmvPlan plan;
    if (const char* err = mnk::schur_spmv_plan(in, T, plan)) { mnk::set_error("%s", err); return -1; }
    const mnk::SchurSpmvOp& op = plan.op[which];
    counts[0] = op.rows; counts[1] = op.nnz(); counts[2] = (int64_t)op.long_rows.size(); counts[3] = plan.T;
    if (row_ptr) std::copy(op.ptr.begin(), op.ptr.end(), row_ptr);
    if (col_idx) std::copy(op.idx.begin(), op.idx.end(), col_idx);
    if (perm) std::copy(op.perm.begin(), op.perm.end(), perm);
    if (long_rows) std::copy(op.long_rows.begin(), op.long_rows.end(), long_rows);
    return 0;
}

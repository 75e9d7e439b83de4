// The planner of the Schur stage's device-side assembly (mnk_schur_set_structure / mnk_schur_assemble): from the COO patterns of a
// two-stage problem and the Gram row threshold T it makes
//   * the SOURCE LISTS: one segment per touched entry of [A | C | S0], its sources in the reference's scatter order (Hessian
//     entries, diagonal terms, equality-row Jacobian entries, the condensation pairs J' D J of the SHORT inequality rows:
//     schur.jl:935-972) -- what schur_assemble_kernel sums, one thread per segment;
//   * the LONG ROWS: an inequality row with more than T COO entries (duplicates counted) contributes no pairs -- their number
//     grows with the square of the row's length.  Its entries are staged into dense, zero-padded operands per local scenario
//     (Wv_k: nvp x Kp, Wd_k: ndp x Kp, element (column c, long row j) at c + j * ld; the weighted twins D W share the offsets) and
//     the condensation becomes three weighted Gram products on the matrix cores (schur.hip: schur_gram_kernel);
//   * the STAGING SLOT LISTS: one segment per distinct (long row, column), its COO entries in COO order -- duplicates are summed by
//     one thread in that order (schur_gram_stage_kernel).
// Host only and plain C++ -- no HIP header, no runtime call, no kernel -- so the unit (schur_plan.hip) also compiles with a host
// compiler and runs under its sanitizers (tools/schur_plan_check.cpp), and a CPU test checks the rules through
// mnk_debug_schur_assembly_plan (tests/test_schur_gram_plan_cpu.py).  The executor that uploads a plan and launches what it says is
// in schur.hip.
#pragma once
#include <cstdint>
#include <vector>

namespace mnk {

constexpr int64_t SCHUR_GRAM_DEFAULT_T = 64;   // rows with more COO entries than this take the Gram path
constexpr int64_t SCHUR_GRAM_TILE = 64;        // the Gram kernel's workgroup tile: nv and nd are padded to it
constexpr int64_t SCHUR_GRAM_BK = 16;          // ... and its k-tile depth: the long rows of a scenario are padded to it

// The arguments of mnk_schur_set_structure and the three numbers of the handle they are checked against.
struct SchurPatterns {
    int64_t ns_local, blk, nd;
    int64_t n, m, nv, nc;
    int64_t nnzh;
    const int32_t *hess_I, *hess_J;
    int64_t nnzj;
    const int32_t *jac_I, *jac_J;
    int64_t n_ineq;
    const int64_t* ind_ineq;
    int64_t n_eq;
    const int64_t* ind_eq;
    int index_base;
    int64_t ns_global;
    const int64_t* local_scen;   // NULL: all scenarios are local, in order
    int own_design;
    int64_t T;                   // Gram row threshold; negative: SCHUR_GRAM_DEFAULT_T; INT64_MAX: never
};

struct SchurAssemblyPlan {
    // source lists (schur_assemble_kernel): kind 0 hess[a], 1 jac[a], 2 pr_diag[a], 3 du_diag[a], 4 jac[a] * D[w] * jac[b]
    std::vector<int64_t> seg_dst;   // virtual offset into [A | C | S0]
    std::vector<int32_t> seg_ptr, a, b, w;
    std::vector<int8_t> kind;
    std::vector<int64_t> ineq0;     // 0-based constraint row of slack p
    // long rows
    int64_t T = 0;                  // the threshold in force
    int64_t R = 0;                  // long rows of a local scenario (the largest count, should the scenarios differ)
    int64_t long_rows = 0;          // ... over the local scenarios
    int64_t nvp = 0, ndp = 0, Kp = 0;
    std::vector<std::vector<int32_t>> long_p;   // per local scenario: the slack indices of its long rows, ascending
    // staging slots (schur_gram_stage_kernel): slot t sums jac[slot_src[q]], q in [slot_ptr[t], slot_ptr[t + 1]), into offset
    // slot_dst[t] of [Wv_0 .. | Wd_0 ..] and writes D[slot_p[t]] times the sum at the same offset of the weighted twin
    std::vector<int64_t> slot_dst;
    std::vector<int32_t> slot_ptr, slot_src, slot_p;
    int64_t size_wv() const { return (int64_t)long_p.size() * nvp * Kp; }
    int64_t size_wd() const { return (int64_t)long_p.size() * ndp * Kp; }
    int64_t staged_doubles() const { return 2 * (size_wv() + size_wd()); }
    int64_t nsrc() const { return (int64_t)kind.size(); }
    int64_t nseg() const { return (int64_t)seg_dst.size(); }
    // out[0] pair-list terms, out[1] segments, out[2] long rows over the local scenarios, out[3] staged doubles, out[4] T
    void stats(int64_t* out) const { out[0] = nsrc(); out[1] = nseg(); out[2] = long_rows; out[3] = staged_doubles(); out[4] = T; }
};

// Checks the layout (what _build_schur_symbolic checks, schur.jl:140-236) and fills `out`.  Returns nullptr, or the message of the
// check that failed (a string literal).
const char* schur_assembly_plan(const SchurPatterns& in, SchurAssemblyPlan& out);

// ---- the sparse products of the device-side solve_kkt! / mul! / jtprod! / mul_hess_blk! (mnk_schur_solve_kkt and its kin) ----
// Three operators over the COO value arrays of the last mnk_schur_assemble, each a ROW LIST: the entries of row r are
// q in [ptr[r], ptr[r + 1]), entry q multiplies x[idx[q]] by vals[perm[q]] (perm: position in the COO value array -- there is
// no compress step, duplicates stay separate terms), in COO order within a row.  J: m rows over jac; Jt: n rows over jac;
// H = Symmetric(hess, :L): n rows over hess, every entry forced to the lower triangle and mirrored, a diagonal entry once.
// A row with more than T entries is LONG (the design rows of Jt and H collect entries of every scenario): schur_spmv_long_kernel
// gives it one 64-lane wavefront, the others are summed by one thread each.  `long_rows`: the long rows, ascending.
constexpr int64_t SCHUR_SPMV_DEFAULT_T = 64;   // one entry per lane at the break-even
enum { SCHUR_OP_J = 0, SCHUR_OP_JT = 1, SCHUR_OP_H = 2 };

struct SchurSpmvOp {
    int64_t rows = 0;
    std::vector<int32_t> ptr, idx, perm, long_rows;
    int64_t nnz() const { return (int64_t)idx.size(); }
};

struct SchurSpmvPlan {
    int64_t T = 0;              // the threshold in force
    SchurSpmvOp op[3];          // SCHUR_OP_J, SCHUR_OP_JT, SCHUR_OP_H
    std::vector<int64_t> eq_rows;   // the equality rows in ascending order: scenario k's are [k * nc_eq, (k + 1) * nc_eq) of it
};

// Single rank only (all scenarios local, the design block owned).  T negative: SCHUR_SPMV_DEFAULT_T; INT64_MAX: no long rows.
// Returns nullptr, or the message of the check that failed (a string literal).
const char* schur_spmv_plan(const SchurPatterns& in, int64_t T, SchurSpmvPlan& out);

}  // namespace mnk

// Internal layout of the opaque handles (shared by factor.hip, solve.hip, ls.hip, kkt units).  mnk_ls is the tiled Cholesky / LDL^T solver; QR, LU and EVD live behind mnk_ls_alt and keep their state in their own units.
#pragma once
#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "dag_plan.h"
#include "factor_plan.h"
#include "solve_plan.h"
#include "stream_plan.h"

struct mnk_sc {
    mnk_ctx* ctx = nullptr;
    int64_t n = 0, m = 0, nnzj = 0, nnzh = 0;
    int64_t nnz_jt = 0, nnz_hess = 0, nnz_aug = 0, len_jptr = 0;
    // host copies of the derived structures (0-based)
    std::vector<int32_t> jt_colptr, jt_rowval, h_colptr, h_rowval, aug_colptr, aug_rowval;
    // ENVELOPE per 128-row tile row of the condensed matrix (padding rows of a solver's order are their own first nonzero):
    // tile_env[I] = (first nonzero column over the rows of tile I) / 128.  Row i of a static-pivot L is zero left of row i's
    // first nonzero, so the tiles L(I, J), J < tile_env[I], are exact zeros (the task-DAG bulk kernel skips them, dag.hip)
    std::vector<int32_t> tile_env;
    mnk::DevBuf<int32_t> d_tile_env;
    // the same per 64-row HALF of a tile row, in 64-column units (mnk_tile_envelope with 64-row blocks): tile_envh[2I], tile_envh[2I + 1];
    // tile_env[I] = min of the two / 2.  The bulk kernel's waves skip the k-tiles left of their own half (option "envelope_half")
    std::vector<int32_t> tile_envh;
    mnk::DevBuf<int32_t> d_tile_envh;
    std::vector<int64_t> jt_map, h_map;
    std::vector<int32_t> d_dst, d_src, hp_dst, hp_src, j_dst, j_c, j_k, j_l;
    // device: COO -> CSC segmented transfer (sources grouped by destination slot)
    mnk::DevBuf<int32_t> jt_seg_ptr, jt_seg_src, h_seg_ptr, h_seg_src;
    // device: condensation lists grouped by aug_com slot
    mnk::DevBuf<int32_t> aug_hptr, aug_hsrc;   // per slot: range into hsrc (H.nz indices)
    mnk::DevBuf<int32_t> aug_dsrc;             // per slot: pr_diag index or -1
    mnk::DevBuf<int32_t> aug_jptr, aug_jc, aug_jk, aug_jl;
    mnk::DevBuf<int32_t> aug_row, aug_col;     // coordinates of every aug_com slot (densify)
    mnk::DevBuf<int32_t> d_jt_colptr, d_jt_rowval, d_jt_colidx, d_h_colptr, d_h_rowval, d_h_colidx;
    // device values
    mnk::DevBuf<double> jac_coo, hess_coo, jt_nz, h_nz, aug_nz, diag_buffer, pr_diag, du_diag;
    void* extra = nullptr;  // unit-private device structures (sparse_kkt.hip), owned by the handle
    mnk_lbfgs* lbfgs = nullptr;   // attached compact L-BFGS handle (lbfgs.hip; not owned): solve_kkt! / mul! include its low-rank term
    // dies with the handle: a linear solver that keeps a way back to this handle's matrix (mnk_ls::src) holds a
    // weak reference and refuses to touch a destroyed handle
    std::shared_ptr<int> alive = std::make_shared<int>(0);
};

// Envelope of a lower-triangular pattern of order n per block of `block` rows (128: tile_env, 64: tile_envh; see mnk_sc):
// entries (row[k], col[k]), col <= row; entries outside the order are ignored.  One entry per row block of the order padded to
// 128: (first nonzero column over the block's rows) / block.  A padding row is its own first nonzero, so a block of padding
// rows points at its own diagonal.
inline std::vector<int32_t> mnk_tile_envelope(int64_t n, const int32_t* row, const int32_t* col, int64_t nnz, int64_t block) {
    std::vector<int32_t> fnz(n);
    for (int64_t i = 0; i < n; ++i) fnz[i] = (int32_t)i;
    for (int64_t k = 0; k < nnz; ++k)
        if (row[k] >= 0 && row[k] < n && col[k] < fnz[row[k]]) fnz[row[k]] = col[k];
    const int64_t nblock = (n + 127) / 128 * (128 / block);
    std::vector<int32_t> env(nblock);
    for (int64_t I = 0; I < nblock; ++I) {
        int32_t f = (int32_t)(block * I);
        for (int64_t i = block * I; i < std::min<int64_t>(n, block * I + block); ++i) f = std::min(f, fnz[i]);
        env[I] = (int32_t)(f / block);
    }
    return env;
}

struct mnk_dc {
    mnk_ctx* ctx = nullptr;
    int condensed = 1;
    bool mirror_pending = false;   // build_kkt! wrote the lower triangle only (all the factorization reads); mnk_dc_get_aug mirrors it on demand
    int64_t n = 0, m = 0, ns = 0, n_eq = 0, order = 0;
    std::vector<int64_t> ind_ineq, ind_eq;
    mnk::DevBuf<int64_t> d_ind_ineq, d_ind_eq;
    mnk::DevBuf<double> hess, jac, aug, pr_diag, du_diag, diag_buffer;
    mnk::DevBuf<double> jis;  // sqrt(D)-scaled, zero-padded inequality Jacobian^T workspace
    int64_t ld_jis = 0, kpad = 0, npad = 0;
    void* extra = nullptr;  // unit-private device structures (dense_kkt.hip), owned by the handle
    void* qn = nullptr;     // quasi-Newton state (qn.hip: scalar block + workspace), owned by the handle; NULL until mnk_dc_qn_init
    void* coo = nullptr;    // COO structure and values (dense_coo.hip), owned by the handle; NULL until mnk_dc_coo_attach
    // something other than the COO scatter has written jac / hess since they were last all zero outside the COO structure
    // (mnk_dc_set_jac / mnk_dc_set_hess, a quasi-Newton init or update): mnk_dc_compress_* clears the buffer first, then only
    bool jac_dirty = false, hess_dirty = false;
    std::shared_ptr<int> alive = std::make_shared<int>(0);  // (see mnk_sc::alive)
};
void mnk_dc_qn_release(mnk_dc* dc);   // qn.hip: frees mnk_dc::qn
void mnk_dc_coo_release(mnk_dc* dc);  // dense_coo.hip: frees mnk_dc::coo

struct mnk_ls;
// lbfgs.hip, for the sparse condensed handle an mnk_lbfgs is attached to (w_x, x_x: the n leading entries of device KKT vectors)
int64_t mnk_lbfgs_order(const mnk_lbfgs* qn);
int mnk_lbfgs_solve_correct(mnk_lbfgs* qn, mnk_ls* ls, double* wx);   // w_x -= H W E'w_x behind the condensed solve with `ls` (builds H, T, W when `ls`, its factorization or the memory changed)
int mnk_lbfgs_mul_add(mnk_lbfgs* qn, double* wx, const double* xx, double alpha);   // w_x += alpha E P E'x_x
int mnk_lbfgs_check(mnk_lbfgs* qn, const char* who);   // -4 (and the message) if a singular T has been flagged since the last build; reads a pinned word, no synchronization

// An algorithm that factors the transferred matrix by something other than the tiled Cholesky / LDL^T: QR (qr.hip), LU (lu.hip),
// EVD (evd.hip).  It owns its buffers; the matrix, the factor buffer, dvec, xwork and the pinned words are the solver's.
// ls_alt.hip maps an algorithm to its factory and holds what the three share (the bookkeeping around factor, the loop over
// right-hand sides); the entry points of the tiled path hand over to it with one `if (ls->alt)` each.
struct mnk_ls_alt {
    virtual ~mnk_ls_alt() = default;
    virtual int alloc(mnk_ls* ls) = 0;
    virtual int factor(mnk_ls* ls) = 0;       // enqueues the factorization of the transferred lower triangle and (ls_alt.hip: verdict.queued() follows)
    virtual int fetch_info(mnk_ls* ls) = 0;   // waits for it; verdict.accept() with info and (where the algorithm reveals it) the inertia
    // One right-hand side of N entries on the device, b -> x (x may be b).  Workspace: the solver's xwork BEHIND its first Np
    // entries, which are the staging slot of host-resident right-hand sides (mnk_ls_alt_solve).
    virtual int solve_vec(mnk_ls* ls, const double* b, double* x) = 0;
    virtual const char* no_inertia_message() const { return nullptr; }   // mnk_ls_inertia's refusal; nullptr: fetch_info fills the inertia
    virtual double stat(const char* key) { (void)key; return 0.0; }      // mnk_ls_get_stat keys that belong to one algorithm
};

// The spare factor buffer and its zero-fill (operations: ls.hip).  Sparse sources are scattered into a ZEROED dense buffer (8 Np^2 / 2
// bytes of zeros per factorization: 116 us at C3, HBM-bound).  With `prefill` the zeros are written in the background into a second
// buffer -- on the context's side stream, or (option dag_fill) by DAG_FILL tasks of the factorization's own bulk queue -- and the
// next transfer swaps the two (costs a second factor buffer, so only up to MAX_ROWS).  States:
//   Dirty            no spare buffer, or an old factor in it: the next transfer fills the factor buffer in line
//   Pending          a sparse matrix was transferred; the spare buffer is to be zeroed once its factorization is queued
//   PendingDagFills  ... and the launch that was just queued zeroes it itself
//   ZeroedBySide     a fill on the side stream is queued (ev_zeroed): the next transfer swaps
//   ZeroedByDag      the queue of the factorization queued last zeroes it -- IF that one runs to its end (a time-out or a breakdown
//                    drops the rest of its queue): trusted only once somebody has looked at `info`; failed() takes it back to Dirty
// acquire() leaves Pending (with prefill off: what it found), so a second transfer for the same factorize! (the pivoted tier, a redo
// after a time-out) never swaps the old factor back in; only a COMPLETED queued() makes the other buffer count as zeroed again.
struct SpareFill {
    static constexpr int64_t MAX_ROWS = 24576;
    int prefill = 1;    // option
    bool wanted(int64_t Np) const { return prefill && Np <= MAX_ROWS; }
    int acquire(mnk_ls* ls);      // a sparse transfer begins: a zeroed lower triangle in ls->fact (by swap or in line) on the home stream
    double* dag_target() const { return pending() ? buf.p : nullptr; }   // what the DAG_FILL tasks of the launch being built should zero
    void dag_fills(bool yes) { if (pending()) state = yes ? State::PendingDagFills : State::Pending; }   // ... and whether it took it
    int queued(mnk_ls* ls);       // the factorization has been queued: the side-stream fill, if one is due
    void failed() { if (state == State::ZeroedByDag) state = State::Dirty; }   // the factorization queued last ended with info != 0
    bool give_up();               // memory is short: frees the buffer (and turns prefill off) unless a fill of it is queued
    void destroy(mnk_ctx* ctx);   // waits for the side stream, destroys the events (the buffer frees itself)
   private:
    enum class State { Dirty, Pending, PendingDagFills, ZeroedBySide, ZeroedByDag };
    State state = State::Dirty;
    bool pending() const { return state == State::Pending || state == State::PendingDagFills; }
    bool zeroed() const { return state == State::ZeroedBySide || state == State::ZeroedByDag; }
    mnk::DevBuf<double> buf;
    hipEvent_t ev_zeroed = nullptr, ev_free = nullptr;   // "the fill is done" / "everything queued before the fill has run"
};

// The task-DAG plan: the task list of the schedule for this solver's order (dag_plan.h) and what is derived from it.  Built by
// mnk_ls_dag_prepare (dag.hip) when there is none; every option the list depends on calls invalidate().
struct DagPlan {
    // What batch_flush groups solvers of one device, order and algorithm by, and what (with ntile, the instances and their shift)
    // makes a merged list reusable.  dag_deep_rows and the dag_js2 override enter through js2, dag_fill and prefill through
    // has_fill; dag_xcd_queues and dag_gang only deal the DEVICE list of a single factorization and are not compared.
    struct Key {
        int chunk = 0, taper0 = 0, band = 0;   // the options dag_chunk, dag_taper0, dag_band the list was built with
        int js2 = 0;                           // first strip-column of the second phase
        bool has_fill = false;                 // the list contains DAG_FILL tasks
        bool operator==(const Key& o) const { return chunk == o.chunk && taper0 == o.taper0 && band == o.band && js2 == o.js2 && has_fill == o.has_fill; }
    };
    Key key;
    mnk::DevBuf<int> tasks;                  // 4 ints per task, dealt into the per-XCD queues of the single-factorization bulk kernel (dag_plan.h: dag_deal_list)
    mnk::DagTaskList list;                   // the list as built (kept on the host: a batch merges the lists of its instances, the statistics count from it)
    int nq[2] = {0, 0};                      // queues per phase (0: one queue, the list as built)
    mnk::DevBuf<int> qoff;                   // per phase 16 ints: the nq + 1 offsets of the queues in the phase's part of the list
    mnk::DevBuf<int> qheads;                 // per phase DAG_QHEAD_WORDS ints: the queue heads, 128 bytes apart, then the count of stolen tasks
    mnk::DevBuf<int> flags;                  // progress words [2 queue counters | front: Np/64 | af, tprog: ntile^2 each], zeroed per factorization
    bool valid() const { return tasks.p != nullptr; }
    void invalidate() { tasks.release(); }   // the next task-DAG factorization builds the plan again
    static size_t progress_words(int64_t Np);
    size_t trace_words() const;              // option dag_trace: tasks | chain strips | per-workgroup statistics (2 x 512), 8 words each
};

// What the last factorize! call factored (ls.hip).
struct MatrixSource {
    std::function<int()> retransfer;   // puts the matrix back into `fact` (the pivoted tier, a redo after a time-out, the completion of an early-rejected factorization); empty once the source is gone
    bool persistent = false;           // the source outlives the call (KKT handles): a rejected factorization can be completed later
    // Envelope (options "envelope", "envelope_half"; set_envelope): the device arrays tile_env / tile_envh of the source (a KKT handle's, or
    // env_own / envh_own for a lower CSC), nullptr for dense sources, and their host copies (statistics).  Only the task-DAG schedule reads them.
    const int32_t *env_dev = nullptr, *envh_dev = nullptr;
    std::vector<int32_t> env_host, envh_host;
    bool env_armed = false;            // a transfer may have marked env_word[0] since a task-DAG factorization last consumed it
};

// Back-off of the persistent schedules (4 and 5) after a bounded device-side wait expired: schedule 1 for 16, then 64, 256, ...
// factorizations, then another try (a time-out may have been transient).
struct PersistBackoff {
    int64_t count = 0;                 // factorizations of this solver
    int fallbacks = 0, last_site = 0;  // statistics "pp_fallbacks" / "timeout_site": which wait expired last
    bool blocked_now() { ++count; if (count >= retry_at) blocked = false; return blocked; }   // counts a factorization; true: it keeps to schedule 1
    void wait_expired() { blocked = true; retry_at = count + backoff + 1; backoff *= 4; ++fallbacks; }   // (+1: the redo that follows counts)
   private:
    bool blocked = false;
    int64_t retry_at = 0, backoff = 16;
};

// The verdict of the factorization queued last (operations: factor.hip).  A verdict belongs to ONE factorization: queued() forgets
// the previous one's, "rejected early" included, so a solve that never fetches the info word cannot meet it and refactor a valid
// factor.  Stages and who moves them:
//   None      nothing counts as factorized (a new solver; launch_failed(): a batch launch failed with the NEW matrices in the buffers)
//   Queued    queued(): the launches are in the stream, nothing is known (run_factorization_body, batch_finish, mnk_ls_alt_factorize)
//   Accepted  accept(): info and inertia fetched, the factor is usable (mnk_ls_fetch_info, the fetch_info of QR / LU / EVD)
//   Rejected  reject_early(): stopped at its first non-positive pivot, or never started because the leading-block probe failed:
//             info = 1, the inertia is a lower bound on num_neg and there is NO usable factor (solve / get_factor complete it first)
// pivoted(): the factor in the buffer is the pivoted tier's, P A P^T = L D L^T with 2x2 blocks (bk.hip sets it between Queued and
// Accepted; every queued() and reject_early() clears it, launch_failed() leaves it).
struct FactorVerdict {
    // what a known verdict says (everybody reads, only accept() and reject_early() write) and the statistics "early_rejects",
    // "early_reject_col" (the last valid pivot of the latest one), "early_reject_redone"
    int info = 0;
    int64_t npos = 0, nzero = 0, nneg = 0;
    int64_t early_rejects = 0, early_reject_col = -1, early_reject_redone = 0;
    int64_t serial = 0;   // factorizations queued by this solver: what a cache of something solved with the factor is keyed on (lbfgs.hip)
    void queued() { stage = Stage::Queued; bk = false; ++serial; }
    void launch_failed() { stage = Stage::None; }
    void accept(int info_, int64_t npos_, int64_t nzero_, int64_t nneg_) { stage = Stage::Accepted; info = info_; npos = npos_; nzero = nzero_; nneg = nneg_; }
    void reject_early(int64_t npos_, int64_t nzero_, int64_t N, int64_t col) {   // the one place that writes an early-rejected verdict
        stage = Stage::Rejected; bk = false; info = 1; npos = npos_; nzero = nzero_; nneg = N - npos_ - nzero_;
        ++early_rejects; early_reject_col = col;
    }
    void pivoted() { bk = true; }
    void completed_after_all() { ++early_reject_redone; }   // ensure_complete_factor factored a rejected matrix to the end
    bool has_factorization() const { return stage != Stage::None; }
    bool known() const { return stage == Stage::Accepted || stage == Stage::Rejected; }
    bool usable() const { return stage != Stage::Rejected; }
    bool is_pivoted() const { return bk; }
    int arm_reject(mnk_ls* ls, hipStream_t s);   // sets info[2] on the device (the leaf stops at the first pivot that is not positive) to what this factorization wants
    bool reject_armed() const { return reject_on_device == 1; }
    int record_info_event(hipStream_t s);   // behind finish_info_kernel: mnk_ls_fetch_info waits for THAT point, not for what the caller queued behind it
    int wait_info(hipStream_t s);           // ... or for the stream, while no event has been recorded (QR / LU / EVD never do)
    void destroy() { if (ev_info) (void)hipEventDestroy(ev_info); ev_info = nullptr; }
   private:
    enum class Stage { None, Queued, Accepted, Rejected } stage = Stage::None;
    bool bk = false, ev_info_recorded = false;
    int reject_on_device = -1;           // what info[2] on the device currently says
    hipEvent_t ev_info = nullptr;
};

// LEADING-BLOCK PROBE (operations: ls.hip; option "probe", effective while early rejection is armed): after a rejection that stopped
// in the first half of the columns, a matrix that follows an ACCEPTED one is first probed through its leading principal block (a
// child solver of that order on the same KKT handle) -- probe_leading_block.  History, moved by note_verdict() alone:
//   hint_col       where the last early rejection of the first half stopped (-1: none yet)
//   since_hint     verdicts noted since then (saturating): a rejection in the first half re-arms the hint, every other verdict ages it
//   last_rejected  the verdict noted last was an early rejection (the matrix that follows is the regularized one: no probe)
struct LeadingBlockProbe {
    int on = 1;                          // option "probe"
    int64_t hits = 0, misses = 0;        // statistics: matrices rejected by the probe alone / probes that passed
    void note_verdict(bool rejected, int64_t col, int64_t N) {
        last_rejected = rejected;
        if (rejected && 2 * col < N) { hint_col = col; since_hint = 0; }
        else if (since_hint < (1 << 20)) ++since_hint;
    }
    int64_t order_due(int64_t N) const {   // 0, or the order of the block the next matrix is probed through
        if (last_rejected || hint_col < 0 || since_hint > 3) return 0;
        const int64_t m = (hint_col + 256) / 256 * 256;
        return m >= 512 && 2 * m <= N ? m : 0;
    }
    mnk_ls* child(mnk_ls* ls, int64_t m);   // the child of order m (created, recreated or reused) with the parent's verdict-deciding options; nullptr: no memory, no probe
    void destroy() { if (ls_child) (void)mnk_ls_destroy(ls_child); ls_child = nullptr; }
   private:
    mnk_ls* ls_child = nullptr;          // owned, of order `order`
    int64_t order = 0, hint_col = -1;
    int since_hint = 1 << 20;
    bool last_rejected = false;
};

// The pivoted (Bunch-Kaufman) tier and the growth guard of the static-pivot tier in front of it (operations: bk.hip; BUNCHKAUFMAN
// only; options under the names of their keys).  mnk_ls_fetch_info takes the tier when the static-pivot factorization broke down or grew.
// The guard: the pivots are entries of the successive Schur complements, so max|d_k| / max|a_ij| is a lower bound of the element
// growth of the elimination; dsytrf's pivoting bounds the growth, static pivoting does not on a matrix that is not quasi-definite
// (a pivot of 1e-14 is "not zero" and the next Schur complement is 1e14 times the matrix).  Above bk_growth_tol the factor is
// discarded and the pivoted tier takes over.  SPD matrices never trip it (growth <= 1).  Matrices whose pivots come out "all
// positive, then all negative" have a positive definite leading block and a negative definite Schur complement -- the
// quasi-definite structure of the KKT systems, for which the unpivoted factorization is the intended one and whose growth
// |J|^2 / lambda_min(H) is a property of the data, not of the pivot order: they get the lenient bound bk_growth_tol_qd.
// ran_multi / mw_blocked: the multi-workgroup panel ran last / one of its bounded waits expired once, so run() keeps to one
// workgroup per panel from then on (n_mw_fallbacks counts); only run() moves them.
struct BkTier {
    bool requested = false;      // mnk_ls_create was called with MNK_BUNCHKAUFMAN (MNK_LDL: static pivoting only)
    int bk_fallback = 1;         // option: 0 = never take the pivoted tier (a breakdown is reported as num_zero)
    int bk_panel_wgs = 0;        // option: 0 = a workgroup per 256 rows of the panel, 1 = one workgroup per panel (round 3)
    int bk_max_wgs = 0;          // option: cap on the workgroups of a multi-workgroup panel (0: one per CU); panels with more
                                 // than 256 x this many rows are factored by the one-workgroup kernel
    long bk_spin_limit = 1L << 21;   // option: polls one of its message rounds may take (~1 s) before the tier falls back
    int debug_bk_missing = -1;   // option (tests): a workgroup of the multi-workgroup panel that never takes part
    double bk_growth_tol = 64.0, bk_growth_tol_qd = 1e8;   // options
    double last_growth = 0.0;    // max(|d_k|, |v_ik|) / max|a_ij| of the last static-pivot factorization (diagnostics, tests)
    int64_t last_sign_changes = 0;
    int count = 0;               // how many factorizations took the pivoted tier (diagnostics, tests)
    mnk::DevBuf<unsigned long long> amax_dev;  // [0] max|a_ij| as transferred (folded from the slots below when the info is published), [1] max(|d_k|, |v_ik|) (bit patterns), [2] sign changes of the pivots; [AMAX_SLOT0 + AMAX_STRIDE i]: partial max|a_ij| of the transfer kernels
    bool wanted(const mnk_ls* ls) const;                        // the tier may be needed: the transfers record max|a_ij| (amax_word)
    unsigned long long* growth_word(const mnk_ls* ls) const;    // ... and the word exists: where the kernels being launched fold max(|d|, |v|) (NULL: guard off)
    bool guard_fetched(const mnk_ls* ls) const;                 // ... and there is a way back to the matrix: mnk_ls_fetch_info reads the growth and may act on it
    bool may_take_over(const mnk_ls* ls) const;                 // the pivoted tier may factor again (a zero pivot takes it without the guard: no amax word asked for)
    void note_growth(double am, double dm, int64_t sign_changes) { last_growth = am > 0.0 ? dm / am : (dm > 0.0 ? HUGE_VAL : 0.0); last_sign_changes = sign_changes; }
    bool grew() const { return !(last_growth <= (last_sign_changes <= 1 ? bk_growth_tol_qd : bk_growth_tol)); }
    int run(mnk_ls* ls);                  // factors the matrix in ls->fact with 1x1 / 2x2 pivoting (falls back to one workgroup per panel by itself)
    int permute(mnk_ls* ls, double* x, double* tmp, bool forward);   // x <- P x (forward) / P^T x
    int dsolve(mnk_ls* ls, double* y);                               // y <- D^-1 y, 1x1 / 2x2 blocks
    int inertia(mnk_ls* ls, unsigned long long* out_dev);
    int read_pivots(mnk_ls* ls, int32_t* perm_host, double* doff_host);   // mnk_ls_bk_info (either may be NULL)
    bool multi_last() const { return ran_multi; }
    int mw_fallbacks() const { return n_mw_fallbacks; }
   private:
    int factor(mnk_ls* ls, bool multi);
    mnk::DevBuf<int> perm, ptype;
    mnk::DevBuf<double> doff, dcoup, work;  // (work: the panel's W = L D and its zero-padded copy of L, 2 x Np x 72)
    mnk::DevBuf<char> state;
    // multi-workgroup panel: W by stored row, staging of the per-panel permutation, message ring, rowof | lists
    mnk::DevBuf<double> wv, tmp; mnk::DevBuf<unsigned long long> msg; mnk::DevBuf<int> aux;
    bool ran_multi = false, mw_blocked = false;
    int n_mw_fallbacks = 0;
};

// The state of the solves (operations: solve.hip; options under the names of their keys).  The one-launch (persistent) solve
// publishes its blocks through two buffers used alternately: the next solve polls pub_next, which must be all sentinel (pub_clean),
// and every solve clears the other one in passing; mnk_ls_run_solve and the solve batch move them through the operations below.
// A solve that gives up raises the pinned abort word; take_abort() is the one answer to it: the word is cleared, `persistent_solve`
// goes off for this solver and both publication buffers count as dirty.
struct SolveState {
    int persistent_solve = 1;  // option: both sweeps of a solve in one launch; 0: one launch per step
    int solve512 = 0;          // option: the one-launch solve steps over 512 columns (32-row blocks, 512x512 explicit inverses) from 4096 rows on.  C3: solve! 0.46 -> 0.33 ms, but the extra inverses cost factorize! +0.37 ms (they finish 0.3 ms after the chain): worth it from ~4 solves per factorization
    int linv_mfma = 1;         // option: 256x256 explicit inverses on the matrix cores (0: the scalar LDS kernel, ~70 us per workgroup)
    long ps_spin_limit = 6000000;   // option: polls (~0.5 us each) a persistent-solve wait may take before it gives up
    int debug_ps_missing = -1; // option (tests): this workgroup of the persistent solve leaves at once (a peer that never became resident)
    mnk::DevBuf<double> linv512, linv512t, linv512tmp;
    mnk::DevBuf<unsigned long long> trace;  // diagnostics: 8 time stamps per 64-row block (option solve_trace)
    int last_path = mnk::SOLVE_NONE;        // statistic "solve_path": how this solver's last solve ran (solve_plan.h: SolvePath), noted where the path is chosen
    int64_t multi_rhs_min = 4;              // option: solves of this many right-hand sides or more run blocked (SOLVE_BLOCKED, solve_multi.hip); 0: never.  Default: the smallest count from which the blocked path beat the column loop at N = 2048 and N = 11 192 (profiles/solve_multi_ab.json)
    int last_rhs_chunks = 0;                // statistic "solve_rhs_chunks": passes over the factor per sweep of the last blocked solve
    int create();                            // the pinned abort word
    void destroy();
    int* abort_word() const { return abort; }   // what the solve kernels raise (the host reads it without a sync)
    bool abort_raised() const { return abort && *abort != 0; }
    bool take_abort();                       // after a stream synchronization: true (and the give-up sequence above) if a persistent solve gave up since the last check
    int poll_buffer() const { return pub_next; }
    bool reset_due(int b) { const bool due = !pub_clean[b]; pub_clean[b] = true; return due; }   // b is about to be polled: true if the caller must queue the sentinel fill first
    void dirtied(int b) { pub_clean[b] = false; }   // b was used as scratch (the pivoted tier's permutation, the 512-column solve)
    // a one-launch solve polls poll_buffer() and leaves the other one all sentinel (not with a test's missing workgroup): they swap roles
    void solve_queued(bool other_cleared) { pub_clean[pub_next] = false; pub_clean[pub_next ^ 1] = other_cleared; pub_next ^= 1; }
   private:
    int* abort = nullptr;                // pinned host word
    int pub_next = 0;
    bool pub_clean[2] = {false, false};
};

struct mnk_ls {
    mnk_ctx* ctx = nullptr;
    int64_t N = 0, Np = 0, ld = 0, ldw = 0, nbo = 512;
    bool nbo_auto = true;   // outer_block = 0: the width of the outer panels by size (mnk_ls_effective_nbo)
    int algo = MNK_LDL;
    double pivot_tol = 0.0;
    int lookahead = 1;
    int share = 1;         // look-ahead only: the panel stream's CUs join the trailing update through a tile queue
    int small_tiles = 400;  // (a)-updates with fewer 128x128 tiles than this use 64x64 workgroup tiles
    int64_t single_rows = 2560;  // systems up to this (padded) order are factored as ONE outer panel on the whole chip (with the fused tail panels the look-ahead schedule wins from N = 3072 on: 2.12 vs 2.34 ms at 4096)
    mnk::DevBuf<int> tile_ctr;  // one work-queue counter per outer step
    mnk::DevBuf<double> fact, wbuf[2], linv, dblk, inv16, linv256, linv256t, dvec, dinv, xwork;
    mnk::DevBuf<double> xmulti;   // the blocked solve's two working blocks and its staging block (solve_multi.hip), allocated by the first blocked solve
    SpareFill spare;   // the second factor buffer of sparse sources and its background zero-fill
    int epoch = 0;    // value the hand-off flags of the current factorization carry
    mnk::DevBuf<int> flag_p;
    int algo_now = 1;    // the panel algorithm of the current factorization (panel_algo, or 1 where 4 is not safe)
    PersistBackoff pp;
    double stall_ms_total = 0.0; // host time between the launch of a factorization whose bounded wait expired and the moment the expiry was seen: what the fall-backs of this solver have cost (get_stat "stall_ms_total"; "stall_ms_process": all solvers)
    double t_fact_launch_ms = 0.0;   // host clock (ms) when the current factorization was enqueued
    std::vector<mnk::FactorStep> steps;   // schedules 1 and 4: the steps of the current factorization (factor_plan.h), refilled by every one
    int64_t pp_fuse_rows = 4096; // > 0: once this many rows (or fewer) remain, persistent panel launches apply the columns in front of them themselves
    // task-DAG schedule (panel_algo = 5, dag.hip)
    DagPlan plan;
    int dag_fill = 1;             // option: the zero-fill of the spare factor buffer (sparse sources) runs as DAG_FILL tasks of the bulk queue instead of on a side stream beside the solves
    hipEvent_t ev_defer = nullptr;   // batch: "matrix transferred" on this solver's stream / "batch done"
    bool deferred = false;        // a factorize! call of this solver is pending in an open batch
    int dag_xcd_queues = 1;      // option: 0 = one queue popped by every workgroup
    int dag_gang = 4;             // option: tasks of one group (same B rows, same k-range) dealt to one queue together; < 0: all tasks to queue 0 (tests)
    mnk::DevBuf<double> vfull;    // LDL^T: V = L D of every column, same layout as `fact` (B operand of the left-looking updates)
    mnk::DevBuf<unsigned long long> dag_trace;  // diagnostics (option dag_trace): time stamps per bulk task / chain strip
    bool dag_trace_on = false;
    int64_t inv_done = 0;         // strip-columns whose diagonal blocks the current factorization has already inverted for the solves
    int dag_band = 16;            // 64-row strips per band of the persistent pivot chain (a multiple of 4 in 8..64, i.e. dag_band / 2 tiles; with more strips than the chain has CUs -- 16 unless MNK_DAG_CUS says otherwise -- choose_schedule keeps schedule 4; 8, 12 and 16 run under test)
    int dag_taper0 = 2;           // (1: -0.5 .. -1 % slower, alternating runs on two boxes) length of the last chunk in front of a tile's closing task; the chunks double from there (1, 2, 4, ...)
    long dag_spin_limit = 0;  // option: polls (~0.17 us each) a device-side wait of the schedule may take before it gives up
                              // (info = -7); 0 = by the order of the matrix (mnk_ls_dag_spin_limit)
    int dag_chunk = 64;           // tile columns (of 128) per bulk task behind the doubling taper 1, 2, 4, ... (every task ends with a read-modify-write of its tile; C3 at the end of round 3: 12 -> 9.58 ms, 48 / 64 / 88 / 128 / 1024 -> 9.30; N = 16 384: 26.3 -> 25.9 ms, N = 24 576: 82.0 / 82.5 ms; in the middle of the round, with slower closing tasks, 10-16 was the optimum)
    int64_t dag_min_rows = 1280;  // smaller systems keep the launch-per-panel schedules (round 6, LDL: N = 1024 0.441 (schedule 4) / 0.452 ms (this one), N = 1280 0.573 / 0.551; rounds 3-5: 1536)
    int64_t dag_deep_rows = 5376; // systems up to this order put every row into the chain's band (and at most 64 x MNK_DAG_CUS2 rows); larger ones: band + bulk kernel
    MatrixSource src;
    int envelope = 1, envelope_half = 1;   // options: the bulk kernel skips by the tile envelope of a sparse source / by its 64-row halves too (ignored with envelope = 0)
    mnk::DevBuf<int32_t> env_own, envh_own;   // the envelopes of a lower-CSC source (a KKT handle keeps its own)
    // [0] set by a transfer that met a NaN / Inf entry, [1] that verdict for the factorization being run: dag_reset_kernel moves
    // [0] into [1] and clears [0]; the bulk kernel skips nothing when [1] != 0 (a NaN spreads through 0 * NaN in the dense order)
    mnk::DevBuf<int> env_word;
    bool env_used = false, envh_used = false;   // the last task-DAG factorization was launched with the envelope / the half-tile envelope (statistics)
    int64_t dag_max_rows = 30720; // larger ones too: their trailing updates already run at the update kernel's rate (round 6, LDL, schedule 4 / this one: N = 24 576 87.4 / 81.7 ms, 28 672 133.6 / 128.6, 32 768 188.2 / 190.2; rounds 3-5: 24 576)
    int panel_algo = 5;  // 5: task-DAG schedule (dag.hip: persistent pivot chain + persistent left-looking bulk kernel); 4: persistent panel kernel per 256 columns + one trailing update per outer panel (also what 5 uses outside [dag_min_rows, dag_max_rows]); 1: one launch per piece, the fallback of 4 and 5
    SolveState solves;
    std::vector<std::string> env_keys;   // options fixed by MNK_OPTIONS for this process
    int dag_js2_override = -1;
    int debug_pp_missing = -1;     // tests only: this diagonal strip of every persistent panel launch never publishes
    mnk::DevBuf<int> info_dev;
    mnk::DevBuf<unsigned long long> inertia_dev;
    unsigned long long* pin = nullptr;  // 7 pinned, device-mapped host words: inertia counters, info, max|A|, growth numerator (bit patterns), sign changes are stored here by a kernel
    unsigned long long* pin_dev = nullptr;  // the same words as the device sees them
    FactorVerdict verdict;       // of the factorization queued last
    BkTier bk;                   // the pivoted tier (BUNCHKAUFMAN) and the growth guard in front of it
    int early_reject = 0;        // option (with accept_only_pd): stop the static-pivot LDL^T at the first pivot that is not positive (leaf64.h); the factor
                                 // of a rejected matrix is then not usable and its inertia is a lower bound on num_neg
    LeadingBlockProbe probe;
    int accept_only_pd = 0;      // option: the caller accepts positive definite matrices only: "not PD" from the static tier is final
    bool src_lowrank = false;    // the KKT handle factored last has a compact L-BFGS handle attached: its solves need mnk_sc_solve_kkt (mnk_ls_solve_batch refuses)
    int dag_debug = 0;           // option: keep the progress words of a factorization that timed out (mnk_ls_debug_dag_state)
    mnk::DevBuf<int> dag_dbg;    // 8 words per chain strip (PpDag::dbg)
    std::vector<int> dbg_flags, dbg_chain;
    std::unique_ptr<mnk_ls_alt> alt;   // QR / LU / EVD: the algorithm that factors and solves instead of the tiled path (null for CHOLESKY / LDL)
};

int64_t mnk_ls_effective_nbo(const mnk_ls* ls);
std::unique_ptr<mnk_ls_alt> mnk_qr_new();    // qr.hip: blocked Householder QR (dgeqrf / ormqr / trsv)
std::unique_ptr<mnk_ls_alt> mnk_lu_new();    // lu.hip: blocked LU with partial pivoting (dgetrf / dgetrs)
std::unique_ptr<mnk_ls_alt> mnk_evd_new();   // evd.hip: block Jacobi eigendecomposition (dsyevd)
int mnk_launch_tril_to_full(hipStream_t s, double* F, int64_t ld, int64_t N, int64_t Np);   // qr.hip: upper(F) = lower(F)^T
int mnk_launch_upper_bsolve(hipStream_t s, const double* F, int64_t ld, int64_t Np, double* y, double* x);   // qr.hip: x = U^-1 y (y is overwritten)
std::unique_ptr<mnk_ls_alt> mnk_ls_alt_new(int algo);   // ls_alt.hip: the algorithm's mnk_ls_alt (null for CHOLESKY / LDL)
int mnk_ls_alt_factorize(mnk_ls* ls);   // ls_alt.hip: factorize! of a solver with ls->alt (the matrix has been transferred)
int mnk_ls_alt_solve(mnk_ls* ls, double* x, int64_t nrhs, int64_t ldx, int loc);   // ls_alt.hip: solve! of a solver with ls->alt
int mnk_ls_run_factorization(mnk_ls* ls);
int mnk_ls_run_factorization_now(mnk_ls* ls);      // factor.hip: the launch part (the schedule has been chosen; batches call it for leftovers)
int mnk_ls_launch_finish_info(mnk_ls* ls, hipStream_t s);   // factor.hip: inertia / growth words / info -> pinned host words
bool mnk_solve_defer(mnk_ls* ls, double* xuser);   // solve.hip: true if the calling thread has a solve batch open and queued this solve
int mnk_solve_sync_deferred(mnk_ls* ls);           // solve.hip: runs the queued solves if one of them belongs to this solver
int mnk_solve_batch_flush_pending(void);           // solve.hip: runs every solve the calling thread has queued (nested batches: schur.hip)
int mnk_ls_factorize_dense_dev_async(mnk_ls* ls, const double* Adev, int64_t lda);   // ls.hip
double mnk_host_ms();                               // factor.hip: steady host clock in ms
void mnk_add_process_stall_ms(double ms);           // factor.hip: time lost to expired device-side waits, all solvers of the process
double mnk_process_stall_ms();
bool mnk_ls_pending_elsewhere(const mnk_ls* ls);   // dag_batch.hip: queued in a factorization batch of ANOTHER thread
bool mnk_batch_active();                           // dag_batch.hip: the calling thread has a factorization batch open
size_t mnk_pchain_sys_bytes();                     // factor.hip: size of one record of mnk_launch_pchain_multi's table
int mnk_launch_pchain_multi(mnk_ls* const* v, int n, hipStream_t sp, void* table);   // factor.hip: the chains of n small systems in one launch (table: n records of mnk_pchain_fill_sys, uploaded)
bool mnk_batch_defer(mnk_ls* ls);                  // dag_batch.hip: true if the calling thread has a batch open and took the factorization into it
int mnk_ls_sync_deferred(mnk_ls* ls);              // dag_batch.hip: runs what the open batches of this thread hold for this solver (queued solves, a pending factorization)
int mnk_ls_sync_deferred_fact(mnk_ls* ls);         // dag_batch.hip: ... the pending factorization only
int mnk_ls_fetch_info(mnk_ls* ls);
int mnk_ls_run_factorization_dag(mnk_ls* ls);   // dag.hip: the task-DAG schedule (panel_algo = 5)
int mnk_ls_dag_prepare(mnk_ls* ls);             // dag.hip: its buffers (0: ready; otherwise the device cannot hold them -> schedule 4)
int mnk_launch_pchain(mnk_ls* ls, hipStream_t sp, const mnk::PpDag& dag, int js_begin, int js_end, unsigned strips);  // factor.hip
int mnk_ls_run_solve(mnk_ls* ls, double* xdev /* the solver's work vector */, double* xuser = nullptr /* N entries on the device, or NULL: xdev holds the padded rhs */);
mnk::SolveShape mnk_ls_solve_shape(const mnk_ls* ls);   // solve.hip: what the planner reads of a solver (solve_plan.h)
mnk::SolveMultiPlan mnk_ls_plan_multi(const mnk_ls* ls, int64_t nrhs);   // solve_multi.hip: solve_plan_multi for this solver and its option multi_rhs_min
int mnk_ls_run_solve_multi(mnk_ls* ls, double* x, int64_t nrhs, int64_t ldx, int loc, const mnk::SolveMultiPlan& mp);   // solve_multi.hip: the blocked solve (mp.path == SOLVE_BLOCKED)
int mnk_ls_build_inverses(mnk_ls* ls, hipStream_t s, int64_t sc0, int64_t sc1);  // 256x256 triangles of the strip-columns [sc0, sc1)
int mnk_ls_invert_blocks(mnk_ls* ls, hipStream_t s, int64_t sc0, int64_t sc1);   // 64x64 blocks + 256x256 triangles
// Right-side triangular solve of `nrows` free-standing rows (multiple of 16) against the factored diagonal block that
// starts at column j0: V = B L_jj^-T, X = V D^-1 (LDL) / X = B L_jj^-T (Cholesky).  B is read from / X written to
// Xrows(:, j0:j0+64), V written to Vrows(:, j0:j0+64) (LDL only); both row blocks have leading dimension ldr.
int mnk_ls_right_trsm_rows(mnk_ls* ls, hipStream_t s, int64_t j0, double* Xrows, double* Vrows, int64_t ldr, int64_t nrows);
long mnk_ls_dag_spin_limit(const mnk_ls* ls);   // dag.hip
namespace mnk {
// What a bulk task needs to know about the factorization it belongs to.  One launch may serve SEVERAL independent
// factorizations of the same order (mnk_factorize_batch_*: the task lists of the instances are merged into one queue, each
// task carries its instance index), so these live in a per-instance record instead of the kernel's argument block.
struct DagInst {
    double* F;
    int64_t ld;
    double* V;            // LDL^T: V = L D, same layout as F (the B operand of the updates); Cholesky: nullptr (V = L)
    const double* dinv;   // 1 / d_k
    const double* dblk;   // factored 64x64 diagonal blocks
    const double* inv16;  // inverses of their 16x16 diagonal sub-blocks
    int* front;
    int* af;
    int* tprog;           // [I * ntile + J]: chunks of tile (I, J) that are in memory
    int* info;
    unsigned long long* vmax;   // growth monitor of the static-pivot LDL^T (factor.hip growth_fold): receives max|V|, or NULL
    double* zfill;        // DAG_FILL tasks: the buffer that becomes the NEXT factorization's zeroed factor buffer (or NULL)
    int64_t N;            // order of the matrix (rows / columns N .. Np - 1 are padding: unit diagonal)
    const int* env;       // envelope per tile row (mnk_sc::tile_env): L(I, k) = 0 for tile columns k < env[I]; NULL: dense
    const int* envgate;   // != 0: a NaN / Inf entry was transferred, the envelope is off for this factorization (mnk_ls::env_word)
    const int* envh;      // envelope per 64-row half of a tile row in 64-column units (mnk_sc::tile_envh; only dag_bulk_kernel1 reads it); NULL: none
};
struct SmallSysRec;
// dag.hip, for the batches of dag_batch.hip.  The record of `ls` for its next task-DAG launch, with what the solver remembers
// about that launch (spare fill, env_used / envh_used); `dense`: the launch ignores the envelope.
DagInst dag_prepare_instance(mnk_ls* ls, bool dense);
// dag_reset_kernel for a member of a merged launch: its progress words, info and envelope word; its record goes to `rec_dst`
void dag_reset_member(hipStream_t s, mnk_ls* ls, const DagInst& rec, DagInst* rec_dst);
// ... for a round of `k` small systems of padded order Np (their records and progress words: recs_dev)
void dag_reset_round(hipStream_t s, int64_t Np, const SmallSysRec* recs_dev, int k);
// the bulk kernel of a merged queue (dag_plan.h: dag_merge_tasks) over the instance records `insts`
int launch_dag_bulk_merged(hipStream_t s, bool ldl, const DagInst* insts, const int* tasks, int ntasks, int ntile, int* qctr,
                           long spin_limit, int nwg);

// One system of a batch of SMALL factorizations (dag_batch.hip: batch_run_group_small): what the kernels around the shared chain
// launch need, so that they are ONE launch per batch round instead of one per system (blockIdx.z / .y / .x = system; the
// host's launch rate was the bound: ~8 launches per system, 9 of the 10.9 ms of a 128-scenario Schur build).
struct SmallSysRec {
    int* flags; int64_t nflags; int* info;                 // progress words to zero, the info words (dag_reset_kernel)
    double* F; int64_t ld; const double* dblk; double* linv; double* linv256; double* linv256t; int64_t Np;   // inverses for the solves
    const double* dvec; int64_t ninertia; unsigned long long* pin_dev; const unsigned long long* amax;       // finish_info_kernel
};
}  // namespace mnk
int mnk_ls_invert_blocks_batch(hipStream_t s, bool ldl, const mnk::SmallSysRec* recs_dev, int n, int64_t Np);   // factor.hip (+ solve.hip)
int mnk_ls_build_inverses_batch(hipStream_t s, const mnk::SmallSysRec* recs_dev, int n, int64_t Np);           // solve.hip
int mnk_ls_finish_info_batch(hipStream_t s, const mnk::SmallSysRec* recs_dev, int n, int threads);             // factor.hip
void mnk_ls_fill_small_rec(mnk_ls* ls, mnk::SmallSysRec* rec);                                                  // factor.hip
void mnk_pchain_fill_sys(mnk_ls* ls, void* rec_host, int* front, const int* af);                               // factor.hip (one PcSys record)
int mnk_launch_trsm64_batch(hipStream_t s, bool ldl, const mnk::TrsmBatchRec* recs_dev, int nbatch, int64_t j0, int64_t nrows,
                            int64_t ldr);   // factor.hip
inline bool mnk_ls_take_solve_abort(mnk_ls* ls) { return ls->solves.take_abort(); }   // (SolveState::take_abort, for the KKT units)

// The planner of the launch-per-panel factorization schedules (factor_plan.h): outer panel boundaries, the binary-carry update
// inside an outer panel, the late-columns gate, the (a) split and the shared-(b) decision of the look-ahead schedule, and the
// host-only entry through which the tests and tools read the lists.  Plain C++.
#include "factor_plan.h"

#include <algorithm>

#include "../../include/madnlp_hip.h"

namespace mnk {

int gemm_nt_lower_tiles(int64_t M, int64_t N) {
    const int ntm = (int)((M + 127) / 128), ntn = (int)((N + 127) / 128);
    const int nc = ntn < ntm ? ntn : ntm;
    return nc * ntm - nc * (nc - 1) / 2;
}

namespace {

constexpr int64_t NB = 64;   // one block (common.h: NBI)
// middle-level updates (inside an outer panel) with fewer 128x128 tiles than this use 64x64 workgroup tiles
constexpr int SMALL_TILES_MID = 1000;
constexpr int64_t PP_BLOCKS = 4;  // 64-column blocks per persistent launch (8 was built and measured slower: 197 + 256 registers)

// Columns in front of a persistent launch that it applies itself (ppanel_kernel's prologue); K = 0: none
struct Prologue { int64_t src = 0, K = 0; int rhalf = -1; int64_t rko = 0; };
// Columns of an outer panel from `from` on that another stream delivers late: the first kernel that touches them waits for `event`
struct LateGate { int event = -1, index = 0; int64_t from = 0; };

struct Planner {
    const FactorPlanIn& in;
    std::vector<FactorStep>& steps;

    FactorStep& add(int kind, int stream) {
        steps.push_back(FactorStep{kind, stream, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, -1, 0, 0, 0});
        return steps.back();
    }
    void record(int stream, int event, int64_t index = 0) { FactorStep& s = add(FS_RECORD, stream); s.event = event; s.index = (int32_t)index; }
    void wait(int stream, int event, int64_t index = 0) { FactorStep& s = add(FS_WAIT, stream); s.event = event; s.index = (int32_t)index; }

    // C[col.., col..col+ncols) -= L[.., src..src+K) W^T, W from the buffer `half` of the outer panel that starts at `ko`
    void update(int stream, int variant, int64_t col, int64_t ncols, int64_t src, int64_t K, int half, int64_t ko, int slot = 0, int cus = 0) {
        FactorStep& s = add(FS_UPDATE, stream);
        s.col = (int32_t)col; s.n = (int32_t)ncols; s.rows = (int32_t)(in.Np - col); s.src = (int32_t)src; s.K = (int32_t)K;
        s.variant = variant; s.slot = slot; s.cus = cus;
        if (in.ldl) { s.rhalf = half; s.rko = (int32_t)ko; }
    }

    // One outer panel [ko, kend) on `stream`, its W columns into buffer `half`.  Schedule 1 factors it in units of one block
    // (leaf + triangular solve), schedule 4 in units of one persistent launch of PP_BLOCKS blocks; after `jj` finished units the
    // contribution of the last unit * (jj & -jj) columns is applied to as many columns behind them (binary carry: every column
    // receives every earlier column of the panel exactly once, in updates whose K doubles with their distance).
    void outer_panel(int stream, int64_t ko, int64_t kend, int half, LateGate gate = LateGate(), Prologue pro = Prologue()) {
        const bool pp = in.algo_now == 4;
        const int64_t unit = pp ? NB * PP_BLOCKS : NB;
        const int whalf = in.ldl ? half : -1;
        bool waited = gate.event < 0;
        auto touch = [&](int64_t end) {   // the late-columns gate: before the first kernel that reaches past ko + gate.from
            if (!waited && end > ko + gate.from) { wait(stream, gate.event, gate.index); waited = true; }
        };
        const bool fuse_mid = pp && in.pp_fuse_rows > 0 && in.Np - ko <= in.pp_fuse_rows;
        for (int64_t p = ko; p < kend; p += unit) {
            int64_t p1;
            if (pp) {
                const int64_t nbk = std::min<int64_t>(PP_BLOCKS, (kend - p) / NB);
                p1 = p + NB * nbk;
                touch(p1);
                FactorStep& s = add(FS_PPANEL, stream);
                s.col = (int32_t)p; s.n = (int32_t)nbk; s.whalf = whalf; s.wko = (int32_t)ko;
                if (pro.K > 0) { s.src = (int32_t)pro.src; s.K = (int32_t)pro.K; s.rhalf = in.ldl ? pro.rhalf : -1; s.rko = (int32_t)pro.rko; }
                pro = Prologue();
            } else {
                add(FS_LEAF, stream).col = (int32_t)p;
                p1 = p + NB;
                const int64_t M = in.Np - p1;
                if (M <= 0) break;
                FactorStep& s = add(FS_TRSM, stream);
                // 16-row strips per wave: one while the panel is short (more workgroups, shortest chain), two beyond
                s.col = (int32_t)p; s.n = M / 64 > 2 * (int64_t)in.num_cu ? 2 : 1; s.whalf = whalf; s.wko = (int32_t)ko;
            }
            if (p1 >= kend) break;
            const int64_t jj = (p1 - ko) / unit;   // units of this outer panel that are finished
            const int64_t w = unit * (jj & -jj);    // columns whose contribution is applied now
            const int64_t p0 = p1 - w;
            const int64_t ncols = std::min<int64_t>(w, kend - p1);
            if (fuse_mid && w == unit && ncols <= unit) {  // exactly the next launch's columns: it applies them itself
                pro.src = p0; pro.K = w; pro.rhalf = half; pro.rko = ko;
                continue;
            }
            touch(p1 + ncols);
            update(stream, gemm_nt_lower_tiles(in.Np - p1, ncols) < SMALL_TILES_MID ? FS_SMALL : FS_PLAIN, p1, ncols, p0, w, half, ko);
        }
    }

    FactorPlanShape build() {
        const int64_t Np = in.Np, NBO = in.nbo;
        // Outer panel boundaries.  Once the remaining matrix is small the factorization is bound by the panel
        // chain, not by the update: narrower outer panels (TAIL_NBO) then drop the middle-level update and halve
        // the depth of the (a) piece the chain waits for (measured: 355 -> ~300 us per 512 columns of the tail).
        // The outer panels are TAIL_NBO wide once TAIL_ROWS rows (or fewer) remain: one persistent launch per panel with the
        // fused prologue, no inner update (C3: 11.80 -> 11.71 ms).
        constexpr int64_t TAIL_ROWS = 4096, TAIL_NBO = 256;
        std::vector<int64_t> bnd{0};
        for (int64_t pos = 0; pos < Np;) {
            const bool tail = in.lookahead && NBO < Np && Np - pos <= TAIL_ROWS && TAIL_NBO < NBO;
            pos = std::min<int64_t>(pos + (tail ? TAIL_NBO : NBO), Np);
            bnd.push_back(pos);
        }
        const int64_t npanel = (int64_t)bnd.size() - 1;
        const bool la = in.lookahead && npanel > 1;
        steps.clear();
        if (!la) {   // (without the tail the boundaries are the multiples of NBO)
            for (int64_t k = 0; k < npanel; ++k) {
                const int64_t ko = bnd[k], kend = bnd[k + 1];
                outer_panel(FS_CALLER, ko, kend, 0);
                if (Np - kend > 0) update(FS_CALLER, FS_PLAIN, kend, Np - kend, ko, kend - ko, 0, ko);
            }
            return FactorPlanShape{(int)npanel, false};
        }
        // look-ahead: panel stream (high priority) factors panel k+1 while the update
        // stream applies panel k to the rest of the trailing matrix.
        // One CU partition for every size: a quarter of the CUs for the panel stream.  (A second pair with an
        // eighth, for "update-bound" sizes, measured slower at every N once the panel stream's CUs join the
        // trailing update: N = 30 000 156 vs 178 ms, N = 11 192 +0.5 ms per step taken on it.)
        // Work sharing: while the trailing update is the longer leg, the panel stream's CUs would
        // idle once panel k+1 is factored; (b) is then launched as a tile queue on both streams
        // (update stream right after (a), panel stream after the panel) and the two launches drain
        // one counter.  Estimated leg lengths only decide whether the second launch is worth it.
        const int pcus = in.panel_cus;
        const int ucus = pcus > 0 ? in.num_cu - pcus : in.num_cu;
        // Panel 0 has nothing to overlap with: it runs on the caller's stream, i.e. on the whole chip (its
        // triangular solves and inner updates are throughput-bound at this height), before the fork.
        outer_panel(FS_CALLER, 0, bnd[1], 0);
        record(FS_CALLER, FS_EV_A);
        wait(FS_PANEL, FS_EV_A);
        wait(FS_UPDATE_STREAM, FS_EV_A);
        record(FS_PANEL, FS_EV_PANEL, 0);
        for (int64_t k = 0; k + 1 < npanel; ++k) {
            const int64_t ko = bnd[k], kend = bnd[k + 1];
            const int64_t Mt = Np - kend;
            if (Mt <= 0) break;
            const int64_t nnext = bnd[k + 2] - kend;
            const int half = (int)(k & 1);   // W of panel k; panel k+1 writes the other buffer
            const int64_t Kw = kend - ko;
            // ev_panel[k] is recorded after panel k and after the panel stream's share of (b)_{k-1}
            wait(FS_UPDATE_STREAM, FS_EV_PANEL, k);
            // (a) columns of the next outer panel, delivered in two pieces: the columns the panel stream starts on
            // at once, then the remaining ones (needed only when those are finished)
            auto update_a = [&](int stream, int64_t c0, int64_t c1) {
                update(stream, gemm_nt_lower_tiles(Mt - c0, c1 - c0) < in.small_tiles ? FS_SMALL : FS_PLAIN, kend + c0, c1 - c0, ko, Kw, half, ko);
            };
            // The first OWN_COLS columns of the next panel are updated on the PANEL stream itself, right behind
            // panel k (no cross-stream hand-over before the next pivot block starts); the update stream delivers
            // the other columns while they are being factored.
            // Few rows left (the pivot chain is the critical path): the first persistent launch of the next panel applies
            // panel k to its own 256 columns itself (ppanel_kernel's prologue) -- no (a) kernel and no cross-stream
            // hand-over in front of the chain; the update stream delivers the other columns of the panel meanwhile.
            const bool fuse_a = in.algo_now == 4 && in.pp_fuse_rows > 0 && Mt <= in.pp_fuse_rows && Kw <= 512;
            constexpr int64_t OWN_COLS = 128;
            const bool own_first = !fuse_a && nnext > NB;
            const int64_t n1 = own_first ? std::min<int64_t>(OWN_COLS, nnext - NB) : std::min<int64_t>(256, nnext);
            const bool split_a = nnext > n1;
            if (fuse_a) {
                if (k > 0) wait(FS_PANEL, FS_EV_BDONE, k - 1);  // (b)_{k-1} touched these columns
                if (split_a) {
                    update_a(FS_UPDATE_STREAM, n1, nnext);
                    record(FS_UPDATE_STREAM, FS_EV_NEXT2, k);
                }
            } else if (own_first) {
                if (k > 0) wait(FS_PANEL, FS_EV_BDONE, k - 1);  // (b)_{k-1} touched these columns
                update_a(FS_PANEL, 0, n1);
                update_a(FS_UPDATE_STREAM, n1, nnext);
                record(FS_UPDATE_STREAM, FS_EV_NEXT2, k);
            } else {   // (a next panel of one 64-column block: nothing to split)
                update_a(FS_UPDATE_STREAM, 0, nnext);
                record(FS_UPDATE_STREAM, FS_EV_NEXT, k);
            }
            // (b) the rest of the trailing matrix
            const int64_t Mb = Mt - nnext;
            bool shared_b = false;
            if (Mb > 0) {
                const int ntiles = gemm_nt_lower_tiles(Mb, Mb);
                // CU-us per 128x128xKw tile at ~80 % of the MFMA rate; ~55 us of panel stream per 64 columns
                const double t_upd = ntiles * (68.0 * (double)Kw / 512.0) / ucus;
                const double t_pan = 55.0 * (double)nnext / 64.0 * (pcus > 0 ? 64.0 / pcus : 1.0);
                shared_b = in.share != 0 && pcus > 0 && (t_upd > t_pan || in.share == 2);
                update(FS_UPDATE_STREAM, shared_b ? FS_QUEUE : FS_PLAIN, kend + nnext, Mb, ko, Kw, half, ko, shared_b ? (int)k : 0, shared_b ? ucus : 0);
            }
            record(FS_UPDATE_STREAM, FS_EV_BDONE, k);
            // panel k+1 on the panel stream, as soon as (a) is done
            if (!own_first && !fuse_a) wait(FS_PANEL, FS_EV_NEXT, k);
            LateGate gate;
            if (split_a) gate.event = FS_EV_NEXT2, gate.index = (int)k;
            gate.from = own_first ? n1 : 256;
            Prologue pro;
            if (fuse_a) pro.src = ko, pro.K = Kw, pro.rhalf = half, pro.rko = ko;
            outer_panel(FS_PANEL, kend, kend + nnext, half ^ 1, gate, pro);
            if (shared_b) update(FS_PANEL, FS_QUEUE, kend + nnext, Mb, ko, Kw, half, ko, (int)k, pcus);
            record(FS_PANEL, FS_EV_PANEL, k + 1);
        }
        record(FS_PANEL, FS_EV_A);
        record(FS_UPDATE_STREAM, FS_EV_B);
        wait(FS_CALLER, FS_EV_A);
        wait(FS_CALLER, FS_EV_B);
        return FactorPlanShape{(int)npanel, true};
    }
};

}  // namespace

FactorPlanShape factor_plan_build(const FactorPlanIn& in, std::vector<FactorStep>& steps) { return Planner{in, steps}.build(); }

}  // namespace mnk

// The steps of one factorization of schedule `algo_now` (1 or 4), FACTOR_STEP_INTS (16) ints per step in the order of
// FactorStep's members; at most `cap` steps are written.  Returns the number of steps, -1 on bad arguments.  shape[0] receives
// the number of outer panels, shape[1] whether the look-ahead streams are used.
extern "C" int mnk_debug_factor_plan(int64_t Np, int ldl, int algo_now, int lookahead, int64_t outer_width, int64_t pp_fuse_rows, int share,
                                     int small_tiles, int num_cu, int panel_cus, int32_t* out, int cap, int* shape) {
    if (Np <= 0 || Np % 64 != 0 || Np > (1 << 30) || (algo_now != 1 && algo_now != 4) || outer_width <= 0 || outer_width % 64 != 0 ||
        pp_fuse_rows < 0 || share < 0 || share > 2 || num_cu <= 0 || panel_cus < 0 || panel_cus >= num_cu || cap < 0 || (out == nullptr && cap > 0))
        return -1;
    const mnk::FactorPlanIn in{Np, ldl != 0, algo_now, lookahead != 0, outer_width, pp_fuse_rows, share, small_tiles, num_cu, panel_cus};
    std::vector<mnk::FactorStep> steps;
    const mnk::FactorPlanShape shape_ = mnk::factor_plan_build(in, steps);
    if (shape != nullptr) { shape[0] = shape_.npanel; shape[1] = shape_.lookahead ? 1 : 0; }
    const size_t n = std::min<size_t>(steps.size(), (size_t)cap);
    for (size_t t = 0; t < n; ++t) {
        const int32_t* w = &steps[t].kind;
        std::copy(w, w + mnk::FACTOR_STEP_INTS, out + mnk::FACTOR_STEP_INTS * t);
    }
    return (int)steps.size();
}

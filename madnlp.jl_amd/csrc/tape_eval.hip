// Model-agnostic device evaluation of NLP callbacks: expression tapes interpreted per pattern (the general
// form of opf_eval.hip, the way ExaModels compiles the models of the reference's GPU benchmarks).  A model is a list of patterns,
// each one scalar expression applied to R rows of index and parameter data; `madnlp_jl_amd.tape_model` compiles every pattern to
// three straight-line tapes (value | first derivatives | second derivatives of the local pairs j >= l) and is the host mirror of
// this file: the same instructions in the same order, so everything built from + - * / and negation is bit-identical
// (no FMA contraction), and so are abs / sign / step / min / max, which are comparisons and a sign-bit mask on both sides;
// sin / cos / exp / log / pow / tan / atan / tanh come from another math library.
//
//   instruction   (op, dst, a, b), 4 x int32; operand = kind << 24 | index: 0 slot, 1 local variable, 2 parameter column,
//                 3 constant pool; unary operations read `a` only.  Opcodes 0 .. 9 and 16 .. 24 (10 .. 15 are unassigned).
//   two kernels   ONE body, instantiated twice: tape_kernel<false> knows opcodes 0 .. 9 and is, instruction for instruction,
//                 the kernel from before opcodes 16 .. 24 existed (the registers of pow / tan / atan / tanh would halve the
//                 occupancy of every model that never calls them, and any further branch lengthens the path of every
//                 interpreted instruction); tape_kernel<true> knows 16 .. 24 as well.  mnk_tape_finalize picks per callback
//                 launch (does any tape of it hold an opcode >= 16?); a launch stays one launch over all patterns.
//   outputs       tape output o of row r is stored at out[base + o * R + r]; Hessian outputs are multiplied by y[rows[r]]
//                 (constraint pattern) or obj_weight (objective pattern) on the way out
//   kernel        one thread per pattern row, one launch per callback through a block -> (tape, first row) table; the instruction
//                 stream is block-uniform (scalar loads, scalar branches); a lane's slots, local variables and parameters live in
//                 LDS, one column per lane (lds[column * TAPE_BS + lane]: consecutive lanes, consecutive words -- conflict-free),
//                 never in a runtime-indexed private array
//   cons, grad    the tapes write per-term buffers; one ordered segmented sum per callback adds the terms of a destination in
//                 term order (the host mirror's np.add.at order) and writes 0 where there is none.  No atomics.
//
// Algorithmic bytes per callback (k local variables, q parameters, R rows per pattern): (12 k + 8 q) R read for the gathers,
// 8 R per output written (+ 4 R rows and 8 R multipliers for hess_coord), cons / grad 20 bytes per term more for the sum.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>

#include "common.h"

using namespace mnk;

namespace {

constexpr int TAPE_SLOT_MAX = 32;   // LDS: (32 + 8 + 8) columns x 128 lanes x 8 bytes = 48 KiB per workgroup at the very most
constexpr int TAPE_K_MAX = 8;
constexpr int TAPE_Q_MAX = 8;
constexpr int TAPE_BS = 128;
constexpr int TAPE_NOPS = 10;       // 0 .. 9: add sub mul div neg sin cos exp log sqrt
enum { OP_POW = 16, OP_TAN, OP_ATAN, OP_TANH, OP_ABS, OP_SIGN, OP_STEP, OP_MIN, OP_MAX, OP_END };
constexpr int64_t TAPE_COUNT_MAX = (1LL << 31) - 2 * TAPE_BS;

enum { G_OBJ = 0, G_GRAD, G_CONS, G_JAC, G_HESS, G_COUNT };

struct TapeDesc {      // one tape of one pattern as the kernel sees it
    int R, k, q, nslot, ninstr, nout, wmode, pad;   // wmode 0: plain store, 1: times y[rows[r]], 2: times obj_weight
    int64_t vi_off, par_off, rows_off, code_off, const_off, outs_off, out_base;
};

struct HostTape {
    int nslot = 0;
    bool extended = false;          // has an instruction with an opcode >= 16
    std::vector<int32_t> code;      // 4 per instruction; operands already LDS columns (>= 0) or ~constant index (< 0)
    std::vector<int32_t> outs;
    std::vector<double> consts;
    std::vector<int32_t> out_j, out_l;
};

struct HostPattern {
    int kind = 0, k = 0, q = 0;
    int64_t R = 0;
    std::vector<int32_t> vi, rows;  // vi column-major: [j * R + r]
    std::vector<double> par;        // column-major: [c * R + r]
    HostTape t[3];
};

// `o` is wave-uniform: a scalar branch between an LDS read and a scalar load.  (The empty asm keeps the two arms apart: the
// compiler otherwise sinks the two loads into one load through a selected POINTER, which is a flat load.)
__device__ __forceinline__ double tape_fetch(const double* col, const double* __restrict__ consts, int o) {
    if (o >= 0) {
        double v = col[o * TAPE_BS];
        asm volatile("" : "+v"(v));
        return v;
    }
    return consts[~o];
}

// EXT: the instantiation that knows opcodes 16 .. 24.  The selection operations are comparisons, not fmin / fmax /
// copysign: min = (b < a) ? b : a, max = (b > a) ? b : a, step = (a >= 0), sign = (a > 0) - (a < 0), abs clears the sign bit.
template <bool EXT>
__global__ __launch_bounds__(TAPE_BS) void tape_kernel(const TapeDesc* __restrict__ descs, const int2* __restrict__ blocks,
                                                        const int32_t* __restrict__ vi, const double* __restrict__ par,
                                                        const int32_t* __restrict__ rows, const int4* __restrict__ code,
                                                        const double* __restrict__ consts, const int32_t* __restrict__ outs,
                                                        const double* __restrict__ x, const double* __restrict__ y, double w,
                                                        double* __restrict__ out) {
    extern __shared__ double tape_lds[];
    const int2 blk = blocks[blockIdx.x];
    const TapeDesc d = descs[__builtin_amdgcn_readfirstlane(blk.x)];
    const int r = __builtin_amdgcn_readfirstlane(blk.y) + (int)threadIdx.x;
    if (r >= d.R) return;                       // (no barrier below: a lane only ever touches its own column)
    double* col = tape_lds + threadIdx.x;
    for (int j = 0; j < d.k; ++j) col[(d.nslot + j) * TAPE_BS] = x[vi[d.vi_off + (int64_t)j * d.R + r]];
    for (int c = 0; c < d.q; ++c) col[(d.nslot + d.k + c) * TAPE_BS] = par[d.par_off + (int64_t)c * d.R + r];
    const int4* __restrict__ pc = code + d.code_off;
    const double* __restrict__ cp = consts + d.const_off;
    for (int i = 0; i < d.ninstr; ++i) {
        const int4 ins = pc[i];
        const int op = __builtin_amdgcn_readfirstlane(ins.x), dst = __builtin_amdgcn_readfirstlane(ins.y);
        const double a = tape_fetch(col, cp, __builtin_amdgcn_readfirstlane(ins.z));
        double v;
        if (op < 4) {
            const double b = tape_fetch(col, cp, __builtin_amdgcn_readfirstlane(ins.w));
            v = op == 0 ? a + b : op == 1 ? a - b : op == 2 ? a * b : a / b;
        } else if (EXT && op >= OP_POW) {
            const double b = tape_fetch(col, cp, __builtin_amdgcn_readfirstlane(ins.w));      // (the unary ones carry `a` twice)
            switch (op) {
                case OP_POW: v = pow(a, b); break;
                case OP_TAN: v = tan(a); break;
                case OP_ATAN: v = atan(a); break;
                case OP_TANH: v = tanh(a); break;
                case OP_ABS: v = __longlong_as_double(__double_as_longlong(a) & 0x7FFFFFFFFFFFFFFFLL); break;
                case OP_SIGN: v = a > 0.0 ? 1.0 : a < 0.0 ? -1.0 : 0.0; break;
                case OP_STEP: v = a >= 0.0 ? 1.0 : 0.0; break;
                case OP_MIN: v = b < a ? b : a; break;
                default: v = b > a ? b : a; break;
            }
        } else {
            switch (op) {
                case 4: v = -a; break;
                case 5: v = sin(a); break;
                case 6: v = cos(a); break;
                case 7: v = exp(a); break;
                case 8: v = log(a); break;
                default: v = sqrt(a); break;
            }
        }
        col[dst * TAPE_BS] = v;
    }
    const int32_t* __restrict__ op_out = outs + d.outs_off;
    double* __restrict__ o_ptr = out + d.out_base + r;
    if (d.wmode == 0) {
        for (int o = 0; o < d.nout; ++o)
            o_ptr[(int64_t)o * d.R] = tape_fetch(col, cp, __builtin_amdgcn_readfirstlane(op_out[o]));
    } else {
        const double wt = d.wmode == 1 ? y[rows[d.rows_off + r]] : w;
        for (int o = 0; o < d.nout; ++o)
            o_ptr[(int64_t)o * d.R] = wt * tape_fetch(col, cp, __builtin_amdgcn_readfirstlane(op_out[o]));
    }
}

// dst[s] = sum of src[idx[k]] over the segment of s, in the order of the list (sparse_kkt.hip: segsum_kernel); an empty segment gives 0
__global__ void tape_segsum_kernel(double* __restrict__ dst, const double* __restrict__ src, const int32_t* __restrict__ ptr,
                                   const int32_t* __restrict__ idx, int64_t nseg) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    double acc = 0.0;
    for (int32_t k = ptr[s]; k < ptr[s + 1]; ++k) acc += src[idx[k]];
    dst[s] = acc;
}

// Everything the kernel will index with is checked here; operands are rewritten to LDS columns / constant indices.
int check_tape(const char* what, int k, int q, int64_t ninstr, const int32_t* code, int64_t nconst, const double* consts, int64_t nout,
               const int32_t* out_operand, const int32_t* out_j, const int32_t* out_l, int nslot, int which, HostTape& T) {
#define TAPE_FAIL(...)                  \
    do {                                \
        set_error(__VA_ARGS__);         \
        return -1;                      \
    } while (0)
    if (nslot < 0 || nslot > TAPE_SLOT_MAX) TAPE_FAIL("mnk_tape_add_pattern: %s tape: nslot = %d is outside [0, SLOT_MAX = %d]", what, nslot, TAPE_SLOT_MAX);
    if (ninstr < 0 || ninstr > (1 << 16) || nconst < 0 || nconst > (1 << 16))
        TAPE_FAIL("mnk_tape_add_pattern: %s tape: %lld instructions / %lld constants (at most 65536 each)", what, (long long)ninstr, (long long)nconst);
    const int64_t nout_max = which == 0 ? 1 : which == 1 ? k : k * (k + 1) / 2;
    if (nout < (which == 0 ? 1 : 0) || nout > nout_max)
        TAPE_FAIL("mnk_tape_add_pattern: %s tape: %lld outputs (k = %d allows at most %lld)", what, (long long)nout, k, (long long)nout_max);
    if ((ninstr > 0 && !code) || (nconst > 0 && !consts) || (nout > 0 && !out_operand) || (which >= 1 && nout > 0 && !out_j) ||
        (which == 2 && nout > 0 && !out_l))
        TAPE_FAIL("mnk_tape_add_pattern: %s tape: NULL array", what);
    bool written[TAPE_SLOT_MAX] = {};
    auto column = [&](int32_t o, int64_t at, const char* role, int32_t* col) -> int {
        const int kind = (int)((uint32_t)o >> 24), idx = (int)(o & 0xFFFFFF);
        if (o < 0 || kind > 3) TAPE_FAIL("mnk_tape_add_pattern: %s tape, %s %lld: operand kind %d is not one of 0 .. 3", what, role, (long long)at, o < 0 ? -1 : kind);
        if (kind == 0) {
            if (idx >= nslot) TAPE_FAIL("mnk_tape_add_pattern: %s tape, %s %lld: slot %d is out of range (nslot = %d)", what, role, (long long)at, idx, nslot);
            if (!written[idx]) TAPE_FAIL("mnk_tape_add_pattern: %s tape, %s %lld: slot %d is read before it is written", what, role, (long long)at, idx);
            *col = idx;
        } else if (kind == 1) {
            if (idx >= k) TAPE_FAIL("mnk_tape_add_pattern: %s tape, %s %lld: local variable %d is out of range (k = %d)", what, role, (long long)at, idx, k);
            *col = nslot + idx;
        } else if (kind == 2) {
            if (idx >= q) TAPE_FAIL("mnk_tape_add_pattern: %s tape, %s %lld: parameter column %d is out of range (q = %d)", what, role, (long long)at, idx, q);
            *col = nslot + k + idx;
        } else {
            if (idx >= nconst) TAPE_FAIL("mnk_tape_add_pattern: %s tape, %s %lld: constant %d is out of range (nconst = %lld)", what, role, (long long)at, idx, (long long)nconst);
            *col = ~idx;
        }
        return 0;
    };
    T.nslot = nslot;
    T.extended = false;
    T.code.resize(4 * ninstr);
    for (int64_t i = 0; i < ninstr; ++i) {
        const int32_t op = code[4 * i], dst = code[4 * i + 1];
        if (op < 0 || (op >= TAPE_NOPS && op < OP_POW) || op >= OP_END)
            TAPE_FAIL("mnk_tape_add_pattern: %s tape, instruction %lld: bad opcode %d (0 .. %d, %d .. %d)", what, (long long)i, op, TAPE_NOPS - 1, (int)OP_POW, OP_END - 1);
        if (dst < 0 || dst >= nslot) TAPE_FAIL("mnk_tape_add_pattern: %s tape, instruction %lld: destination slot %d is out of range (nslot = %d)", what, (long long)i, dst, nslot);
        int32_t ca = 0, cb = 0;
        if (column(code[4 * i + 2], i, "instruction", &ca)) return -1;
        if (op < 4 || op == OP_POW || op == OP_MIN || op == OP_MAX) {
            if (column(code[4 * i + 3], i, "instruction", &cb)) return -1;
        } else {
            cb = ca;
        }
        T.extended |= op >= OP_POW;
        written[dst] = true;
        T.code[4 * i] = op; T.code[4 * i + 1] = dst; T.code[4 * i + 2] = ca; T.code[4 * i + 3] = cb;
    }
    T.outs.resize(nout);
    T.out_j.assign(nout, 0);
    T.out_l.assign(nout, 0);
    for (int64_t o = 0; o < nout; ++o) {
        if (column(out_operand[o], o, "output", &T.outs[o])) return -1;
        if (which >= 1) {
            T.out_j[o] = out_j[o];
            T.out_l[o] = which == 2 ? out_l[o] : 0;
            if (T.out_j[o] < 0 || T.out_j[o] >= k || T.out_l[o] < 0 || T.out_l[o] > T.out_j[o])
                TAPE_FAIL("mnk_tape_add_pattern: %s tape, output %lld: local variable (pair) (%d, %d) is not 0 <= l <= j < k = %d", what, (long long)o, T.out_j[o], T.out_l[o], k);
        }
    }
    T.consts.assign(consts, consts + nconst);
    return 0;
}

// CSR of contributions by destination, each segment in term order
void contributions_csr(int64_t nseg, const std::vector<int32_t>& dest, std::vector<int32_t>& ptr, std::vector<int32_t>& idx) {
    ptr.assign(nseg + 1, 0);
    for (int32_t d : dest) ptr[d + 1]++;
    for (int64_t i = 0; i < nseg; ++i) ptr[i + 1] += ptr[i];
    idx.resize(dest.size());
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (size_t t = 0; t < dest.size(); ++t) idx[fill[dest[t]]++] = (int32_t)t;
}

}  // namespace

struct mnk_tape {
    mnk_ctx* ctx = nullptr;
    int64_t n = 0, m = 0, nterms = 0, ngterm = 0, ncterm = 0, nnzj = 0, nnzh = 0;
    bool finalized = false;
    std::vector<HostPattern> pats;
    std::vector<int32_t> jac_I, jac_J, hess_I, hess_J;
    DevBuf<TapeDesc> descs;
    DevBuf<int2> blocks[G_COUNT];
    int64_t nblocks[G_COUNT] = {};
    size_t lds_bytes[G_COUNT] = {};
    bool extended[G_COUNT] = {};    // the launch has a tape with an opcode >= 16: tape_kernel<true>
    DevBuf<int32_t> vi, rows, code, outs, g_ptr, g_idx, c_ptr, c_idx;
    DevBuf<double> par, consts, gterm, cterm;
};

extern "C" {

#define TAPE_ENTER(h, cond, who)                                                        \
    MNK_REQUIRE((h) != nullptr && (cond), who ": NULL argument");                        \
    MNK_REQUIRE((h)->finalized, who ": mnk_tape_finalize has not been called");          \
    MNK_HIP(hipSetDevice((h)->ctx->device))

int mnk_tape_create(mnk_ctx* ctx, int64_t n, int64_t m, void* out_) {
    mnk_tape** out = static_cast<mnk_tape**>(out_);
    MNK_REQUIRE(ctx && out, "mnk_tape_create: NULL argument");
    MNK_REQUIRE(n > 0 && m >= 0 && n < TAPE_COUNT_MAX && m < TAPE_COUNT_MAX, "mnk_tape_create: bad sizes");
    auto* h = new mnk_tape();
    h->ctx = ctx;
    h->n = n;
    h->m = m;
    mnk_ctx_child_added(ctx);
    *out = h;
    return 0;
}

int mnk_tape_destroy(void* tape) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    if (!h) return 0;
    mnk_ctx* ctx = h->ctx;
    (void)hipSetDevice(ctx->device);
    (void)mnk::stream_wait(ctx->stream);
    delete h;
    mnk_ctx_child_gone(ctx);
    return 0;
}

int mnk_tape_add_pattern(void* tape, int kind, int64_t R, int k, int q, const int32_t* var_index, const double* params,
                         const int32_t* rows,
                         int64_t ninstr0, const int32_t* code0, int64_t nconst0, const double* consts0, int64_t nout0,
                         const int32_t* out_operand0, const int32_t* out_j0, const int32_t* out_l0, int nslot0,
                         int64_t ninstr1, const int32_t* code1, int64_t nconst1, const double* consts1, int64_t nout1,
                         const int32_t* out_operand1, const int32_t* out_j1, const int32_t* out_l1, int nslot1,
                         int64_t ninstr2, const int32_t* code2, int64_t nconst2, const double* consts2, int64_t nout2,
                         const int32_t* out_operand2, const int32_t* out_j2, const int32_t* out_l2, int nslot2) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    MNK_REQUIRE(h != nullptr && var_index != nullptr, "mnk_tape_add_pattern: NULL argument");
    MNK_REQUIRE(!h->finalized, "mnk_tape_add_pattern: the handle is finalized");
    MNK_REQUIRE(kind == 0 || kind == 1, "mnk_tape_add_pattern: kind must be 0 (objective) or 1 (constraint)");
    MNK_REQUIRE(R >= 1 && R < TAPE_COUNT_MAX / (TAPE_K_MAX * (TAPE_K_MAX + 1) / 2), "mnk_tape_add_pattern: bad row count R");
    MNK_REQUIRE(k >= 1 && k <= TAPE_K_MAX, "mnk_tape_add_pattern: k must be 1 .. 8 local variables");
    MNK_REQUIRE(q >= 0 && q <= TAPE_Q_MAX && (q == 0 || params != nullptr), "mnk_tape_add_pattern: q must be 0 .. 8 parameter columns (and params non-NULL)");
    MNK_REQUIRE(kind == 0 || rows != nullptr, "mnk_tape_add_pattern: a constraint pattern needs rows");
    HostPattern P;
    P.kind = kind; P.R = R; P.k = k; P.q = q;
    for (int64_t r = 0; r < R; ++r) {
        for (int j = 0; j < k; ++j) {
            const int32_t v = var_index[r * k + j];
            if (v < 0 || v >= h->n) {
                set_error("mnk_tape_add_pattern: var_index[%lld, %d] = %d is out of range (n = %lld)", (long long)r, j, v, (long long)h->n);
                return -1;
            }
            for (int l = 0; l < j; ++l)
                if (var_index[r * k + l] == v) {
                    set_error("mnk_tape_add_pattern: row %lld of var_index names variable %d twice", (long long)r, v);
                    return -1;
                }
        }
        if (kind == 1 && (rows[r] < 0 || rows[r] >= h->m)) {
            set_error("mnk_tape_add_pattern: rows[%lld] = %d is out of range (m = %lld)", (long long)r, rows[r], (long long)h->m);
            return -1;
        }
    }
    if (check_tape("value", k, q, ninstr0, code0, nconst0, consts0, nout0, out_operand0, out_j0, out_l0, nslot0, 0, P.t[0])) return -1;
    if (check_tape("first-derivative", k, q, ninstr1, code1, nconst1, consts1, nout1, out_operand1, out_j1, out_l1, nslot1, 1, P.t[1])) return -1;
    if (check_tape("second-derivative", k, q, ninstr2, code2, nconst2, consts2, nout2, out_operand2, out_j2, out_l2, nslot2, 2, P.t[2])) return -1;
    // totals stay below 2^31 (int32 term indices in the segmented sums, int32 COO structure)
    int64_t nt = 0, ng = 0, nc = 0, nj = 0, nh = 0;
    for (const HostPattern& p : h->pats) {
        (p.kind == 0 ? nt : nc) += p.R;
        (p.kind == 0 ? ng : nj) += p.R * (int64_t)p.t[1].outs.size();
        nh += p.R * (int64_t)p.t[2].outs.size();
    }
    (kind == 0 ? nt : nc) += R;
    (kind == 0 ? ng : nj) += R * nout1;
    nh += R * nout2;
    MNK_REQUIRE(std::max({nt, ng, nc, nj, nh}) < TAPE_COUNT_MAX && (int64_t)h->pats.size() < (1 << 20), "mnk_tape_add_pattern: the model is too large (2^31 entries)");
    P.vi.resize(R * k);
    for (int64_t r = 0; r < R; ++r)
        for (int j = 0; j < k; ++j) P.vi[j * R + r] = var_index[r * k + j];
    P.par.resize(R * q);
    for (int64_t r = 0; r < R; ++r)
        for (int c = 0; c < q; ++c) P.par[c * R + r] = params[r * q + c];
    if (kind == 1) P.rows.assign(rows, rows + R);
    h->pats.push_back(std::move(P));
    return 0;
}

int mnk_tape_finalize(void* tape) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    MNK_REQUIRE(h != nullptr, "mnk_tape_finalize: NULL handle");
    MNK_REQUIRE(!h->finalized, "mnk_tape_finalize: called twice");
    MNK_HIP(hipSetDevice(h->ctx->device));
    std::vector<TapeDesc> descs;
    std::vector<int2> blocks[G_COUNT];
    std::vector<int32_t> vi, rows, code, outs, gdest, cdest;
    std::vector<double> par, consts;
    int maxcol[G_COUNT] = {};
    for (const HostPattern& p : h->pats) {
        const int64_t vi_off = (int64_t)vi.size(), par_off = (int64_t)par.size(), rows_off = (int64_t)rows.size();
        vi.insert(vi.end(), p.vi.begin(), p.vi.end());
        par.insert(par.end(), p.par.begin(), p.par.end());
        rows.insert(rows.end(), p.rows.begin(), p.rows.end());
        for (int w = 0; w < 3; ++w) {
            const HostTape& t = p.t[w];
            const int group = w == 2 ? G_HESS : p.kind == 0 ? (w == 0 ? G_OBJ : G_GRAD) : (w == 0 ? G_CONS : G_JAC);
            int64_t* total = group == G_OBJ ? &h->nterms : group == G_GRAD ? &h->ngterm : group == G_CONS ? &h->ncterm : group == G_JAC ? &h->nnzj : &h->nnzh;
            TapeDesc d{};
            d.R = (int)p.R; d.k = p.k; d.q = p.q; d.nslot = t.nslot; d.ninstr = (int)(t.code.size() / 4); d.nout = (int)t.outs.size();
            d.wmode = w == 2 ? (p.kind == 1 ? 1 : 2) : 0;
            d.vi_off = vi_off; d.par_off = par_off; d.rows_off = rows_off;
            d.code_off = (int64_t)code.size() / 4; d.const_off = (int64_t)consts.size(); d.outs_off = (int64_t)outs.size();
            d.out_base = *total;
            code.insert(code.end(), t.code.begin(), t.code.end());
            consts.insert(consts.end(), t.consts.begin(), t.consts.end());
            outs.insert(outs.end(), t.outs.begin(), t.outs.end());
            for (int o = 0; o < d.nout; ++o)
                for (int64_t r = 0; r < p.R; ++r) {
                    const int32_t gj = p.vi[t.out_j[o] * p.R + r], gl = p.vi[t.out_l[o] * p.R + r];
                    if (group == G_GRAD) gdest.push_back(gj);
                    if (group == G_CONS) cdest.push_back(p.rows[r]);
                    if (group == G_JAC) { h->jac_I.push_back(p.rows[r]); h->jac_J.push_back(gj); }
                    if (group == G_HESS) { h->hess_I.push_back(std::max(gj, gl)); h->hess_J.push_back(std::min(gj, gl)); }
                }
            *total += p.R * d.nout;
            if (d.nout > 0) {
                for (int64_t r0 = 0; r0 < p.R; r0 += TAPE_BS) blocks[group].push_back(int2{(int)descs.size(), (int)r0});
                maxcol[group] = std::max(maxcol[group], t.nslot + p.k + p.q);
                h->extended[group] |= t.extended;
            }
            descs.push_back(d);
        }
    }
    std::vector<int32_t> gp, gi, cp, ci;
    contributions_csr(h->n, gdest, gp, gi);
    contributions_csr(h->m, cdest, cp, ci);
    hipStream_t s = h->ctx->stream;
    int rc = h->descs.upload(descs, s) | h->vi.upload(vi, s) | h->rows.upload(rows, s) | h->code.upload(code, s) | h->outs.upload(outs, s) |
             h->par.upload(par, s) | h->consts.upload(consts, s) | h->g_ptr.upload(gp, s) | h->g_idx.upload(gi, s) |
             h->c_ptr.upload(cp, s) | h->c_idx.upload(ci, s) | h->gterm.alloc(h->ngterm) | h->cterm.alloc(h->ncterm);
    for (int g = 0; g < G_COUNT; ++g) {
        rc |= h->blocks[g].upload(blocks[g], s);
        h->nblocks[g] = (int64_t)blocks[g].size();
        h->lds_bytes[g] = (size_t)maxcol[g] * TAPE_BS * sizeof(double);
    }
    if (rc) return -2;
    h->pats.clear();
    h->pats.shrink_to_fit();
    h->finalized = true;
    return 0;
}

int mnk_tape_sizes(void* tape, int64_t* n, int64_t* m, int64_t* nterms, int64_t* nnzj, int64_t* nnzh) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    MNK_REQUIRE(h != nullptr && h->finalized, "mnk_tape_sizes: NULL or unfinalized handle");
    if (n) *n = h->n;
    if (m) *m = h->m;
    if (nterms) *nterms = h->nterms;
    if (nnzj) *nnzj = h->nnzj;
    if (nnzh) *nnzh = h->nnzh;
    return 0;
}

// which callback launches run the extended kernel: obj = 1, grad = 2, cons = 4, jac = 8, hess = 16
int mnk_tape_extended(void* tape, int* mask) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    MNK_REQUIRE(h != nullptr && mask != nullptr && h->finalized, "mnk_tape_extended: NULL argument or unfinalized handle");
    *mask = 0;
    for (int g = 0; g < G_COUNT; ++g) *mask |= (int)h->extended[g] << g;
    return 0;
}

int mnk_tape_get_structure(void* tape, int32_t* jac_I, int32_t* jac_J, int32_t* hess_I, int32_t* hess_J) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    MNK_REQUIRE(h != nullptr && h->finalized, "mnk_tape_get_structure: NULL or unfinalized handle");
    if (jac_I) std::copy(h->jac_I.begin(), h->jac_I.end(), jac_I);
    if (jac_J) std::copy(h->jac_J.begin(), h->jac_J.end(), jac_J);
    if (hess_I) std::copy(h->hess_I.begin(), h->hess_I.end(), hess_I);
    if (hess_J) std::copy(h->hess_J.begin(), h->hess_J.end(), hess_J);
    return 0;
}

static int tape_launch(mnk_tape* h, int g, const double* x, const double* y, double w, double* out) {
    if (h->nblocks[g] == 0) return 0;
    hipLaunchKernelGGL(h->extended[g] ? tape_kernel<true> : tape_kernel<false>, dim3((unsigned)h->nblocks[g]), dim3(TAPE_BS), h->lds_bytes[g], h->ctx->stream, h->descs.p,
                       h->blocks[g].p, h->vi.p, h->par.p, h->rows.p, (const int4*)h->code.p, h->consts.p, h->outs.p, x, y, w, out);
    MNK_HIP(hipGetLastError());
    return 0;
}

static int tape_segsum(mnk_tape* h, double* dst, const double* src, const int32_t* ptr, const int32_t* idx, int64_t nseg) {
    if (nseg == 0) return 0;
    hipLaunchKernelGGL(tape_segsum_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, h->ctx->stream, dst, src, ptr, idx, nseg);
    MNK_HIP(hipGetLastError());
    return 0;
}

// per-row terms of the objective patterns; the caller sums them (mnk_ipm_get_sum) -- NLPModels.obj
int mnk_tape_obj_terms(void* tape, const double* x, double* terms) {
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    TAPE_ENTER(h, x && (terms || h->nterms == 0), "mnk_tape_obj_terms");
    return tape_launch(h, G_OBJ, x, nullptr, 0.0, terms);
}

int mnk_tape_grad(void* tape, const double* x, double* g) {   // NLPModels.grad!
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    TAPE_ENTER(h, x && g, "mnk_tape_grad");
    int rc = tape_launch(h, G_GRAD, x, nullptr, 0.0, h->gterm.p);
    return rc ? rc : tape_segsum(h, g, h->gterm.p, h->g_ptr.p, h->g_idx.p, h->n);
}

int mnk_tape_cons(void* tape, const double* x, double* c) {   // NLPModels.cons!
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    TAPE_ENTER(h, x && (c || h->m == 0), "mnk_tape_cons");
    int rc = tape_launch(h, G_CONS, x, nullptr, 0.0, h->cterm.p);
    return rc ? rc : tape_segsum(h, c, h->cterm.p, h->c_ptr.p, h->c_idx.p, h->m);
}

int mnk_tape_jac_coord(void* tape, const double* x, double* jac) {   // NLPModels.jac_coord!
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    TAPE_ENTER(h, x && (jac || h->nnzj == 0), "mnk_tape_jac_coord");
    return tape_launch(h, G_JAC, x, nullptr, 0.0, jac);
}

int mnk_tape_hess_coord(void* tape, const double* x, const double* y, double obj_weight, double* hess) {   // NLPModels.hess_coord!
    mnk_tape* h = static_cast<mnk_tape*>(tape);
    TAPE_ENTER(h, x && (y || h->m == 0) && (hess || h->nnzh == 0), "mnk_tape_hess_coord");
    return tape_launch(h, G_HESS, x, y, obj_weight, hess);
}

}  // extern "C"

// The `mnk_ipm` handle (include/madnlp_hip.h): what the `mnk_ipm_*` entry points of ipm_vec.hip, nlp_scale.hip and krylov.hip
// share -- the context whose stream every launch goes to, the bound index sets, the reduction scratch of the get_* calls and
// the batch protocol they follow.
#pragma once
#include <functional>
#include <utility>
#include <vector>

#include "common.h"

namespace mnk {
constexpr int IPM_BLOCKS = 256;
constexpr int IPM_SLOTS = 32;  // reductions in flight: up to four per call (sixteen for the quality function), several calls per batch
constexpr int IPM_THREADS = 256;
}  // namespace mnk

struct mnk_ipm {
    mnk_ctx* ctx = nullptr;
    int64_t ntot = 0, nlb = 0, nub = 0;
    int64_t nllb = 0, nuub = 0;
    mnk::DevBuf<int64_t> ind_lb, ind_ub, ind_llb, ind_uub;
    mnk::DevBuf<double> gemv_part;   // column-slab partial sums of mnk_ipm_gemv (grown on demand)
    mnk::DevBuf<double> part;   // IPM_SLOTS x IPM_BLOCKS partials
    mnk::DevBuf<double> qf_alpha;   // IPM_SLOTS step lengths of mnk_ipm_quality_function, read by its second pass on the device
    mnk::DevBuf<double> kry_res;    // IPM_SLOTS results of mnk_ipm_krylov_dots / _normalize, slot by slot: the device-side copy
    mnk::DevBuf<double> kry_part;   // IPM_BLOCKS partial sums of u . u that mnk_ipm_krylov_project leaves for _normalize
    const double* kry_last = nullptr;   // where the most recent mnk_ipm_krylov_dots left its results (inside kry_res)
    double* pin = nullptr;     // IPM_SLOTS pinned, device-mapped host words: the final reduction stores its result here
    double* pin_dev = nullptr;
    // batch mode (mnk_ipm_batch_begin / _end): the get_* calls only enqueue their reductions into successive slots and
    // leave a finalizer behind; ONE synchronization at batch_end, then every deferred `out` receives its value
    bool batching = false;
    int next_slot = 0;
    std::vector<std::pair<int, std::function<void(const double*)>>> pending;  // (first slot, finalizer)
};

namespace mnk {

// first slot of a call that needs `count` reductions (-1: the batch is full)
inline int ipm_slot_base(mnk_ipm* h, int count) {
    if (!h->batching) return 0;
    if (h->next_slot + count > IPM_SLOTS) {
        set_error("mnk_ipm: more than %d reductions in one batch", IPM_SLOTS);
        return -1;
    }
    const int b = h->next_slot;
    h->next_slot += count;
    return b;
}

// Outside a batch: wait for the stream, read the `count` results that start at slot `base` and run the finalizer (which
// writes the caller's `out`).  Inside a batch: keep the finalizer for mnk_ipm_batch_end.
template <class Fin>
int ipm_finish(mnk_ipm* h, int base, int count, Fin fin) {
    if (h->batching) {
        h->pending.emplace_back(base, std::function<void(const double*)>(fin));
        return 0;
    }
    // the final reductions stored their results straight into pinned, device-mapped host memory
    MNK_HIP(mnk::stream_wait(h->ctx->stream));
    volatile double* pw = h->pin + base;
    double r[IPM_SLOTS];
    for (int i = 0; i < count; ++i) r[i] = pw[i];
    fin(r);
    return 0;
}

}  // namespace mnk

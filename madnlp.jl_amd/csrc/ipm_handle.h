// The `mnk_ipm` handle (include/madnlp_hip.h): what the `mnk_ipm_*` entry points of ipm_vec.hip and nlp_scale.hip share -- the
// context whose stream every launch goes to, the bound index sets and the reduction scratch of the get_* calls.
#pragma once
#include <functional>
#include <utility>
#include <vector>

#include "common.h"

struct mnk_ipm {
    mnk_ctx* ctx = nullptr;
    int64_t ntot = 0, nlb = 0, nub = 0;
    int64_t nllb = 0, nuub = 0;
    mnk::DevBuf<int64_t> ind_lb, ind_ub, ind_llb, ind_uub;
    mnk::DevBuf<double> gemv_part;   // column-slab partial sums of mnk_ipm_gemv (grown on demand)
    mnk::DevBuf<double> part;   // IPM_SLOTS x IPM_BLOCKS partials
    mnk::DevBuf<double> qf_alpha;   // IPM_SLOTS step lengths of mnk_ipm_quality_function, read by its second pass on the device
    double* pin = nullptr;     // IPM_SLOTS pinned, device-mapped host words: the final reduction stores its result here
    double* pin_dev = nullptr;
    // batch mode (mnk_ipm_batch_begin / _end): the get_* calls only enqueue their reductions into successive slots and
    // leave a finalizer behind; ONE synchronization at batch_end, then every deferred `out` receives its value
    bool batching = false;
    int next_slot = 0;
    std::vector<std::pair<int, std::function<void(const double*)>>> pending;  // (first slot, finalizer)
};

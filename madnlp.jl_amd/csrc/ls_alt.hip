// The linear solver's algorithms beside the tiled Cholesky / LDL^T (mnk_ls_alt, ls.h): which unit serves which algorithm, and
// what QR, LU and EVD share -- the bookkeeping around a factorization and the loop over the right-hand sides of a solve.
// mnk_ls_create, mnk_ls_run_factorization, mnk_ls_fetch_info and mnk_ls_solve hand over to this unit when ls->alt is set.
#include "ls.h"

using namespace mnk;

std::unique_ptr<mnk_ls_alt> mnk_ls_alt_new(int algo) {
    if (algo == MNK_QR) return mnk_qr_new();
    if (algo == MNK_LU) return mnk_lu_new();
    if (algo == MNK_EVD) return mnk_evd_new();
    return nullptr;
}

// factorize! (not merged into a factorization batch: runs when called; EVD also runs to its end before it returns)
int mnk_ls_alt_factorize(mnk_ls* ls) {
    ++ls->pp.count;
    ls->t_fact_launch_ms = mnk_host_ms();
    int rc = ls->alt->factor(ls);
    if (rc) return rc;
    ls->verdict.queued();
    return 0;
}

// solve_linear_system! (never queued in a solve batch: runs at once): nrhs columns of x (leading dimension ldx, host or
// device), in place.  A host column goes through the staging slot, the first Np entries of xwork.
int mnk_ls_alt_solve(mnk_ls* ls, double* x, int64_t nrhs, int64_t ldx, int loc) {
    hipStream_t s = ls->ctx->stream;
    const size_t bytes = (size_t)ls->N * sizeof(double);
    double* stage = ls->xwork.p;
    for (int64_t k = 0; k < nrhs; ++k) {
        double* xk = x + k * ldx;
        double* xd = loc == MNK_DEVICE ? xk : stage;
        if (xd != xk) MNK_HIP(h2d_copy(stage, xk, bytes, s));
        int rc = ls->alt->solve_vec(ls, xd, xd);
        if (rc) return rc;
        if (xd != xk) MNK_HIP(d2h_copy(xk, stage, bytes, s));
    }
    return 0;
}

// tu_policy_advance_large.hip -- the receding-horizon advance for clusters of 60 < n_x <= 240 (policy_advance_large.hpp) and its
// launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance_large.hpp"

namespace dpilqr {

// The families that can exceed 60 states with k <= 20: (4, 2), (6, 3), (12, 4).  Every refusal is answered before any launch.
int32_t launch_policy_advance_large(const dpilqr_batch_desc& D, const double* X, const double* U, const double* K, int32_t h,
                                    const int32_t* scen, int32_t n_scen, int32_t L, int32_t n_d, const double* W, const double* u_lim,
                                    double* x_cur, int32_t* n_done, double* X_exec, double* U_exec, double* J_exec, double* min_sep,
                                    double* dist_left, double* U_next, double* X_next, hipStream_t st) {
    const int n = D.k * D.n_s;
    if (n <= 60)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_large: n_x=%d, clusters up to n_x = 60 are served by dpilqr_policy_advance", n);
    if (n > kPolicyLargeMaxNx || D.k > kPolicyLargeMaxK)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_large: n_x=%d, k=%d, served are 60 < n_x <= %d with k <= %d", n, D.k,
                    kPolicyLargeMaxNx, kPolicyLargeMaxK);
#define POLICY_ADVANCE_LARGE_CASE(NS_, NC_)                                                                                          \
    case NS_: {                                                                                                                      \
        if (D.n_c != NC_) break;                                                                                                     \
        if (D.B == 0) return DPILQR_OK;      /* an empty batch */                                                                    \
        const size_t lds = advance_large_lds_bytes(NS_, NC_, D.k);                                                                   \
        const int32_t rc = allow_lds(k_policy_advance_large<NS_, NC_>, lds);                                                         \
        if (rc) return rc;                                                                                                           \
        hipLaunchKernelGGL((k_policy_advance_large<NS_, NC_>), dim3((unsigned)D.B), dim3(kPolicyThreads), lds, st, D, X, U, K, (int)h, \
                           scen, (int)n_scen, (int)L, (int)n_d, W, u_lim, x_cur, n_done, X_exec, U_exec, J_exec, min_sep, dist_left,  \
                           U_next, X_next);                                                                                          \
        HIP_TRY(hipGetLastError());                                                                                                  \
        return DPILQR_OK;                                                                                                            \
    }
    switch (D.n_s) {
        POLICY_ADVANCE_LARGE_CASE(4, 2)
        POLICY_ADVANCE_LARGE_CASE(6, 3)
        POLICY_ADVANCE_LARGE_CASE(12, 4)
        default: break;
    }
#undef POLICY_ADVANCE_LARGE_CASE
    return fail(DPILQR_EUNSUPPORTED, "policy_advance_large: the (%d, %d) family cannot exceed 60 states at k <= %d", D.n_s, D.n_c,
                kPolicyLargeMaxK);
}

}  // namespace dpilqr

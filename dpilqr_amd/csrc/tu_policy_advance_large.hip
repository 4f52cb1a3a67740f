// tu_policy_advance_large.hip -- the receding-horizon advance for clusters of 60 < n_x <= 240 (policy_advance_large.hpp) and its
// launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance_large.hpp"

namespace dpilqr {

// The families that can exceed 60 states with k <= 20: (4, 2), (6, 3), (12, 4).  Every refusal is answered before any launch.
static_assert(kRouteLargeMaxNx == kPolicyLargeMaxNx && kRouteLargeMaxK == kPolicyLargeMaxK, "the kernel is built for the route's bounds");

int32_t launch_policy_advance_large(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, hipStream_t st) {
    const int n = D.k * D.n_s;
    if (n <= kRouteSmallMaxNx)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_large: n_x=%d, clusters up to n_x = 60 are served by dpilqr_policy_advance", n);
    if (n > kRouteLargeMaxNx || D.k > kRouteLargeMaxK)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_large: n_x=%d, k=%d, served are 60 < n_x <= %d with k <= %d", n, D.k,
                    kRouteLargeMaxNx, kRouteLargeMaxK);
#define POLICY_ADVANCE_LARGE_CASE(NS_, NC_)                                                                                          \
    case NS_: {                                                                                                                      \
        if (D.n_c != NC_) break;                                                                                                     \
        if (D.B == 0) return DPILQR_OK;      /* an empty batch */                                                                    \
        const size_t lds = advance_large_lds_bytes(NS_, NC_, D.k);                                                                   \
        const int32_t rc = allow_lds(k_policy_advance_large<NS_, NC_>, lds);                                                         \
        if (rc) return rc;                                                                                                           \
        hipLaunchKernelGGL((k_policy_advance_large<NS_, NC_>), dim3((unsigned)D.B), dim3(kPolicyThreads), lds, st, D, a.plan.X, a.plan.U, a.plan.K, \
                           (int)a.h, a.scen, (int)a.n_scen, (int)a.L, (int)a.n_d, a.W, a.u_lim, a.x_cur, a.n_done, a.X_exec, a.U_exec, \
                           a.J_exec, a.min_sep, a.dist_left, a.U_next, a.X_next);                                                    \
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
                kRouteLargeMaxK);
}

}  // namespace dpilqr

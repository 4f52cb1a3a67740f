// tu_policy_large.hip -- the closed-loop ensemble rollout for clusters of 60 < n_x <= 240 (policy_large.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_large.hpp"

namespace dpilqr {

// The families that can exceed 60 states with k <= 20: (4, 2), (6, 3), (12, 4).  Every refusal is answered before any launch.
static_assert(kRouteLargeMaxNx == kPolicyLargeMaxNx && kRouteLargeMaxK == kPolicyLargeMaxK, "the kernel is built for the route's bounds");

int32_t launch_policy_rollout_large(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st) {
    const int n = D.k * D.n_s;
    if (n <= kRouteSmallMaxNx)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_large: n_x=%d, clusters up to n_x = 60 are served by dpilqr_policy_rollout", n);
    if (n > kRouteLargeMaxNx || D.k > kRouteLargeMaxK)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_large: n_x=%d, k=%d, served are 60 < n_x <= %d with k <= %d", n, D.k,
                    kRouteLargeMaxNx, kRouteLargeMaxK);
    const int spw = kPolicyThreads / D.k;                      // samples of one item per workgroup
    const int64_t chunks = ((int64_t)a.n_samples + spw - 1) / spw;
    if (chunks * D.B > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_rollout_large: %lld workgroups", (long long)(chunks * D.B));
    const unsigned blocks = (unsigned)(chunks * D.B);
#define POLICY_LARGE_CASE(NS_, NC_)                                                                                                  \
    case NS_: {                                                                                                                      \
        if (D.n_c != NC_) break;                                                                                                     \
        if (blocks == 0) return DPILQR_OK;      /* an empty batch */                                                                 \
        const size_t lds = policy_large_lds_bytes(NS_, NC_, D.k);                                                                    \
        const int32_t rc = allow_lds(k_policy_rollout_large<NS_, NC_>, lds);                                                         \
        if (rc) return rc;                                                                                                           \
        hipLaunchKernelGGL((k_policy_rollout_large<NS_, NC_>), dim3(blocks), dim3(kPolicyThreads), lds, st, D, a.plan.X, a.plan.U, a.plan.K, \
                           (int)a.n_samples, (int)chunks, a.x0s, a.W, a.u_lim, a.Xs, a.Us, a.J, a.min_sep, a.goal_dist);             \
        HIP_TRY(hipGetLastError());                                                                                                  \
        return DPILQR_OK;                                                                                                            \
    }
    switch (D.n_s) {
        POLICY_LARGE_CASE(4, 2)
        POLICY_LARGE_CASE(6, 3)
        POLICY_LARGE_CASE(12, 4)
        default: break;
    }
#undef POLICY_LARGE_CASE
    return fail(DPILQR_EUNSUPPORTED, "policy_rollout_large: the (%d, %d) family cannot exceed 60 states at k <= %d", D.n_s, D.n_c,
                kRouteLargeMaxK);
}

}  // namespace dpilqr

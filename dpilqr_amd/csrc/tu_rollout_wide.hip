// tu_rollout_wide.hip -- the full-team rollout for up to 256 agents (rollout_wide.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "rollout_wide.hpp"

namespace dpilqr {

int32_t launch_rollout_wide(const dpilqr_batch_desc& D, const double* x0, const double* U, double* X, double* J, double* min_sep,
                            double* goal_dist, hipStream_t st) {
    if (D.k > kRolloutWideAgents)
        return fail(DPILQR_EUNSUPPORTED, "rollout_wide: k=%d agents, the full-team rollout serves up to %d", D.k, kRolloutWideAgents);
    if (D.B == 0) return DPILQR_OK;
    DISPATCH_FAMILY_ALL(D.n_s, {
        hipLaunchKernelGGL((k_rollout_wide<NS, NC>), dim3((unsigned)D.B), dim3(kRolloutWideThreads), 0, st, D, x0, U, X, J, min_sep, goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

// tu_policy_dec_team.hip -- the closed loop of a distributed solution for teams of up to 64 agents (policy_dec_team.hpp) and its
// launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_dec_team.hpp"

namespace dpilqr {

int32_t launch_policy_rollout_dec_team(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st) {
    if (D.k > kPolicyTeamAgents)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec_team: k=%d agents, a neighbourhood mask is one word of %d bits", D.k, kPolicyTeamAgents);
    if (const int32_t rc = check_kc_max("policy_rollout_dec_team", D, a.plan.kc_max)) return rc;
    const int spw = kPolicyTeamThreads / D.k;                  // samples of one item per workgroup
    const int64_t chunks = ((int64_t)a.n_samples + spw - 1) / spw;
    if (chunks * D.B > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec_team: %lld workgroups", (long long)(chunks * D.B));
    if (D.B == 0) return DPILQR_OK;
    DISPATCH_FAMILY_ALL(D.n_s, {
        hipLaunchKernelGGL((k_policy_rollout_dec_team<NS, NC, 1>), dim3((unsigned)(chunks * D.B)), dim3(kPolicyTeamThreads), 0, st, D, a.plan.X,
                           a.plan.U, a.plan.K, (int)a.plan.kc_max, reinterpret_cast<const unsigned long long*>(a.plan.nbr_bits),
                           1, (int)a.n_samples, (int)chunks, a.x0s, a.W, a.u_lim, a.Xs, a.Us, a.J, a.min_sep, a.goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

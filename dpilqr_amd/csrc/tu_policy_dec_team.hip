// tu_policy_dec_team.hip -- the closed loop of a distributed solution for teams of up to 64 agents (policy_dec_team.hpp) and its
// launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_dec_team.hpp"

namespace dpilqr {

int32_t launch_policy_rollout_dec_team(const dpilqr_batch_desc& D, const double* X, const double* U_ff, const double* Kc, int32_t kc_max,
                                       const uint64_t* nbr_bits, int32_t n_samples, const double* x0s, const double* W,
                                       const double* u_lim, double* Xs, double* Us, double* J, double* min_sep, double* goal_dist,
                                       hipStream_t st) {
    if (D.k > kPolicyTeamAgents)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec_team: k=%d agents, a neighbourhood mask is one word of %d bits", D.k, kPolicyTeamAgents);
    if (kc_max < 1 || kc_max > D.k)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec_team: kc_max=%d, a neighbourhood has 1 .. k = %d members", kc_max, D.k);
    const int spw = kPolicyTeamThreads / D.k;                  // samples of one item per workgroup
    const int64_t chunks = ((int64_t)n_samples + spw - 1) / spw;
    if (chunks * D.B > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec_team: %lld workgroups", (long long)(chunks * D.B));
    if (D.B == 0) return DPILQR_OK;
    DISPATCH_FAMILY_ALL(D.n_s, {
        hipLaunchKernelGGL((k_policy_rollout_dec_team<NS, NC>), dim3((unsigned)(chunks * D.B)), dim3(kPolicyTeamThreads), 0, st, D, X, U_ff,
                           Kc, (int)kc_max, reinterpret_cast<const unsigned long long*>(nbr_bits), (int)n_samples, (int)chunks, x0s, W,
                           u_lim, Xs, Us, J, min_sep, goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

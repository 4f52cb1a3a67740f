// tu_policy_advance_dec_team.hip -- the receding-horizon advance under a distributed solution's policy for teams of up to 64 agents
// (policy_advance_dec_team.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance_dec_team.hpp"

namespace dpilqr {

int32_t launch_policy_advance_dec_team(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, hipStream_t st) {
    if (D.k > kPolicyTeamAgents)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_team: k=%d agents, a neighbourhood mask is one word of %d bits", D.k, kPolicyTeamAgents);
    if (const int32_t rc = check_kc_max("policy_advance_dec_team", D, a.plan.kc_max)) return rc;
    const int ipw = kPolicyTeamThreads / D.k;                  // items per workgroup
    const int64_t blocks = ((int64_t)D.B + ipw - 1) / ipw;
    if (blocks > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_team: %lld workgroups", (long long)blocks);
    if (D.B == 0) return DPILQR_OK;
    DISPATCH_FAMILY_ALL(D.n_s, {
        hipLaunchKernelGGL((k_policy_advance_dec_team<NS, NC, 1>), dim3((unsigned)blocks), dim3(kPolicyTeamThreads), 0, st, D, a.plan.X, a.plan.U,
                           a.plan.K, (int)a.plan.kc_max, reinterpret_cast<const unsigned long long*>(a.plan.nbr_bits), 1, (int)a.h, a.scen,
                           (int)a.n_scen, (int)a.L, (int)a.n_d, a.W, a.u_lim, a.x_cur, a.n_done, a.X_exec, a.U_exec, a.J_exec, a.min_sep,
                           a.dist_left, a.U_next, a.X_next);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

// tu_policy_advance_dec_wide.hip -- the receding-horizon advance under a distributed solution's policy for teams of up to 256
// agents (policy_advance_dec_team.hpp, four mask words) and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance_dec_team.hpp"

namespace dpilqr {

int32_t launch_policy_advance_dec_wide(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, int32_t n_words, hipStream_t st) {
    if (D.k > kPolicyWideAgents)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_wide: k=%d agents, the wide advance serves up to %d", D.k, kPolicyWideAgents);
    const int kc_lim = D.k < kPolicyWideMembers ? D.k : kPolicyWideMembers;
    if (a.plan.kc_max < 1 || a.plan.kc_max > kc_lim)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_wide: kc_max=%d, a neighbourhood has 1 .. min(k, %d) = %d members",
                    a.plan.kc_max, kPolicyWideMembers, kc_lim);
    if (n_words != (D.k + 63) / 64)
        return fail(DPILQR_EINVAL, "policy_advance_dec_wide: n_words=%d, k=%d agents take ceil(k / 64) = %d words", n_words, D.k, (D.k + 63) / 64);
    const int ipw = kPolicyTeamThreads / D.k;                  // items per workgroup
    const int64_t blocks = ((int64_t)D.B + ipw - 1) / ipw;
    if (blocks > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_wide: %lld workgroups", (long long)blocks);
    if (D.B == 0) return DPILQR_OK;
    DISPATCH_FAMILY_ALL(D.n_s, {
        hipLaunchKernelGGL((k_policy_advance_dec_team<NS, NC, kPolicyWideWords>), dim3((unsigned)blocks), dim3(kPolicyTeamThreads), 0, st, D, a.plan.X, a.plan.U,
                           a.plan.K, (int)a.plan.kc_max, reinterpret_cast<const unsigned long long*>(a.plan.nbr_bits), (int)n_words, (int)a.h,
                           a.scen, (int)a.n_scen, (int)a.L, (int)a.n_d, a.W, a.u_lim, a.x_cur, a.n_done, a.X_exec, a.U_exec, a.J_exec,
                           a.min_sep, a.dist_left, a.U_next, a.X_next);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

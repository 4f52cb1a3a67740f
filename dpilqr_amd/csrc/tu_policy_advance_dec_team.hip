// tu_policy_advance_dec_team.hip -- the receding-horizon advance under a distributed solution's policy for teams of up to 64 agents
// (policy_advance_dec_team.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance_dec_team.hpp"

namespace dpilqr {

int32_t launch_policy_advance_dec_team(const dpilqr_batch_desc& D, const double* X, const double* U_ff, const double* Kc, int32_t kc_max,
                                       const uint64_t* nbr_bits, int32_t h, const int32_t* scen, int32_t n_scen, int32_t L, int32_t n_d,
                                       const double* W, const double* u_lim, double* x_cur, int32_t* n_done, double* X_exec,
                                       double* U_exec, double* J_exec, double* min_sep, double* dist_left, double* U_next,
                                       double* X_next, hipStream_t st) {
    if (D.k > kPolicyTeamAgents)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_team: k=%d agents, a neighbourhood mask is one word of %d bits", D.k, kPolicyTeamAgents);
    if (kc_max < 1 || kc_max > D.k)
        return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_team: kc_max=%d, a neighbourhood has 1 .. k = %d members", kc_max, D.k);
    const int ipw = kPolicyTeamThreads / D.k;                  // items per workgroup
    const int64_t blocks = ((int64_t)D.B + ipw - 1) / ipw;
    if (blocks > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_advance_dec_team: %lld workgroups", (long long)blocks);
    if (D.B == 0) return DPILQR_OK;
    DISPATCH_FAMILY_ALL(D.n_s, {
        hipLaunchKernelGGL((k_policy_advance_dec_team<NS, NC>), dim3((unsigned)blocks), dim3(kPolicyTeamThreads), 0, st, D, X, U_ff, Kc,
                           (int)kc_max, reinterpret_cast<const unsigned long long*>(nbr_bits), (int)h, scen, (int)n_scen, (int)L, (int)n_d,
                           W, u_lim, x_cur, n_done, X_exec, U_exec, J_exec, min_sep, dist_left, U_next, X_next);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

// tu_policy.hip -- the closed-loop ensemble rollouts (policy.hpp; policy_dec.hpp for a distributed solution) and their launchers.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_dec.hpp"

namespace dpilqr {

struct PolicyGrid { unsigned blocks; int chunks; size_t lds; };      // blocks == 0: an empty batch, nothing to launch

// What the two launchers share, `who` naming the caller in the messages: the served shapes (the K[t] image has kc_max * n_s columns,
// the dense one kc_max = k, and fits the `stage` elements a thread copies per step), policy.hpp's launch geometry, the LDS grant.
template <typename Kern>
static int32_t policy_grid(const char* who, Kern kern, const dpilqr_batch_desc& D, int kc_max, int stage, int32_t n_samples, PolicyGrid& g) {
    const int n = D.k * D.n_s, m = D.k * D.n_c, kw = kc_max * D.n_s;
    if (n > kRouteSmallMaxNx || D.k > kRouteSmallMaxK)
        return fail(DPILQR_EUNSUPPORTED, "%s: n_x=%d, k=%d, the closed-loop rollout serves clusters up to n_x = 60 and k = 20", who, n, D.k);
    if (const int32_t rc = check_kc_max(who, D, kc_max)) return rc;
    if (m * kw > stage * kPolicyThreads)      // (cannot happen at n_x <= 60, kc_max <= k: the stages are sized for it)
        return fail(DPILQR_EUNSUPPORTED, "%s: K[t] of %d x %d exceeds the %d elements a workgroup copies per step", who, m, kw, stage * kPolicyThreads);
    const int spw = kPolicyThreads / D.k;                      // samples of one item per workgroup
    const int64_t chunks = ((int64_t)n_samples + spw - 1) / spw;
    if (chunks * D.B > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "%s: %lld workgroups", who, (long long)(chunks * D.B));
    g = {(unsigned)(chunks * D.B), (int)chunks, policy_lds_bytes(D.n_s, D.n_c, D.k)};
    return g.blocks ? allow_lds(kern, g.lds) : DPILQR_OK;
}

int32_t launch_policy_rollout(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st) {
    PolicyGrid g;
    DISPATCH_FAMILY_ALL(D.n_s, {
        const int32_t rc = policy_grid("policy_rollout", k_policy_rollout<NS, NC>, D, D.k, DenseGains<NS, NC>::kStage, a.n_samples, g);
        if (rc || g.blocks == 0) return rc;
        hipLaunchKernelGGL((k_policy_rollout<NS, NC>), dim3(g.blocks), dim3(kPolicyThreads), g.lds, st, D, a.plan.X, a.plan.U, a.plan.K,
                           (int)a.n_samples, g.chunks, a.x0s, a.W, a.u_lim, a.Xs, a.Us, a.J, a.min_sep, a.goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

int32_t launch_policy_rollout_dec(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st) {
    PolicyGrid g;
    DISPATCH_FAMILY_ALL(D.n_s, {
        const int32_t rc = policy_grid("policy_rollout_dec", k_policy_rollout_dec<NS, NC>, D, a.plan.kc_max, CompactGains<NS, NC>::kStage,
                                       a.n_samples, g);
        if (rc || g.blocks == 0) return rc;
        hipLaunchKernelGGL((k_policy_rollout_dec<NS, NC>), dim3(g.blocks), dim3(kPolicyThreads), g.lds, st, D, a.plan.X, a.plan.U, a.plan.K,
                           (int)a.plan.kc_max, reinterpret_cast<const unsigned long long*>(a.plan.nbr_bits), (int)a.n_samples, g.chunks,
                           a.x0s, a.W, a.u_lim, a.Xs, a.Us, a.J, a.min_sep, a.goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

// tu_policy.hip -- the closed-loop ensemble rollouts (policy.hpp; policy_dec.hpp for a distributed solution) and their launchers.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_dec.hpp"

namespace dpilqr {

int32_t launch_policy_rollout(const dpilqr_batch_desc& D, const double* X, const double* U, const double* K, int32_t n_samples,
                              const double* x0s, const double* W, const double* u_lim, double* Xs, double* Us, double* J,
                              double* min_sep, double* goal_dist, hipStream_t st) {
    const int n = D.k * D.n_s, m = D.k * D.n_c;
    if (n > 60) return fail(DPILQR_EUNSUPPORTED, "policy_rollout: n_x=%d, the closed-loop rollout serves clusters up to n_x = 60", n);
    if (m * n > kPolicyStage * kPolicyThreads)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout: K[t] of %d x %d exceeds the %d elements a workgroup copies per step", m, n,
                    kPolicyStage * kPolicyThreads);
    if (D.B == 0) return DPILQR_OK;
    const int spw = kPolicyThreads / D.k;                      // samples of one item per workgroup
    const int64_t chunks = ((int64_t)n_samples + spw - 1) / spw;
    if (chunks * D.B > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_rollout: %lld workgroups", (long long)(chunks * D.B));
    const size_t lds = policy_lds_bytes(D.n_s, D.n_c, D.k);
    DISPATCH_FAMILY_ALL(D.n_s, {
        int32_t rc = allow_lds(k_policy_rollout<NS, NC>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL((k_policy_rollout<NS, NC>), dim3((unsigned)(chunks * D.B)), dim3(kPolicyThreads), lds, st, D, X, U, K,
                           (int)n_samples, (int)chunks, x0s, W, u_lim, Xs, Us, J, min_sep, goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

int32_t launch_policy_rollout_dec(const dpilqr_batch_desc& D, const double* X, const double* U_ff, const double* Kc, int32_t kc_max,
                                  const uint64_t* nbr_bits, int32_t n_samples, const double* x0s, const double* W, const double* u_lim,
                                  double* Xs, double* Us, double* J, double* min_sep, double* goal_dist, hipStream_t st) {
    const int n = D.k * D.n_s, m = D.k * D.n_c;
    if (n > 60 || D.k > 20)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec: n_x=%d, k=%d, the closed-loop rollout serves n_x <= 60 and k <= 20", n, D.k);
    if (kc_max < 1 || kc_max > D.k)
        return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec: kc_max=%d, a neighbourhood has 1 .. k = %d members", kc_max, D.k);
    const int kw = kc_max * D.n_s;
    if (D.B == 0) return DPILQR_OK;
    const int spw = kPolicyThreads / D.k;
    const int64_t chunks = ((int64_t)n_samples + spw - 1) / spw;
    if (chunks * D.B > 0x7fffffffLL) return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec: %lld workgroups", (long long)(chunks * D.B));
    const size_t lds = policy_lds_bytes(D.n_s, D.n_c, D.k);
    DISPATCH_FAMILY_ALL(D.n_s, {
        if (m * kw > kPolicyDecStage<NS, NC> * kPolicyThreads)      // (cannot happen at n_x <= 60, kc_max <= k: the stage is sized for it)
            return fail(DPILQR_EUNSUPPORTED, "policy_rollout_dec: Kc[t] of %d x %d exceeds the %d elements a workgroup copies per step", m, kw,
                        kPolicyDecStage<NS, NC> * kPolicyThreads);
        int32_t rc = allow_lds(k_policy_rollout_dec<NS, NC>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL((k_policy_rollout_dec<NS, NC>), dim3((unsigned)(chunks * D.B)), dim3(kPolicyThreads), lds, st, D, X, U_ff, Kc,
                           (int)kc_max, reinterpret_cast<const unsigned long long*>(nbr_bits), (int)n_samples, (int)chunks, x0s, W, u_lim,
                           Xs, Us, J, min_sep, goal_dist);
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

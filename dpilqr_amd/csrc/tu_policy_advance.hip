// tu_policy_advance.hip -- the receding-horizon advance (policy_advance.hpp), dense and compact gains, and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance.hpp"

namespace dpilqr {

// kc_max == 0: the dense form (K[B][T][n_u][n_x]); otherwise K is Kc[B][T][k][n_c][kc_max * n_s] with the masks nbr_bits
int32_t launch_policy_advance(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, hipStream_t st) {
    const PolicyPlan& p = a.plan;
    const char* who = p.kc_max ? "policy_advance_dec" : "policy_advance";
    const int n = D.k * D.n_s;
    if (n > kRouteSmallMaxNx || D.k > kRouteSmallMaxK)
        return fail(DPILQR_EUNSUPPORTED, "%s: n_x=%d, k=%d, the receding-horizon advance serves clusters up to n_x = 60 and k = 20", who, n, D.k);
    if (D.B == 0) return DPILQR_OK;
    const int ipw = kPolicyThreads / D.k;                      // items per workgroup
    const unsigned blocks = (unsigned)(((int64_t)D.B + ipw - 1) / ipw);
    const size_t lds = advance_lds_bytes(D.n_s, D.k);
    DISPATCH_FAMILY_ALL(D.n_s, {
        if (p.kc_max) {
            const int32_t rc = allow_lds(k_policy_advance_dec<NS, NC>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL((k_policy_advance_dec<NS, NC>), dim3(blocks), dim3(kPolicyThreads), lds, st, D, p.X, p.U, p.K, (int)p.kc_max,
                               reinterpret_cast<const unsigned long long*>(p.nbr_bits), (int)a.h, a.scen, (int)a.n_scen, (int)a.L, (int)a.n_d,
                               a.W, a.u_lim, a.x_cur, a.n_done, a.X_exec, a.U_exec, a.J_exec, a.min_sep, a.dist_left, a.U_next, a.X_next);
        } else {
            const int32_t rc = allow_lds(k_policy_advance<NS, NC>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL((k_policy_advance<NS, NC>), dim3(blocks), dim3(kPolicyThreads), lds, st, D, p.X, p.U, p.K, (int)a.h, a.scen,
                               (int)a.n_scen, (int)a.L, (int)a.n_d, a.W, a.u_lim, a.x_cur, a.n_done, a.X_exec, a.U_exec, a.J_exec, a.min_sep,
                               a.dist_left, a.U_next, a.X_next);
        }
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

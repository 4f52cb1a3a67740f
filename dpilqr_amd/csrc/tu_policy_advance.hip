// tu_policy_advance.hip -- the receding-horizon advance (policy_advance.hpp), dense and compact gains, and its launcher.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "policy_advance.hpp"

namespace dpilqr {

// kc_max == 0: the dense form (K[B][T][n_u][n_x]); otherwise K is Kc[B][T][k][n_c][kc_max * n_s] with the masks nbr_bits
int32_t launch_policy_advance(const dpilqr_batch_desc& D, const double* X, const double* U, const double* K, int32_t kc_max,
                              const uint64_t* nbr_bits, int32_t h, const int32_t* scen, int32_t n_scen, int32_t L, int32_t n_d,
                              const double* W, const double* u_lim, double* x_cur, int32_t* n_done, double* X_exec, double* U_exec,
                              double* J_exec, double* min_sep, double* dist_left, double* U_next, double* X_next, hipStream_t st) {
    const char* who = kc_max ? "policy_advance_dec" : "policy_advance";
    const int n = D.k * D.n_s;
    if (n > 60 || D.k > 20)
        return fail(DPILQR_EUNSUPPORTED, "%s: n_x=%d, k=%d, the receding-horizon advance serves clusters up to n_x = 60 and k = 20", who, n, D.k);
    if (D.B == 0) return DPILQR_OK;
    const int ipw = kPolicyThreads / D.k;                      // items per workgroup
    const unsigned blocks = (unsigned)(((int64_t)D.B + ipw - 1) / ipw);
    const size_t lds = advance_lds_bytes(D.n_s, D.k);
    DISPATCH_FAMILY_ALL(D.n_s, {
        if (kc_max) {
            const int32_t rc = allow_lds(k_policy_advance_dec<NS, NC>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL((k_policy_advance_dec<NS, NC>), dim3(blocks), dim3(kPolicyThreads), lds, st, D, X, U, K, (int)kc_max,
                               reinterpret_cast<const unsigned long long*>(nbr_bits), (int)h, scen, (int)n_scen, (int)L, (int)n_d, W, u_lim,
                               x_cur, n_done, X_exec, U_exec, J_exec, min_sep, dist_left, U_next, X_next);
        } else {
            const int32_t rc = allow_lds(k_policy_advance<NS, NC>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL((k_policy_advance<NS, NC>), dim3(blocks), dim3(kPolicyThreads), lds, st, D, X, U, K, (int)h, scen,
                               (int)n_scen, (int)L, (int)n_d, W, u_lim, x_cur, n_done, X_exec, U_exec, J_exec, min_sep, dist_left,
                               U_next, X_next);
        }
    })
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

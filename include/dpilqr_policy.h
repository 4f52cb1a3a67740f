/*
 * dpilqr_policy.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * Additive: DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, fp64, row-major, `stream`, error codes): dpilqr_hip.h.
 */
#ifndef DPILQR_POLICY_H
#define DPILQR_POLICY_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

/* The closed-loop ensemble rollout.
 * Runs the time-varying feedback policy a solution defines -- nominal X[B][T+1][n_x], U[B][T][n_u], gains K[B][T][n_u][n_x] of
 * a backward pass at that (X, U) -- from n_samples = S starts per item, in one launch.  Not a reference function (the reference
 * only ever applies a plan open loop); the step, the cost and its summation order are dpilqr_rollout's.
 * Per (item b, sample s):
 *     x_0 = x0s[b][s]                                                   x0s[B][S][n_x]
 *     for t = 0 .. T-1:
 *         u_t = U[b][t] + K[b][t] (x_t - X[b][t])                       (the sum over columns 0 .. n_x-1 in that order)
 *         u_t = u < lo ? lo : (u > hi ? hi : u)   per entry             u_lim[2][n_u]: lower row, upper row, shared by all
 *                                                                       items; NULL: no limits.  A NaN stays a NaN.
 *         x_{t+1} = step(x_t, u_t)                                      the per-agent model step of dpilqr_rollout (five RK4
 *                                                                       sub-steps; BikeDynamics5D: one RK4 step)
 *         x_{t+1} += W[b][s][t]                                         W[B][S][T][n_x] additive disturbance; NULL: none
 *     J[b][s]         = sum_t cost(x_t, u_t) + cost(x_T, 0, terminal)   summed as the rollout sums it: pairs in combinations
 *                                                                       order, agents in order, then time -- dpilqr_rollout fed
 *                                                                       Us[b][s] from x0s[b][s] (W = NULL) returns the same J
 *     min_sep[b][s]   = min over t in [0, T] and pairs i < j of the distance ProximityCost measures (cost.py:117-133): over
 *                       min(n_dims_i, n_dims_j) coordinates, or the planar distance when every agent has the same n_dims
 *                       (quirk Q5); +inf for k = 1
 *     goal_dist[b][s][a] = |x_T - xf| over agent a's first n_dims_a coordinates
 * Xs[B][S][T+1][n_x], Us[B][S][T][n_u]: the samples' trajectories; either may be NULL (not stored).  min_sep, goal_dist may be
 * NULL.  Served: every family with n_x <= 60, models mixed within a family; DPILQR_EUNSUPPORTED beyond, before any launch.
 * fp64 only.  Enqueue only, nothing is allocated.  One workgroup holds floor(256 / k) samples of one item and reads K[t], X[t],
 * U[t] once per step for all of them (csrc/policy.hpp). */
int32_t dpilqr_policy_rollout(const dpilqr_batch_desc* desc, const double* X, const double* U, const double* K,
                              int32_t n_samples, const double* x0s, const double* W, const double* u_lim, double* Xs,
                              double* Us, double* J, double* min_sep, double* goal_dist, void* stream);

#endif /* DPILQR_POLICY_H */

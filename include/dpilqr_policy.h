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

/* The same rollout for LARGE clusters, 60 < n_x <= 240 with k <= 20: the four-, six- and twelve-state families, models mixed
 * within a family (the padded HumanDynamics6D among twelve-state agents included) -- BASELINE config 5's twenty heterogeneous
 * agents, n_x = 240, n_u = 80, are the largest.  Arguments, shapes and results are dpilqr_policy_rollout's, with ONE difference
 * in the arithmetic: K[b][t] (x_t - X[b][t]) of all the samples a workgroup holds is one (n_u x n_x)(n_x x samples) product on
 * the fp64 matrix pipe, so each u_t entry is U[b][t] + (the sum over columns 0 .. n_x-1 in that order, ONE FUSED multiply-add
 * per term, starting from zero) -- where dpilqr_policy_rollout rounds every product and every addition separately.  K[t] is
 * read from global memory once per workgroup and step and never staged (csrc/policy_large.hpp).
 * DPILQR_EINVAL: the NULL, alignment and n_samples conditions of dpilqr_policy_rollout.  DPILQR_EUNSUPPORTED, before any launch:
 * n_x <= 60 (that is dpilqr_policy_rollout's range), n_x > 240, k > 20, more than 2^31 - 1 workgroups.  B = 0: DPILQR_OK, nothing
 * is launched.  fp64 only.  Enqueue only, nothing is allocated. */
int32_t dpilqr_policy_rollout_large(const dpilqr_batch_desc* desc, const double* X, const double* U, const double* K,
                                    int32_t n_samples, const double* x0s, const double* W, const double* u_lim, double* Xs,
                                    double* Us, double* J, double* min_sep, double* goal_dist, void* stream);

/* The closed loop of a DISTRIBUTED solution (dpilqr_dispatch_* of dpilqr_hip.h): every agent runs the feedback law of the
 * sub-problem solved for its own neighbourhood.  Agent i of item b has the neighbourhood mask nbr_bits[b][i] (bit j = agent j;
 * bit i set; the masks need not be symmetric), C_i its members in ascending order, kc_i their number, kw = kc_max * n_s.
 * Per (item b, sample s), with the steps, limits, disturbance and results of dpilqr_policy_rollout on the FULL k-agent problem
 * of `desc` (all pairs in combinations order, quirk Q5):
 *     u_i(t) = U_ff[b][t][i] + sum_col Kc[b][t][i][.][col] (x_{C_i}(t) - X[b][t]_{C_i})[col]     col = 0 .. kc_i * n_s - 1, ascending
 * X[B][T+1][n_x]: the stitched trajectory X_dec; U_ff[B][T][n_u]; Kc[B][T][k][n_c][kw] compact gains: agent i's n_c rows, the
 * columns C_i's members in ascending order.  Columns at and past kc_i * n_s are never read (they may hold anything, NaN included).
 * Limits: fp64, n_x <= 60, k <= 20, 1 <= kc_max <= k; DPILQR_EUNSUPPORTED beyond, before any launch.
 * The caller's contract, NOT checked here (the masks are device memory and this call only enqueues): every mask has its own
 * bit and at most kc_max bits among the low k.  A mask that breaks it makes that agent's controls meaningless (members past
 * the kc_max-th are dropped); no memory outside the arguments is touched.  The Python wrapper checks the masks on the host and answers DPILQR_EINVAL.
 * Enqueue only, nothing is allocated.  The kernel reads k n_c kw doubles of gains per step and workgroup where the dense form
 * reads n_u n_x (csrc/policy_dec.hpp). */
int32_t dpilqr_policy_rollout_dec(const dpilqr_batch_desc* desc, const double* X, const double* U_ff, const double* Kc,
                                  int32_t kc_max, const uint64_t* nbr_bits, int32_t n_samples, const double* x0s, const double* W,
                                  const double* u_lim, double* Xs, double* Us, double* J, double* min_sep, double* goal_dist,
                                  void* stream);

/* The same closed loop for a whole TEAM of up to 64 agents, whatever n_x = k n_s is (64 double integrators: n_x = 256, beyond
 * every centralised kernel): neighbourhood-only feedback is what a large team can still run.  Arguments, shapes and results are
 * dpilqr_policy_rollout_dec's and so is the definition, unchanged:
 *     u_i(t) = clamp( U_ff[b][t][i] + sum ),   sum = columns 0 .. kc_i*n_s-1 of Kc[b][t][i] times (x_{C_i}(t) - X[b][t]_{C_i}),
 *              ascending, starting from zero, one multiply and one add per term (no contraction)
 *     x_{t+1} = step(x_t, u_t) [+ W]
 * with J, min_sep and goal_dist as dpilqr_policy_rollout defines them on the full k-agent problem (all k (k - 1) / 2 pairs,
 * quirk Q5).  Where both entries serve a shape, Xs, Us and goal_dist agree bit for bit; J and min_sep agree to rounding: a
 * sample's stage cost is summed agent by agent (each agent's share of the pairs first), in an order that depends on k alone --
 * no floating-point atomics, the same bits whatever n_samples, the batch or the item's place in it.
 * A thread per (sample, agent) reads its own compact rows straight from global memory; the K[t] image is never staged
 * (csrc/policy_dec_team.hpp).  A mask is ONE 64-bit word: bit 63 is a member like any other.
 * Served: 1 <= k <= 64, every family (models mixed within a family), 1 <= kc_max <= k.  DPILQR_EINVAL: the NULL, alignment and
 * n_samples < 1 conditions of dpilqr_policy_rollout (nbr_bits as in dpilqr_policy_rollout_dec); (n_s, n_c) not a model family.
 * DPILQR_EUNSUPPORTED, before any launch: k > 64; more than 12 agents of the five-state family (dpilqr_rollout's limit); kc_max
 * outside 1 .. k; more than 2^31 - 1 workgroups (one holds floor(256 / k) samples of one item).  B = 0: DPILQR_OK, nothing is
 * launched.  The masks are the caller's contract as for dpilqr_policy_rollout_dec (own bit, at most kc_max bits among the low
 * k): a mask that breaks it makes that agent's controls meaningless (members past the kc_max-th are dropped) and no address
 * depends on it beyond the Kc[b][t] image.  Columns at and past kc_i * n_s are never read.  fp64 only.  Enqueue only, nothing is
 * allocated. */
int32_t dpilqr_policy_rollout_dec_team(const dpilqr_batch_desc* desc, const double* X, const double* U_ff, const double* Kc,
                                       int32_t kc_max, const uint64_t* nbr_bits, int32_t n_samples, const double* x0s,
                                       const double* W, const double* u_lim, double* Xs, double* Us, double* J, double* min_sep,
                                       double* goal_dist, void* stream);

/* Gains of the solved sub-problems, per cluster size kc, beside dpilqr_bucket_results (same slices [first, first + count)):
 * K[kc] is [count][T][kc*n_c][kc*n_s], a backward pass at that bucket's (X, U). */
typedef struct dpilqr_bucket_gains {
    const double* K[DPILQR_MAX_AGENTS + 1];
} dpilqr_bucket_gains;

/* The stitch of the distributed policy, after dpilqr_dispatch_stitch has filled X_dec: for every (scenario s, agent i) whose
 * sub-problem (neighbourhood C_i of kc members, i at rank pos, solution X^i, U^i, gains K^i) is among `results`,
 *     Kc[s][t][i][c][col]   = K^i[t][pos*n_c + c][col]   for col < kc*n_s, 0 for kc*n_s <= col < kc_max*n_s
 *     U_ff[s][t][i*n_c + c] = U^i[t][pos*n_c + c] + sum_col K^i[t][pos*n_c + c][col] (X_dec[s][t]_{C_i}[col] - X^i[t][col])
 * (columns ascending, one multiply and one add per term): the nominal of dpilqr_policy_rollout_dec, for which
 * u_i = U^i_i + K^i_i (x_{C_i} - X^i).  Where C_i is the whole scenario U_ff equals U_dec.  kc_max: at least the largest
 * populated cluster size (DPILQR_EINVAL otherwise).  Kc[S][T][k][n_c][kc_max*n_s], U_ff[S][T][k*n_c].  Enqueue only. */
int32_t dpilqr_dispatch_stitch_policy(int32_t S, int32_t k, int32_t n_s, int32_t n_c, int32_t T, int32_t kc_max, const uint64_t* bits,
                                      const int32_t* rep, const int32_t* size, const int32_t* slot,
                                      const dpilqr_bucket_results* results, const dpilqr_bucket_gains* gains, const double* X_dec,
                                      double* Kc, double* U_ff, void* stream);

/* The step between two solves of a receding-horizon loop: execute h steps of each running scenario's CURRENT plan on the plant
 * and do the loop's bookkeeping, in one launch.  `desc` describes the B items of this round -- the scenarios still running,
 * compact -- with their plans X[B][T+1][n_x], U[B][T][n_u] and gains K[B][T][n_u][n_x] (K NULL: the plan is executed open loop).
 * The loop's state is indexed by SCENARIO: item j is scenario s = scen[j] (scen NULL: s = j) of n_scen; it has executed
 * n_done[s] steps so far out of a capacity of L.  Per item j:
 *     he = min(h, L - n_done[s])                            never past the capacity
 *     x  = x_cur[s];  g = n_done[s]                         x_cur[n_scen][n_x], n_done[n_scen]
 *     if g == 0: min_sep[s] = separation(x)                 the start state counts (a caller sets min_sep to +inf otherwise)
 *     for i = 0 .. he-1:
 *         u = U[j][i] + K[j][i] (x - X[j][i])               the sum over columns 0 .. n_x-1 in that order, as dpilqr_policy_rollout
 *         u = u < lo ? lo : (u > hi ? hi : u)   per entry   u_lim[2][n_u], NULL: no limits.  A NaN stays a NaN.
 *         X_exec[s][g+i] = x;  U_exec[s][g+i] = u           X_exec[n_scen][L+1][n_x], U_exec[n_scen][L][n_u]
 *         J_exec[s] = J_exec[s] + cost(x, u)                ONE addition per step, in time order; the stage cost summed as the
 *                                                           rollout sums it (pairs in combinations order, agents in order)
 *         x = step(x, u)   [+ W[s][g+i]]                    W[n_scen][L][n_x] additive disturbance, NULL: none
 *         min_sep[s] = min(min_sep[s], separation(x))       the distance dpilqr_policy_rollout's min_sep measures (quirk Q5)
 *     X_exec[s][g+he] = x;  x_cur[s] = x;  n_done[s] = g + he
 *     dist_left[s][a] = |x - xf| over agent a's first n_d coordinates          dist_left[n_scen][k]
 *     U_next[s][t] = U[j][t+he] for t < T-he, 0 beyond                         U_next[n_scen][T][n_u]: the next warm start
 *     X_next[s][0] = x;  X_next[s][t] = X[j][min(t+he, T)] for 1 <= t <= T     X_next[n_scen][T+1][n_x]
 * The step, the cost and the separation are dpilqr_policy_rollout's, statement for statement: X_exec / U_exec equal the prefix
 * of that rollout's Xs / Us bit for bit, and two calls of h1 and h2 steps equal one of h1 + h2 (on the shifted plan).
 * U_next / X_next must not alias U / X.  Scenarios not named in scen are not touched; an entry of scen outside [0, n_scen) is
 * skipped; scen must not name a scenario twice.
 * DPILQR_EINVAL: a NULL among desc, X, U, x_cur, n_done, X_exec, U_exec, J_exec, min_sep, dist_left, U_next, X_next; h < 1 or
 * h > T; L < 1; n_d < 1 or n_d > n_s; n_scen < B; a pointer not aligned to its element type.  DPILQR_EUNSUPPORTED, before
 * any launch: n_x > 60 or k > 20.  B = 0: DPILQR_OK, nothing is launched.  fp64 only.  Enqueue only, nothing is allocated.
 * One workgroup holds floor(256 / k) ITEMS (csrc/policy_advance.hpp). */
int32_t dpilqr_policy_advance(const dpilqr_batch_desc* desc, const double* X, const double* U, const double* K, int32_t h,
                              const int32_t* scen, int32_t n_scen, int32_t L, int32_t n_d, const double* W, const double* u_lim,
                              double* x_cur, int32_t* n_done, double* X_exec, double* U_exec, double* J_exec, double* min_sep,
                              double* dist_left, double* U_next, double* X_next, void* stream);

/* The same step for LARGE clusters, 60 < n_x <= 240 with k <= 20: the four-, six- and twelve-state families, models mixed within
 * a family (the padded HumanDynamics6D among twelve-state agents included).  Arguments, shapes and semantics are
 * dpilqr_policy_advance's, statement for statement (he, scen, X_exec / U_exec / J_exec with ONE addition per step, min_sep with
 * the start state when g == 0, dist_left, x_cur, n_done, the shifted U_next / X_next, K NULL: open loop, scenarios not named
 * untouched, entries of scen out of range skipped), with ONE difference in the arithmetic, the one
 * dpilqr_policy_rollout_large has against dpilqr_policy_rollout: each entry of K[j][i] (x - X[j][i]) is the sum over columns
 * 0 .. n_x-1 in that order, ONE FUSED multiply-add per term, starting from zero (the fp64 matrix pipe).  X_exec / U_exec of the
 * he executed steps equal the prefix of dpilqr_policy_rollout_large's Xs / Us bit for bit (one sample from x_cur[s], W padded
 * to the horizon).  One workgroup per item; K[i] is read from global memory once per step and never staged
 * (csrc/policy_advance_large.hpp).
 * DPILQR_EINVAL: the conditions of dpilqr_policy_advance.  DPILQR_EUNSUPPORTED, before any launch: n_x <= 60 (that is
 * dpilqr_policy_advance's range), n_x > 240, k > 20, a family other than (4, 2), (6, 3), (12, 4).  B = 0: DPILQR_OK, nothing is
 * launched.  fp64 only.  Enqueue only, nothing is allocated. */
int32_t dpilqr_policy_advance_large(const dpilqr_batch_desc* desc, const double* X, const double* U, const double* K, int32_t h,
                                    const int32_t* scen, int32_t n_scen, int32_t L, int32_t n_d, const double* W,
                                    const double* u_lim, double* x_cur, int32_t* n_done, double* X_exec, double* U_exec,
                                    double* J_exec, double* min_sep, double* dist_left, double* U_next, double* X_next,
                                    void* stream);

/* The same step under a DISTRIBUTED solution's policy: X is the stitched X_dec, the nominal U_ff[B][T][n_u], the gains
 * Kc[B][T][k][n_c][kc_max * n_s] and the masks nbr_bits[B][k] as dpilqr_policy_rollout_dec defines them (members lowest bit
 * first; columns at and past kc_i * n_s are never read; the masks are the caller's contract).  Kc NULL: u = U_ff (open loop:
 * pass U_dec), nbr_bits may then be NULL too.  Further DPILQR_EUNSUPPORTED: kc_max outside 1 .. k. */
int32_t dpilqr_policy_advance_dec(const dpilqr_batch_desc* desc, const double* X, const double* U_ff, const double* Kc,
                                  int32_t kc_max, const uint64_t* nbr_bits, int32_t h, const int32_t* scen, int32_t n_scen,
                                  int32_t L, int32_t n_d, const double* W, const double* u_lim, double* x_cur, int32_t* n_done,
                                  double* X_exec, double* U_exec, double* J_exec, double* min_sep, double* dist_left,
                                  double* U_next, double* X_next, void* stream);

/* The same step for a whole TEAM of up to 64 agents, whatever n_x = k n_s is: the receding-horizon advance of the teams
 * dpilqr_policy_rollout_dec_team serves.  Arguments and shapes are dpilqr_policy_advance_dec's, and the semantics are
 * dpilqr_policy_advance's, statement for statement: he = min(h, L - n_done[s]); scen maps items to scenarios, an entry out of
 * range is skipped, scenarios not named are untouched; X_exec, U_exec and J_exec are appended at the scenario's own offset, with
 * ONE addition to J_exec per executed step, in time order; the start state opens min_sep when n_done[s] == 0; dist_left over n_d
 * coordinates; x_cur and n_done updated; the shifted U_next / X_next (which must not alias the plan); Kc NULL: U_ff is executed
 * open loop and the masks are not read (nbr_bits may then be NULL).  The arithmetic is dpilqr_policy_rollout_dec_team's:
 *     u_i = clamp( U_ff[j][t][i] + sum ),   sum = columns 0 .. kc_i*n_s-1 of Kc[j][t][i] times (x_{C_i} - X[j][t]_{C_i}),
 *           ascending, starting from zero, one multiply and one add per term; the members of the 64-bit mask lowest bit first
 *     x = step(x, u) [+ W[s][g+t]]                          the model step is taken, then W is added
 *     the stage cost of a step: the k per-agent terms added in agent order, each w_prox times that agent's pair costs in
 *     ascending partner offset plus w_ref times its reference cost
 * so X_exec / U_exec of the he executed steps equal the prefix of dpilqr_policy_rollout_dec_team's Xs / Us bit for bit (one
 * sample from x_cur[s], W padded to the horizon).  Where dpilqr_policy_advance_dec also serves the shape, X_exec, U_exec, x_cur,
 * n_done, dist_left, U_next and X_next agree with it bit for bit; J_exec and min_sep agree to rounding (the relation the two
 * rollouts have).  No floating-point atomics: the same bits whatever the batch or the item's place in it.  One workgroup holds
 * floor(256 / k) ITEMS, a thread per (item, agent) reads its own compact rows straight from global memory
 * (csrc/policy_advance_dec_team.hpp).
 * Served: 1 <= k <= 64, every family (models mixed within a family), 1 <= kc_max <= k.  DPILQR_EINVAL: the conditions of
 * dpilqr_policy_advance; nbr_bits NULL while Kc is given, or misaligned; (n_s, n_c) not a model family.  DPILQR_EUNSUPPORTED,
 * before any launch: k > 64; more than 12 agents of the five-state family (dpilqr_rollout's limit); kc_max outside 1 .. k; more
 * than 2^31 - 1 workgroups.  B = 0: DPILQR_OK, nothing is launched.  The masks are the caller's contract as for
 * dpilqr_policy_rollout_dec (own bit, at most kc_max bits among the low k): a mask that breaks it makes that agent's controls
 * meaningless (members past the kc_max-th are dropped) and no address depends on it beyond the item's own Kc[j][t] image.
 * Columns at and past kc_i * n_s are never read.  fp64 only.  Enqueue only, nothing is allocated. */
int32_t dpilqr_policy_advance_dec_team(const dpilqr_batch_desc* desc, const double* X, const double* U_ff, const double* Kc,
                                       int32_t kc_max, const uint64_t* nbr_bits, int32_t h, const int32_t* scen, int32_t n_scen,
                                       int32_t L, int32_t n_d, const double* W, const double* u_lim, double* x_cur,
                                       int32_t* n_done, double* X_exec, double* U_exec, double* J_exec, double* min_sep,
                                       double* dist_left, double* U_next, double* X_next, void* stream);

#endif /* DPILQR_POLICY_H */

/*
 * dpilqr_swarm_policy.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * The closed-loop ROLLOUT of a distributed solution for teams of MORE than 64 agents: the stitch of the sub-problems' gains and
 * the rollout itself, over the multi-word neighbourhood masks of dpilqr_swarm.h.  Additive: DPILQR_ABI_VERSION is unchanged.
 * Conventions (device pointers, fp64, row-major, `stream`, error codes): dpilqr_hip.h.
 * The receding-horizon advance of such teams: dpilqr_swarm_advance.h.  Not built for such teams: fp32.
 */
#ifndef DPILQR_SWARM_POLICY_H
#define DPILQR_SWARM_POLICY_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

/* dpilqr_dispatch_stitch_policy (dpilqr_policy.h) for 1 <= k <= DPILQR_MAX_TEAM agents: the narrow entry's arguments, in its
 * order, plus n_words before `stream`; bits[S][k][n_words], word w bit b = agent 64 w + b.  The definition is the narrow entry's,
 * unchanged: for every (scenario s, agent i) whose sub-problem (neighbourhood C_i of kc members in ascending order, i at rank
 * pos -- the number of lower members, counted across the words --, solution X^i, U^i, gains K^i) is among `results`,
 *     Kc[s][t][i][c][col]   = K^i[t][pos*n_c + c][col]   for col < kc*n_s, 0 for kc*n_s <= col < kc_max*n_s
 *     U_ff[s][t][i*n_c + c] = U^i[t][pos*n_c + c] + sum_col K^i[t][pos*n_c + c][col] (X_dec[s][t]_{C_i}[col] - X^i[t][col])
 * (columns ascending, one multiply and one add per term).  A neighbourhood is a sub-problem: at most DPILQR_MAX_AGENTS members.
 * Kc[S][T][k][n_c][kc_max*n_s], U_ff[S][T][k*n_c].  With n_words = 1 both equal the narrow entry's bit for bit.
 * DPILQR_EINVAL before any launch: k < 1, k > DPILQR_MAX_TEAM, n_words != ceil(k / 64), kc_max outside
 * 1 .. min(k, DPILQR_MAX_AGENTS), and the narrow entry's conditions (a NULL pointer; a populated cluster size above kc_max or
 * without results).  Enqueue only. */
int32_t dpilqr_dispatch_stitch_policy_wide(int32_t S, int32_t k, int32_t n_s, int32_t n_c, int32_t T, int32_t kc_max,
                                           const uint64_t* bits, const int32_t* rep, const int32_t* size, const int32_t* slot,
                                           const dpilqr_bucket_results* results, const dpilqr_bucket_gains* gains,
                                           const double* X_dec, double* Kc, double* U_ff, int32_t n_words, void* stream);

/* dpilqr_policy_rollout_dec_team (dpilqr_policy.h) for a team of 1 <= k <= DPILQR_MAX_TEAM agents: that entry's arguments, in its
 * order, plus n_words before `stream`, and its definition and results, unchanged:
 *     u_i(t) = clamp( U_ff[b][t][i] + sum ),   sum = columns 0 .. kc_i*n_s-1 of Kc[b][t][i] times (x_{C_i}(t) - X[b][t]_{C_i}),
 *              ascending, starting from zero, one multiply and one add per term (no contraction)
 *     x_{t+1} = step(x_t, u_t) [+ W]
 * with J, min_sep and goal_dist as dpilqr_policy_rollout defines them on the full k-agent problem (all k (k - 1) / 2 pairs, quirk
 * Q5); Xs, Us may be NULL (not stored), min_sep and goal_dist too.
 * The masks are nbr_bits[B][k][n_words], n_words = ceil(k / 64): word w bit b = agent 64 w + b; C_i are agent i's members in
 * ascending order -- word by word, lowest bit first.  A neighbourhood is a sub-problem of the distributed solve: 1 <= kc_max <=
 * min(k, DPILQR_MAX_AGENTS) members, whatever k is; Kc[B][T][k][n_c][kc_max * n_s].
 * A sample's stage cost is the k per-agent terms added in agent order, each w_prox times that agent's pair costs in ascending
 * partner offset (1 .. k / 2) plus w_ref times its reference cost: no floating-point atomics, a summation shape that depends on
 * k alone, the same bits whatever n_samples, the batch or the item's place in it.  With n_words = 1 and k <= 64 all five results
 * (Xs, Us, J, min_sep, goal_dist) equal dpilqr_policy_rollout_dec_team's bit for bit.
 * A thread per (sample, agent), floor(256 / k) samples of one item per workgroup, the compact rows read straight from global
 * memory (csrc/policy_dec_team.hpp at four mask words).
 * DPILQR_EINVAL: the NULL, alignment and n_samples < 1 conditions of dpilqr_policy_rollout_dec_team; n_words != ceil(k / 64);
 * (n_s, n_c) not a model family.  DPILQR_EUNSUPPORTED, before any launch: k > DPILQR_MAX_TEAM; kc_max outside
 * 1 .. min(k, DPILQR_MAX_AGENTS); more than 12 agents of the five-state family (dpilqr_rollout's limit); more than 2^31 - 1
 * workgroups.  B = 0: DPILQR_OK, nothing is launched.  The masks are the caller's contract, as for dpilqr_policy_rollout_dec:
 * own bit set, at most kc_max members, nothing at or past bit k.  A mask that breaks it makes that agent's controls meaningless
 * (only the lowest kc_max members among the low k bits are kept) and no address depends on it beyond the agent's own Kc rows
 * and the sample's own state.  Columns at and past kc_i * n_s are never read.  fp64 only.  Enqueue only, nothing is allocated. */
int32_t dpilqr_policy_rollout_dec_wide(const dpilqr_batch_desc* desc, const double* X, const double* U_ff, const double* Kc,
                                       int32_t kc_max, const uint64_t* nbr_bits, int32_t n_samples, const double* x0s,
                                       const double* W, const double* u_lim, double* Xs, double* Us, double* J, double* min_sep,
                                       double* goal_dist, int32_t n_words, void* stream);

#endif /* DPILQR_SWARM_POLICY_H */

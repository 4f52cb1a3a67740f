/*
 * dpilqr_swarm_advance.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * The RECEDING-HORIZON step of a distributed solution for teams of MORE than 64 agents: the advance between two solves over the
 * multi-word neighbourhood masks of dpilqr_swarm.h, and the cost of a point of such a team (the loop's terminal cost).
 * Additive: DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, fp64, row-major, `stream`, error codes): dpilqr_hip.h.
 * Not built for such teams: fp32.
 */
#ifndef DPILQR_SWARM_ADVANCE_H
#define DPILQR_SWARM_ADVANCE_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

/* dpilqr_policy_advance_dec_team (dpilqr_policy.h) for a team of 1 <= k <= DPILQR_MAX_TEAM agents: that entry's arguments, in its
 * order, plus n_words before `stream`, and its semantics, statement for statement: he = min(h, L - n_done[s]); scen maps items to
 * scenarios, an entry out of range is skipped, scenarios not named are untouched; X_exec, U_exec and J_exec are appended at the
 * scenario's own offset, with ONE addition to J_exec per executed step, in time order; the start state opens min_sep when
 * n_done[s] == 0; dist_left over n_d coordinates; x_cur and n_done updated; the shifted U_next / X_next (which must not alias the
 * plan); Kc NULL: U_ff is executed open loop and the masks are not read (nbr_bits may then be NULL).
 * The masks are nbr_bits[B][k][n_words], n_words = ceil(k / 64): word w bit b = agent 64 w + b; C_i are agent i's members in
 * ascending order -- word by word, lowest bit first.  A neighbourhood is a sub-problem of the distributed solve: 1 <= kc_max <=
 * min(k, DPILQR_MAX_AGENTS) members, whatever k is; Kc[B][T][k][n_c][kc_max * n_s].
 * The arithmetic is dpilqr_policy_rollout_dec_wide's (dpilqr_swarm_policy.h), so X_exec / U_exec of the he executed steps equal the
 * prefix of that rollout's Xs / Us bit for bit (one sample from x_cur[s], W padded to the horizon).  With n_words = 1 and k <= 64
 * all nine state fields equal dpilqr_policy_advance_dec_team's bit for bit.  No floating-point atomics: the same bits whatever the
 * batch or the item's place in it.  One workgroup holds floor(256 / k) ITEMS -- 3 at k = 65 .. 85, 2 at 86 .. 128, 1 above --, a
 * thread per (item, agent) reads its own compact rows straight from global memory; thread a takes the pairs (a, a + dd mod k),
 * dd = 1 .. k / 2 (csrc/policy_advance_dec_team.hpp at four mask words).
 * DPILQR_EINVAL: the conditions of dpilqr_policy_advance_dec_team (a NULL pointer; h < 1 or h > T; L < 1; n_d outside 1 .. n_s;
 * n_scen < B; a misaligned pointer; nbr_bits NULL while Kc is given; (n_s, n_c) not a model family); n_words != ceil(k / 64).
 * DPILQR_EUNSUPPORTED, before any launch: k > DPILQR_MAX_TEAM; kc_max outside 1 .. min(k, DPILQR_MAX_AGENTS) (checked whether or
 * not Kc is given, as the team entry checks it: pass 1 with Kc NULL); more than 12 agents of the five-state family; more than
 * 2^31 - 1 workgroups.  B = 0: DPILQR_OK, nothing is launched.  The masks are the caller's contract as for
 * dpilqr_policy_rollout_dec_wide: a mask that breaks it makes that agent's controls meaningless (only the lowest kc_max members
 * among the low k bits are kept) and no address depends on it beyond the agent's own Kc rows and the item's own state.  Columns at
 * and past kc_i * n_s are never read.  fp64 only.  Enqueue only, nothing is allocated. */
int32_t dpilqr_policy_advance_dec_wide(const dpilqr_batch_desc* desc, const double* X, const double* U_ff, const double* Kc,
                                       int32_t kc_max, const uint64_t* nbr_bits, int32_t h, const int32_t* scen, int32_t n_scen,
                                       int32_t L, int32_t n_d, const double* W, const double* u_lim, double* x_cur,
                                       int32_t* n_done, double* X_exec, double* U_exec, double* J_exec, double* min_sep,
                                       double* dist_left, double* U_next, double* X_next, int32_t n_words, void* stream);

/* dpilqr_cost_eval (dpilqr_hip.h) for a team of 1 <= k <= DPILQR_MAX_TEAM agents: that entry's arguments, definition and kernel
 * (one thread per point, the k (k - 1) / 2 pair terms in combinations order), so at k <= 64 the results equal dpilqr_cost_eval's
 * bit for bit.  DPILQR_EUNSUPPORTED: k > DPILQR_MAX_TEAM; more than 12 agents of the five-state family.  The pair terms of a
 * point are serial (32,640 at k = 256): meant for a few points, such as the terminal cost of a receding-horizon loop's final
 * state, not for a trajectory. */
int32_t dpilqr_cost_eval_wide(const dpilqr_batch_desc* desc, int32_t n_pts, const double* x, const double* u,
                              int32_t terminal, double* cost, void* stream);

#endif /* DPILQR_SWARM_ADVANCE_H */

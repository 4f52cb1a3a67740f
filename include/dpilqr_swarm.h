/*
 * dpilqr_swarm.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * Distributed solves for teams of MORE than 64 agents: section 7's front and back end over multi-word neighbourhood masks, and the
 * full-team rollout behind J_full.  Additive: DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, fp64, row-major,
 * `stream`, error codes): dpilqr_hip.h.
 */
#ifndef DPILQR_SWARM_H
#define DPILQR_SWARM_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

#define DPILQR_MAX_TEAM 256 /* agents of ONE problem the wide entries serve; a sub-problem (cluster) still has at most DPILQR_MAX_AGENTS */

/* dispatch_graph / dispatch_gather / dispatch_stitch (dpilqr_hip.h, section 7) for 1 <= k <= DPILQR_MAX_TEAM agents: the narrow
 * entry's arguments, in its order, plus n_words before `stream`.
 * A neighbourhood is n_words = ceil(k / 64) words: bits[S][k][n_words], word w bit b = agent 64 w + b.  The definitions are the
 * narrow entries': a neighbour is within 2 * radius (planar, sqrt(dx*dx + dy*dy) < 2 radius, no fused multiply-add) on any sampled
 * row; the agent's own bit is always set; rep = the first agent with an identical mask (quirk Q11; ignored agents: -1); the sort of
 * the representatives by cluster size is stable; an owner's columns sit at the number of lower members of its mask, counted
 * across the words.  With n_words = 1 every output equals the narrow entry's, bit for bit.
 * bucket_start / bucket_count[k+1] are indexed by cluster size 0 .. k.  dpilqr_bucket_results, and with it gather and stitch,
 * serve cluster sizes up to DPILQR_MAX_AGENTS: a caller that finds a populated size beyond that in bucket_count must not go on
 * (gather_wide answers DPILQR_EINVAL for kc > DPILQR_MAX_AGENTS; stitch_wide leaves such owners' columns untouched).
 * DPILQR_EINVAL before any launch: k < 1, k > DPILQR_MAX_TEAM, n_words != ceil(k / 64), and the narrow entries' conditions.
 * The graph is one workgroup per scenario: the sampled rows' planar positions are staged in LDS (at most 19 rows x 256 agents x 2
 * doubles) and a wavefront produces one mask word at a time, as a wave64 ballot (csrc/frontend_wide.hpp). */
int32_t dpilqr_dispatch_graph_wide(int32_t S, int32_t N, int32_t k, int32_t n_s, const double* X, const double* radius,
                                   int64_t radius_stride, const int32_t* ignore, uint64_t* bits, int32_t* rep, int32_t* size,
                                   int32_t* order, int32_t* slot, int32_t* bucket_start, int32_t* bucket_count, int32_t n_words,
                                   void* stream);
int32_t dpilqr_dispatch_gather_wide(int32_t k, int32_t n_s, int32_t n_c, int32_t T, int32_t n_rows, int32_t kc, const int32_t* order,
                                    int32_t first, int32_t count, const uint64_t* bits, const double* X, const double* U,
                                    const double* xf, int64_t xf_stride, double* x0_out, double* xf_out, double* U_out,
                                    int32_t* members, int32_t n_words, void* stream);
int32_t dpilqr_dispatch_stitch_wide(int32_t S, int32_t k, int32_t n_s, int32_t n_c, int32_t T, const uint64_t* bits,
                                    const int32_t* rep, const int32_t* size, const int32_t* slot,
                                    const dpilqr_bucket_results* results, double* X_dec, double* U_dec, int32_t n_words, void* stream);

/* dpilqr_rollout's definition (ilqrSolver._rollout, control.py:80-93) for a full team of 1 <= k <= DPILQR_MAX_TEAM agents of any
 * family dpilqr_rollout serves, models and n_dims mixed as there: J_full of a distributed solve.
 *     x0[B][n_x], U[B][T][n_u] -> X[B][T+1][n_x] (may be NULL: not stored), J[B]
 *     min_sep[B], goal_dist[B][k] (either may be NULL): dpilqr_policy_rollout's definitions -- the smallest distance ProximityCost
 *     measures between any two agents over t in [0, T] (planar when every agent has the same n_dims, quirk Q5; +inf for k = 1), and
 *     |x_T - xf| over each agent's first n_dims coordinates.
 * A stage cost is w_prox * (sum over pairs) + w_ref * (sum over agents), accumulated over t, then the terminal cost.  The sums
 * have a fixed shape that depends on k alone (per-thread partial sums, a butterfly per wavefront, the wavefronts in order;
 * csrc/rollout_wide.hpp) and use no floating-point atomics: results are reproducible bit for bit, and agree with
 * dpilqr_rollout's, which sums in the reference's order, to rounding -- not bit for bit.
 * One workgroup per item, one thread per agent for the model step, the k (k - 1) / 2 pair terms of a step dealt over its 256
 * threads.  DPILQR_EUNSUPPORTED before any launch: k > DPILQR_MAX_TEAM (and dpilqr_rollout's own limits on the five-state family).
 * DPILQR_EINVAL: a NULL x0, U or J, a misaligned pointer, a bad descriptor.  fp64 only.  Enqueue only, nothing is allocated. */
int32_t dpilqr_rollout_wide(const dpilqr_batch_desc* desc, const double* x0, const double* U, double* X, double* J,
                            double* min_sep, double* goal_dist, void* stream);

#endif /* DPILQR_SWARM_H */

/*
 * dpilqr_nearest.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * The interaction graph of a distributed solve with every neighbourhood capped at its m nearest agents.  Additive:
 * DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, fp64, row-major, `stream`, error codes): dpilqr_hip.h.
 */
#ifndef DPILQR_NEAREST_H
#define DPILQR_NEAREST_H
#ifndef DPILQR_SWARM_H
#error "include dpilqr_hip.h, which includes this header after dpilqr_swarm.h"
#endif

/* dpilqr_dispatch_graph_wide (dpilqr_swarm.h) with a cap m = max_cluster on the size of a neighbourhood: that entry's arguments, in
 * its order, plus max_cluster behind `ignore` and dropped behind bucket_count.  Opt-in: no other entry changes.
 *
 * Definition.  For scenario s the graph samples rows 0, st, 2 st, ... of X[s] (st = max(N / 10, 1)), as the other graph entries do.
 *     d_r(i, j)  = sqrt(dx*dx + dy*dy) over the planar positions of row r, i != j (no fused multiply-add: dispatch_graph_wide's
 *                  expression and order of operations)
 *     key(i, j)  = min_r d_r(i, j).  A comparison with a NaN is false: a NaN distance is never the minimum, a NaN key never a
 *                  neighbour, as in the other graph entries.
 *     nbr(i)     = {i} + { j : key(i, j) < 2 radius[s] } -- dispatch_graph_wide's neighbourhood exactly (any_r (d_r < thr) <=>
 *                  min_r d_r < thr, the minimum being one of the values)
 *     mask_m(i)  = nbr(i) if |nbr(i)| <= m; otherwise {i} and the m - 1 members j != i of nbr(i) that are smallest under the
 *                  lexicographic order on (key(i, j), j): ties go to the lower agent index
 *     dropped(i) = |nbr(i)| - |mask_m(i)|
 * bits[S][k][n_words] holds mask_m (word w, bit b = agent 64 w + b); dropped[S][k] (int32, may be NULL) the counts, for ignored
 * agents too.  `ignore` keeps its meaning: an ignored agent gets rep = -1, size = 0 and stays a candidate in the other agents'
 * neighbourhoods.  rep, size, order, slot, bucket_start, bucket_count are what dispatch_graph_wide derives from its masks, derived
 * from these by the same kernels.  A capped mask need not be symmetric (j in mask_m(i) does not imply i in mask_m(j)); gather,
 * stitch, stitch_policy[_wide] and the closed-loop entries take masks as they come.
 * Consequences: with m >= max_i |nbr(i)| all seven arrays equal dispatch_graph_wide's bit for bit, and with n_words = 1
 * dispatch_graph's; m = 1 gives every agent its own bit only (k independent single-agent problems); no cluster is larger than m, so
 * with m <= DPILQR_MAX_AGENTS every team the wide entries serve can be planned.
 * Serves 1 <= k <= DPILQR_MAX_TEAM with n_words = ceil(k / 64).  DPILQR_EINVAL before any launch: dispatch_graph_wide's conditions;
 * max_cluster < 1; max_cluster > min(k, DPILQR_MAX_AGENTS) (the message names the value and the bound).  S == 0: bucket_start and
 * bucket_count are zeroed, nothing else is touched.
 * One workgroup of 256 threads per scenario; LDS: the sampled rows' planar positions (at most 19 rows x 256 agents x 2 doubles)
 * plus a 2 KB strip of keys per wavefront, 86,016 B at most (csrc/frontend_nearest.hpp).  Enqueue only, nothing is allocated. */
int32_t dpilqr_dispatch_graph_nearest(int32_t S, int32_t N, int32_t k, int32_t n_s, const double* X, const double* radius,
                                      int64_t radius_stride, const int32_t* ignore, int32_t max_cluster, uint64_t* bits, int32_t* rep,
                                      int32_t* size, int32_t* order, int32_t* slot, int32_t* bucket_start, int32_t* bucket_count,
                                      int32_t* dropped, int32_t n_words, void* stream);

#endif /* DPILQR_NEAREST_H */

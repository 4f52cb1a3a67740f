/*
 * dpilqr_order.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * The solve loop orders its active list by sweep cost where the fused four-state wavefront sweep serves a batch
 * (csrc/admit_order.hpp); these entries run the two steps of that ordering stand-alone, for tests and measurements.
 * Additive: DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, `stream`, error codes): dpilqr_hip.h.
 */
#ifndef DPILQR_ORDER_H
#define DPILQR_ORDER_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

#define DPILQR_ORDER_SPREAD 1  /* rank r -> list position r */
#define DPILQR_ORDER_GROUPED 2 /* consecutive ranks share a sweep workgroup, workgroups in launch order */

/* keys[pos] = the number of steps t in 0..T of trajectory X[items[pos]] ([B][T+1][k*4], four-state agents, planar positions) at
 * which some pair of agents is near by the fused sweep's own criterion, !(dx*dx + dy*dy > r*r*(1 + 1e-12)), r = the item's radius.
 * items / n_items NULL: the batch in index order (keys[B]).  k = 1 has no pairs: every key is 0.
 * DPILQR_EUNSUPPORTED for any family but the four-state one.  Enqueue only. */
int32_t dpilqr_cost_keys(const dpilqr_batch_desc* desc, const double* X, const int32_t* items, const int32_t* n_items, int32_t* keys,
                         void* stream);

/* out <- the *n_items entries of items, sorted by the class of their keys (keys[pos] belongs to items[pos]; at most 64 classes of
 * the count 0..T+1), heaviest first, order within a class arbitrary, rank r stored at dpilqr_order_position(r, ...).  items and out
 * must not overlap.  waves: 4, 8 or 12 wavefronts per sweep workgroup; n_cus >= 1.  Enqueue only, one workgroup. */
int32_t dpilqr_order_list(const int32_t* items, const int32_t* n_items, const int32_t* keys, int32_t T, int32_t n_cus, int32_t waves,
                          int32_t order, int32_t* out, void* stream);

/* Host only: the list position of rank `rank` (0 = heaviest) in a list of n items for a sweep of `waves` wavefronts per workgroup
 * on n_cus compute units; a permutation of 0..n-1 for either order.  DPILQR_EINVAL (negative) for arguments out of range. */
int32_t dpilqr_order_position(int32_t rank, int32_t n, int32_t n_cus, int32_t waves, int32_t order);

#endif /* DPILQR_ORDER_H */

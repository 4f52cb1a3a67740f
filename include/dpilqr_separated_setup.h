/*
 * dpilqr_separated_setup.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * Random scenarios with a minimum separation, on the device: the default branch of the reference's randomize_locs (random=False,
 * rel_dist=; util.py:125-149) applied to start and goal positions that are already drawn, bit for bit NumPy's.
 * Additive: DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, fp64, row-major, `stream`, error codes): dpilqr_hip.h.
 */
#ifndef DPILQR_SEPARATED_SETUP_H
#define DPILQR_SEPARATED_SETUP_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

#define DPILQR_SETUP_SEPARATE_MAX_ITER 4096 /* the largest max_iter */
#define DPILQR_SETUP_SEPARATE_LDS 8232      /* bytes of LDS of a workgroup: one point set, its norms, its centre */

/* x0, xf [S][k * n_s] hold RAW draws: the first n_d states of an agent are its position, var * uniform(-1, 1), as
 * dpilqr_trial_inputs(..., energy = 0, ...) writes them.  The call transforms the position columns in place into what
 *     np.random.seed(seed_s); x0, xf = random_setup(k, n_s, is_rotation=False, rel_dist=rel_dist, var=var, n_d=n_d, random=False,
 *                                                   energy=energy)
 * returns.  randomize_locs draws a set and then pushes it apart without drawing again, starts first, then goals, so the stream of a
 * trial (csrc/trial_inputs.hpp) and the warm starts that follow are those of random=True.  For one set x (k, n_d):
 *     D = 0.1 * k                                  (a double product: 0.1 * 3 is 0.30000000000000004)
 *     repeat:
 *         c      = mean of x over the points, per coordinate (rows added in order, then / k; with n_d = 1 the set is one contiguous
 *                  vector to NumPy, which adds it as its pairwise sum -- the order of the sum of the norms below)
 *         d_ij   = sqrt(dx*dx + dy*dy) over the FIRST TWO coordinates only (n_d = 3 ignores z; n_d = 1 uses its one coordinate)
 *         flag_i = any j != i with d_ij <= rel_dist  (a NaN compares false)
 *         if no flag: stop
 *         every flagged i, once, all from the old x and the same c:  x_i = x_i + D * (x_i - c)   (three roundings, no fused multiply-add)
 * The body runs at least once.  n_iter [S][2] receives the number of rounds of the start set ([s][0]) and of the goal set ([s][1]),
 * the last round, which finds no flag, included: at least 1.  A set that still has a flagged point in round max_iter gets -1 there:
 * its positions stay as they stand after that round's push, and it is not normalised.  Every other set is normalised as
 * dpilqr_trial_inputs normalises (include/dpilqr_swarm_study.h: NumPy's summation orders) when energy != 0 -- with n_d = 1 the
 * centre as above, which is NumPy's; that entry adds in order there and differs from NumPy in the last bits from 9 agents on.
 * Nothing else is written: neither the other columns of x0, xf nor any other row.
 * One workgroup of 256 threads per (scenario, set), grid (S, 2), the set in LDS (DPILQR_SETUP_SEPARATE_LDS bytes, no scratch);
 * thread i owns point i and walks all j != i; the exit of the loop is read by every thread from one LDS word behind a barrier and
 * the trip count is bounded by max_iter (csrc/separated_setup.hpp).
 * DPILQR_EINVAL, with a dpilqr_last_error text, before any launch: S < 0; k outside 2 .. DPILQR_MAX_TEAM (the reference raises for
 * one agent); n_d outside 1 .. 3 or above n_s; max_iter outside 1 .. DPILQR_SETUP_SEPARATE_MAX_ITER; x0, xf or n_iter NULL;
 * rel_dist NaN.  S = 0: DPILQR_OK, nothing is launched.  The call only enqueues; nothing is allocated. */
int32_t dpilqr_setup_separate(int32_t S, int32_t k, int32_t n_s, int32_t n_d, double rel_dist, double energy, int32_t max_iter,
                              double* x0, double* xf, int32_t* n_iter, void* stream);

#endif /* DPILQR_SEPARATED_SETUP_H */

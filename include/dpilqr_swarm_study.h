/*
 * dpilqr_swarm_study.h -- extension of the C ABI of libdpilqr_hip.so (dpilqr_hip.h, which includes this file: include that one).
 * The INPUTS of the Monte-Carlo study for teams of up to DPILQR_MAX_TEAM agents, drawn on the device: start and goal positions and
 * the warm starts of the two receding-horizon loops of a trial, bit for bit NumPy's.
 * Additive: DPILQR_ABI_VERSION is unchanged.  Conventions (device pointers, fp64, row-major, `stream`, error codes): dpilqr_hip.h.
 */
#ifndef DPILQR_SWARM_STUDY_H
#define DPILQR_SWARM_STUDY_H
#ifndef DPILQR_HIP_H
#error "include dpilqr_hip.h, which includes this header after the types it needs"
#endif

#define DPILQR_TRIAL_INPUTS_LDS 37888 /* bytes of LDS of a workgroup of the generator: two scenarios, a wavefront each */

/* For scenario s = 0 .. S - 1, with seed_s = seeds[s] (seeds: device int64[S]) or seed0 + s (seeds NULL), the outputs of
 *     np.random.seed(seed_s)
 *     x0, xf = random_setup(k, n_s, is_rotation=False, var=var, n_d=n_d, random=True, energy=energy)       (util.py:125-217)
 *     U_a = np.random.rand(N, n_u) * warm_scale                                                             (n_warm >= 1)
 *     U_b = np.random.rand(N, n_u) * warm_scale                                                             (n_warm == 2)
 * bit for bit: x0, xf [S][k * n_s] (the first n_d states of an agent are its position, the rest zero), U_a, U_b [S][N][n_u].
 * That is the draw order of a trial of the study (scripts/analysis.py:45-54, then distributed.py:152 once per branch); with
 * n_warm = 0 it is dpilqr_random_setup for any team of up to DPILQR_MAX_TEAM agents, with which it agrees bit for bit where both
 * serve.  energy = 0: no normalisation.  Otherwise normalize_energy with NumPy's summation orders: the mean of a coordinate is the
 * sum over the agents in order, divided by k; an agent's norm is the sum of its n_d squares in order, then sqrt; the sum of the k
 * norms is NumPy's pairwise sum -- eight running sums for 8 <= k <= 128, and above that sum(a[:n2]) + sum(a[n2:]) with n2 = k / 2
 * less its remainder by 8, applied again to either part (129 -> 64 + 65, 255 -> 120 + (64 + 71), 256 -> 128 + 128).
 * One wavefront per scenario, two per workgroup, the 624-word MT19937 state and the positions in LDS (DPILQR_TRIAL_INPUTS_LDS
 * bytes, no scratch); a scenario takes ceil((2 k n_d + n_warm N n_u) / 312) twists, each in three lane-parallel phases
 * (csrc/trial_inputs.hpp).  Rows s of the outputs are written by scenario s's lanes only and nothing else is written.
 * DPILQR_EINVAL, with a dpilqr_last_error text, before any launch: S < 0; k outside 1 .. DPILQR_MAX_TEAM; n_d outside 1 .. 3 or
 * above n_s; n_warm outside 0 .. 2; N < 1 or n_u < 1 with n_warm > 0; x0 or xf NULL, U_a NULL with n_warm >= 1, U_b NULL with
 * n_warm = 2 (outputs that n_warm does not require may be NULL and are not touched); a seed outside [0, 2^32).  S = 0: DPILQR_OK,
 * nothing is launched.  With seeds NULL the call only enqueues.  With seeds given it first copies them to the host and waits for
 * `stream`, to check their range: not for use under stream capture.  Nothing is allocated on the device. */
int32_t dpilqr_trial_inputs(int32_t S, int64_t seed0, const int64_t* seeds, int32_t k, int32_t n_s, int32_t n_d, double var,
                            double energy, int32_t n_warm, int32_t N, int32_t n_u, double warm_scale, double* x0, double* xf,
                            double* U_a, double* U_b, void* stream);

#endif /* DPILQR_SWARM_STUDY_H */

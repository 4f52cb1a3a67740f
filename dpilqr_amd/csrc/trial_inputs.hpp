// trial_inputs.hpp -- what one trial of the Monte-Carlo study draws (analysis.trial_inputs: scripts/analysis.py:45-54, then
// distributed.py:152), for S trials of any team of 1 .. 256 agents at once and bit for bit as NumPy draws it:
//   np.random.seed(seed_s)
//   x0, xf = random_setup(k, n_s, is_rotation=False, var=var, n_d=n_d, random=True, energy=energy)      (util.py:125-217)
//   U_a = np.random.rand(N, n_u) * warm_scale;  U_b likewise, from the same stream
// NumPy's legacy global generator is MT19937 seeded by init_genrand; a double is made of two consecutive 32-bit outputs.  The
// stream of one trial, counted in DOUBLES: [0, k n_d) the start positions in C order, [k n_d, 2 k n_d) the goal positions, then
// n_warm blocks of N n_u warm-start values.  Double d is made of outputs 2 d and 2 d + 1, that is of pair d % 312 of twist d / 312:
// 624 is even, so a pair never straddles a twist.
//
// k_random_setup (frontend.hpp) keeps a scenario's 624-word state and its positions in ONE thread's private memory, which is what
// stops it at 64 agents and makes a warm start (25,600 doubles at k = 256, N = 50: 83 twists) out of the question.  Here a
// WAVEFRONT owns a scenario and the state lives in LDS:
//   twist      three phases whose words do not depend on each other: i < 227 reads old words only (i, i + 1, i + 397), 227 <= i <
//              454 reads old i, i + 1 and the NEW i - 227 of the first phase, 454 <= i < 624 old i, i + 1 (new word 0 for i = 623)
//              and the new i - 227 of the second.  Inside a phase every lane reads all its operands before any lane writes.
//   tempering  and the pairing into doubles: a lane per pair, 312 pairs per twist; warm-start doubles go straight to global
//              memory (consecutive lanes, consecutive addresses), positions stay in LDS until they are normalised.
//   energy     normalize_energy with NumPy's summation orders (below): the centre a lane per coordinate, the norms a lane per
//              agent, the sum of the norms one lane per point set.
// Everything that DEFINES the bits -- the phase bounds, a word of the twist, the tempering, the pairing, the stream layout, the
// three summation orders -- is plain C++ for host and device: tests/trial_inputs_check.cpp compiles it without HIP, emulates the
// lanes (per phase: read all, then write all) and is held to the fixture the GPU tests use.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef DPILQR_HD
#if defined(__HIPCC__)
#define DPILQR_HD __host__ __device__
#else
#define DPILQR_HD
#endif
#endif

namespace dpilqr {

constexpr int kMtWords = 624, kMtShift = 397, kMtPairs = kMtWords / 2;
constexpr int kTrialMaxAgents = 256;      // DPILQR_MAX_TEAM
constexpr int kTrialMaxDims = 3;

// ---- MT19937 (numpy/random/src/mt19937: init_genrand, mt19937_gen, the tempering of mt19937_next)
DPILQR_HD inline uint32_t mt_seed_next(uint32_t prev, int i) { return 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i; }

// the three phases of a twist: words [mt_phase_lo(p), mt_phase_hi(p)), p = 0, 1, 2
DPILQR_HD constexpr int mt_phase_lo(int p) { return p == 0 ? 0 : p == 1 ? kMtWords - kMtShift : 2 * (kMtWords - kMtShift); }
DPILQR_HD constexpr int mt_phase_hi(int p) { return p == 0 ? kMtWords - kMtShift : p == 1 ? 2 * (kMtWords - kMtShift) : kMtWords; }

// word i of the twisted state, from the state as it stands when i's phase begins (the earlier phases written, this one not)
DPILQR_HD inline uint32_t mt_twist_word(const uint32_t* mt, int i) {
    const int nxt = i + 1 == kMtWords ? 0 : i + 1;
    const int far = i + kMtShift >= kMtWords ? i + kMtShift - kMtWords : i + kMtShift;
    const uint32_t y = (mt[i] & 0x80000000u) | (mt[nxt] & 0x7fffffffu);
    return mt[far] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

DPILQR_HD inline uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
    return y;
}

// pair j of a twisted state -> a double of [0, 1) (random_standard_uniform of the legacy generator)
DPILQR_HD inline double mt_pair_double(const uint32_t* mt, int j) {
    const uint32_t a = mt_temper(mt[2 * j]) >> 5, b = mt_temper(mt[2 * j + 1]) >> 6;
    return (a * 67108864.0 + b) / 9007199254740992.0;
}

// ---- the layout of a trial's stream, in doubles
DPILQR_HD inline int64_t trial_setup_doubles(int k, int n_d) { return 2 * (int64_t)k * n_d; }
DPILQR_HD inline int64_t trial_doubles(int k, int n_d, int n_warm, int N, int n_u) {
    return trial_setup_doubles(k, n_d) + (int64_t)n_warm * N * n_u;
}
DPILQR_HD inline int64_t trial_twists(int k, int n_d, int n_warm, int N, int n_u) {
    return (trial_doubles(k, n_d, n_warm, N, n_u) + kMtPairs - 1) / kMtPairs;
}
// np.random.uniform(-1, 1) scaled by var (util.py:132), and np.random.rand() * warm_scale (distributed.py:152)
DPILQR_HD inline double trial_position(double u, double var) { return var * (-1.0 + 2.0 * u); }
DPILQR_HD inline double trial_warm(double u, double warm_scale) { return u * warm_scale; }

// ---- normalize_energy's sums in NumPy's orders
// the mean of coordinate c over the agents: add.reduce along axis 0 walks the rows in order; np.mean divides the sum by k
DPILQR_HD inline double trial_centre(const double* pos, int k, int n_d, int c) {
    double acc = 0.0;
    for (int a = 0; a < k; ++a) acc += pos[a * n_d + c];
    return acc / k;
}
// np.linalg.norm(axis=1): the squares rounded one by one, added in order, then sqrt
DPILQR_HD inline double trial_norm(const double* p, int n_d) {
    double q = 0.0;
    for (int c = 0; c < n_d; ++c) q += p[c] * p[c];
    return sqrt(q);
}
// pairwise_sum (numpy/core/src/umath/loops_utils.h) of a block of n <= 128: in order below 8, eight running sums from there
DPILQR_HD inline double numpy_block_sum(const double* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}
// ... and above 128: sum(a[:n2]) + sum(a[n2:]) with n2 = n / 2 less its remainder by 8, applied again to either half
DPILQR_HD inline int numpy_split(int n) { const int n2 = n / 2; return n2 - n2 % 8; }
// The recursion written out for n <= kTrialMaxAgents (device code keeps no call stack): the left half has at most 128 terms, the
// right at most 135, whose own halves are blocks (129 -> 64 + 65; 255 -> 120 + (64 + 71); 256 -> 128 + 128).
DPILQR_HD inline double numpy_pairwise_sum_wide(const double* a, int n) {
    if (n <= 128) return numpy_block_sum(a, n);
    const int n2 = numpy_split(n), rest = n - n2;
    const double left = numpy_block_sum(a, n2);
    if (rest <= 128) return left + numpy_block_sum(a + n2, rest);
    const int m2 = numpy_split(rest);
    return left + (numpy_block_sum(a + n2, m2) + numpy_block_sum(a + n2 + m2, rest - m2));
}
static_assert(kTrialMaxAgents <= 256, "numpy_pairwise_sum_wide writes two levels out: a right half of at most 135 terms");

#if defined(__HIPCC__) && defined(DPILQR_TRIAL_INPUTS_KERNELS)   // tu_trial_inputs.hip: no device code crosses a file boundary

constexpr int kTrialWaves = 2;                    // scenarios per workgroup, a wavefront each
constexpr int kTrialThreads = 64 * kTrialWaves;
struct TrialLds {                                 // one scenario's: 18,944 B
    double pos[2 * kTrialMaxAgents * kTrialMaxDims];      // starts, then goals, k n_d each
    double nrm[2 * kTrialMaxAgents];                      // the agents' norms, starts then goals
    double ctr[8];                                        // centres [which * 3 + c], the two scales at 6, 7
    uint32_t mt[kMtWords];
};
constexpr int kTrialLdsBytes = (int)sizeof(TrialLds) * kTrialWaves;
static_assert(kTrialLdsBytes == 37888, "the LDS the header states (include/dpilqr_swarm_study.h)");

// One wavefront per scenario.  A wavefront touches its own TrialLds only and every loop count is a kernel argument, so the
// barriers below are reached by all wavefronts alike; the wavefront past the last scenario computes scenario S - 1 again and
// stores nothing.  Output rows s of x0, xf, U_a, U_b are written by scenario s's lanes only.
__global__ void __launch_bounds__(kTrialThreads) k_trial_inputs(int S, int64_t seed0, const int64_t* __restrict__ seeds, int k, int n_s,
                                                                int n_d, double var, double energy, int n_warm, int N, int n_u,
                                                                double warm_scale, double* __restrict__ x0, double* __restrict__ xf,
                                                                double* __restrict__ U_a, double* __restrict__ U_b) {
    __shared__ TrialLds lds[kTrialWaves];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int s_raw = (int)blockIdx.x * kTrialWaves + wave;
    const bool live = s_raw < S;
    const int s = live ? s_raw : S - 1;
    TrialLds& L = lds[wave];
    if (lane == 0) {
        uint32_t v = (uint32_t)(seeds ? seeds[s] : seed0 + s);
        L.mt[0] = v;
        for (int i = 1; i < kMtWords; ++i) { v = mt_seed_next(v, i); L.mt[i] = v; }
    }
    __syncthreads();
    const int n_pos = k * n_d;
    const int64_t n_setup = trial_setup_doubles(k, n_d), n_row = (int64_t)N * n_u, total = trial_doubles(k, n_d, n_warm, N, n_u);
    for (int64_t base = 0; base < total; base += kMtPairs) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {      // a phase has at most 227 words: four per lane, all read before any is written
            const int hi = mt_phase_hi(p), i0 = mt_phase_lo(p) + lane, i1 = i0 + 64, i2 = i0 + 128, i3 = i0 + 192;
            const uint32_t v0 = i0 < hi ? mt_twist_word(L.mt, i0) : 0u, v1 = i1 < hi ? mt_twist_word(L.mt, i1) : 0u;
            const uint32_t v2 = i2 < hi ? mt_twist_word(L.mt, i2) : 0u, v3 = i3 < hi ? mt_twist_word(L.mt, i3) : 0u;
            __syncthreads();
            if (i0 < hi) L.mt[i0] = v0;
            if (i1 < hi) L.mt[i1] = v1;
            if (i2 < hi) L.mt[i2] = v2;
            if (i3 < hi) L.mt[i3] = v3;
            __syncthreads();
        }
        for (int j = lane; j < kMtPairs; j += 64) {
            const int64_t d = base + j;
            if (d >= total) break;
            const double u = mt_pair_double(L.mt, j);
            if (d < n_setup) L.pos[d] = trial_position(u, var);
            else if (live) {
                const int64_t e = d - n_setup;
                if (e < n_row) U_a[(int64_t)s * n_row + e] = trial_warm(u, warm_scale);
                else U_b[(int64_t)s * n_row + (e - n_row)] = trial_warm(u, warm_scale);
            }
        }
        __syncthreads();
    }
    if (energy != 0.0) {
        if (lane < 2 * n_d) {
            const int which = lane / n_d, c = lane - which * n_d;
            L.ctr[which * 3 + c] = trial_centre(L.pos + which * n_pos, k, n_d, c);
        }
        __syncthreads();
        for (int e = lane; e < 2 * n_pos; e += 64) {
            const int which = e >= n_pos ? 1 : 0, c = (e - which * n_pos) % n_d;
            L.pos[e] -= L.ctr[which * 3 + c];
        }
        __syncthreads();
        for (int a = lane; a < 2 * k; a += 64) L.nrm[a] = trial_norm(L.pos + a * n_d, n_d);
        __syncthreads();
        if (lane < 2) L.ctr[6 + lane] = energy / numpy_pairwise_sum_wide(L.nrm + lane * k, k);
        __syncthreads();
        for (int e = lane; e < 2 * n_pos; e += 64) L.pos[e] *= L.ctr[6 + (e >= n_pos ? 1 : 0)];
        __syncthreads();
    }
    if (!live) return;
    double* o0 = x0 + (int64_t)s * k * n_s;
    double* of = xf + (int64_t)s * k * n_s;
    for (int q = lane; q < k * n_s; q += 64) {
        const int a = q / n_s, c = q - a * n_s;
        o0[q] = c < n_d ? L.pos[a * n_d + c] : 0.0;
        of[q] = c < n_d ? L.pos[n_pos + a * n_d + c] : 0.0;
    }
}

#endif  // DPILQR_TRIAL_INPUTS_KERNELS

}  // namespace dpilqr

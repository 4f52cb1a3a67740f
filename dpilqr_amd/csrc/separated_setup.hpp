// separated_setup.hpp -- the default branch of the reference's randomize_locs (util.py:125-149: random=False, rel_dist=) on point
// sets that are already drawn, for S scenarios of 2 .. 256 agents at once and bit for bit as NumPy computes it.  random_setup calls
// randomize_locs twice, starts then goals; the loop below draws nothing, so the stream layout of trial_inputs.hpp is untouched
// and the raw draws are dpilqr_trial_inputs' with energy 0.  For one set x (k, n_d):
//   D = 0.1 * k
//   repeat:  c = mean of x per coordinate (rows in order, / k: trial_centre; NumPy's pairwise sum if n_d = 1: sep_centre)
//            d_ij = sqrt(dx dx + dy dy) over the FIRST TWO coordinates (compute_pairwise_distance's default n_d = 2; one if n_d = 1)
//            flag_i = any j != i with d_ij <= rel_dist                      (a NaN compares false)
//            no flag: stop.  Every flagged i, once, from the old x and the same c:  x_i = x_i + D * (x_i - c)
// The body runs at least once.  The reference's fancy-indexed += writes a point of several close pairs several times with the same
// value, so "once" is exact.  Afterwards normalize_energy in k_trial_inputs' orders (the centre by sep_centre), when energy != 0.
//
// A kernel of its own: k_trial_inputs runs two scenarios per workgroup, a wavefront each, behind shared barriers whose count is a
// kernel argument; a trip count that depends on the data would leave one wavefront waiting at a barrier the other never reaches.
// Here a workgroup of 256 threads owns one (scenario, set); thread i owns point i and walks all j != i (d_ij is symmetric bit for
// bit: neither the squares nor their sum depend on the sign of dx), so there is no pair-index decode and no atomic.  Every thread
// reads the workgroup's one flag word after a barrier: the loop's exit is uniform, its trip count is bounded by max_iter, and no
// barrier sits under a condition that differs between threads.
// Everything that DEFINES the bits is plain C++ for host and device; tests/separated_setup_check.cpp compiles it without HIP,
// emulates the threads (per phase: all read, then all write) and is held to the fixture the GPU tests use.
#pragma once
#include "trial_inputs.hpp"      // trial_centre, trial_norm, numpy_pairwise_sum_wide, kTrialMaxAgents, kTrialMaxDims

namespace dpilqr {

constexpr int kSepThreads = 256;          // a thread per point
constexpr int kSepMinAgents = 2;          // one agent raises in the reference (compute_pairwise_distance)
constexpr int kSepMaxIter = 4096;
static_assert(kSepThreads >= kTrialMaxAgents, "thread i owns point i");

// the step away from the centre, as a fraction of the offset: the double product 0.1 * k (0.1 * 3 is 0.30000000000000004)
DPILQR_HD inline double sep_push(int k) { return 0.1 * k; }
// numpy_pairwise_sum_wide's value with its at most three blocks -- [0, n2), [n2, n2 + m2), [n2 + m2, n) -- walked by ONE loop, so
// that a call site holds one copy of numpy_block_sum and not three: with three at each of the kernel's two sites the compiler
// spills scalar registers.  tests/separated_setup_check.cpp holds it to numpy_pairwise_sum_wide for every n of 1 .. 256.
DPILQR_HD inline double sep_pairwise_sum(const double* a, int n) {
    const int n2 = n <= 128 ? n : numpy_split(n);
    const int rest = n - n2, m2 = rest <= 128 ? rest : numpy_split(rest);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int lo = 0;
    for (int b = 0; b < 3 && lo < n; ++b) {
        const int len = b == 0 ? n2 : b == 1 ? m2 : rest - m2;
        const double v = numpy_block_sum(a + lo, len);
        if (b == 0) s0 = v; else if (b == 1) s1 = v; else s2 = v;
        lo += len;
    }
    return rest == 0 ? s0 : m2 == rest ? s0 + s1 : s0 + (s1 + s2);
}
// np.mean(x, axis=0) of a (k, n_d) set: the rows added in order (trial_centre) -- but a set of ONE coordinate is a contiguous vector
// to NumPy, which adds it as its pairwise sum (the same below 8 terms, eight running sums from there)
DPILQR_HD inline double sep_centre(const double* pos, int k, int n_d, int c) {
    return n_d == 1 ? sep_pairwise_sum(pos, k) / k : trial_centre(pos, k, n_d, c);
}
// the coordinates a distance looks at: compute_pairwise_distance is called with its default n_d = 2, whatever the points have
DPILQR_HD inline int sep_dist_dims(int n_d) { return n_d < 2 ? n_d : 2; }
// np.linalg.norm(dX, axis=0): the squares rounded one by one, added in order, then sqrt
DPILQR_HD inline double sep_distance(const double* a, const double* b, int n_dist) {
    double q = 0.0;
    for (int c = 0; c < n_dist; ++c) {
        const double d = a[c] - b[c];
        q += d * d;
    }
    return sqrt(q);
}
DPILQR_HD inline bool sep_close(double d, double rel_dist) { return d <= rel_dist; }
// whether point i has any other point within rel_dist: pos is the set, (k, n_d) in C order
DPILQR_HD inline bool sep_flag(const double* pos, int k, int n_d, int i, double rel_dist) {
    const int n_dist = sep_dist_dims(n_d);
    bool flag = false;
    for (int j = 0; j < k; ++j)
        if (j != i && sep_close(sep_distance(pos + i * n_d, pos + j * n_d, n_dist), rel_dist)) flag = true;
    return flag;
}
// x += D * (x - c): three separately rounded operations (the unit is compiled with -ffp-contract=off)
DPILQR_HD inline double sep_pushed(double x, double c, double push) {
    const double off = x - c;
    const double step = push * off;
    return x + step;
}

#if defined(__HIPCC__) && defined(DPILQR_SEPARATED_SETUP_KERNELS)   // tu_separated_setup.hip: no device code crosses a file boundary

struct SepLds {                                    // 8,232 B
    double pos[kTrialMaxAgents * kTrialMaxDims];
    double nrm[kTrialMaxAgents];
    double ctr[4];                                 // the centre per coordinate, the scale at 3
    int any;
};

// One workgroup per (scenario, set): blockIdx.x the scenario, blockIdx.y 0 the starts (x0), 1 the goals (xf).  Thread i < k owns
// point i; the threads from k on own nothing, raise no flag and take every barrier.  `any` is cleared by thread 0 before the
// round's first barrier, raised between the first and the second, read by all between the second and the third.
__global__ void __launch_bounds__(kSepThreads) k_setup_separate(int k, int n_s, int n_d, double rel_dist, double energy, int max_iter,
                                                                double* __restrict__ x0, double* __restrict__ xf,
                                                                int32_t* __restrict__ n_iter) {
    __shared__ SepLds L;
    const int tid = (int)threadIdx.x, s = (int)blockIdx.x, which = (int)blockIdx.y;
    double* row = (which ? xf : x0) + (int64_t)s * k * n_s;
    const int n_pos = k * n_d;
    const bool mine = tid < k;
    if (mine)
        for (int c = 0; c < n_d; ++c) L.pos[tid * n_d + c] = row[tid * n_s + c];
    const double push = sep_push(k);
    int rounds = -1;
    for (int it = 0; it < max_iter; ++it) {
        __syncthreads();      // the positions of the load or of the last round are written; `any` of the last round is read
        if (tid == 0) L.any = 0;
        if (tid < n_d) L.ctr[tid] = sep_centre(L.pos, k, n_d, tid);
        __syncthreads();
        const bool flag = mine && sep_flag(L.pos, k, n_d, tid, rel_dist);
        if (flag) L.any = 1;
        __syncthreads();
        if (!L.any) { rounds = it + 1; break; }      // one word, read by all after the barrier: uniform
        if (flag)
            for (int c = 0; c < n_d; ++c) L.pos[tid * n_d + c] = sep_pushed(L.pos[tid * n_d + c], L.ctr[c], push);
    }
    __syncthreads();
    // normalize_energy, the orders of k_trial_inputs; `rounds` is uniform.  Its centre is the mean of the positions as they stand,
    // which the last round -- the one that found no flag and moved nothing -- has left in ctr
    if (rounds > 0 && energy != 0.0) {
        for (int e = tid; e < n_pos; e += kSepThreads) L.pos[e] -= L.ctr[e % n_d];
        __syncthreads();
        if (mine) L.nrm[tid] = trial_norm(L.pos + tid * n_d, n_d);
        __syncthreads();
        if (tid == 0) L.ctr[3] = energy / sep_pairwise_sum(L.nrm, k);
        __syncthreads();
        for (int e = tid; e < n_pos; e += kSepThreads) L.pos[e] *= L.ctr[3];
        __syncthreads();
    }
    if (mine)
        for (int c = 0; c < n_d; ++c) row[tid * n_s + c] = L.pos[tid * n_d + c];
    if (tid == 0) n_iter[2 * s + which] = rounds;
}

#endif  // DPILQR_SEPARATED_SETUP_KERNELS

}  // namespace dpilqr

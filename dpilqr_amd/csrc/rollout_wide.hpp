// rollout_wide.hpp -- ilqrSolver._rollout (control.py:80-93) for a FULL team of up to 256 agents: J_full of a distributed solve,
// the stitched controls rolled out on the whole problem (distributed.py:100-101), where every sub-problem is small but the team
// is not.  dpilqr_rollout's definition (forward.hpp) with min_sep / goal_dist as dpilqr_policy_rollout defines them (policy.hpp);
// the step and the cost terms are the device functions those kernels share: integrate_rt, ref_cost, pair_cost, pair_dist2.
//
// Launch: one workgroup of 256 threads per item.
//   model step   thread a < k is agent a: it keeps x_a in registers, reads u_a[t] from global memory, evaluates its reference
//                cost and steps.  Its position (the first three coordinates) goes to LDS once per
//                step, by parity.
//   pair terms   the k (k - 1) / 2 pairs of a step -- 32,640 at k = 256 -- are dealt over ALL the threads: thread tid is
//                (group g = tid / k, agent a = tid % k) and takes the pairs (a, a + dd mod k) for dd = 1 + g, 1 + g + G, ... up to
//                k / 2, G = floor(256 / k) groups (at even k the offset k / 2 pairs each couple once: only a < k / 2 takes it).
//                Every pair is evaluated as (lower, higher) agent.
//   reduction    a thread adds its pair terms in ascending dd; the 64 partial sums of a wavefront are combined by a five-level
//                butterfly of lane exchanges (every lane ends with the same value), the four wavefronts' sums are added in
//                wavefront order by thread 0: stage cost = w_prox * pairs + w_ref * agents, accumulated over t, then the terminal
//                cost.  The shape depends on k alone, never on the launch, and no floating-point atomic is involved: the result
//                is the same bits run after run.  (It is not dpilqr_rollout's summation order: the two agree to rounding.)
// One barrier per step: at the top of step t the agents publish x_t in the buffers of parity t & 1 and step; behind the barrier
// everyone evaluates the pairs of x_t, and thread 0 folds the wavefront sums of step t - 1 (parity (t - 1) & 1) into J.  A buffer
// written in step t was last read in step t - 2, and the barrier of step t - 1 lies in between.
#pragma once
#include <hip/hip_runtime.h>

#include "policy.hpp"      // pair_dist2; cost.hpp, lds_sync.hpp, models.hpp

namespace dpilqr {

constexpr int kRolloutWideAgents = 256;
constexpr int kRolloutWideThreads = 256;

// the sum / the minimum over a wavefront, in every lane: xor-butterfly over 1, 2, 4, 8, 16, 32
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_min64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}

// X [B][T+1][n_x] (may be null); J [B]; min_sep [B], goal_dist [B][k] (may be null)
template <int NS, int NC>
__global__ __launch_bounds__(kRolloutWideThreads) void k_rollout_wide(dpilqr_batch_desc D, const double* __restrict__ x0,
        const double* __restrict__ U, double* __restrict__ X, double* __restrict__ J_out, double* __restrict__ min_sep,
        double* __restrict__ goal_dist) {
    constexpr int nth = kRolloutWideThreads, nwv = nth / 64;
    constexpr int PD = 3;      // coordinates a pair can ask for (n_dims <= 3 <= NS)
    __shared__ double s_pos[2][kRolloutWideAgents * 3];      // agent a's position at a * 3: an odd stride
    __shared__ double s_prox[2][nwv], s_ref[2][nwv], s_sep[nwv];
    __shared__ int32_t s_nd[kRolloutWideAgents];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC;
    const ItemParams P = item_params(D, b);
    const bool agent = tid < k;
    const int a = agent ? tid : 0;
    // the pairs this thread takes
    const int G = nth / k, g = tid / k, pa = tid - g * k;
    const bool pairing = g < G;
    const int half = k / 2;

    const int nd_own = P.n_dims[a];
    if (agent) s_nd[tid] = nd_own;
    const bool homog = __syncthreads_and(!agent || nd_own == P.n_dims[0]) != 0;      // (also orders s_nd)
    const double dtr = D.dt, radius = P.radius, w_prox = D.w_prox, w_ref = D.w_ref;
    const int model = P.model[a];
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;
    const double* Qfa = P.Qf + a * NS * NS;
    const double* Ub = U + (int64_t)b * T * m + a * NC;
    double* Xw = (X && agent) ? X + (int64_t)b * (T + 1) * n + a * NS : nullptr;

    double x[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = agent ? x0[(int64_t)b * n + a * NS + i] : 0.0;

    double J = 0.0, sep2 = __builtin_huge_val();
    // this thread's pairs at the positions of parity p; the reference cost `rc` of its agent rides along: both are reduced over the
    // wavefront and left for thread 0 in the wavefront sums of parity p
    auto stage_terms = [&](int p, double rc) {
        const double* sp = s_pos[p];
        double ps = 0.0;
        if (pairing)
            for (int dd = 1 + g; dd <= half; dd += G) {
                if (2 * dd == k && pa >= dd) break;
                const int o = pa + dd < k ? pa + dd : pa + dd - k;
                const int l = pa < o ? pa : o, h = pa < o ? o : pa;
                const int nd = homog ? 2 : min(min(s_nd[l], s_nd[h]), PD);
                sep2 = fmin(sep2, pair_dist2(sp + l * 3, sp + h * 3, nd));
                ps += pair_cost(sp + l * 3, sp + h * 3, nd, radius);
            }
        ps = wave_sum64(ps);
        rc = wave_sum64(rc);
        if (lane == 0) { s_prox[p][wave] = ps; s_ref[p][wave] = rc; }
    };
    auto fold = [&](int p) {      // thread 0: J += the stage cost whose wavefront sums lie at parity p
        double prox = 0.0, ref = 0.0;
#pragma unroll
        for (int w = 0; w < nwv; ++w) { prox += s_prox[p][w]; ref += s_ref[p][w]; }
        J += w_prox * prox + w_ref * ref;
    };

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        double rc = 0.0;
        if (agent) {
            double ut[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) ut[c] = Ub[(int64_t)t * m + c];
#pragma unroll
            for (int i = 0; i < PD; ++i) s_pos[par][a * 3 + i] = x[i];
            if (Xw) {
#pragma unroll
                for (int i = 0; i < NS; ++i) Xw[(int64_t)t * n + i] = x[i];
            }
            double xn[NS];
            integrate_rt<NS>(model, x, ut, dtr, xn);
            // the reference cost of (x_t, u_t) BEHIND the step: in front of it, its n_s * n_s + n_c * n_c weights (160 loads at twelve
            // states) are fetched early and held across the model step, whose own peak they then push into scratch -- 132 spilled
            // registers at twelve states, none this way round
            rc = ref_cost<NS, NC>(x, ut, xf, Qa, Ra, false);
#pragma unroll
            for (int i = 0; i < NS; ++i) x[i] = xn[i];
        }
        __syncthreads();
        if (tid == 0 && t > 0) fold(par ^ 1);
        stage_terms(par, rc);
    }
    // x_T: the terminal cost cost(x_T, 0, terminal=True) (control.py:91); its pairs count for min_sep too
    const int par = T & 1;
    double rc = 0.0;
    if (agent) {
#pragma unroll
        for (int i = 0; i < PD; ++i) s_pos[par][a * 3 + i] = x[i];
        if (Xw) {
#pragma unroll
            for (int i = 0; i < NS; ++i) Xw[(int64_t)T * n + i] = x[i];
        }
        double uz[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) uz[c] = 0.0;
        rc = ref_cost<NS, NC>(x, uz, xf, Qfa, Ra, true);
    }
    __syncthreads();
    if (tid == 0) fold(par ^ 1);      // of step T - 1 (T >= 1)
    stage_terms(par, rc);
    sep2 = wave_min64(sep2);
    if (lane == 0) s_sep[wave] = sep2;
    __syncthreads();
    if (tid == 0) {
        fold(par);
        J_out[b] = J;
        if (min_sep) {
            double mn2 = __builtin_huge_val();      // no pair (k = 1): +inf
#pragma unroll
            for (int w = 0; w < nwv; ++w) mn2 = fmin(mn2, s_sep[w]);
            min_sep[b] = sqrt(mn2);
        }
    }
    if (goal_dist && agent) goal_dist[(int64_t)b * k + a] = sqrt(pair_dist2(x, xf, min(nd_own, NS)));
}

}  // namespace dpilqr

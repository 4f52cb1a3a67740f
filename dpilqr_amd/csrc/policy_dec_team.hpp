// policy_dec_team.hpp -- the closed loop of a DISTRIBUTED solution for a whole TEAM: up to 64 agents behind one mask word
// (NW = 1, dpilqr_policy_rollout_dec_team), up to 256 behind ceil(k / 64) words (NW = 4, dpilqr_policy_rollout_dec_wide).
// dpilqr_policy_rollout_dec's definition (include/dpilqr_policy.h, policy_dec.hpp), unchanged,
//     u_i(t) = U_ff_i[t] + Kc_i[t] (x_{C_i}(t) - X_dec[t]_{C_i})   [clamped to u_lim]      x_{t+1} = step(x_t, u_t)   [+ W[t]]
// where the full problem is beyond any centralised kernel (n_x = 256 at 64 double integrators) but the per-agent work is still
// n_c x kc_i n_s multiply-adds per step.  The step, the cost terms and the product are the device functions the other rollouts
// share: integrate_rt, ref_cost, pair_cost, pair_dist2, policy_block -- X and U agree with k_policy_rollout_dec bit for bit where
// both serve a shape (same product order, same step), goal_dist too; J and min_sep to rounding (the sums below have their own shape).
//
// Launch: 256 threads, thread tid = (sample sl = tid / k, agent a = tid % k), as policy.hpp deals them.  A workgroup holds
// G = floor(256 / k) samples of ONE item; an item's samples take ceil(S / G) consecutive workgroups, the grid is items x chunks.
// Lanes past the last sample take part in the barriers and in nothing else.  A thread keeps x_a in registers.
//   gains       the K[t] image is NEVER staged: k n_c kw doubles (262 KB at k = kc_max = 64) do not fit LDS, and an agent needs
//               only its own n_c rows of it.  Lane (sl, a) walks the set bits of ITS 64-bit mask, lowest first, and reads block p
//               (its p-th member) of its own compact rows Kc[b][t][a] straight from global memory: NS consecutive doubles per
//               row.  The samples of a workgroup read the same words (one item); neighbouring agents' rows are n_c kw doubles
//               apart, so one wavefront-wide load touches up to 64 cache lines -- and that, not the round trip, is what a step
//               costs at large neighbourhoods: requesting four blocks' operands ahead of their use (and X[t + 1], U_ff[t + 1] a
//               step ahead) left a one-item launch of 64 full neighbourhoods at 2.27 ms and, at 257 registers against 179,
//               made 32 items slower (4.68 against 3.48 ms): that variant was not kept (profiles/policy_dec_team.txt).
//               Only the lowest kc_max members among the low k bits are kept when the mask is read, so no address
//               depends on a mask's value beyond row a of the Kc[b][t] image and the sample's own dx row.
//   NW          the kernel is ONE text over the number of mask words a lane keeps, a template parameter: bits [B][k][n_words],
//               n_words = ceil(k / 64) <= NW, word w, bit b = agent 64 w + b (frontend_wide.hpp).  A neighbourhood still has at
//               most kc_max <= 64 members (a sub-problem's limit), so an agent's work per step is what it is in a team of 64 --
//               only the pairs grow, up to 128 per thread and step at k = 256, and G = floor(256 / k) falls to 3 samples per
//               workgroup at k = 65 .. 85, 2 at 86 .. 128, 1 above.  Lane (sl, a) reads its n_words words once and keeps, word
//               by word and lowest bit first, only the lowest kc_max members among the low k bits: NW truncated words in
//               registers (words at and past n_words are zero).  Each step walks them in that order; block p of the agent's
//               compact rows belongs to its p-th member (p < kc_max, member < k).  At NW = 1 the read is the single-word form
//               under `if constexpr`, the walk's word loop has one trip, and the instantiation keeps the instructions,
//               registers and LDS of the one-word kernel this header used to hold (profiles/policy_dec_words_refactor.txt);
//               with n_words = 1 and k <= 64 the NW = 4 instantiation gives all five results bit for bit (same device
//               functions, same order).
//   exchange    each step a thread publishes dx_a = x_a - X[t]_a (stride NS | 1, odd) and its position (three coordinates) in
//               LDS.  SINGLE buffers behind a second barrier instead of policy.hpp's parities: two parities of 256 x 13 doubles
//               plus the positions pass 64 KB at twelve states, and a barrier is small change beside a step's gain reads.
//               Barrier B at the top of a step (everyone has read step t - 1's exchange), publish, barrier A, then the product,
//               the pairs, the model step.
//   pair terms  the k (k - 1) / 2 pairs of a sample are dealt over that sample's k threads as forward.hpp deals them: thread a
//               takes (a, a + dd mod k) for dd = 1 .. k / 2 (at even k the offset k / 2 by a < k / 2 only), each evaluated as (lower,
//               higher), and adds its pair costs in ascending dd.
//   reduction   thread (sl, a) leaves  w_prox * (its pair costs) + w_ref * (its reference cost)  in the sample's row of LDS; the
//               sample's lane a = 0 adds the k terms in agent order (between the next step's barriers B and A) into J.  The shape
//               depends on k alone -- not on S, the chunk, the item's place in the batch or the sample's place in the workgroup --
//               and there is no floating-point atomic and NO wavefront-wide operation: samples straddle wavefronts whenever k
//               does not divide 64.  min_sep: every thread keeps the smallest squared distance of its own pairs, lane a = 0 takes
//               the minimum of the sample's k values at the end.
// Static LDS: 256 (NS | 1) + 256 x 3 + 256 doubles and 64 NW ints (n_dims) -- 35 KB at twelve states and NW = 1, 36 KB at NW = 4.
#pragma once
#include <hip/hip_runtime.h>

#include "policy.hpp"      // pair_dist2, policy_block; cost.hpp, lds_sync.hpp, models.hpp

namespace dpilqr {

constexpr int kPolicyTeamThreads = 256;
constexpr int kPolicyTeamAgents = 64;      // one mask word
constexpr int kPolicyWideWords = 4;
constexpr int kPolicyWideAgents = 64 * kPolicyWideWords;     // one thread per agent of a sample
constexpr int kPolicyWideMembers = 64;     // a neighbourhood is a sub-problem: at most 64 agents

// X [B][T+1][n_x]: X_dec; U [B][T][n_u]: U_ff; K: Kc [B][T][k][NC][kc_max * NS]; bits [B][k][n_words]
// Xs [B][S][T+1][n_x], Us [B][S][T][n_u] (either may be null); J, min_sep [B][S]; goal_dist [B][S][k] (the last two may be null)
template <int NS, int NC, int NW>
__global__ __launch_bounds__(kPolicyTeamThreads) void k_policy_rollout_dec_team(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int kc_max, const unsigned long long* __restrict__ bits,
        int n_words, int S, int chunks, const double* __restrict__ x0s, const double* __restrict__ W,
        const double* __restrict__ u_lim, double* __restrict__ Xs, double* __restrict__ Us, double* __restrict__ J_out,
        double* __restrict__ min_sep, double* __restrict__ goal_dist) {
    constexpr int nth = kPolicyTeamThreads, AS = NS | 1;
    constexpr int PD = 3;      // coordinates a pair can ask for (n_dims <= 3 <= NS)
    __shared__ double s_dx[nth * AS];       // lane tid's dx at tid * AS
    __shared__ double s_pos[nth * PD];      // lane tid's position at tid * 3: an odd stride
    __shared__ double s_term[nth];          // lane tid's share of its sample's stage cost
    __shared__ int32_t s_nd[64 * NW];
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - b * chunks;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC, kw = kc_max * NS;
    const int G = nth / k, sl = tid / k, a = tid - sl * k;
    const int s = chunk * G + sl;
    const bool active = sl < G && s < S;      // a lane past the last sample: the barriers only
    const ItemParams P = item_params(D, b);

    if (tid < k) s_nd[tid] = P.n_dims[tid];
    const bool homog = __syncthreads_and(tid >= k || P.n_dims[tid] == P.n_dims[0]) != 0;      // (also orders s_nd)
    const double dtr = D.dt, radius = P.radius, w_prox = D.w_prox, w_ref = D.w_ref;
    const int model = P.model[a];
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;
    const double* Qfa = P.Qf + a * NS * NS;

    const double* Xb = X + (int64_t)b * (T + 1) * n + a * NS;
    const double* Ub = U + (int64_t)b * T * m + a * NC;
    const double* Kb = K + (int64_t)b * T * m * kw + (int64_t)a * NC * kw;      // this agent's compact rows
    const int64_t smp = (int64_t)b * S + (active ? s : 0);
    const double* Wp = W ? W + smp * T * n + a * NS : nullptr;
    double* Xw = (Xs && active) ? Xs + smp * (T + 1) * n + a * NS : nullptr;
    double* Uw = (Us && active) ? Us + smp * T * m + a * NC : nullptr;
    const bool clamp = u_lim != nullptr, noisy = W != nullptr;      // uniform: no per-lane pointer test inside the loop

    // the mask, read once per lane: only its lowest kc_max members among the low k bits are kept, counted across the words
    unsigned long long mask[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) mask[w] = 0ull;
    double x[NS];
    if (active) {
        if constexpr (NW == 1) {
            unsigned long long rem = bits[(int64_t)b * k + a];
            if (k < 64) rem &= (1ull << k) - 1ull;
            for (int p = 0; p < kc_max && rem != 0ull; ++p, rem &= rem - 1ull) mask[0] |= rem & (0ull - rem);
        } else {
            int left = kc_max;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int hi = k - 64 * w;      // bits of this word below k
                unsigned long long rem = (w < n_words && hi > 0) ? bits[((int64_t)b * k + a) * n_words + w] : 0ull;
                if (hi < 64) rem &= (1ull << (hi > 0 ? hi : 0)) - 1ull;
                for (; left > 0 && rem != 0ull; --left, rem &= rem - 1ull) mask[w] |= rem & (0ull - rem);
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            x[i] = x0s[smp * n + a * NS + i];
            if (Xw) Xw[i] = x[i];
        }
    }

    const double* dxs = s_dx + sl * k * AS;     // the sample's rows (read only by its active lanes)
    const double* poss = s_pos + sl * k * PD;
    const double* terms = s_term + sl * k;
    double J = 0.0, sep2 = __builtin_huge_val();
    // this agent's share of the sample's pairs at the published positions, added in ascending dd; the smallest squared distance is kept
    auto pairs = [&]() {
        double ps = 0.0;
        for (int dd = 1; 2 * dd <= k; ++dd) {
            if (2 * dd == k && a >= dd) break;
            const int o = a + dd < k ? a + dd : a + dd - k;
            const int l = a < o ? a : o, h = a < o ? o : a;
            const int nd = homog ? 2 : min(min(s_nd[l], s_nd[h]), PD);
            sep2 = fmin(sep2, pair_dist2(poss + l * PD, poss + h * PD, nd));
            ps += pair_cost(poss + l * PD, poss + h * PD, nd, radius);
        }
        return ps;
    };

    for (int t = 0; t < T; ++t) {
        __syncthreads();      // B: step t - 1's exchange and stage-cost terms are read / written
        if (active) {
#pragma unroll
            for (int i = 0; i < NS; ++i) s_dx[tid * AS + i] = x[i] - Xb[(int64_t)t * n + i];      // dx = x_t - X[t]
#pragma unroll
            for (int i = 0; i < PD; ++i) s_pos[tid * PD + i] = x[i];
            if (a == 0 && t > 0) J += sum_in_order(terms, k);      // the stage cost of step t - 1
        }
        __syncthreads();      // A
        if (active) {
            double sum[NC], ut[NC];      // Kc_a[t] dx over the neighbourhood, this agent's NC rows
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = 0.0;
            const double* krow = Kb + (int64_t)t * m * kw;
            int pos = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w)      // word by word, lowest bit first: the members in ascending order
                for (unsigned long long rem = mask[w]; rem != 0ull; rem &= rem - 1ull, ++pos)
                    policy_block<NS, NC>(sum, krow, dxs, pos, 64 * w + __ffsll(rem) - 1, 1, kw, AS);      // (rs = 1, row stride kw: global memory)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = Ub[(int64_t)t * m + c] + sum[c];
                if (clamp) {
                    const double lo = u_lim[a * NC + c], hi = u_lim[m + a * NC + c];
                    v = v < lo ? lo : (v > hi ? hi : v);     // a NaN stays a NaN
                }
                ut[c] = v;
                if (Uw) Uw[(int64_t)t * m + c] = v;
            }
            const double ps = pairs();
            double xn[NS];
            integrate_rt<NS>(model, x, ut, dtr, xn);
            // the reference cost of (x_t, u_t) BEHIND the step, as rollout_wide.hpp has it: its weights are not held across the model step
            s_term[tid] = w_prox * ps + w_ref * ref_cost<NS, NC>(x, ut, xf, Qa, Ra, false);
#pragma unroll
            for (int i = 0; i < NS; ++i) x[i] = noisy ? xn[i] + Wp[(int64_t)t * n + i] : xn[i];
            if (Xw) {
#pragma unroll
                for (int i = 0; i < NS; ++i) Xw[(int64_t)(t + 1) * n + i] = x[i];
            }
        }
    }
    // x_T: the last stage cost, then the terminal cost cost(x_T, 0, terminal=True) (control.py:91); its pairs count for min_sep too
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < PD; ++i) s_pos[tid * PD + i] = x[i];
        if (a == 0) J += sum_in_order(terms, k);      // of step T - 1 (T >= 1)
    }
    __syncthreads();
    if (active) {
        double uz[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) uz[c] = 0.0;
        const double ps = pairs();
        s_term[tid] = w_prox * ps + w_ref * ref_cost<NS, NC>(x, uz, xf, Qfa, Ra, true);
        s_dx[tid] = sep2;      // (the exchange is done with: the sample's smallest squared distances, lane tid's at tid)
    }
    __syncthreads();
    if (active) {
        if (a == 0) {
            J += sum_in_order(terms, k);
            J_out[smp] = J;
            if (min_sep) {
                double mn2 = __builtin_huge_val();      // no pair (k = 1): +inf
                for (int i = 0; i < k; ++i) mn2 = fmin(mn2, s_dx[sl * k + i]);
                min_sep[smp] = sqrt(mn2);
            }
        }
        if (goal_dist) goal_dist[smp * k + a] = sqrt(pair_dist2(x, xf, min(P.n_dims[a], NS)));
    }
}

}  // namespace dpilqr

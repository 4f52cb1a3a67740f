// policy_advance_dec_team.hpp -- the step between two solves of a receding-horizon loop under a DISTRIBUTED solution's policy, for a
// whole TEAM at any n_x -- up to 64 agents behind one mask word (NW = 1, dpilqr_policy_advance_dec_team), up to 256 behind
// ceil(k / 64) words (NW = 4, dpilqr_policy_advance_dec_wide): dpilqr_policy_advance_dec's semantics (include/dpilqr_policy.h,
// policy_advance.hpp), statement for statement, with k_policy_rollout_dec_team's arithmetic (policy_dec_team.hpp):
//     u_i = clamp( U_ff[j][i] + Kc_i[j][i] (x_{C_i} - X[j][i]_{C_i}) )      x <- step(x, u_i)   [+ W[s][g + i]]
// The step, the cost terms and the product are the shared device functions -- policy_block, integrate_rt, ref_cost, pair_cost,
// pair_dist2, sum_in_order are called, not restated -- so the executed prefix equals k_policy_rollout_dec_team's bit for bit, and
// X_exec, U_exec, x_cur, n_done, dist_left, U_next, X_next equal k_policy_advance_dec's where both serve a shape; J_exec and
// min_sep agree with it to rounding (a stage cost is summed agent by agent here, as the team rollout sums it).
//
// Why not k_policy_advance_dec: its mask is a 32-bit word, and AdvanceLds keeps two parities of k (k - 1) / 2 pair costs per item
// (129 KB at k = 64 with four items per workgroup, before the exchange buffers).  Why not k_policy_rollout_dec_team: there a
// workgroup holds samples of ONE item; here every scenario has its own plan, gains, masks and parameters.
//
// Launch: 256 threads, thread tid = (item slot tid / k, agent a = tid % k); a workgroup holds ipw = floor(256 / k) ITEMS (12 at
// k = 21, 7 at k = 33, 4 at k = 64), the grid is ceil(B / ipw).  Lanes without an item -- past ipw * k, past the last item, an item
// whose scen entry is out of range or whose n_done lies outside 0 .. L -- take part in the barriers and the cooperative shift,
// and in nothing else.  A thread keeps x_a in registers.
//   gains       never staged: lane (slot, a) walks the set bits of ITS 64-bit mask, lowest first, and reads block p (its p-th
//               member) of its own compact rows Kc[j][i][a] straight from global memory.  Unlike the rollout no two slots of a
//               workgroup share a gain: a wavefront-wide load touches up to 64 cache lines, all of them used once.  Only the
//               lowest kc_max members among the low k bits are kept when the mask is read, so no address depends on a mask's
//               value beyond row a of the item's own Kc[j][i] image and the item's own dx rows.  Kc == nullptr: the masks are
//               not read, the sum is zero.
//   NW          ONE text over the number of mask words a lane keeps, as in policy_dec_team.hpp: bits [B][k][n_words], n_words =
//               ceil(k / 64) <= NW, word w, bit b = agent 64 w + b.  Lane (slot, a) reads its n_words words once and keeps, word
//               by word and lowest bit first, only the lowest kc_max <= 64 members among the low k bits (words at and past
//               n_words are zero); each step walks the words in that order, block p of the lane's compact rows belongs to its
//               p-th member (p < kc_max, member < k).  An agent's work per step is what it is in a team of 64 -- only the pairs
//               grow, up to 128 per lane and step at k = 256, and ipw falls to 3 items per workgroup at k = 65 .. 85, 2 at
//               86 .. 128, 1 above.  At NW = 1 the read is the single-word form under `if constexpr` and the instantiation
//               keeps the instructions, registers and LDS of the one-word kernel this header used to hold; with n_words = 1
//               and k <= 64 the NW = 4 instantiation gives all nine state fields bit for bit
//               (profiles/policy_dec_words_refactor.txt).
//               The NW truncated words are held in REGISTERS, as the rollout holds them.  At (12, 4) and NW = 1 the kernel
//               sits near the register budget of a 256-thread workgroup (512 per lane), so for NW = 4 the alternative -- the
//               words in LDS, lane tid's word w at w * 256 + tid, 8 KB more -- was built too and both code objects were read
//               (scripts/kernel_resources.py; profiles/policy_advance_dec_wide_checks.txt has the table): in registers the
//               twelve-state instantiation takes 360 + 104 registers, 0 spilled, no scratch, 41984 B LDS; in LDS 352 + 96 and
//               50176 B.  Neither form spills in any family, so the registers are kept and the LDS is the same at both NW.
//   exchange    SINGLE buffers behind two barriers per step (policy_dec_team.hpp): dx at stride NS | 1, positions at stride 3.
//               Every loop whose trip count feeds a barrier runs to the uniform h: an item near its capacity executes he < h
//               steps and its lanes idle through the rest.
//   stage cost  lane (slot, a) leaves  w_prox * (its pair costs, ascending partner offset) + w_ref * (its reference cost, behind
//               the model step)  in the item's row; the item's lane a = 0 adds the k terms with sum_in_order and makes ONE
//               addition to J_exec per executed step, in time order.  No floating-point atomics and NO wavefront-wide operation
//               on an item's data: items straddle wavefronts whenever k does not divide 64.
//   n_dims      whether the n_dims are homogeneous (quirk Q5: planar distances) is a property of the ITEM: every lane publishes
//               its agent's n_dims and each lane decides from its own item's k entries.
//   min_sep     every lane keeps the smallest squared distance of its own pairs over the states 0 .. he, lane a = 0 takes the
//               minimum of the item's k at the end.  The per-lane value and the item's executed cost are kept in LDS words that
//               only their own lane touches, not in registers: held across the twelve-state model step beside the rollout's
//               per-lane state (and he, and the second set of output pointers) they were the two values the compiler spilled;
//               with them in LDS every instantiation keeps its registers (0 spilled, no scratch).
//   shift       policy_advance.hpp's cooperative copy: item after item of the workgroup, consecutive lanes on consecutive words,
//               the source index clamped, U_next zero beyond the plan.  U_next / X_next must not alias the plan.
// Static LDS: 256 (NS | 1) + 256 x 3 + 3 x 256 doubles (stage-cost terms, separations, executed costs), 256 ints (n_dims) and
// 2 x 256 ints (he, scenario per slot; ipw = 256 at k = 1): 41 KB at twelve states (41984 B), 21 KB at three (21504 B) -- the
// team rollout's 35 KB plus the advance's bookkeeping, at either NW.  At 256 + 98 registers per lane (NW = 1; 360 + 104 at NW = 4)
// one workgroup is resident per CU, so LDS does not bound the occupancy.
#pragma once
#include <hip/hip_runtime.h>

#include "policy_dec_team.hpp"      // kPolicyTeamThreads, kPolicyTeamAgents, kPolicyWide*; policy.hpp: pair_dist2, policy_block

namespace dpilqr {

// X [B][T+1][n_x]: X_dec; U [B][T][n_u]: U_ff; K: Kc [B][T][k][NC][kc_max * NS] or null (open loop); bits [B][k][n_words]
// the loop's state, by scenario (include/dpilqr_policy.h, dpilqr_policy_advance)
template <int NS, int NC, int NW>
__global__ __launch_bounds__(kPolicyTeamThreads) void k_policy_advance_dec_team(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int kc_max, const unsigned long long* __restrict__ bits,
        int n_words, int h, const int* __restrict__ scen, int n_scen, int L, int n_d, const double* __restrict__ W,
        const double* __restrict__ u_lim, double* __restrict__ x_cur, int* __restrict__ n_done, double* __restrict__ X_exec,
        double* __restrict__ U_exec, double* __restrict__ J_exec, double* __restrict__ min_sep, double* __restrict__ dist_left,
        double* __restrict__ U_next, double* __restrict__ X_next) {
    constexpr int nth = kPolicyTeamThreads, AS = NS | 1;
    constexpr int PD = 3;      // coordinates a pair can ask for (n_dims <= 3 <= NS)
    __shared__ double s_dx[nth * AS];       // lane tid's dx at tid * AS
    __shared__ double s_pos[nth * PD];      // lane tid's position at tid * 3: an odd stride
    __shared__ double s_term[nth];          // lane tid's share of its item's stage cost
    __shared__ int32_t s_nd[nth];           // lane tid's n_dims
    __shared__ double s_sep[nth];           // lane tid's smallest squared pair distance so far: that lane alone reads and writes it
    __shared__ double s_J[nth];             // slot q's executed cost at q: lane a = 0 alone reads and writes it
    __shared__ int32_t s_slot[2 * nth];     // (he or -1, scenario) per slot, for the shift
    const int tid = (int)threadIdx.x;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC, kw = kc_max * NS;
    const int ipw = nth / k, slot = tid / k, a = tid - slot * k;
    const int64_t j0 = (int64_t)blockIdx.x * ipw;
    bool active = slot < ipw && j0 + slot < D.B;      // a lane without an item: the barriers and the cooperative copy only
    const int j = active ? (int)(j0 + slot) : 0;
    int s = 0, g = 0;
    if (active) {
        s = scen ? scen[j] : j;
        active = s >= 0 && s < n_scen;
        s = active ? s : 0;
        g = n_done[s];
        active = active && g >= 0 && g <= L;
        g = active ? g : 0;
    }
    const int he = active ? min(h, L - g) : 0;      // never past the capacity
    const ItemParams P = item_params(D, j);

    s_nd[tid] = P.n_dims[a];
    if (slot < ipw && a == 0) {
        s_slot[2 * slot] = active ? he : -1;
        s_slot[2 * slot + 1] = s;
    }
    __syncthreads();
    bool homog = true;      // of THIS item: its own k entries (slot < ipw: below ipw * k <= nth)
    if (active)
        for (int i = 1; i < k; ++i) homog = homog && s_nd[slot * k + i] == s_nd[slot * k];
    const int32_t* nds = s_nd + slot * k;

    const double dtr = D.dt, radius = P.radius, w_prox = D.w_prox, w_ref = D.w_ref;
    const int model = P.model[a];
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;

    const bool gains = K != nullptr, clamp = u_lim != nullptr, noisy = W != nullptr;      // uniform: no per-lane pointer test inside the loop
    const double* Xj = X + (int64_t)j * (T + 1) * n + a * NS;
    const double* Uj = U + (int64_t)j * T * m + a * NC;
    const double* Kj = gains ? K + (int64_t)j * T * m * kw + (int64_t)a * NC * kw : nullptr;      // this agent's compact rows
    const double* Wp = noisy ? W + ((int64_t)s * L + g) * n + a * NS : nullptr;
    double* Xe = X_exec + ((int64_t)s * (L + 1) + g) * n + a * NS;
    double* Ue = U_exec + ((int64_t)s * L + g) * m + a * NC;

    // the mask, read once per lane: only its lowest kc_max members among the low k bits are kept, counted across the words
    unsigned long long mask[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) mask[w] = 0ull;
    double x[NS];
    if (active) {
        if (gains) {
            if constexpr (NW == 1) {
                unsigned long long rem = bits[(int64_t)j * k + a];
                if (k < 64) rem &= (1ull << k) - 1ull;
                for (int p = 0; p < kc_max && rem != 0ull; ++p, rem &= rem - 1ull) mask[0] |= rem & (0ull - rem);
            } else {
                int left = kc_max;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int hi = k - 64 * w;      // bits of this word below k
                    unsigned long long rem = (w < n_words && hi > 0) ? bits[((int64_t)j * k + a) * n_words + w] : 0ull;
                    if (hi < 64) rem &= (1ull << (hi > 0 ? hi : 0)) - 1ull;
                    for (; left > 0 && rem != 0ull; --left, rem &= rem - 1ull) mask[w] |= rem & (0ull - rem);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = x_cur[(int64_t)s * n + a * NS + i];
    }

    const double* dxs = s_dx + slot * k * AS;     // the item's rows (read only by its active lanes)
    const double* poss = s_pos + slot * k * PD;
    const double* terms = s_term + slot * k;
    // (the executed cost and the smallest squared distance live in LDS, not in registers of every lane: held across the
    // twelve-state step they are what the register file cannot take -- the compiler moved them to spill slots)
    if (active && a == 0) s_J[slot] = J_exec[s];
    s_sep[tid] = __builtin_huge_val();
    // this agent's share of the item's pairs at the published positions, added in ascending dd; the smallest squared distance is kept
    auto pairs = [&]() {
        double ps = 0.0, sep2 = s_sep[tid];
        for (int dd = 1; 2 * dd <= k; ++dd) {
            if (2 * dd == k && a >= dd) break;
            const int o = a + dd < k ? a + dd : a + dd - k;
            const int l = a < o ? a : o, hh = a < o ? o : a;
            const int nd = homog ? 2 : min(min(nds[l], nds[hh]), PD);
            sep2 = fmin(sep2, pair_dist2(poss + l * PD, poss + hh * PD, nd));
            ps += pair_cost(poss + l * PD, poss + hh * PD, nd, radius);
        }
        s_sep[tid] = sep2;
        return ps;
    };

    for (int i = 0; i < h; ++i) {      // to the uniform h: the barriers
        const bool run = i < he;      // (he = 0 without an item)
        __syncthreads();      // B: step i - 1's exchange and stage-cost terms are read / written
        if (run) {
#pragma unroll
            for (int q = 0; q < NS; ++q) s_dx[tid * AS + q] = x[q] - Xj[(int64_t)i * n + q];      // dx = x - X[i]
#pragma unroll
            for (int q = 0; q < PD; ++q) s_pos[tid * PD + q] = x[q];
        }
        if (a == 0 && i > 0 && i <= he) s_J[slot] = s_J[slot] + sum_in_order(terms, k);      // the stage cost of step i - 1: ONE addition
        __syncthreads();      // A
        if (run) {
            double sum[NC], ut[NC];      // Kc_a[i] dx over the neighbourhood, this agent's NC rows
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = 0.0;
            const double* krow = Kj + (int64_t)i * m * kw;
            int pos = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w)      // word by word, lowest bit first: the members in ascending order
                for (unsigned long long rem = mask[w]; rem != 0ull; rem &= rem - 1ull, ++pos)
                    policy_block<NS, NC>(sum, krow, dxs, pos, 64 * w + __ffsll(rem) - 1, 1, kw, AS);      // (rs = 1, row stride kw: global memory)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = Uj[(int64_t)i * m + c] + sum[c];
                if (clamp) {
                    const double lo = u_lim[a * NC + c], hi = u_lim[m + a * NC + c];
                    v = v < lo ? lo : (v > hi ? hi : v);     // a NaN stays a NaN
                }
                ut[c] = v;
                Ue[(int64_t)i * m + c] = v;
            }
#pragma unroll
            for (int q = 0; q < NS; ++q) Xe[(int64_t)i * n + q] = x[q];
            const double ps = pairs();
            double xn[NS];
            integrate_rt<NS>(model, x, ut, dtr, xn);
            // the reference cost of (x, u) BEHIND the step, as the team rollout has it
            s_term[tid] = w_prox * ps + w_ref * ref_cost<NS, NC>(x, ut, xf, Qa, Ra, false);
#pragma unroll
            for (int q = 0; q < NS; ++q) x[q] = noisy ? xn[q] + Wp[(int64_t)i * n + q] : xn[q];
        }
    }
    // the state the plant ends in: it counts for the separation; the last stage cost where the loop has not added it
    __syncthreads();
    if (active) {
#pragma unroll
        for (int q = 0; q < PD; ++q) s_pos[tid * PD + q] = x[q];
        if (a == 0 && he == h) s_J[slot] = s_J[slot] + sum_in_order(terms, k);      // of step h - 1 (h >= 1)
    }
    __syncthreads();
    if (active) {
        pairs();      // leaves the lane's smallest squared distance over the states 0 .. he in s_sep[tid]
    }
    __syncthreads();
    if (active) {
        const int64_t sc = s_slot[2 * slot + 1];      // the scenario, from its slot: not held in a register across the steps
        if (a == 0) {
            const int gc = n_done[sc];      // (read again for the same reason; nobody else writes it)
            J_exec[sc] = s_J[slot];
            double mn2 = __builtin_huge_val();      // no pair (k = 1): +inf
            for (int q = 0; q < k; ++q) mn2 = fmin(mn2, s_sep[slot * k + q]);
            const double sep = sqrt(mn2);
            min_sep[sc] = gc == 0 ? sep : fmin(min_sep[sc], sep);      // the first round's start state opens the record
            n_done[sc] = gc + he;
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            Xe[(int64_t)he * n + q] = x[q];
            x_cur[sc * n + a * NS + q] = x[q];
            X_next[sc * (T + 1) * n + a * NS + q] = x[q];
        }
        dist_left[sc * k + a] = sqrt(pair_dist2(x, xf, n_d));
    }
    // the warm start of the next round: U_next[t] = U[t + he] (0 beyond the plan), X_next[t] = X[min(t + he, T)] for t >= 1
    const int TM = T * m, TN = T * n;
    for (int q = 0; q < ipw; ++q) {
        const int heq = s_slot[2 * q];      // uniform over the workgroup
        if (heq < 0) continue;
        const int64_t sq = s_slot[2 * q + 1], jq = j0 + q;
        const double* Uq = U + jq * TM;
        double* Un = U_next + sq * TM;
        for (int e = tid; e < TM; e += nth) {
            const int src = e + heq * m;
            const double v = Uq[src < TM ? src : TM - 1];
            Un[e] = src < TM ? v : 0.0;
        }
        const double* Xq = X + jq * (TN + n);
        double* Xn = X_next + sq * (TN + n) + n;
        for (int e = tid; e < TN; e += nth) {
            const int src = e + n + heq * n;
            Xn[e] = Xq[src < TN + n ? src : TN + (e - (e / n) * n)];
        }
    }
}

}  // namespace dpilqr

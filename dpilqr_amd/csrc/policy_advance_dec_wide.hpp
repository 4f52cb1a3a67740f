// policy_advance_dec_wide.hpp -- the step between two solves of a receding-horizon loop under a DISTRIBUTED solution's policy, for a
// whole team of up to 256 agents: policy_advance_dec_team.hpp's semantics, launch shape, exchange, pair deal, reduction and shift,
// statement for statement, over the multi-word neighbourhood masks of policy_dec_wide.hpp
//     u_i = clamp( U_ff[j][i] + Kc_i[j][i] (x_{C_i} - X[j][i]_{C_i}) )      x <- step(x, u_i)   [+ W[s][g + i]]
// nbr_bits[B][k][n_words], n_words = ceil(k / 64): word w, bit b = agent 64 w + b.  A neighbourhood still has at most kc_max <= 64
// members, so an agent's work per step is what it is in a team of 64 -- only the pairs grow, k / 2 per thread.  The body of
// k_policy_advance_dec_team is RESTATED here, not shared: that kernel and k_policy_rollout_dec_wide keep their code objects,
// registers and LDS (as policy_dec_wide.hpp and policy_advance_large.hpp restate theirs).  The device functions are the ones the
// team advance calls, in its order -- policy_block, integrate_rt, ref_cost, pair_cost, pair_dist2, sum_in_order -- so the executed
// prefix equals k_policy_rollout_dec_wide's bit for bit, and with n_words = 1 and k <= 64 all nine state fields equal
// k_policy_advance_dec_team's bit for bit.
//
// What differs from policy_advance_dec_team.hpp:
//   masks       lane (slot, a) reads its n_words words once and keeps, word by word and lowest bit first, only the lowest kc_max
//               members among the low k bits (words at and past n_words are zero).  Each step walks the words in that order;
//               block p of the lane's compact rows belongs to its p-th member.  No address depends on a mask beyond row a of the
//               item's own Kc[j][i] image (p < kc_max) and the item's own dx rows (member < k).  Kc == nullptr: the masks are not
//               read, the sum is zero.
//               The kPolicyWideWords truncated words are held in REGISTERS, as policy_dec_wide.hpp holds them.  The team advance
//               at (12, 4) sits near the register budget of a 256-thread workgroup (512 per lane), so the alternative -- the
//               words in LDS, lane tid's word w at w * 256 + tid, 8 KB more -- was built too and both code objects were read
//               (scripts/kernel_resources.py; profiles/policy_advance_dec_wide_checks.txt has the table): in registers the
//               twelve-state instantiation takes 360 + 104 registers, 0 spilled, no scratch, 41984 B LDS; in LDS 352 + 96 and
//               50176 B.  Neither form spills in any family, so the registers are kept and the LDS stays the team advance's.
//   items       ipw = floor(256 / k): 3 items per workgroup at k = 65 .. 85, 2 at 86 .. 128, 1 above (256 at k = 1, as there).
//   pairs       lane a takes (a, a + dd mod k) for dd = 1 .. k / 2: up to 128 pairs per lane and step at k = 256.
// Every loop that feeds a barrier runs to the uniform h.  The stage cost is the k per-agent terms added in agent order by the
// item's lane a = 0: no floating-point atomics, no wavefront-wide operation on an item's data (items straddle wavefronts).
// Static LDS: the team advance's 256 (NS | 1) + 256 x 3 + 3 x 256 doubles and 256 + 2 x 256 ints: 41 KB at twelve states
// (41984 B), 21 KB at three (21504 B).
#pragma once
#include <hip/hip_runtime.h>

#include "policy_dec_wide.hpp"      // kPolicyWideThreads, kPolicyWideAgents, kPolicyWideWords; policy.hpp: pair_dist2, policy_block

namespace dpilqr {

// X [B][T+1][n_x]: X_dec; U [B][T][n_u]: U_ff; K: Kc [B][T][k][NC][kc_max * NS] or null (open loop); bits [B][k][n_words]
// the loop's state, by scenario (include/dpilqr_policy.h, dpilqr_policy_advance)
template <int NS, int NC>
__global__ __launch_bounds__(kPolicyWideThreads) void k_policy_advance_dec_wide(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int kc_max, const unsigned long long* __restrict__ bits,
        int n_words, int h, const int* __restrict__ scen, int n_scen, int L, int n_d, const double* __restrict__ W,
        const double* __restrict__ u_lim, double* __restrict__ x_cur, int* __restrict__ n_done, double* __restrict__ X_exec,
        double* __restrict__ U_exec, double* __restrict__ J_exec, double* __restrict__ min_sep, double* __restrict__ dist_left,
        double* __restrict__ U_next, double* __restrict__ X_next) {
    constexpr int nth = kPolicyWideThreads, AS = NS | 1, NW = kPolicyWideWords;
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
            int left = kc_max;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int hi = k - 64 * w;      // bits of this word below k
                unsigned long long rem = (w < n_words && hi > 0) ? bits[((int64_t)j * k + a) * n_words + w] : 0ull;
                if (hi < 64) rem &= (1ull << (hi > 0 ? hi : 0)) - 1ull;
                for (; left > 0 && rem != 0ull; --left, rem &= rem - 1ull) mask[w] |= rem & (0ull - rem);
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = x_cur[(int64_t)s * n + a * NS + i];
    }

    const double* dxs = s_dx + slot * k * AS;     // the item's rows (read only by its active lanes)
    const double* poss = s_pos + slot * k * PD;
    const double* terms = s_term + slot * k;
    // (the executed cost and the smallest squared distance live in LDS, not in registers of every lane: held across the
    // twelve-state step they are what the register file cannot take)
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

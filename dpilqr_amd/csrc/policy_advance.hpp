// policy_advance.hpp -- the step between two solves of a receding-horizon loop: every running scenario executes h steps of ITS OWN
// current plan on the plant,
//     u_i = U[j][i] + K[j][i] (x - X[j][i])   [clamped to u_lim]      x <- step(x, u_i)   [+ W[s][g + i]]
// from the scenario's plant state, and the loop's bookkeeping is done in the same launch: the executed states, controls and
// cost are appended to the scenario's buffers at its own offset g = n_done[s], the smallest separation and the distance left
// to the goal are kept, and the plan is shifted into the warm start of the next round (include/dpilqr_policy.h,
// dpilqr_policy_advance, states the semantics).  Not a reference function: the reference's loop (scripts/experiment.py,
// distributed.py:106-221) has an ideal plant.  The step, the cost, the separation and the K dx product are policy.hpp's,
// statement for statement -- policy_block, pair_dist2, pair_cost, ref_cost, sum_in_order, integrate_rt are called, not restated --
// so the executed prefix equals k_policy_rollout's bit for bit.
//
// Why not k_policy_rollout: there one workgroup holds floor(256 / k) SAMPLES of one item, which share K[t], X[t], U[t]; here every
// scenario has its own plan, one sample per item.  Launch: 256 threads, thread tid = (item slot tid / k, agent a = tid % k); a
// workgroup holds ipw = floor(256 / k) ITEMS, the grid is ceil(B / ipw).  Lanes that hold no item (past ipw * k, past the last
// item, or an item whose scen entry is out of range) take part in the barriers and the cooperative copies, and in nothing else.
//
// K[i] is read from global memory by the lane that uses it and is NOT staged through LDS: no two lanes of different items share
// a gain, and ipw images do not fit (twenty CarDynamics3D agents: 40 x 60 x 8 B = 19.2 KB per item and step, times 12 items).
// Lane (item, a) reads its NC rows; a row is n_x (dense) or kc_max * n_s (compact) contiguous doubles, the item's lanes cover
// the image's rows once: every byte of an item's K[i] is fetched once.  What that read pattern costs against a staged copy has
// not been measured.  X[i], U[i], W are read by the lane that uses them too.  No load is guarded per element: an inactive lane
// skips the step as a whole, the shift clamps its source index.
//
// One barrier per step.  At the top of step i a lane publishes dx = x - X[i] and x in the exchange buffers of parity i & 1; then
// the barrier; then K[i] dx over the item's dx rows, the reference cost and this agent's share of the pair costs into the
// cost-term buffers of parity i & 1, the stores, the step.  Lane a = 0 adds the stage cost of step i - 1 (parity (i - 1) & 1)
// behind the barrier of step i: J_exec takes ONE addition per step, in time order.  A buffer written in step i was last read in
// step i - 2, and every thread has passed a barrier in between.  An item near its capacity executes he < h steps: its lanes
// idle through the remaining iterations (the barriers are uniform: the loop runs to h).
//
// LDS (doubles; AdvanceLds): dx, x -- lane tid's entries at tid * as, as = n_s | 1 odd (PolicyLds' padding), two parities; per
// item k reference costs and k (k - 1) / 2 pair costs in combinations order, two parities; k squared separations; two ints (he,
// scenario) per slot for the shift.  The largest of every family: twelve-state, k = 5 (51 items): 117.9 KiB; six-state, k = 10
// (25 items): 78.3 KiB; five-state, k = 12 (21 items): 67.1 KiB; four-state, k = 15 (17 items): 73.8 KiB; three-state, k = 20
// (12 items): 63.8 KiB -- all below the 160 KiB of a workgroup.  The whole allocation is zeroed before the first step, a lane reads
// only rows of its own item, which that item's lanes wrote before the barrier in between, and sum_in_order's look-ahead stays
// inside the item's terms: no lane reads a word that neither it nor a thread ordered before it by a barrier has written.
//
// The shift of U and X into U_next / X_next is a cooperative copy by all 256 threads, item after item of the workgroup,
// consecutive lanes on consecutive words.  U_next / X_next must not alias U / X (other workgroups still read them).
#pragma once
#include "policy_dec.hpp"

namespace dpilqr {

struct AdvanceLds {   // offsets in doubles
    int dx, xs, cref, cpair, sep, slots, total;
    int as, ipw, np1;
    __host__ __device__ AdvanceLds(int ns, int k) {
        const int npairs = k * (k - 1) / 2;
        ipw = kPolicyThreads / k;
        as = ns | 1;
        np1 = npairs > 0 ? npairs : 1;
        int o = 0;
        dx = o;    o += 2 * ipw * k * as;
        xs = o;    o += 2 * ipw * k * as;
        cref = o;  o += 2 * ipw * k;
        cpair = o; o += 2 * ipw * np1;
        sep = o;   o += ipw * k;
        slots = o; o += ipw;      // two ints per slot
        total = (o + 1) & ~1;
    }
};
inline size_t advance_lds_bytes(int ns, int k) { return sizeof(double) * (size_t)AdvanceLds(ns, k).total; }

// DEC: K is the compact Kc[B][T][k][NC][kc_max * NS] and `bits` the neighbourhood masks (policy_dec.hpp); otherwise K[B][T][n_u][n_x].
// K == nullptr: the plan is executed open loop.  The pointers are the kernels' __restrict__ parameters.
template <int NS, int NC, bool DEC>
__device__ __forceinline__ void policy_advance_body(const dpilqr_batch_desc& D, const double* X, const double* U, const double* K,
        int kc_max, const unsigned long long* bits, int h, const int* scen, int n_scen, int L, int n_d, const double* W,
        const double* u_lim, double* x_cur, int* n_done, double* X_exec, double* U_exec, double* J_exec, double* min_sep,
        double* dist_left, double* U_next, double* X_next) {
    constexpr int nth = kPolicyThreads;
    const int tid = (int)threadIdx.x;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC, npairs = k * (k - 1) / 2;
    const AdvanceLds O(NS, k);
    const int AS = O.as, rows = O.ipw * k;
    const int slot = tid / k, a = tid - slot * k;
    const int64_t j0 = (int64_t)blockIdx.x * O.ipw;
    bool active = slot < O.ipw && j0 + slot < D.B;      // a lane without an item: the barriers and the cooperative copy only
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
    const bool homog = homogeneous_ndims(P.n_dims, k);
    const double dtr = D.dt, radius = P.radius, w_prox = D.w_prox, w_ref = D.w_ref;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* lds = reinterpret_cast<double*>(lds_raw);
    int* sslot = reinterpret_cast<int*>(lds + O.slots);

    const bool gains = K != nullptr, clamp = u_lim != nullptr, noisy = W != nullptr;      // uniform
    const int cols = DEC ? kc_max * NS : n;      // columns of a row of K[i]
    const int64_t mn = (int64_t)m * cols;
    const double* Xj = X + (int64_t)j * (T + 1) * n + a * NS;
    const double* Uj = U + (int64_t)j * T * m + a * NC;
    const double* Kj = gains ? K + (int64_t)j * T * mn + (int64_t)a * NC * cols : nullptr;      // this agent's NC rows
    const double* Wp = noisy ? W + ((int64_t)s * L + g) * n + a * NS : nullptr;
    double* Xe = X_exec + ((int64_t)s * (L + 1) + g) * n + a * NS;
    double* Ue = U_exec + ((int64_t)s * L + g) * m + a * NC;

    const int model = active ? P.model[a] : 0;
    CompactGains<NS, NC> G(k, DEC ? kc_max : 0, bits);
    if constexpr (DEC) G.setup(tid, j, a, active && gains);      // the mask, its lowest kc_max members (policy_dec.hpp)
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;

    for (int e = tid; e < O.total; e += nth) lds[e] = 0.0;
    lds_handoff(false);
    if (slot < O.ipw && a == 0) {
        sslot[2 * slot] = active ? he : -1;
        sslot[2 * slot + 1] = s;
    }

    double x[NS], lo[NC], hi[NC];
    if (active) {
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = x_cur[(int64_t)s * n + a * NS + i];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            lo[c] = u_lim ? u_lim[a * NC + c] : 0.0;
            hi[c] = u_lim ? u_lim[m + a * NC + c] : 0.0;
        }
    }
    // the dimensions of this agent's pairs, two bits per partner offset (policy.hpp)
    unsigned long long nd_pack = 0ull;
    if (active && !homog)
        for (int dd = 1; 2 * dd <= k; ++dd) {
            const int o = a + dd < k ? a + dd : a + dd - k;
            nd_pack |= (unsigned long long)(min(P.n_dims[a], P.n_dims[o]) & 3) << (2 * dd);
        }

    double J = (active && a == 0) ? J_exec[s] : 0.0, sep2 = __builtin_huge_val();
    // this agent's share of the item's pairs at the positions in `sxs` (policy.hpp); cp == nullptr: the separation only
    auto pairs = [&](const double* sxs, double* cp) {
        for (int dd = 1; 2 * dd <= k; ++dd) {
            if (2 * dd == k && a >= dd) break;
            const int o = a + dd < k ? a + dd : a + dd - k;
            const int l = a < o ? a : o, hh = a < o ? o : a;
            const int nd = homog ? 2 : (int)((nd_pack >> (2 * dd)) & 3ull);
            sep2 = fmin(sep2, pair_dist2(sxs + l * AS, sxs + hh * AS, nd));
            if (cp) cp[pair_index(l, hh, k)] = pair_cost(sxs + l * AS, sxs + hh * AS, nd, radius);
        }
    };
    auto add_stage_cost = [&](int p) {      // J += the stage cost whose terms lie in the buffers of parity p (lane a = 0)
        const double* cr = lds + O.cref + (p * O.ipw + slot) * k;
        const double* cp = lds + O.cpair + (p * O.ipw + slot) * O.np1;
        const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
        J += w_prox * prox + w_ref * ref;
    };

    for (int i = 0; i < h; ++i) {
        const int par = i & 1;
        const bool run = active && i < he;
        double* sdx = lds + O.dx + par * rows * AS;      // the workgroup's; lane tid's entries at tid * AS
        double* sxs = lds + O.xs + par * rows * AS;
        double ut[NC], wt[NS];
        if (run) {
            const double* Xi = Xj + (int64_t)i * n;
            const double* Ui = Uj + (int64_t)i * m;
#pragma unroll
            for (int c = 0; c < NC; ++c) ut[c] = Ui[c];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                sdx[tid * AS + q] = x[q] - Xi[q];       // dx = x - X[i]
                sxs[tid * AS + q] = x[q];
                wt[q] = noisy ? Wp[(int64_t)i * n + q] : 0.0;
            }
        }
        lds_handoff(false);
        if (active && a == 0 && i > 0 && i <= he) add_stage_cost(par ^ 1);      // of step i - 1
        if (run) {
            double sum[NC];      // K[i] dx, this agent's NC rows
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = 0.0;
            if (gains) {
                const double* kp = Kj + (int64_t)i * mn;
                const double* dxs = sdx + slot * k * AS;
                if constexpr (DEC) {
                    int pos = 0;
                    for (unsigned rem = G.mask; rem != 0u; rem &= rem - 1u, ++pos)
                        policy_block<NS, NC>(sum, kp, dxs, pos, __ffs((int)rem) - 1, 1, cols, AS);
                } else {
                    for (int o = 0; o < k; ++o) policy_block<NS, NC>(sum, kp, dxs, o, o, 1, cols, AS);
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = ut[c] + sum[c];
                if (clamp) v = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);     // a NaN stays a NaN
                ut[c] = v;
            }
            lds[O.cref + (par * O.ipw + slot) * k + a] = ref_cost<NS, NC>(x, ut, xf, Qa, Ra, false);
            pairs(sxs + slot * k * AS, lds + O.cpair + (par * O.ipw + slot) * O.np1);
#pragma unroll
            for (int q = 0; q < NS; ++q) Xe[(int64_t)i * n + q] = x[q];
#pragma unroll
            for (int c = 0; c < NC; ++c) Ue[(int64_t)i * m + c] = ut[c];
            double xn[NS];
            integrate_rt<NS>(model, x, ut, dtr, xn);
#pragma unroll
            for (int q = 0; q < NS; ++q) x[q] = noisy ? xn[q] + wt[q] : xn[q];
        }
    }
    // the state the plant ends in: it counts for the separation; the last stage cost where the loop has not added it
    {
        double* sxs = lds + O.xs + (he & 1) * rows * AS;
        if (active) {
#pragma unroll
            for (int q = 0; q < NS; ++q) sxs[tid * AS + q] = x[q];
        }
        lds_handoff(false);
        if (active) {
            if (a == 0 && he == h) add_stage_cost((h - 1) & 1);
            pairs(sxs + slot * k * AS, nullptr);
            lds[O.sep + tid] = sep2;
        }
        lds_handoff(false);
    }
    if (active) {
        if (a == 0) {
            J_exec[s] = J;
            double mn2 = __builtin_huge_val();      // no pair (k = 1): +inf
            for (int q = 0; q < k; ++q) mn2 = fmin(mn2, lds[O.sep + slot * k + q]);
            const double sep = sqrt(mn2);
            min_sep[s] = g == 0 ? sep : fmin(min_sep[s], sep);      // the first round's start state opens the record
            n_done[s] = g + he;
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            Xe[(int64_t)he * n + q] = x[q];
            x_cur[(int64_t)s * n + a * NS + q] = x[q];
            X_next[(int64_t)s * (T + 1) * n + a * NS + q] = x[q];
        }
        dist_left[(int64_t)s * k + a] = sqrt(pair_dist2(x, xf, n_d));
    }
    // the warm start of the next round: U_next[t] = U[t + he] (0 beyond the plan), X_next[t] = X[min(t + he, T)] for t >= 1
    const int TM = T * m, TN = T * n;
    for (int q = 0; q < O.ipw; ++q) {
        const int heq = sslot[2 * q];      // uniform over the workgroup
        if (heq < 0) continue;
        const int64_t sq = sslot[2 * q + 1], jq = j0 + q;
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

template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_advance(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int h, const int* __restrict__ scen, int n_scen, int L, int n_d,
        const double* __restrict__ W, const double* __restrict__ u_lim, double* __restrict__ x_cur, int* __restrict__ n_done,
        double* __restrict__ X_exec, double* __restrict__ U_exec, double* __restrict__ J_exec, double* __restrict__ min_sep,
        double* __restrict__ dist_left, double* __restrict__ U_next, double* __restrict__ X_next) {
    policy_advance_body<NS, NC, false>(D, X, U, K, 0, nullptr, h, scen, n_scen, L, n_d, W, u_lim, x_cur, n_done, X_exec, U_exec, J_exec,
                                       min_sep, dist_left, U_next, X_next);
}

template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_advance_dec(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int kc_max, const unsigned long long* __restrict__ bits, int h,
        const int* __restrict__ scen, int n_scen, int L, int n_d, const double* __restrict__ W, const double* __restrict__ u_lim,
        double* __restrict__ x_cur, int* __restrict__ n_done, double* __restrict__ X_exec, double* __restrict__ U_exec,
        double* __restrict__ J_exec, double* __restrict__ min_sep, double* __restrict__ dist_left, double* __restrict__ U_next,
        double* __restrict__ X_next) {      // X: X_dec, U: U_ff, K: Kc
    policy_advance_body<NS, NC, true>(D, X, U, K, kc_max, bits, h, scen, n_scen, L, n_d, W, u_lim, x_cur, n_done, X_exec, U_exec, J_exec,
                                      min_sep, dist_left, U_next, X_next);
}

}  // namespace dpilqr

// policy_dec.hpp -- the closed loop of a DISTRIBUTED solution: every agent runs the feedback law of its own sub-problem,
//     u_i(t) = U_ff_i[t] + Kc_i[t] (x_{C_i}(t) - X_dec[t]_{C_i})   [clamped to u_lim]
// where C_i is agent i's neighbourhood (a bit mask, bit i set, not necessarily symmetric), Kc_i its n_c rows of the gains of
// the sub-problem solved for C_i, the columns C_i's members in ascending order, and U_ff the sub-problem's own nominal folded
// onto the stitched trajectory (frontend.hpp, k_stitch_policy).  Step, disturbance, cost, min_sep and goal_dist are those of the
// FULL k-agent problem: the kernel is policy.hpp's k_policy_rollout -- its launch, its one barrier per step, its cooperative copy a
// step ahead, its cost and separation code, statement for statement -- except for:
//
//   K[t] image  Kc[b][t] is [k][NC][kw] in global memory, kw = kc_max * NS columns: k NC kw doubles per step against n_u n_x.
//             The copy's element e is (row e / kw, column e % kw); a thread stages ceil(k NC kw / 256) <= kPolicyDecStage of
//             them and issues no load past the image.  In LDS column j lies at j * rs, row a * NC + c of it at
//             c * k + a, rs = n_u | 1 -- policy.hpp's K[t] layout with kw columns.
//   product   Lane (sample, a) walks the set bits of ITS mask, lowest first (so in ascending agent order; only the lowest kc_max
//             are kept when the mask is read): iteration p handles its p-th member o_a.  The lanes of a wavefront advance in lock step on p, not on the
//             agent: a lane with fewer than p + 1 members has left the loop.
//             K reads: block p of the lane's own compact row, word (p * NS + i) * rs + c * k + a -- whatever the masks are,
//             the agents of a sample read consecutive words and the samples of a wavefront (one item, so the same masks) the
//             same ones: at most k <= 20 distinct, consecutive addresses per read, as in policy.hpp.
//             dx reads: word (sl * k + o_a) * as + i of the exchange buffer.  o_a differs per lane, so this is no broadcast: up
//             to k distinct words per sample (all masks full: one; all alone: each lane the entry it published).  as = NS | 1 is
//             odd, so two words share a bank exactly where their indices sl * k + o differ by a multiple of 32; the indices a
//             32-lane group reads lie within the samples it spans, fewer than 64 consecutive ones: at most two-way.  Not
//             measured with counters.
//   columns past kc_a * NS of a row are copied but never read: the product loop ends with the mask's last bit.
//   X, U      X_dec, U_ff in policy.hpp's X[t], U[t] layouts.
// LDS: policy.hpp's PolicyLds(NS, NC, k) as it is -- the K[t] buffers are sized for n_x columns and hold kw <= n_x of them at
// stride kw * rs; zeroed before the first step.  A mask with more than kc_max bits (the caller's contract forbids it) loses its
// members past the kc_max-th: the product never indexes past the K[t] image, and no address at all depends on a mask's value
// beyond that.
#pragma once
#include "policy.hpp"

namespace dpilqr {

// Kc[t] elements a thread copies per step: k NC kw <= (60 / NS) NC 60 within the served shapes (n_x <= 60, kw <= n_x) -- ten for the
// three-state family (policy.hpp's kPolicyStage), five for the twelve-state one, whose step needs the registers
template <int NS, int NC>
constexpr int kPolicyDecStage = ((60 / NS) * NC * 60 + kPolicyThreads - 1) / kPolicyThreads;

// Xs [B][S][T+1][n_x], Us [B][S][T][n_u] (either may be null); J, min_sep [B][S]; goal_dist [B][S][k] (the last two may be null)
template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_rollout_dec(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int kc_max, const unsigned long long* __restrict__ bits,
        int S, int chunks, const double* __restrict__ x0s, const double* __restrict__ W, const double* __restrict__ u_lim,
        double* __restrict__ Xs, double* __restrict__ Us, double* __restrict__ J_out, double* __restrict__ min_sep,
        double* __restrict__ goal_dist) {      // X: X_dec, U: U_ff, K: Kc
    constexpr int nth = kPolicyThreads, kStage = kPolicyDecStage<NS, NC>;
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - b * chunks;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC;
    const int kw = kc_max * NS, mn = m * kw;      // columns of a row of Kc[t], elements of Kc[t]
    const int npairs = k * (k - 1) / 2;
    const PolicyLds O(NS, NC, k);
    const int AS = O.as, AC = O.ac;
    const int sl = tid / k, a = tid - sl * k;
    const int s = chunk * O.spw + sl;
    const bool active = sl < O.spw && s < S;      // a lane past the last sample: the cooperative copies and the barriers only
    const ItemParams P = item_params(D, b);
    const bool homog = homogeneous_ndims(P.n_dims, k);
    const double dtr = D.dt, radius = P.radius, w_prox = D.w_prox, w_ref = D.w_ref;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* lds = reinterpret_cast<double*>(lds_raw);

    const double* Xb = X + (int64_t)b * (T + 1) * n;
    const double* Ub = U + (int64_t)b * T * m;
    const double* Kb = K + (int64_t)b * T * mn;
    const int64_t smp = (int64_t)b * S + (active ? s : 0);
    const double* Wp = W ? W + smp * T * n + a * NS : nullptr;
    double* Xw = (Xs && active) ? Xs + smp * (T + 1) * n + a * NS : nullptr;
    double* Uw = (Us && active) ? Us + smp * T * m + a * NC : nullptr;

    const int model = active ? P.model[a] : 0;
    // read once per lane (k <= 20); only its lowest kc_max members are kept, so that the product never leaves the K[t] image
    unsigned mask = 0u;
    if (active) {
        unsigned rem = (unsigned)bits[(int64_t)b * k + a] & ((1u << k) - 1u);
        for (int p = 0; p < kc_max && rem != 0u; ++p, rem &= rem - 1u) mask |= rem & (0u - rem);
    }
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;
    const double* Qfa = P.Qf + a * NS * NS;

    // the cooperative copy: element e = tid + q nth of Kc[t] is (row e / kw, column e % kw); thread tid < n holds an entry of X,
    // thread 128 + i (i < n_u) one of U
    int kdst[kStage];
#pragma unroll
    for (int q = 0; q < kStage; ++q) {
        const int e = tid + q * nth;
        const int row = e / kw, j = e - row * kw;
        kdst[q] = e < mn ? j * O.rs + (row % NC) * k + row / NC : -1;
    }
    const bool has_x = tid < n, has_u = tid >= 128 && tid - 128 < m;
    const int xdst = has_x ? (tid / NS) * AS + tid % NS : 0;
    const int udst = has_u ? ((tid - 128) / NC) * AC + (tid - 128) % NC : 0;
    double stK[kStage], stX = 0.0, stU = 0.0;
    auto fetch = [&](int t) {     // registers <- global memory: K[t], X[t + 1], U[t + 1]
        const double* Kt = Kb + (int64_t)t * mn;
#pragma unroll
        for (int q = 0; q < kStage; ++q)
            if (q * nth < mn) stK[q] = Kt[tid + q * nth < mn ? tid + q * nth : 0];      // no load past the image's last 256 elements
        if (t + 1 < T) {
            if (has_x) stX = Xb[(int64_t)(t + 1) * n + tid];
            if (has_u) stU = Ub[(int64_t)(t + 1) * m + (tid - 128)];
        }
    };

    for (int e = tid; e < O.total; e += nth) lds[e] = 0.0;
    lds_handoff(false);
    if (has_x) lds[O.Xt + xdst] = Xb[tid];
    if (has_u) lds[O.Ut + udst] = Ub[tid - 128];

    double x[NS], w[NS], lo[NC], hi[NC];
    if (active) {
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = x0s[smp * n + a * NS + i];
        if (Xw) {
#pragma unroll
            for (int i = 0; i < NS; ++i) Xw[i] = x[i];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) w[i] = Wp ? Wp[i] : 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            lo[c] = u_lim ? u_lim[a * NC + c] : 0.0;
            hi[c] = u_lim ? u_lim[m + a * NC + c] : 0.0;
        }
    }
    // the dimensions of this agent's pairs (min of the two agents' n_dims, cost.py:145), two bits per partner offset (k <= 20)
    unsigned long long nd_pack = 0ull;
    if (active && !homog) {
        for (int dd = 1; 2 * dd <= k; ++dd) {
            const int o = a + dd < k ? a + dd : a + dd - k;
            nd_pack |= (unsigned long long)(min(P.n_dims[a], P.n_dims[o]) & 3) << (2 * dd);
        }
    }
    fetch(0);
    lds_handoff(false);

    double J = 0.0, sep2 = __builtin_huge_val();
    // this agent's share of the sample's pairs at the positions in `sxs`: (a, a + 1), ..., (a, a + k / 2) mod k, each computed as
    // (lower, higher) and put where the sum in combinations order finds it (forward.hpp); the smallest squared distance is kept
    auto pairs = [&](const double* sxs, double* cp) {
        for (int dd = 1; 2 * dd <= k; ++dd) {
            if (2 * dd == k && a >= dd) break;
            const int o = a + dd < k ? a + dd : a + dd - k;
            const int l = a < o ? a : o, h = a < o ? o : a;
            const int nd = homog ? 2 : (int)((nd_pack >> (2 * dd)) & 3ull);
            sep2 = fmin(sep2, pair_dist2(sxs + l * AS, sxs + h * AS, nd));
            cp[pair_index(l, h, k)] = pair_cost(sxs + l * AS, sxs + h * AS, nd, radius);
        }
    };

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        double* sK = lds + O.Kt + par * kw * O.rs;
#pragma unroll
        for (int q = 0; q < kStage; ++q)
            if (kdst[q] >= 0) sK[kdst[q]] = stK[q];
        if (t + 1 < T) {
            if (has_x) lds[O.Xt + (par ^ 1) * k * AS + xdst] = stX;
            if (has_u) lds[O.Ut + (par ^ 1) * k * AC + udst] = stU;
        }
        double* sdx = lds + O.dx + par * O.spw * k * AS;      // the workgroup's; lane tid's entries at tid * AS
        double* sxs = lds + O.xs + par * O.spw * k * AS;
        double ut[NC], wt[NS];
        if (active) {
            const double* sX = lds + O.Xt + par * k * AS + a * AS;
            const double* sU = lds + O.Ut + par * k * AC + a * AC;
#pragma unroll
            for (int c = 0; c < NC; ++c) ut[c] = sU[c];
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                sdx[tid * AS + i] = x[i] - sX[i];       // dx = x_t - X[t]
                sxs[tid * AS + i] = x[i];
                wt[i] = w[i];
            }
            if (Wp && t + 1 < T) {
#pragma unroll
                for (int i = 0; i < NS; ++i) w[i] = Wp[(int64_t)(t + 1) * n + i];
            }
        }
        if (t + 1 < T) fetch(t + 1);
        lds_handoff(false);
        if (active) {
            // Kc[t] dx over the set bits of the mask in ascending agent order o -- block pos (the rank of o in the neighbourhood)
            // of this agent's NC compact rows --, the columns in ascending order, one multiply and one add per term
            double sum[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = 0.0;
            const double* kp = sK + a;
            const double* dxs = sdx + sl * k * AS;
            int pos = 0;
            for (unsigned rem = mask; rem != 0u; rem &= rem - 1u) {
                const int o = __ffs((int)rem) - 1;
                double dxv[NS], kv[NS][NC];
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    dxv[i] = dxs[o * AS + i];
#pragma unroll
                    for (int c = 0; c < NC; ++c) kv[i][c] = kp[(pos * NS + i) * O.rs + c * k];
                }
#pragma unroll
                for (int i = 0; i < NS; ++i)
#pragma unroll
                    for (int c = 0; c < NC; ++c) sum[c] += kv[i][c] * dxv[i];
                ++pos;
            }
            if (a == 0 && t > 0) {  // stage cost of step t - 1 (other parity), summed in the reference's order
                const double* cr = lds + O.cref + ((par ^ 1) * O.spw + sl) * k;
                const double* cp = lds + O.cpair + ((par ^ 1) * O.spw + sl) * O.np1;
                const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
                J += w_prox * prox + w_ref * ref;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = ut[c] + sum[c];
                if (u_lim) v = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);     // a NaN stays a NaN
                ut[c] = v;
            }
            lds[O.cref + (par * O.spw + sl) * k + a] = ref_cost<NS, NC>(x, ut, xf, Qa, Ra, false);
            pairs(sxs + sl * k * AS, lds + O.cpair + (par * O.spw + sl) * O.np1);
            if (Uw) {
#pragma unroll
                for (int c = 0; c < NC; ++c) Uw[(int64_t)t * m + c] = ut[c];
            }
            double xn[NS];
            integrate_rt<NS>(model, x, ut, dtr, xn);
#pragma unroll
            for (int i = 0; i < NS; ++i) x[i] = Wp ? xn[i] + wt[i] : xn[i];
            if (Xw) {
#pragma unroll
                for (int i = 0; i < NS; ++i) Xw[(int64_t)(t + 1) * n + i] = x[i];
            }
        }
    }
    {
        // last stage cost, then the terminal cost cost(x_T, 0, terminal=True) (control.py:91); x_T counts for min_sep too
        const int par = T & 1;
        double* sxs = lds + O.xs + par * O.spw * k * AS;
        if (active) {
#pragma unroll
            for (int i = 0; i < NS; ++i) sxs[tid * AS + i] = x[i];
        }
        lds_handoff(false);
        if (active) {
            if (a == 0) {
                const double* cr = lds + O.cref + ((par ^ 1) * O.spw + sl) * k;
                const double* cp = lds + O.cpair + ((par ^ 1) * O.spw + sl) * O.np1;
                const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
                J += w_prox * prox + w_ref * ref;
            }
            double uz[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) uz[c] = 0.0;
            lds[O.cref + (par * O.spw + sl) * k + a] = ref_cost<NS, NC>(x, uz, xf, Qfa, Ra, true);
            pairs(sxs + sl * k * AS, lds + O.cpair + (par * O.spw + sl) * O.np1);
            lds[O.sep + tid] = sep2;
        }
        lds_handoff(false);
        if (active) {
            if (a == 0) {
                const double* cr = lds + O.cref + (par * O.spw + sl) * k;
                const double* cp = lds + O.cpair + (par * O.spw + sl) * O.np1;
                const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
                J += w_prox * prox + w_ref * ref;
                J_out[smp] = J;
                if (min_sep) {
                    double mn2 = __builtin_huge_val();      // no pair (k = 1): +inf
                    for (int i = 0; i < k; ++i) mn2 = fmin(mn2, lds[O.sep + sl * k + i]);
                    min_sep[smp] = sqrt(mn2);
                }
            }
            if (goal_dist) {
                const int nd = P.n_dims[a];
                double g2 = 0.0;
                for (int c = 0; c < nd && c < NS; ++c) {
                    const double df = x[c] - xf[c];
                    g2 += df * df;
                }
                goal_dist[smp * k + a] = sqrt(g2);
            }
        }
    }
}

}  // namespace dpilqr

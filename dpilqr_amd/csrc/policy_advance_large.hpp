// policy_advance_large.hpp -- the step between two solves of a receding-horizon loop for LARGE clusters, 60 < n_x <= 240
// (include/dpilqr_policy.h, dpilqr_policy_advance_large): what policy_advance.hpp computes -- every running scenario executes h
// steps of ITS OWN plan on the plant,
//     u_i = U[j][i] + K[j][i] (x - X[j][i])   [clamped to u_lim]      x <- step(x, u_i)   [+ W[s][g + i]]
// and the loop's bookkeeping (the executed states, controls and cost appended at g = n_done[s], the smallest separation, the
// distance left, the plan shifted into the next warm start) is done in the same launch -- where K[i] is 154 KB at n_x = 240,
// n_u = 80 and a lane that walks its own NC rows of it, as policy_advance.hpp's does, would stream it alone.  The semantics are
// dpilqr_policy_advance's, statement for statement, with ONE difference, the one policy_large.hpp has against policy.hpp:
//   ORDER OF THE SUM: each entry of K[j][i] (x - X[j][i]) is the sum over the columns 0 .. n_x - 1 in ascending order, ONE FUSED
//   multiply-add per term, starting from zero (the fp64 matrix pipe).
// The executed prefix equals k_policy_rollout_large's bit for bit: the product below is that kernel's, restated with ONE column
// tile that holds ONE live column -- the same 16 x 16 x 4 tiles (PolicyMfma), the same batches of kPolicyBatch reduction steps,
// the same treatment of the columns beyond n_x; a tile's columns do not mix, so the fifteen zero columns beside the live one
// change nothing in it.  The per-step part -- the clamp, the step, the disturbance, the stage cost's terms and the order of their
// sum, the separation -- calls policy.hpp's helpers (pair_dist2, pair_cost, ref_cost, sum_in_order, integrate_rt).
//
// Launch: ONE workgroup of 256 threads per item (every item has its own K: nothing is shared between items), the grid is B.
// Lanes 0 .. k - 1 are the item's agents; all four wavefronts form K[i] dx, row tiles wv and wv + 4 on wavefront wv; all 256
// threads do the shift copy.  The item's scenario s = scen[j], its step count g = n_done[s] and he = min(h, L - g) are the same
// in every thread: the loop runs to he, and a workgroup whose scen entry or step count is out of range leaves as a whole,
// before its first barrier.
//
// Two barriers per step.  Top of step i: the agents read X[i], U[i] (from global memory: no other lane shares them), publish
// dx = x - X[i] in row 0 of the dx image and their position; every wavefront requests its first two sets of A operands.  Barrier.
// The wavefronts form K[i] dx and store it in the du image.  Barrier.  The agents pick up their NC rows of du; lane 0 adds the
// stage cost of step i - 1 (J_exec takes ONE addition per step, in time order); clamp, cost terms, stores, step.  dx and du are
// single (policy_large.hpp); the positions and the stage-cost terms are read one step after they were written and are buffered
// by parity.  K == nullptr: the product is skipped as a whole, K dx = 0.
//
// Nothing outside the arguments is touched and no access sits behind a per-element test (policy_large.hpp's rules):
//   rows >= n_u     read row 0 of K[j][i]; their results go to words of the du image that no lane reads
//   columns >= n_x  read the row's last entry and the dx row's first, and BOTH operands are replaced by zero
//   columns 1 .. 15 of the tile   their dx rows exist in LDS and stay zero; their results go to du rows that no lane reads
// LDS (doubles; AdvanceLargeLds): dx 16 rows of ds, ds = the smallest number >= n_x that is 2 mod 32; du 16 rows of
// dus = (16 * row tiles) | 1, row r of K dx at (r % NC) * k + r / NC; pos k agents x 3 coordinates by parity; k reference costs
// and k (k - 1) / 2 pair costs in combinations order by parity; k squared separations.  The whole allocation is zeroed before the
// first step.  The largest served shape, twenty twelve-state agents: 48 KB.
//
// The shift of U and X into U_next / X_next: all 256 threads, consecutive lanes on consecutive words (policy_advance.hpp).
// U_next / X_next must not alias U / X.
#pragma once
#include <hip/hip_runtime.h>

#include "policy_large.hpp"

namespace dpilqr {

struct AdvanceLargeLds {   // offsets in doubles
    int dx, du, pos, cref, cpair, sep, total;
    int ds, dus, np1, mt;
    __host__ __device__ AdvanceLargeLds(int ns, int nc, int k) {
        const int n = k * ns, m = k * nc, npairs = k * (k - 1) / 2;
        mt = ((m + 15) / 16) * 16;
        ds = ((n + 29) / 32) * 32 + 2;      // >= n, = 2 mod 32 (PolicyLargeLds)
        dus = mt | 1;
        np1 = npairs > 0 ? npairs : 1;
        int o = 0;
        dx = o;    o += 16 * ds;
        du = o;    o += 16 * dus;
        pos = o;   o += 2 * k * kPolicyPos;
        cref = o;  o += 2 * k;
        cpair = o; o += 2 * np1;
        sep = o;   o += k;
        total = (o + 1) & ~1;
    }
};
inline size_t advance_large_lds_bytes(int ns, int nc, int k) { return sizeof(double) * (size_t)AdvanceLargeLds(ns, nc, k).total; }

// K[B][T][n_u][n_x] (nullptr: open loop); the state arrays as dpilqr_policy_advance takes them
template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_advance_large(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int h, const int* __restrict__ scen, int n_scen, int L, int n_d,
        const double* __restrict__ W, const double* __restrict__ u_lim, double* __restrict__ x_cur, int* __restrict__ n_done,
        double* __restrict__ X_exec, double* __restrict__ U_exec, double* __restrict__ J_exec, double* __restrict__ min_sep,
        double* __restrict__ dist_left, double* __restrict__ U_next, double* __restrict__ X_next) {
    constexpr int nth = kPolicyThreads, NP = NS < kPolicyPos ? NS : kPolicyPos;
    typedef PolicyMfma Mf;
    constexpr int kFwdBatch = kPolicyBatch;
    typedef Mf::acc_t acc_t;
    const int tid = (int)threadIdx.x;
    const int j = (int)blockIdx.x;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC, mn = m * n, npairs = k * (k - 1) / 2;
    // the item's scenario and step count: the same words in every thread (n_done[s] is written by this workgroup alone, behind
    // its last barrier)
    const int s = __builtin_amdgcn_readfirstlane(scen ? scen[j] : j);
    if (s < 0 || s >= n_scen) return;
    const int g = __builtin_amdgcn_readfirstlane(n_done[s]);
    if (g < 0 || g > L) return;
    const int he = min(h, L - g);      // never past the capacity
    const AdvanceLargeLds O(NS, NC, k);
    const bool active = tid < k;       // the agents; every other lane: the product, the barriers, the shift
    const int a = active ? tid : 0;
    const ItemParams P = item_params(D, j);
    const bool homog = homogeneous_ndims(P.n_dims, k);
    const double dtr = D.dt, radius = P.radius, w_prox = D.w_prox, w_ref = D.w_ref;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* lds = reinterpret_cast<double*>(lds_raw);

    const bool gains = K != nullptr, clamp = u_lim != nullptr, noisy = W != nullptr;      // uniform
    const double* Xj = X + (int64_t)j * (T + 1) * n + a * NS;
    const double* Uj = U + (int64_t)j * T * m + a * NC;
    const double* Kb = gains ? K + (int64_t)j * T * mn : nullptr;
    const double* Wp = noisy ? W + ((int64_t)s * L + g) * n + a * NS : nullptr;
    double* Xe = X_exec + ((int64_t)s * (L + 1) + g) * n + a * NS;
    double* Ue = U_exec + ((int64_t)s * L + g) * m + a * NC;

    const int model = active ? P.model[a] : 0;
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;

    // the matrix pipe's side of this lane (policy_large.hpp): its row of K[i] per row tile (clamped into the matrix), where its
    // four results per tile go in a du row
    const int wv = tid >> 6, g16 = (tid >> 4) & 3, c16 = tid & 15;
    const bool two = __builtin_amdgcn_readfirstlane((int)(16 * (wv + 4) < O.mt)) != 0;   // this wavefront has a second row tile
    const bool one = __builtin_amdgcn_readfirstlane((int)(16 * wv < O.mt)) != 0;         // ... a first one at all (n_u > 16 wv)
    const int r0 = 16 * wv + c16, r1 = 16 * (wv + 4) + c16;
    const int ko0 = (r0 < m ? r0 : 0) * n, ko1 = (r1 < m ? r1 : 0) * n;      // (n_u n_x <= 19 200)
    auto du_word = [&](int r) { return r < m ? (r % NC) * k + r / NC : r; };      // where row r < mt of K[i] dx lies in a du row
    const int nks = (n + 3) >> 2;      // reduction steps

    for (int e = tid; e < O.total; e += nth) lds[e] = 0.0;
    lds_handoff(false);
    if (active) lds[O.sep + tid] = __builtin_huge_val();

    double x[NS];
    if (active) {
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] = x_cur[(int64_t)s * n + a * NS + q];
    }
    // the dimensions of this agent's pairs, two bits per partner offset (policy.hpp)
    unsigned long long nd_pack = 0ull;
    if (active && !homog)
        for (int dd = 1; 2 * dd <= k; ++dd) {
            const int o = a + dd < k ? a + dd : a + dd - k;
            nd_pack |= (unsigned long long)(min(P.n_dims[a], P.n_dims[o]) & 3) << (2 * dd);
        }
    lds_handoff(false);

    double J = (active && a == 0) ? J_exec[s] : 0.0;
    // this agent's share of the item's pairs at the positions in `sp` (agent i's at i * kPolicyPos; policy_large.hpp); the smallest
    // squared distance is kept in the lane's own word of LDS; cp == nullptr: the separation only
    auto pairs = [&](const double* sp, double* cp) {
        double sep2 = lds[O.sep + tid];
        for (int dd = 1; 2 * dd <= k; ++dd) {
            if (2 * dd == k && a >= dd) break;
            const int o = a + dd < k ? a + dd : a + dd - k;
            const int l = a < o ? a : o, hh = a < o ? o : a;
            const int nd = homog ? 2 : (int)((nd_pack >> (2 * dd)) & 3ull);
            sep2 = fmin(sep2, pair_dist2(sp + l * kPolicyPos, sp + hh * kPolicyPos, nd));
            if (cp) cp[pair_index(l, hh, k)] = pair_cost(sp + l * kPolicyPos, sp + hh * kPolicyPos, nd, radius);
        }
        lds[O.sep + tid] = sep2;
    };
    auto add_stage_cost = [&](int p) {      // J += the stage cost whose terms lie in the buffers of parity p (lane a = 0)
        const double* cr = lds + O.cref + p * k;
        const double* cp = lds + O.cpair + p * O.np1;
        const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
        J += w_prox * prox + w_ref * ref;
    };

    double* sdx = lds + O.dx;
    double* sdu = lds + O.du;
    const double* dxc = sdx + c16 * O.ds;
    double* duc = sdu + c16 * O.dus;
    double kA0[kFwdBatch], kA1[kFwdBatch], kB0[kFwdBatch], kB1[kFwdBatch];      // the two sets of A operands, per row tile
    const double* Kt = Kb;
    auto whole = [&](int s0) { return 4 * (s0 + kFwdBatch) <= n; };     // every column of the batch exists, in every lane group
    auto load = [&](double (&k0)[kFwdBatch], double (&k1)[kFwdBatch], int s0) __attribute__((always_inline)) {
        if (!one) return;
        if (s0 == 0 || whole(s0)) {
            const double* q0 = Kt + ko0 + 4 * s0 + g16;
#pragma unroll
            for (int q = 0; q < kFwdBatch; ++q) k0[q] = q0[4 * q];
            if (two) {      // (wave-uniform)
                const double* q1 = Kt + ko1 + 4 * s0 + g16;
#pragma unroll
                for (int q = 0; q < kFwdBatch; ++q) k1[q] = q1[4 * q];
            }
        } else {        // (no load behind a test: a column beyond the row's end reads the row's last entry instead)
#pragma unroll
            for (int q = 0; q < kFwdBatch; ++q) k0[q] = Kt[ko0 + min(4 * (s0 + q) + g16, n - 1)];
            if (two) {
#pragma unroll
                for (int q = 0; q < kFwdBatch; ++q) k1[q] = Kt[ko1 + min(4 * (s0 + q) + g16, n - 1)];
            }
        }
    };

    for (int i = 0; i < he; ++i) {
        const int par = i & 1;
        double* spos = lds + O.pos + par * k * kPolicyPos;      // agent a's at a * kPolicyPos
        double ut[NC], wt[NS], lo[NC], hi[NC];
        if (active) {
            const double* Xi = Xj + (int64_t)i * n;
            const double* Ui = Uj + (int64_t)i * m;
#pragma unroll
            for (int c = 0; c < NC; ++c) ut[c] = Ui[c];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                sdx[a * NS + q] = x[q] - Xi[q];       // dx = x - X[i], the tile's column 0
                wt[q] = noisy ? Wp[(int64_t)i * n + q] : 0.0;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                lo[c] = clamp ? u_lim[a * NC + c] : 0.0;
                hi[c] = clamp ? u_lim[m + a * NC + c] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < NP; ++q) spos[a * kPolicyPos + q] = x[q];
        }
        // the first two sets, ahead of the barrier (policy_large.hpp: batch 0 is whole at any served size, batch 1 from n_x = 96)
        const bool pre1 = whole(kFwdBatch);
        if (gains) {
            Kt = Kb + (int64_t)i * mn;
            load(kA0, kA1, 0);
            if (pre1) load(kB0, kB1, kFwdBatch);
        }
        lds_handoff(false);

        // K[i] dx (the header comment)
        if (gains && one) {
            if (!pre1) {
                int sB = kFwdBatch;
                asm volatile("" : "+s"(sB));
                load(kB0, kB1, sB);
            }
            acc_t acc0 = acc_t{0, 0, 0, 0}, acc1 = acc_t{0, 0, 0, 0};
            auto products = [&](const double (&k0)[kFwdBatch], const double (&k1)[kFwdBatch], int s0) __attribute__((always_inline)) {
                if (whole(s0)) {
                    double bq[kFwdBatch];
                    const double* d0 = dxc + 4 * s0 + g16;
#pragma unroll
                    for (int q = 0; q < kFwdBatch; ++q) bq[q] = d0[4 * q];
#pragma unroll
                    for (int q = 0; q < kFwdBatch; ++q) acc0 = Mf::mac(k0[q], bq[q], acc0);
                    if (two) {
#pragma unroll
                        for (int q = 0; q < kFwdBatch; ++q) acc1 = Mf::mac(k1[q], bq[q], acc1);
                    }
                } else {        // a column beyond the last: both operands zero, the product adds nothing
                    bool jv[kFwdBatch];
                    int jo[kFwdBatch];
#pragma unroll
                    for (int q = 0; q < kFwdBatch; ++q) {
                        const int jj = 4 * (s0 + q) + g16;
                        jv[q] = jj < n;
                        jo[q] = jv[q] ? jj : 0;
                    }
                    double bq[kFwdBatch];
#pragma unroll
                    for (int q = 0; q < kFwdBatch; ++q) {
                        double bb = dxc[jo[q]];
                        asm volatile("" : "+v"(bb));      // (requested whatever jv says: policy_large.hpp)
                        bq[q] = jv[q] ? bb : 0.0;
                    }
#pragma unroll
                    for (int q = 0; q < kFwdBatch; ++q) acc0 = Mf::mac(jv[q] ? k0[q] : 0.0, bq[q], acc0);
                    if (two) {
#pragma unroll
                        for (int q = 0; q < kFwdBatch; ++q) acc1 = Mf::mac(jv[q] ? k1[q] : 0.0, bq[q], acc1);
                    }
                }
            };
            for (int s0 = 0; s0 < nks; s0 += 2 * kFwdBatch) {
                products(kA0, kA1, s0);
                if (s0 + 2 * kFwdBatch < nks) load(kA0, kA1, s0 + 2 * kFwdBatch);
                if (s0 + kFwdBatch < nks) products(kB0, kB1, s0 + kFwdBatch);
                if (s0 + 3 * kFwdBatch < nks) load(kB0, kB1, s0 + 3 * kFwdBatch);
            }
            // the tile's entries to where the agents find them (rows beyond n_u, columns beside the live one: words nobody reads)
            const int rb = 16 * wv + g16;
#pragma unroll
            for (int v = 0; v < 4; ++v) duc[du_word(rb + 4 * v)] = acc0[v];
            if (two) {
#pragma unroll
                for (int v = 0; v < 4; ++v) duc[du_word(rb + 64 + 4 * v)] = acc1[v];
            }
        }
        lds_handoff(false);

        if (active) {
            double sum[NC];      // K[i] dx, this agent's NC rows (zero where no wavefront has written: K == nullptr)
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = sdu[c * k + a];
            if (a == 0 && i > 0) add_stage_cost(par ^ 1);      // of step i - 1
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = ut[c] + sum[c];
                if (clamp) v = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);     // a NaN stays a NaN
                ut[c] = v;
            }
            // (the weights stay in memory: policy_large.hpp)
            const double *xft = xf, *Qt = Qa, *Rt = Ra;
            asm volatile("" : "+v"(xft), "+v"(Qt), "+v"(Rt));
            lds[O.cref + par * k + a] = ref_cost<NS, NC>(x, ut, xft, Qt, Rt, false);
            pairs(spos, lds + O.cpair + par * O.np1);
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
    // the state the plant ends in: it counts for the separation; the last executed step's stage cost
    {
        double* spos = lds + O.pos + (he & 1) * k * kPolicyPos;
        if (active) {
#pragma unroll
            for (int q = 0; q < NP; ++q) spos[a * kPolicyPos + q] = x[q];
        }
        lds_handoff(false);
        if (active) {
            if (a == 0 && he > 0) add_stage_cost((he - 1) & 1);
            pairs(spos, nullptr);
        }
        lds_handoff(false);
    }
    if (active) {
        if (a == 0) {
            J_exec[s] = J;
            double mn2 = __builtin_huge_val();
            for (int q = 0; q < k; ++q) mn2 = fmin(mn2, lds[O.sep + q]);
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
    const double* Uq = U + (int64_t)j * TM;
    double* Un = U_next + (int64_t)s * TM;
    for (int e = tid; e < TM; e += nth) {
        const int src = e + he * m;
        const double v = Uq[src < TM ? src : TM - 1];
        Un[e] = src < TM ? v : 0.0;
    }
    const double* Xq = X + (int64_t)j * (TN + n);
    double* Xn = X_next + (int64_t)s * (TN + n) + n;
    for (int e = tid; e < TN; e += nth) {
        const int src = e + n + he * n;
        Xn[e] = Xq[src < TN + n ? src : TN + (e - (e / n) * n)];
    }
}

}  // namespace dpilqr

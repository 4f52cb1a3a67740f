// policy.hpp -- the closed-loop ensemble rollout: S samples per item run the time-varying feedback policy of an iLQR solution,
//     u_t = U[t] + K[t] (x_t - X[t])   [clamped to u_lim]      x_{t+1} = step(x_t, u_t)   [+ W[t]]
// from their own starts, and report per sample the cost J, the smallest separation of any two agents over the horizon and every
// agent's distance from its goal at the end (include/dpilqr_hip.h, dpilqr_policy_rollout).  Not a reference function: the
// reference's forward pass (control.py:95-114) is the same recursion from X[0] with the feed-forward term; the step, the cost
// and its summation order are those of the rollout (control.py:80-93; forward.hpp).
//
// Launch: 256 threads, thread tid = (sample sl = tid / k, agent a = tid % k).  A workgroup holds spw = floor(256 / k) samples of
// ONE item; an item's samples take ceil(S / spw) consecutive workgroups, the grid is items x chunks.  What the samples of an item
// share -- K[t], X[t], U[t] -- is read from global memory ONCE per workgroup and step, by all 256 threads (a cooperative copy:
// lanes that hold no sample take part in it and in the barriers, and in nothing else), one step ahead of its use into registers,
// then into LDS.  Per sample only x0s / W are read and Xs / Us / the results written.
//
// One barrier per step.  At the top of step t every thread stores K[t] (fetched during step t - 1) into the K buffer of parity
// t & 1 and X[t + 1], U[t + 1] into the X / U buffers of parity (t + 1) & 1; a sample's lanes read X[t], U[t] (parity t & 1: stored
// at the top of step t - 1, behind that step's barrier) and publish dx = x - X[t] and x in the exchange buffers of parity t & 1;
// then the barrier; then K[t] dx, the costs, the step.  A buffer written at the top of step t was last read in step t - 2 (K, the
// exchange, the cost terms) or at the top of step t - 1 (X, U), and every thread has passed a barrier in between.
//
// LDS layout (doubles; ds_read_b64 / ds_write_b64 are served in groups of 32 / 16 lanes over 32 eight-byte banks):
//   K[t]      column j of the matrix at j * rs, row a * NC + c of it at c * k + a, rs = n_u | 1.  The agents of a sample read
//             consecutive words, the samples of a wavefront the same ones (a broadcast): at most k <= 20 distinct, consecutive
//             addresses per read.  The copy's consecutive lanes hold consecutive columns of a row: rs apart, rs odd.
//   X[t], U[t]  agent a's entries at a * as / a * ac, as = NS | 1, ac = NC | 1: the agents' reads an odd stride apart.
//   dx, x     lane tid's entries at tid * as: consecutive lanes an odd stride apart when they publish; reading column j of
//             K[t] dx, the lanes of a sample read one word and the samples of a 32-lane group words k * as apart -- distinct banks
//             for 32 / g consecutive samples, g the largest power of two in k, and a group holds no more than that
//             (k = g: exactly 32 / g, aligned; k >= 3 g: at most 32 / (3 g) + 2).
//   stage-cost terms  per sample k reference costs and k (k - 1) / 2 pair costs, in combinations order, by parity.
// The whole allocation is zeroed before the first step: the padding words (rs, as, ac) are never read, and no lane reads a word
// that neither it nor a thread ordered before it by a barrier has written.
//
// All of the above is policy_rollout_body, written once.  What it leaves to its `Gains` argument is the K[t] image and its use:
//   cols, mn    columns of a row of K[t] and elements of K[t] in global memory (the K buffers' parity stride is cols * rs)
//   kStage      K[t] elements a thread stages per step, a compile-time bound: the staging arrays stay in registers
//   setup, load   per lane, once, before the first fetch; staged element q of K[t] from global memory
//   product     sum[c] += (K[t] dx)[a * NC + c] for lane (sl, a), from the K buffer of this parity and the sample's dx row
// DenseGains (k_policy_rollout): the full n_u x n_x matrix.  CompactGains (policy_dec.hpp): per agent its neighbourhood's columns.
#pragma once
#include <hip/hip_runtime.h>

#include "cost.hpp"
#include "lds_sync.hpp"
#include "models.hpp"

namespace dpilqr {

constexpr int kPolicyThreads = 256;
constexpr int kPolicyStage = 10;    // K[t] elements a thread copies per step: n_u n_x <= 2560 (twenty CarDynamics3D: 40 x 60)

struct PolicyLds {   // offsets in doubles
    int Kt, Xt, Ut, dx, xs, cref, cpair, sep, total;
    int rs, as, ac, spw, np1;
    __host__ __device__ PolicyLds(int ns, int nc, int k) {
        const int n = k * ns, m = k * nc, npairs = k * (k - 1) / 2;
        spw = kPolicyThreads / k;
        rs = m | 1; as = ns | 1; ac = nc | 1;
        np1 = npairs > 0 ? npairs : 1;
        int o = 0;
        Kt = o;    o += 2 * n * rs;
        Xt = o;    o += 2 * k * as;
        Ut = o;    o += 2 * k * ac;
        dx = o;    o += 2 * spw * k * as;
        xs = o;    o += 2 * spw * k * as;
        cref = o;  o += 2 * spw * k;
        cpair = o; o += 2 * spw * np1;
        sep = o;   o += spw * k;
        total = (o + 1) & ~1;
    }
};
inline size_t policy_lds_bytes(int ns, int nc, int k) { return sizeof(double) * (size_t)PolicyLds(ns, nc, k).total; }

// squared distance of two agents over the first nd coordinates: the sum pair_cost (cost.hpp) takes the root of
__device__ __forceinline__ double pair_dist2(const double* a, const double* b, int nd) {
    double s = 0.0;
    for (int c = 0; c < nd; ++c) {
        const double df = a[c] - b[c];
        s += df * df;
    }
    return s;
}

// sum[c] += K_blk dx_o: column block `blk` of this agent's NC rows (kp: the K buffer at word a) times agent o's dx, the columns
// in ascending order, one multiply and one add per term
template <int NS, int NC>
__device__ __forceinline__ void policy_block(double (&sum)[NC], const double* kp, const double* dxs, int blk, int o, int rs, int k, int AS) {
    double dxv[NS], kv[NS][NC];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        dxv[i] = dxs[o * AS + i];
#pragma unroll
        for (int c = 0; c < NC; ++c) kv[i][c] = kp[(blk * NS + i) * rs + c * k];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int c = 0; c < NC; ++c) sum[c] += kv[i][c] * dxv[i];
}

// the dense gains K[b][t] [n_u][n_x]: every agent's rows take every agent's dx, column block o against agent o
template <int NS, int NC>
struct DenseGains {
    static constexpr int kStage = kPolicyStage;
    int k, cols, mn;
    int ksrc[kStage];
    __device__ explicit DenseGains(int k_) : k(k_), cols(k_ * NS), mn((k_ * NC) * (k_ * NS)) {}
    __device__ __forceinline__ void setup(int tid, int /*b*/, int /*a*/, bool /*active*/) {
#pragma unroll      // (no load behind a test: an element past the matrix reads its first entry)
        for (int q = 0; q < kStage; ++q) ksrc[q] = tid + q * kPolicyThreads < mn ? tid + q * kPolicyThreads : 0;
    }
    __device__ __forceinline__ void load(int q, const double* Kt, int /*tid*/, double& st) const { st = Kt[ksrc[q]]; }
    __device__ __forceinline__ void product(double (&sum)[NC], const double* kp, const double* dxs, int rs, int AS) const {
        for (int o = 0; o < k; ++o) policy_block<NS, NC>(sum, kp, dxs, o, o, rs, k, AS);
    }
};

// The rollout, for either form of the gains (the header comment); the pointers are the kernels' __restrict__ parameters.
// Xs [B][S][T+1][n_x], Us [B][S][T][n_u] (either may be null); J, min_sep [B][S]; goal_dist [B][S][k] (the last two may be null)
template <int NS, int NC, class Gains>
__device__ __forceinline__ void policy_rollout_body(Gains G, const dpilqr_batch_desc& D, const double* X, const double* U,
        const double* K, int S, int chunks, const double* x0s, const double* W, const double* u_lim, double* Xs, double* Us,
        double* J_out, double* min_sep, double* goal_dist) {
    constexpr int nth = kPolicyThreads, kStage = Gains::kStage;
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - b * chunks;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC;
    const int cols = G.cols, mn = G.mn, npairs = k * (k - 1) / 2;      // columns of a row of K[t], elements of K[t]
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
    G.setup(tid, b, a, active);
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;
    const double* Qfa = P.Qf + a * NS * NS;

    // the cooperative copy: element e = tid + q nth of K[t] is (row e / cols, column e % cols); thread tid < n holds an entry
    // of X, thread 128 + i (i < n_u) one of U
    int kdst[kStage];
#pragma unroll
    for (int q = 0; q < kStage; ++q) {
        const int e = tid + q * nth;
        const int row = e / cols, j = e - row * cols;
        kdst[q] = e < mn ? j * O.rs + (row % NC) * k + row / NC : -1;
    }
    const bool has_x = tid < n, has_u = tid >= 128 && tid - 128 < m;
    const int xdst = has_x ? (tid / NS) * AS + tid % NS : 0;
    const int udst = has_u ? ((tid - 128) / NC) * AC + (tid - 128) % NC : 0;
    double stK[kStage], stX = 0.0, stU = 0.0;
    auto fetch = [&](int t) {     // registers <- global memory: K[t], X[t + 1], U[t + 1]
        const double* Kt = Kb + (int64_t)t * mn;
#pragma unroll
        for (int q = 0; q < kStage; ++q) G.load(q, Kt, tid, stK[q]);
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
        for (int i = 0; i < NS; ++i) {
            x[i] = x0s[smp * n + a * NS + i];
            if (Xw) Xw[i] = x[i];
            w[i] = Wp ? Wp[i] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            lo[c] = u_lim ? u_lim[a * NC + c] : 0.0;
            hi[c] = u_lim ? u_lim[m + a * NC + c] : 0.0;
        }
    }
    // the dimensions of this agent's pairs (min of the two agents' n_dims, cost.py:145), two bits per partner offset (k <= 20)
    unsigned long long nd_pack = 0ull;
    if (active && !homog)
        for (int dd = 1; 2 * dd <= k; ++dd) {
            const int o = a + dd < k ? a + dd : a + dd - k;
            nd_pack |= (unsigned long long)(min(P.n_dims[a], P.n_dims[o]) & 3) << (2 * dd);
        }
    fetch(0);
    lds_handoff(false);

    const bool clamp = u_lim != nullptr, noisy = W != nullptr;      // uniform: no per-lane pointer test inside the loop
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
    // J += the stage cost whose terms lie in the buffers of parity p, summed in the reference's order (lane a = 0 of a sample)
    auto add_stage_cost = [&](int p) {
        const double* cr = lds + O.cref + (p * O.spw + sl) * k;
        const double* cp = lds + O.cpair + (p * O.spw + sl) * O.np1;
        const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
        J += w_prox * prox + w_ref * ref;
    };

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        double* sK = lds + O.Kt + par * cols * O.rs;
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
            if (noisy && t + 1 < T) {
#pragma unroll
                for (int i = 0; i < NS; ++i) w[i] = Wp[(int64_t)(t + 1) * n + i];
            }
        }
        if (t + 1 < T) fetch(t + 1);
        lds_handoff(false);
        if (active) {
            double sum[NC];      // K[t] dx, this agent's NC rows
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = 0.0;
            G.product(sum, sK + a, sdx + sl * k * AS, O.rs, AS);
            if (a == 0 && t > 0) add_stage_cost(par ^ 1);      // of step t - 1
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = ut[c] + sum[c];
                if (clamp) v = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);     // a NaN stays a NaN
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
            for (int i = 0; i < NS; ++i) x[i] = noisy ? xn[i] + wt[i] : xn[i];
            if (Xw) {
#pragma unroll
                for (int i = 0; i < NS; ++i) Xw[(int64_t)(t + 1) * n + i] = x[i];
            }
        }
    }
    // last stage cost, then the terminal cost cost(x_T, 0, terminal=True) (control.py:91); x_T counts for min_sep too
    const int par = T & 1;
    double* sxs = lds + O.xs + par * O.spw * k * AS;
    if (active) {
#pragma unroll
        for (int i = 0; i < NS; ++i) sxs[tid * AS + i] = x[i];
    }
    lds_handoff(false);
    if (active) {
        if (a == 0) add_stage_cost(par ^ 1);
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
            add_stage_cost(par);
            J_out[smp] = J;
            if (min_sep) {
                double mn2 = __builtin_huge_val();      // no pair (k = 1): +inf
                for (int i = 0; i < k; ++i) mn2 = fmin(mn2, lds[O.sep + sl * k + i]);
                min_sep[smp] = sqrt(mn2);
            }
        }
        if (goal_dist) goal_dist[smp * k + a] = sqrt(pair_dist2(x, xf, min(P.n_dims[a], NS)));
    }
}

template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_rollout(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int S, int chunks, const double* __restrict__ x0s,
        const double* __restrict__ W, const double* __restrict__ u_lim, double* __restrict__ Xs, double* __restrict__ Us,
        double* __restrict__ J_out, double* __restrict__ min_sep, double* __restrict__ goal_dist) {
    policy_rollout_body<NS, NC>(DenseGains<NS, NC>(D.k), D, X, U, K, S, chunks, x0s, W, u_lim, Xs, Us, J_out, min_sep, goal_dist);
}

}  // namespace dpilqr

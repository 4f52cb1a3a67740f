// policy_large.hpp -- the closed-loop ensemble rollout for LARGE clusters, 60 < n_x <= 240 (include/dpilqr_policy.h,
// dpilqr_policy_rollout_large): what policy.hpp computes -- S samples per item under
//     u_t = U[t] + K[t] (x_t - X[t])   [clamped to u_lim]      x_{t+1} = step(x_t, u_t)   [+ W[t]]
// with J, min_sep and goal_dist per sample -- where K[t] no longer fits that kernel: two LDS images of K[t] are 311 KB at
// n_x = 240, n_u = 80, and ten staged elements per thread cover 2560 of its 19 200.  Here K[t] is never staged at all: K[t] dx of
// all the workgroup's samples is ONE (n_u x n_x)(n_x x samples) product on the fp64 MATRIX PIPE, its A operand read straight from
// global memory (forward.hpp's PIPE path, with the samples of an item in place of the line search's candidates).
//
// Launch: as policy.hpp -- 256 threads, thread tid = (sample sl = tid / k, agent a = tid % k), spw = floor(256 / k) samples of
// ONE item per workgroup, ceil(S / spw) consecutive workgroups per item, the grid items x chunks.  Served: 6 <= k <= 20, so
// spw <= 42, at most three column tiles of 16 samples and ceil(n_u / 16) <= 5 row tiles.  The per-sample part -- the clamp, the
// step, the disturbance, the stage cost's terms and the order of their sum, min_sep, goal_dist -- is policy.hpp's, statement by
// statement, on its free helpers (pair_dist2; cost.hpp; lds_sync.hpp).
//
// The product.  16 x 16 x 4 tiles (PolicyMfma): lane (g16 = lane / 16, c16 = lane % 16) of a wavefront supplies
// A = K[t][16 it + c16][4 s + g16] and B = dx[sample 16 ct + c16][4 s + g16] in reduction step s and owns rows g16 + 4 v of column
// c16 of the result.  Row tiles it = wv and wv + 4 belong to wavefront wv (at most two each); a wavefront walks the reduction in
// batches of kPolicyBatch steps, two register sets of A operands used in turn (a set is requested again as soon as its products are
// issued; the first two of a step are requested BEFORE the step's first barrier), and every set serves all the workgroup's column
// tiles before it is replaced: K[t] is read from global memory once per workgroup and step.  A batch is ONE address per row tile
// and per column tile, every load and every LDS read of it at an immediate offset.
//   ORDER OF THE SUM: the columns of K[t] in ascending order, ONE FUSED multiply-add per term (what the matrix pipe does).  This
//   differs from dpilqr_policy_rollout, which rounds the product and the sum of every term separately (policy.hpp, policy_block).
// Nothing outside the arguments is touched and no access sits behind a per-element test:
//   rows >= n_u     read row 0 of K[b][t]; their results go to words of the du image that no lane reads
//   columns >= n_x  (n_x % 4 != 0, or a batch that reaches past the last reduction step) read the row's last entry and the dx
//                   row's first, and BOTH operands are replaced by zero: the term adds an exact zero
//   sample slots >= the workgroup's samples   their dx rows exist in LDS and stay zero (the image has 16 rows per column tile);
//                   their columns of the result go to du rows that no lane reads.  A tile's columns do not mix, so no sample
//                   depends on what its neighbours in the tile hold.  Column tiles without any sample are not computed
//                   (workgroup-uniform).
//
// Two barriers per step.  Top of step t: a sample's lanes read X[t], U[t] and publish dx = x - X[t] and their position; every
// thread requests its entry of X[t + 1], U[t + 1].  Barrier.  The four wavefronts form K[t] dx and store it in the du image; every
// thread stores its entry of X[t + 1], U[t + 1] into the X / U buffers of parity (t + 1) & 1 (last read at the top of step t - 1).
// Barrier.  The lanes pick up their NC rows of du; costs, step.  dx and du
// are single: dx is written at the top of a step and read between its barriers, du written between them and read behind the
// second.  The positions and the stage-cost terms are read one step after they were written and are buffered by parity, as in
// policy.hpp.
//
// LDS layout (doubles; ds_read_b64 is served in two groups of 32 lanes over 32 eight-byte banks, ds_write_b64 in four groups of
// 16 consecutive lanes over 16):
//   dx    sample slot j's row at j * ds, ds = the smallest number >= n_x that is 2 mod 32; 16 * ceil(spw / 16) rows.  The B
//         operand's 32-lane group is g16 in {0, 1} (or {2, 3}) x c16 = 0 .. 15 at c16 * ds + g16 + const: 2 c16 + g16 mod 32, all
//         32 banks once.  (policy.hpp's rows of a * (NS | 1) + i would put reduction steps at varying distances: no immediate
//         offsets.)  Published by lane (sl, a) at sl * ds + a * NS + i: the 16 lanes of a store group are consecutive agents, NS
//         words apart -- 16 / gcd(16, NS)-way distinct: two-way for NS = 6, four-way for 4 and 12, on NS stores per step.
//   du    sample slot j's row at j * dus, dus = (16 * row tiles) | 1; row r = a * NC + c of K[t] dx at (r % NC) * k + r / NC for
//         r < n_u (the agents of a sample read consecutive words), at r beyond.  A tile's store group is one g16, c16 = 0 .. 15:
//         dus apart, dus odd -- 16 banks once.
//   pos   lane tid's first three coordinates (all a pair's distance can take: n_dims <= 3) at tid * 3, by parity.
//   X[t], U[t]   agent a's entries at a * (NS | 1) / a * (NC | 1), by parity (policy.hpp).
//   stage-cost terms   per sample k reference costs and k (k - 1) / 2 pair costs in combinations order, by parity.
// The whole allocation is zeroed before the first step.  The largest served shape, twenty twelve-state agents, takes 101 KB.
#pragma once
#include <hip/hip_runtime.h>

#include "policy.hpp"

namespace dpilqr {

constexpr int kPolicyLargeMaxNx = 240, kPolicyLargeMaxK = 20;
constexpr int kPolicyPos = 3;      // coordinates of an agent the pairs can read
constexpr int kPolicyBatch = 12;   // reduction steps of K[t] dx per register set of A operands, two sets (forward.hpp: kFwdBatch)

// 16x16x4 fp64 matrix-pipe tile (the same helper as forward.hpp's FwdMfma<double>, which this translation unit does not compile):
// lane (g = lane / 16, c = lane % 16) supplies A[row c][reduction g], B[reduction g][column c] and owns rows g + 4 v of column c of D
struct PolicyMfma {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    __device__ static __forceinline__ acc_t mac(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    __device__ static __forceinline__ int row(int v, int g) { return g + 4 * v; }
};

struct PolicyLargeLds {   // offsets in doubles
    int Xt, Ut, dx, du, pos, cref, cpair, sep, total;
    int ds, dus, as, ac, spw, np1, mt, ctiles;
    __host__ __device__ PolicyLargeLds(int ns, int nc, int k) {
        const int n = k * ns, m = k * nc, npairs = k * (k - 1) / 2;
        spw = kPolicyThreads / k;
        ctiles = (spw + 15) / 16;
        mt = ((m + 15) / 16) * 16;
        ds = ((n + 29) / 32) * 32 + 2;      // >= n, = 2 mod 32
        dus = mt | 1;
        as = ns | 1; ac = nc | 1;
        np1 = npairs > 0 ? npairs : 1;
        int o = 0;
        Xt = o;    o += 2 * k * as;
        Ut = o;    o += 2 * k * ac;
        dx = o;    o += 16 * ctiles * ds;
        du = o;    o += 16 * ctiles * dus;
        pos = o;   o += 2 * kPolicyThreads * kPolicyPos;
        cref = o;  o += 2 * spw * k;
        cpair = o; o += 2 * spw * np1;
        sep = o;   o += kPolicyThreads;
        total = (o + 1) & ~1;
    }
};
inline size_t policy_large_lds_bytes(int ns, int nc, int k) { return sizeof(double) * (size_t)PolicyLargeLds(ns, nc, k).total; }

// Xs [B][S][T+1][n_x], Us [B][S][T][n_u] (either may be null); J, min_sep [B][S]; goal_dist [B][S][k] (the last two may be null)
template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_rollout_large(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int S, int chunks, const double* __restrict__ x0s,
        const double* __restrict__ W, const double* __restrict__ u_lim, double* __restrict__ Xs, double* __restrict__ Us,
        double* __restrict__ J_out, double* __restrict__ min_sep, double* __restrict__ goal_dist) {
    constexpr int nth = kPolicyThreads, NP = NS < kPolicyPos ? NS : kPolicyPos;
    typedef PolicyMfma Mf;
    constexpr int kFwdBatch = kPolicyBatch;
    typedef Mf::acc_t acc_t;
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - b * chunks;
    const int k = D.k, T = D.T, n = k * NS, m = k * NC, mn = m * n, npairs = k * (k - 1) / 2;
    const PolicyLargeLds O(NS, NC, k);
    const int AS = O.as, AC = O.ac;
    const int sl = tid / k, a = tid - sl * k;
    const int s = chunk * O.spw + sl;
    const bool active = sl < O.spw && s < S;      // a lane past the last sample: the cooperative copies, the product, the barriers
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
    const double* xf = P.xf + a * NS;
    const double* Qa = P.Q + a * NS * NS;
    const double* Ra = P.R + a * NC * NC;
    const double* Qfa = P.Qf + a * NS * NS;

    // the matrix pipe's side of this lane: its row of K[t] per row tile (clamped into the matrix), its dx row per column tile, where
    // its four results per tile go in a du row
    const int wv = tid >> 6, g16 = (tid >> 4) & 3, c16 = tid & 15;
    const int left = S - chunk * O.spw;                                     // samples of this workgroup, >= 1
    const int nct = ((left < O.spw ? left : O.spw) + 15) >> 4;              // column tiles that hold one (workgroup-uniform)
    const bool two = __builtin_amdgcn_readfirstlane((int)(16 * (wv + 4) < O.mt)) != 0;   // this wavefront has a second row tile
    const bool one = __builtin_amdgcn_readfirstlane((int)(16 * wv < O.mt)) != 0;         // ... a first one at all (n_u > 16 wv)
    const int r0 = 16 * wv + c16, r1 = 16 * (wv + 4) + c16;
    const int ko0 = (r0 < m ? r0 : 0) * n, ko1 = (r1 < m ? r1 : 0) * n;      // (n_u n_x <= 19 200)
    auto du_word = [&](int r) { return r < m ? (r % NC) * k + r / NC : r; };      // where row r < mt of K[t] dx lies in a du row
    const int nks = (n + 3) >> 2;      // reduction steps

    // the cooperative copy: thread tid < n holds an entry of X, thread tid < n_u one of U
    const bool has_x = tid < n, has_u = tid < m;
    const int xdst = has_x ? (tid / NS) * AS + tid % NS : 0;
    const int udst = has_u ? (tid / NC) * AC + tid % NC : 0;

    for (int e = tid; e < O.total; e += nth) lds[e] = 0.0;
    lds_handoff(false);
    lds[O.sep + tid] = __builtin_huge_val();      // (tid < spw k or not: the buffer has 256 words)
    if (has_x) lds[O.Xt + xdst] = Xb[tid];
    if (has_u) lds[O.Ut + udst] = Ub[tid];

    double x[NS];
    if (active) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            x[i] = x0s[smp * n + a * NS + i];
            if (Xw) Xw[i] = x[i];
        }
    }
    // the dimensions of this agent's pairs (min of the two agents' n_dims, cost.py:145), two bits per partner offset (k <= 20)
    unsigned long long nd_pack = 0ull;
    if (active && !homog)
        for (int dd = 1; 2 * dd <= k; ++dd) {
            const int o = a + dd < k ? a + dd : a + dd - k;
            nd_pack |= (unsigned long long)(min(P.n_dims[a], P.n_dims[o]) & 3) << (2 * dd);
        }
    lds_handoff(false);

    const bool clamp = u_lim != nullptr, noisy = W != nullptr;      // uniform: no per-lane pointer test inside the loop
    double J = 0.0;
    // this agent's share of the sample's pairs at the positions in `sp` (agent i's at i * kPolicyPos): (a, a + 1), ...,
    // (a, a + k / 2) mod k, each computed as (lower, higher) and put where the sum in combinations order finds it (forward.hpp);
    // the smallest squared distance is kept -- in the lane's own word of LDS, not in a register pair that would live through the step
    auto pairs = [&](const double* sp, double* cp) {
        double sep2 = lds[O.sep + tid];
        for (int dd = 1; 2 * dd <= k; ++dd) {
            if (2 * dd == k && a >= dd) break;
            const int o = a + dd < k ? a + dd : a + dd - k;
            const int l = a < o ? a : o, h = a < o ? o : a;
            const int nd = homog ? 2 : (int)((nd_pack >> (2 * dd)) & 3ull);
            sep2 = fmin(sep2, pair_dist2(sp + l * kPolicyPos, sp + h * kPolicyPos, nd));
            cp[pair_index(l, h, k)] = pair_cost(sp + l * kPolicyPos, sp + h * kPolicyPos, nd, radius);
        }
        lds[O.sep + tid] = sep2;
    };
    // J += the stage cost whose terms lie in the buffers of parity p, summed in the reference's order (lane a = 0 of a sample)
    auto add_stage_cost = [&](int p) {
        const double* cr = lds + O.cref + (p * O.spw + sl) * k;
        const double* cp = lds + O.cpair + (p * O.spw + sl) * O.np1;
        const double prox = sum_in_order(cp, npairs), ref = sum_in_order(cr, k);
        J += w_prox * prox + w_ref * ref;
    };

    double* sdx = lds + O.dx;
    double* sdu = lds + O.du;
    const double* dxc = sdx + c16 * O.ds;      // column tile ct: + 16 ct ds
    double* duc = sdu + c16 * O.dus;           // ... + 16 ct dus
    double kA0[kFwdBatch], kA1[kFwdBatch], kB0[kFwdBatch], kB1[kFwdBatch];      // the two sets of A operands, per row tile
    const double* Kt = Kb;
    auto whole = [&](int s0) { return 4 * (s0 + kFwdBatch) <= n; };     // every column of the batch exists, in every lane group
    auto load = [&](double (&k0)[kFwdBatch], double (&k1)[kFwdBatch], int s0) __attribute__((always_inline)) {
        if (!one) return;
        if (s0 == 0 || whole(s0)) {
            const double* q0 = Kt + ko0 + 4 * s0 + g16;
#pragma unroll
            for (int q = 0; q < kFwdBatch; ++q) k0[q] = q0[4 * q];
            if (two) {      // (wave-uniform, and known to be: a branch, not a masked region around every load)
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

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        double* spos = lds + O.pos + par * nth * kPolicyPos + sl * k * kPolicyPos;      // the sample's; agent a's at a * kPolicyPos
        // (the limits and W[t] are requested here, a step's length ahead of their use, rather than kept or fetched a step ahead as
        // policy.hpp does: sixteen plus twenty-four registers that the twelve-state step needs)
        double ut[NC], wt[NS], lo[NC], hi[NC];
        if (active) {
            const double* sX = lds + O.Xt + par * k * AS + a * AS;
            const double* sU = lds + O.Ut + par * k * AC + a * AC;
#pragma unroll
            for (int c = 0; c < NC; ++c) ut[c] = sU[c];
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                sdx[sl * O.ds + a * NS + i] = x[i] - sX[i];       // dx = x_t - X[t]
                wt[i] = noisy ? Wp[(int64_t)t * n + i] : 0.0;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                lo[c] = clamp ? u_lim[a * NC + c] : 0.0;
                hi[c] = clamp ? u_lim[m + a * NC + c] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) spos[a * kPolicyPos + i] = x[i];
        }
        double stX = 0.0, stU = 0.0;      // X[t + 1], U[t + 1]: requested here, stored between the barriers
        if (t + 1 < T) {
            if (has_x) stX = Xb[(int64_t)(t + 1) * n + tid];
            if (has_u) stU = Ub[(int64_t)(t + 1) * m + tid];
        }
        Kt = Kb + (int64_t)t * mn;
        // the first two sets, ahead of the barrier: batch 0 is whole at any served size (n_x > 60 >= 4 kFwdBatch); batch 1 is below
        // n_x = 8 kFwdBatch, and then follows behind the barrier -- its start made opaque, or the clamped form's 2 x kFwdBatch
        // offsets, the same in every step, are computed ahead of the loop and kept: 96 registers
        const bool pre1 = whole(kFwdBatch);
        load(kA0, kA1, 0);
        if (pre1) load(kB0, kB1, kFwdBatch);
        lds_handoff(false);
        if (!pre1) {
            int sB = kFwdBatch;
            asm volatile("" : "+s"(sB));
            load(kB0, kB1, sB);
        }

        // K[t] dx of every sample of the workgroup (the header comment)
        if (one) {
            acc_t acc0[3], acc1[3];
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) acc0[ct] = acc1[ct] = acc_t{0, 0, 0, 0};
            auto products = [&](const double (&k0)[kFwdBatch], const double (&k1)[kFwdBatch], int s0) __attribute__((always_inline)) {
                if (whole(s0)) {
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct) {
                        if (ct < nct) {
                            double bq[kFwdBatch];
                            const double* d0 = dxc + ct * 16 * O.ds + 4 * s0 + g16;
#pragma unroll
                            for (int q = 0; q < kFwdBatch; ++q) bq[q] = d0[4 * q];
#pragma unroll
                            for (int q = 0; q < kFwdBatch; ++q) acc0[ct] = Mf::mac(k0[q], bq[q], acc0[ct]);
                            if (two) {
#pragma unroll
                                for (int q = 0; q < kFwdBatch; ++q) acc1[ct] = Mf::mac(k1[q], bq[q], acc1[ct]);
                            }
                        }
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
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct) {
                        if (ct < nct) {
                            double bq[kFwdBatch];
                            const double* d0 = dxc + ct * 16 * O.ds;
#pragma unroll
                            for (int q = 0; q < kFwdBatch; ++q) {
                                double bb = d0[jo[q]];
                                asm volatile("" : "+v"(bb));      // (requested whatever jv says: behind the test, every read is a masked region with its own wait)
                                bq[q] = jv[q] ? bb : 0.0;
                            }
#pragma unroll
                            for (int q = 0; q < kFwdBatch; ++q) acc0[ct] = Mf::mac(jv[q] ? k0[q] : 0.0, bq[q], acc0[ct]);
                            if (two) {
#pragma unroll
                                for (int q = 0; q < kFwdBatch; ++q) acc1[ct] = Mf::mac(jv[q] ? k1[q] : 0.0, bq[q], acc1[ct]);
                            }
                        }
                    }
                }
            };
            for (int s0 = 0; s0 < nks; s0 += 2 * kFwdBatch) {
                products(kA0, kA1, s0);
                if (s0 + 2 * kFwdBatch < nks) load(kA0, kA1, s0 + 2 * kFwdBatch);
                if (s0 + kFwdBatch < nks) products(kB0, kB1, s0 + kFwdBatch);
                if (s0 + 3 * kFwdBatch < nks) load(kB0, kB1, s0 + 3 * kFwdBatch);
            }
            // the tiles' entries to where the samples' lanes find them (rows beyond n_u, slots beyond the samples: words nobody reads).
            // (A column tile's distance is made opaque: eight words of a du row per lane are kept, not twenty-four addresses.)
            int ctd = 16 * O.dus, rb = 16 * wv + g16;
            asm volatile("" : "+s"(ctd), "+v"(rb));
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) {
                if (ct < nct) {
                    double* dd = duc + ct * ctd;
#pragma unroll
                    for (int v = 0; v < 4; ++v) dd[du_word(rb + 4 * v)] = acc0[ct][v];
                    if (two) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) dd[du_word(rb + 64 + 4 * v)] = acc1[ct][v];
                    }
                }
            }
        }
        if (t + 1 < T) {
            if (has_x) lds[O.Xt + (par ^ 1) * k * AS + xdst] = stX;
            if (has_u) lds[O.Ut + (par ^ 1) * k * AC + udst] = stU;
        }
        lds_handoff(false);

        if (active) {
            double sum[NC];      // K[t] dx, this agent's NC rows
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[c] = sdu[sl * O.dus + c * k + a];
            if (a == 0 && t > 0) add_stage_cost(par ^ 1);      // of step t - 1
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double v = ut[c] + sum[c];
                if (clamp) v = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v);     // a NaN stays a NaN
                ut[c] = v;
            }
            // The weights stay in memory: these three pointers are made opaque once per step, or the compiler, which knows that no
            // store of the loop can change what they point to, would load Q, R and xf ahead of the loop and keep them -- 172 values
            // per lane in the twelve-state family, more than the step and the product leave free.
            const double *xft = xf, *Qt = Qa, *Rt = Ra;
            asm volatile("" : "+v"(xft), "+v"(Qt), "+v"(Rt));
            lds[O.cref + (par * O.spw + sl) * k + a] = ref_cost<NS, NC>(x, ut, xft, Qt, Rt, false);
            pairs(spos, lds + O.cpair + (par * O.spw + sl) * O.np1);
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
    double* spos = lds + O.pos + par * nth * kPolicyPos + sl * k * kPolicyPos;
    if (active) {
#pragma unroll
        for (int i = 0; i < NP; ++i) spos[a * kPolicyPos + i] = x[i];
    }
    lds_handoff(false);
    if (active) {
        if (a == 0) add_stage_cost(par ^ 1);
        double uz[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) uz[c] = 0.0;
        lds[O.cref + (par * O.spw + sl) * k + a] = ref_cost<NS, NC>(x, uz, xf, Qfa, Ra, true);
        pairs(spos, lds + O.cpair + (par * O.spw + sl) * O.np1);
    }
    lds_handoff(false);
    if (active) {
        if (a == 0) {
            add_stage_cost(par);
            J_out[smp] = J;
            if (min_sep) {
                double mn2 = __builtin_huge_val();
                for (int i = 0; i < k; ++i) mn2 = fmin(mn2, lds[O.sep + sl * k + i]);
                min_sep[smp] = sqrt(mn2);
            }
        }
        if (goal_dist) goal_dist[smp * k + a] = sqrt(pair_dist2(x, xf, min(P.n_dims[a], NS)));
    }
}

}  // namespace dpilqr

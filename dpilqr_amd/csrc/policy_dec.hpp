// policy_dec.hpp -- the closed loop of a DISTRIBUTED solution: every agent runs the feedback law of its own sub-problem,
//     u_i(t) = U_ff_i[t] + Kc_i[t] (x_{C_i}(t) - X_dec[t]_{C_i})   [clamped to u_lim]
// where C_i is agent i's neighbourhood (a bit mask, bit i set, not necessarily symmetric), Kc_i its n_c rows of the gains of
// the sub-problem solved for C_i, the columns C_i's members in ascending order, and U_ff the sub-problem's own nominal folded
// onto the stitched trajectory (frontend.hpp, k_stitch_policy).  Everything else is the FULL k-agent problem's and policy.hpp's
// policy_rollout_body (X: X_dec, U: U_ff, PolicyLds(NS, NC, k) as it is); this file is the body's compact `Gains`:
//   K[t] image  Kc[b][t] is [k][NC][kw] in global memory, kw = kc_max * NS columns: k NC kw doubles per step against n_u n_x.
//             A thread stages ceil(k NC kw / 256) <= kPolicyDecStage of them and issues no load past the image.  In LDS it is
//             policy.hpp's K[t] layout with kw <= n_x columns, the two parities kw * rs apart in buffers sized for n_x.
//   product   Lane (sample, a) walks the set bits of ITS mask, lowest first (ascending agent order): iteration p handles its
//             p-th member o_a.  The lanes of a wavefront advance in lock step on p, not on the agent: a lane with fewer than
//             p + 1 members has left the loop.
//             K reads: block p of the lane's own compact row, word (p * NS + i) * rs + c * k + a -- whatever the masks are,
//             the agents of a sample read consecutive words and the samples of a wavefront (one item, so the same masks) the
//             same ones: at most k <= 20 distinct, consecutive addresses per read, as in policy.hpp.
//             dx reads: word (sl * k + o_a) * as + i of the exchange buffer.  o_a differs per lane, so this is no broadcast: up
//             to k distinct words per sample (all masks full: one; all alone: each lane the entry it published).  as = NS | 1 is
//             odd, so two words share a bank exactly where their indices sl * k + o differ by a multiple of 32; the indices a
//             32-lane group reads lie within the samples it spans, fewer than 64 consecutive ones: at most two-way.  Not
//             measured with counters.
//   columns past kc_a * NS of a row are copied but never read: the product loop ends with the mask's last bit.  A mask with
//             more than kc_max bits (the caller's contract forbids it) loses its members past the kc_max-th when it is read:
//             the product never indexes past the K[t] image, and no address at all depends on a mask's value beyond that.
#pragma once
#include "policy.hpp"

namespace dpilqr {

// Kc[t] elements a thread copies per step: k NC kw <= (60 / NS) NC 60 within the served shapes (n_x <= 60, kw <= n_x) -- ten for the
// three-state family (policy.hpp's kPolicyStage), five for the twelve-state one, whose step needs the registers
template <int NS, int NC>
constexpr int kPolicyDecStage = ((60 / NS) * NC * 60 + kPolicyThreads - 1) / kPolicyThreads;

template <int NS, int NC>
struct CompactGains {
    static constexpr int kStage = kPolicyDecStage<NS, NC>;
    int k, kc_max, cols, mn;
    const unsigned long long* bits;
    unsigned mask = 0u;
    __device__ CompactGains(int k_, int kc_max_, const unsigned long long* bits_)
        : k(k_), kc_max(kc_max_), cols(kc_max_ * NS), mn((k_ * NC) * (kc_max_ * NS)), bits(bits_) {}
    // the mask, read once per lane (k <= 20): only its lowest kc_max members are kept
    __device__ __forceinline__ void setup(int /*tid*/, int b, int a, bool active) {
        if (!active) return;
        unsigned rem = (unsigned)bits[(int64_t)b * k + a] & ((1u << k) - 1u);
        for (int p = 0; p < kc_max && rem != 0u; ++p, rem &= rem - 1u) mask |= rem & (0u - rem);
    }
    __device__ __forceinline__ void load(int q, const double* Kt, int tid, double& st) const {
        const int e = tid + q * kPolicyThreads;
        if (q * kPolicyThreads < mn) st = Kt[e < mn ? e : 0];      // no load past the image's last 256 elements
    }
    // block pos (the rank of o in the neighbourhood) of this agent's compact rows against agent o's dx
    __device__ __forceinline__ void product(double (&sum)[NC], const double* kp, const double* dxs, int rs, int AS) const {
        int pos = 0;
        for (unsigned rem = mask; rem != 0u; rem &= rem - 1u, ++pos)
            policy_block<NS, NC>(sum, kp, dxs, pos, __ffs((int)rem) - 1, rs, k, AS);
    }
};

template <int NS, int NC>
__global__ __launch_bounds__(kPolicyThreads) void k_policy_rollout_dec(dpilqr_batch_desc D, const double* __restrict__ X,
        const double* __restrict__ U, const double* __restrict__ K, int kc_max, const unsigned long long* __restrict__ bits,
        int S, int chunks, const double* __restrict__ x0s, const double* __restrict__ W, const double* __restrict__ u_lim,
        double* __restrict__ Xs, double* __restrict__ Us, double* __restrict__ J_out, double* __restrict__ min_sep,
        double* __restrict__ goal_dist) {      // X: X_dec, U: U_ff, K: Kc
    policy_rollout_body<NS, NC>(CompactGains<NS, NC>(D.k, kc_max, bits), D, X, U, K, S, chunks, x0s, W, u_lim, Xs, Us, J_out, min_sep, goal_dist);
}

}  // namespace dpilqr

// admit_order.hpp -- the active list ordered by sweep cost, for the batches the fused four-state wavefront sweep serves.
//
// A sweep wavefront's time grows with the number of steps at which some pair of its item's agents is within the proximity radius
// (riccati_mfma_lane.inc: f_prox -- the pair derivatives and everything that consumes them are skipped otherwise).  The active list
// is in arbitrary order: survivors are pushed by atomicAdd (forward_wave.hpp: linesearch_decide), new items appended behind them
// (k_admit), and the sweep deals list positions to (round, CU, SIMD) by position alone.  A workgroup holds its CU until its slowest
// wavefront ends and a launch ends with its slowest CU, so where the slow items land is worth choosing:
//   k_cost_keys   key[pos] = number of steps t in 0..T of the item at list position pos at which the sweep's own criterion
//                 !(s2 > r * r * (1 + 1e-12)) holds for some pair -- the sweep's expression for s2, evaluated on the X the sweep
//                 is about to read, so the count is exactly what the sweep will see.
//                 Optional second output key_dense[pos] = the item's last near step + 1 (0: no near step), at most T + 1: the number
//                 of steps the sweep runs densely since it walks the steps behind the last near pair per agent
//                 (riccati_mfma.hpp, "Decoupled prologue"; the terminal step counts, it decides whether the prologue starts).
//   k_order_list  one workgroup: a counting sort of the list by key class (at most 64 classes, heaviest first; order within a class
//                 is arbitrary), scattered through order_position into the list the sweep and the line search read.
// Two orders, both permutations of 0..n-1 produced by the same kernel:
//   kOrderSpread   rank r -> position r.  With the sweep's layer dealing every (CU, SIMD) gets one item of each layer, so the SIMDs
//                  and CUs of a round carry nearly the same sum of keys, and the heavy layers are the first round's.
//   kOrderGrouped  consecutive ranks share a sweep workgroup (its 4 / 8 / 12 positions), workgroups in blockIdx order: a round's
//                  workgroups are of one cost class and the heavy workgroups are dispatched first.
// Nothing an item computes depends on its position: K, d and the candidates are indexed by list position consistently within an
// iteration, everything else by item id.
//
// SweepDeal and order_position are plain C++ (host and device): tests/test_admit_order_host.py compiles them without HIP.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DPILQR_HD __host__ __device__
#else
#define DPILQR_HD
#endif

namespace dpilqr {

enum CostOrder : int { kOrderOff = 0, kOrderSpread = 1, kOrderGrouped = 2 };
// The solve loop's order.  A/B route switches (launch.hpp: route_env): DPILQR_NO_COST_ORDER, DPILQR_COST_ORDER=0|1|2.
constexpr int kDefaultCostOrder = kOrderSpread;
// The solve loop's key.  A/B route switch DPILQR_COST_KEY=0|1; with the decoupled prologue switched off the count is the key.
enum CostKey : int { kKeyNearCount = 0, kKeyDenseSteps = 1 };
constexpr int kDefaultCostKey = kKeyDenseSteps;

constexpr int kOrderMinLive = 1024;   // lists of at most this many items (the team tier, the latency-bound tail) keep their order
constexpr int kOrderClasses = 64;

// How the wavefront sweep deals n list positions to workgroups (riccati_mfma.hpp, "Items are DEALT to workgroups in layers"): a
// layer is one wavefront on every SIMD of every CU (per_layer = 4 n_cus positions), a round is one workgroup per CU running
// LPR = waves / 4 layers at most, and the layers are spread as evenly as possible over the fewest rounds that hold them.  The
// same constants, in the same expressions, as the sweep's own.
struct SweepDeal {
    int n, n_cus, waves, per_layer, layers, rounds, lo, extra;
    DPILQR_HD SweepDeal(int n_, int n_cus_, int waves_) : n(n_), n_cus(n_cus_), waves(waves_) {
        const int lpr = waves / 4;
        per_layer = 4 * n_cus;
        layers = (n + per_layer - 1) / per_layer;
        rounds = (layers + lpr - 1) / lpr;
        lo = rounds > 0 ? layers / rounds : 0;
        extra = rounds > 0 ? layers - lo * rounds : 0;      // rounds < extra run lo + 1 layers
    }
    DPILQR_HD int layers_of(int round) const { return lo + (round < extra ? 1 : 0); }
    DPILQR_HD int first_layer(int round) const { return round * lo + (round < extra ? round : extra); }
    DPILQR_HD int round_of_layer(int layer) const {
        const int head = extra * (lo + 1);                  // layers of the rounds that run lo + 1
        return layer < head ? layer / (lo + 1) : extra + (layer - head) / (lo > 0 ? lo : 1);
    }
    // list position of wavefront `wave` of workgroup (round, cu), -1: the wavefront has no item
    DPILQR_HD int slot(int round, int cu, int wave) const {
        if (round >= rounds || wave >= 4 * layers_of(round)) return -1;
        const int s = (first_layer(round) + (wave >> 2)) * per_layer + (wave & 3) * n_cus + cu;
        return s < n ? s : -1;
    }
};

// rank (0 = heaviest) -> list position.  Grouped: the workgroups in blockIdx order (round major, CU minor) take consecutive ranks,
// each as many as it has positions below n; inside a workgroup the ranks go to its wavefronts in order.  Every layer but the
// list's last is full, so only the last round's workgroups can differ in size: the last layer holds rem = n - (layers - 1)
// per_layer positions, s n_cus + cu < rem, that is rem / n_cus of them for every CU and one more for the CUs below rem % n_cus.
DPILQR_HD inline int order_position(int rank, const SweepDeal& D, int order) {
    if (order != kOrderGrouped) return rank;
    const int round = D.round_of_layer(rank / D.per_layer);
    const int f = D.first_layer(round), m = D.layers_of(round);
    const int q = rank - f * D.per_layer;                   // rank inside the round
    int base = 4 * m, e = 0;                                // positions per workgroup; the first e workgroups have one more
    if (round == D.rounds - 1) {
        const int rem = D.n - (D.layers - 1) * D.per_layer;
        base = 4 * (m - 1) + rem / D.n_cus;
        e = rem % D.n_cus;
    }
    int cu, w;
    if (q < e * (base + 1)) { cu = q / (base + 1); w = q - cu * (base + 1); }
    else { const int q2 = q - e * (base + 1), per = base > 0 ? base : 1; cu = e + q2 / per; w = q2 - (cu - e) * per; }
    return (f + (w >> 2)) * D.per_layer + (w & 3) * D.n_cus + cu;
}

// near-step count -> class 0 .. kOrderClasses - 1 (monotone; the count itself where T + 1 < kOrderClasses)
DPILQR_HD inline int order_class(int key, int T) {
    const int top = T + 1;
    const int c = top < kOrderClasses ? key : (int)((int64_t)key * (kOrderClasses - 1) / top);
    return c < 0 ? 0 : (c > kOrderClasses - 1 ? kOrderClasses - 1 : c);
}

#if defined(__HIPCC__) && defined(DPILQR_ADMIT_ORDER_KERNELS)   // tu_order.hip: no device code crosses a file boundary

// One wavefront per list position, a lane per step.  X[B][T + 1][4 k] (four-state agents: the position is the first two states),
// list / count null: every item of the batch in index order.  Lists of at most min_live items are left alone (key untouched).
// Up to kKeyStagedAgents agents the wavefront first brings 64 steps' positions into LDS with 16-byte loads that sweep the item's
// rows in address order (a lane reading its own row straight from memory touches 51 cache lines per load instruction: 43 us per
// full cfg2 window against the 50 MB it reads); each lane then takes its step's k positions from there.  The wavefront's LDS
// operations execute in order, so a compiler fence separates the two halves.
constexpr int kKeyStagedAgents = 5;
__global__ void __launch_bounds__(256) k_cost_keys(const double* __restrict__ X, const double* __restrict__ radius, int64_t radius_bstride,
                                                   const int32_t* __restrict__ list, const int32_t* __restrict__ count, int B, int T, int k,
                                                   int min_live, int32_t* __restrict__ key, int32_t* __restrict__ key_dense) {
    __shared__ double2 sP[4][64 * kKeyStagedAgents];
    const int n = count ? *count : B;
    if (n <= min_live) return;
    const int wave = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pos = (int)blockIdx.x * 4 + wave;
    if (pos >= n) return;
    const int b = list ? list[pos] : pos;
    if (b < 0 || b >= B) return;
    const double r = radius[(int64_t)b * radius_bstride];
    const double lim = r * r * (1.0 + 1e-12);
    const int nx = 4 * k;
    const double* Xb = X + (int64_t)b * (T + 1) * nx;
    const bool staged = k <= kKeyStagedAgents;
    int cnt = 0, dense = 0;
    for (int t0 = 0; t0 <= T; t0 += 64) {
        const int rows = min(64, T + 1 - t0);
        bool near = false;
        if (staged) {
            // 16-byte piece 2 e of the chunk is the position of (row e / k, agent e % k): a row is 2 k pieces, position then velocity
            const double2* src = reinterpret_cast<const double2*>(Xb + (int64_t)t0 * nx);
            for (int e = lane; e < rows * k; e += 64) sP[wave][e] = src[2 * e];
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            if (lane < rows) {
                double2 p[kKeyStagedAgents];
#pragma unroll
                for (int i = 0; i < kKeyStagedAgents; ++i) p[i] = sP[wave][lane * k + min(i, k - 1)];
#pragma unroll
                for (int i = 0; i < kKeyStagedAgents; ++i)
#pragma unroll
                    for (int j = i + 1; j < kKeyStagedAgents; ++j) {
                        const double ddx = p[i].x - p[j].x, ddy = p[i].y - p[j].y;
                        const double s2 = ddx * ddx + ddy * ddy;
                        near = near || (j < k && !(s2 > lim));
                    }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        } else if (lane < rows) {
            const double* row = Xb + (int64_t)(t0 + lane) * nx;
            for (int i = 0; i < k; ++i)
                for (int j = i + 1; j < k; ++j) {
                    const double ddx = row[4 * i] - row[4 * j], ddy = row[4 * i + 1] - row[4 * j + 1];
                    const double s2 = ddx * ddx + ddy * ddy;
                    near = near || !(s2 > lim);
                }
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(near);
        cnt += __popcll(mask);
        if (mask) dense = t0 + 64 - __clzll(mask);      // the last near step of the chunk, + 1
    }
    if (lane == 0) {
        if (key) key[pos] = cnt;
        if (key_dense) key_dense[pos] = dense;
    }
}

// One workgroup.  dst <- src reordered: the counting sort of the n = *count listed items by class, heaviest first, rank r stored at
// order_position(r).  n <= min_live, or order == kOrderOff: a plain copy.  src and dst must not overlap.
__global__ void __launch_bounds__(1024) k_order_list(const int32_t* __restrict__ src, int32_t* __restrict__ dst, const int32_t* __restrict__ count,
                                                     const int32_t* __restrict__ key, int T, int n_cus, int waves, int order, int min_live) {
    static_assert(kOrderClasses == 64, "the prefix sums below are one wavefront's, a bin per lane");
    __shared__ int hist[kOrderClasses], cursor[kOrderClasses];
    const int n = *count;
    if (n <= min_live || order == kOrderOff) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
        return;
    }
    if (threadIdx.x < kOrderClasses) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[kOrderClasses - 1 - order_class(key[i], T)], 1);
    __syncthreads();
    if (threadIdx.x < kOrderClasses) {      // the first wavefront: exclusive prefix sums of the 64 bins, one bin per lane
        const int own = hist[threadIdx.x];
        int run = own;
        for (int off = 1; off < kOrderClasses; off <<= 1) {
            const int below = __shfl_up(run, off);
            if ((int)threadIdx.x >= off) run += below;
        }
        cursor[threadIdx.x] = run - own;
    }
    __syncthreads();
    const SweepDeal deal(n, n_cus, waves);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int rank = atomicAdd(&cursor[kOrderClasses - 1 - order_class(key[i], T)], 1);
        const int pos = order_position(rank, deal, order);
        if (pos >= 0 && pos < n) dst[pos] = src[i];
    }
}

#endif  // DPILQR_ADMIT_ORDER_KERNELS

}  // namespace dpilqr

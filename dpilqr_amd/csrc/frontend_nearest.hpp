// frontend_nearest.hpp -- the interaction graph with every neighbourhood capped at its m nearest agents (include/dpilqr_nearest.h).
//
// Definition, for scenario s over the sampled rows r = 0, st, 2 st, ... of X[s] (st = graph_row_step(N), frontend_wide.hpp):
//   d_r(i, j)  = sqrt(dx*dx + dy*dy) over the planar positions of row r        (k_graph_bits_wide's expression and order)
//   key(i, j)  = min_r d_r(i, j); a comparison with a NaN is false, so a NaN distance is never the minimum and never near
//   nbr(i)     = {i} + { j : key(i, j) < 2 radius[s] }                          (today's graph: any_r (d_r < thr) <=> min_r d_r < thr)
//   mask_m(i)  = nbr(i) where |nbr(i)| <= m; otherwise {i} and the m - 1 members j != i of nbr(i) that are smallest under the
//                lexicographic order on (key(i, j), j): ties go to the lower agent index
//   dropped(i) = |nbr(i)| - |mask_m(i)|
// The masks need not be symmetric; nothing behind them asks for that (k_dedup_wide, k_bucket_sort_wide, the gathers and stitches
// consume them as they come).
//
//   k_graph_bits_nearest<NW>   one workgroup of kWideThreads threads per scenario, NW = n_words.  The sampled rows' x and y are
//                              staged in LDS planes [row][agent] as in k_graph_bits_wide.  A wavefront takes agent i: lane l holds
//                              key(i, 64 w + l) for the NW words in registers (a fully unrolled array: no dynamic index), the
//                              ballot of key < thr is the uncapped word and the popcount over the words |nbr(i)|.  Only where
//                              |nbr(i)| > m -- uniform per wavefront -- the wavefront ranks its candidates: the 64 NW keys go to
//                              the wavefront's own LDS strip (+inf for a non-candidate), every lane counts for each of its NW
//                              agents the candidates that precede it under (key, j) -- all lanes read the same strip entry, a
//                              broadcast --, a candidate of rank < m - 1 is kept and the ballot is again the word.  Lane 0 stores
//                              the words and `dropped`.
// LDS: 2 * rows * k doubles (77,824 B at k = 256 with 19 rows) + kWideThreads / 64 strips of kWideMaxAgents doubles (8,192 B):
// 86,016 B at most, under kMaxLds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frontend_wide.hpp"

namespace dpilqr {

constexpr int kNearestWaves = kWideThreads / 64;
inline size_t graph_nearest_lds_bytes(int N, int k) {
    return graph_wide_lds_bytes(N, k) + sizeof(double) * kNearestWaves * kWideMaxAgents;
}

template <int NW>
static __global__ __launch_bounds__(kWideThreads) void k_graph_bits_nearest(int S, int N, int k, int n_s, int m,
        const double* __restrict__ X, const double* __restrict__ radius, int64_t radius_stride,
        unsigned long long* __restrict__ bits, int32_t* __restrict__ dropped) {
    static_assert(NW >= 1 && NW <= kWideMaxWords, "a lane holds one key per word");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int s = blockIdx.x;
    if (s >= S) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int step = graph_row_step(N), n_r = graph_row_count(N);
    double* px = reinterpret_cast<double*>(lds_raw);      // [n_r][k]
    double* py = px + (size_t)n_r * k;
    double* strip = py + (size_t)n_r * k + wave * kWideMaxAgents;      // this wavefront's 64 NW keys
    const double* Xs = X + (int64_t)s * N * k * n_s;
    for (int e = tid; e < n_r * k; e += kWideThreads) {
        const int r = e / k, a = e - r * k;
        const double* p = Xs + ((int64_t)r * step * k + a) * n_s;
        px[e] = p[0];
        py[e] = p[1];
    }
    __syncthreads();
    const double thr = 2 * radius[(int64_t)s * radius_stride];
    const double inf = __builtin_huge_val();
    for (int i = wave; i < k; i += kNearestWaves) {      // uniform per wavefront
        double key[NW];
        unsigned long long word[NW];
        int n = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int j = 64 * w + lane;
            double v = inf;
            if (j < k && j != i)
                for (int r = 0; r < n_r; ++r) {
                    const double dx = px[r * k + i] - px[r * k + j], dy = py[r * k + i] - py[r * k + j];
                    const double d = sqrt(dx * dx + dy * dy);
                    if (d < v) v = d;
                }
            key[w] = v < thr ? v : inf;      // a candidate's key, +inf for every other lane (j == i, j >= k, far, NaN)
            word[w] = __ballot(j == i || key[w] < inf);
            n += __popcll(word[w]);
        }
        if (n > m) {      // uniform per wavefront: n comes from ballots
#pragma unroll
            for (int w = 0; w < NW; ++w) strip[64 * w + lane] = key[w];
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            int before[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) before[w] = 0;
#pragma unroll 4
            for (int c = 0; c < 64 * NW; ++c) {
                const double kc = strip[c];      // one address for the wavefront: a broadcast
#pragma unroll
                for (int w = 0; w < NW; ++w) before[w] += (kc < key[w] || (kc == key[w] && c < 64 * w + lane)) ? 1 : 0;
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");      // the strip is read before the next agent's keys go in
#pragma unroll
            for (int w = 0; w < NW; ++w) word[w] = __ballot(64 * w + lane == i || (key[w] < inf && before[w] < m - 1));
        }
        if (lane == 0) {
#pragma unroll
            for (int w = 0; w < NW; ++w) bits[((int64_t)s * k + i) * NW + w] = word[w];
            if (dropped) dropped[(int64_t)s * k + i] = n > m ? n - m : 0;
        }
    }
}

}  // namespace dpilqr

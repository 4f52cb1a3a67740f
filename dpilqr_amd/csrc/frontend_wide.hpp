// frontend_wide.hpp -- the dispatch front and back end (frontend.hpp) for teams of 64 < k <= 256 agents.
//
// A neighbourhood is n_words = ceil(k / 64) words, bits[S][k][n_words]: word w, bit b = agent 64 w + b.  The definitions are
// frontend.hpp's -- neighbour: planar distance < 2 * radius on any sampled row, own bit always set; representative: the first
// agent with an identical mask (quirk Q11, `ignore` honoured); a stable counting sort of the representatives by cluster size; an
// owner's position inside its cluster: the number of lower members -- and with n_words = 1 every array equals the narrow
// kernels'.  The narrow kernels stay what they are: the k <= 64 path pays nothing for this one.
//
//   k_graph_bits_wide   one workgroup per scenario.  The sampled rows' planar positions are staged in LDS once (x and y in
//                       planes of their own, [row][agent]: consecutive lanes read consecutive words, an agent's own entry is a
//                       broadcast); a wavefront then produces one mask word at a time: lane l tests agent 64 w + l against agent
//                       i over the rows and the wave64 ballot IS the word.  The narrow kernel gives one thread all of an agent's
//                       scattered global reads -- 5,600 of them at k = 256.
//   k_dedup_wide, k_bucket_sort_wide, k_gather_bucket_wide, k_stitch_wide   frontend.hpp's kernels over n_words words
//
// Cluster sizes: a mask may have up to k members, the sub-problem batches (BucketResults, the gathers' member lists) serve
// cluster sizes up to kFrontMaxAgents = 64.  The sort counts every size 0 .. k -- the caller sees a populated size beyond 64 in
// bucket_count and refuses the team --, the gather and the stitch never touch one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frontend.hpp"

namespace dpilqr {

constexpr int kWideMaxAgents = 256;
constexpr int kWideMaxWords = kWideMaxAgents / 64;
constexpr int kWideThreads = 256;       // k_graph_bits_wide: four wavefronts per scenario
constexpr int kWideSortThreads = 128;   // (k + 1) x 128 counters: 131,584 B at k = 256

// rows of X a graph samples: slice(0, N + 1, max(N // 10, 1)) of N rows
__host__ __device__ inline int graph_row_step(int N) { return (N / 10 > 1) ? N / 10 : 1; }
__host__ __device__ inline int graph_row_count(int N) { const int st = graph_row_step(N); return (N + st - 1) / st; }
// (N = 10 s + 9 rows sample 10 + ceil(9 / s) of them: 19 at most, 2 * 19 * 256 doubles = 77,824 B at k = 256)
inline size_t graph_wide_lds_bytes(int N, int k) { return sizeof(double) * 2 * (size_t)graph_row_count(N) * k; }

static __global__ __launch_bounds__(kWideThreads) void k_graph_bits_wide(int S, int N, int k, int n_s, int n_words,
        const double* __restrict__ X, const double* __restrict__ radius, int64_t radius_stride,
        unsigned long long* __restrict__ bits) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int s = blockIdx.x;
    if (s >= S) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int step = graph_row_step(N), n_r = graph_row_count(N);
    double* px = reinterpret_cast<double*>(lds_raw);      // [n_r][k]
    double* py = px + (size_t)n_r * k;
    const double* Xs = X + (int64_t)s * N * k * n_s;
    for (int e = tid; e < n_r * k; e += kWideThreads) {
        const int r = e / k, a = e - r * k;
        const double* p = Xs + ((int64_t)r * step * k + a) * n_s;
        px[e] = p[0];
        py[e] = p[1];
    }
    __syncthreads();
    const double thr = 2 * radius[(int64_t)s * radius_stride];
    for (int task = wave; task < k * n_words; task += kWideThreads / 64) {      // uniform per wavefront
        const int i = task / n_words, w = task - i * n_words;
        const int j = 64 * w + lane;
        bool near = false;
        if (j < k) {
            near = j == i;
            for (int r = 0; r < n_r; ++r) {
                const double dx = px[r * k + i] - px[r * k + j], dy = py[r * k + i] - py[r * k + j];
                near = near || sqrt(dx * dx + dy * dy) < thr;
            }
        }
        const unsigned long long word = __ballot(near);
        if (lane == 0) bits[((int64_t)s * k + i) * n_words + w] = word;
    }
}

__device__ __forceinline__ bool same_mask(const unsigned long long* a, const unsigned long long* b, int n_words) {
    bool eq = true;
    for (int w = 0; w < n_words; ++w) eq = eq && a[w] == b[w];
    return eq;
}

static __global__ void k_dedup_wide(int S, int k, int n_words, const unsigned long long* __restrict__ bits,
                                    const int32_t* __restrict__ ignore, int32_t* __restrict__ rep, int32_t* __restrict__ size) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)S * k) return;
    const int s = (int)(idx / k), i = (int)(idx - (int64_t)s * k);
    if (ignore && ignore[i]) { rep[idx] = -1; size[idx] = 0; return; }
    const unsigned long long* m = bits + idx * n_words;
    int r = i;
    for (int j = 0; j < i; ++j)
        if (same_mask(bits + ((int64_t)s * k + j) * n_words, m, n_words) && !(ignore && ignore[j])) { r = j; break; }
    int c = 0;
    for (int w = 0; w < n_words; ++w) c += __popcll(m[w]);
    rep[idx] = r;
    size[idx] = c;
}

// k_bucket_sort with kWideSortThreads chunks: its (k + 1) x 256 counters are 263 KB at k = 256, more than a workgroup's LDS
static __global__ __launch_bounds__(kWideSortThreads) void k_bucket_sort_wide(int S, int k, const int32_t* __restrict__ rep,
        const int32_t* __restrict__ size, int32_t* __restrict__ order, int32_t* __restrict__ bucket_start,
        int32_t* __restrict__ bucket_count, int32_t* __restrict__ slot) {
    extern __shared__ int32_t cnt_wide[];     // [k + 1][kWideSortThreads]: entries of size c in thread t's chunk
    constexpr int nt = kWideSortThreads;
    const int t = threadIdx.x;
    const int64_t n = (int64_t)S * k;
    const int64_t chunk = (n + nt - 1) / nt, lo = (int64_t)t * chunk < n ? (int64_t)t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    for (int c = 0; c <= k; ++c) cnt_wide[c * nt + t] = 0;
    for (int64_t e = lo; e < hi; ++e)
        if (rep[e] == (int32_t)(e % k)) cnt_wide[size[e] * nt + t] += 1;
    __syncthreads();
    if (t == 0) {                               // exclusive scan in (size, thread) order
        int32_t run = 0;
        for (int c = 0; c <= k; ++c) {
            bucket_start[c] = run;
            for (int q = 0; q < nt; ++q) {
                const int32_t v = cnt_wide[c * nt + q];
                cnt_wide[c * nt + q] = run;
                run += v;
            }
            bucket_count[c] = run - bucket_start[c];
        }
    }
    __syncthreads();
    for (int64_t e = lo; e < hi; ++e) {
        slot[e] = -1;
        if (rep[e] == (int32_t)(e % k)) {
            const int c = size[e];
            const int32_t pos = cnt_wide[c * nt + t]++;
            order[pos] = (int32_t)e;
            slot[e] = pos - bucket_start[c];
        }
    }
}

// members of a mask in ascending order, at most kFrontMaxAgents of them (thread 0 of the workgroup)
__device__ __forceinline__ void mask_members(const unsigned long long* m, int k, int n_words, int* mem) {
    int p = 0;
    for (int w = 0; w < n_words; ++w) {
        unsigned long long word = m[w];
        while (word && p < kFrontMaxAgents) {
            const int b = __ffsll((long long)word) - 1;
            word &= word - 1ull;
            if (64 * w + b < k) mem[p++] = 64 * w + b;
        }
    }
}

// k_gather_bucket over n_words words; kc <= kFrontMaxAgents (the launcher holds it)
static __global__ void k_gather_bucket_wide(int k, int n_s, int n_c, int T, int n_rows, int kc, int n_words,
        const int32_t* __restrict__ order, int first, int count, const unsigned long long* __restrict__ bits,
        const double* __restrict__ X, const double* __restrict__ U, const double* __restrict__ xf, int64_t xf_stride,
        double* __restrict__ x0_out, double* __restrict__ xf_out, double* __restrict__ U_out, int32_t* __restrict__ members) {
    const int j = blockIdx.x;                 // sub-problem within the slice
    if (j >= count) return;
    const int e = order[first + j], s = e / k;
    __shared__ int mem[kFrontMaxAgents];
    if (threadIdx.x == 0) mask_members(bits + (int64_t)e * n_words, k, n_words, mem);
    __syncthreads();
    const double* Xs = X + (int64_t)s * n_rows * k * n_s;        // row 0 = the scenario's current state
    const double* xfs = xf + (int64_t)s * xf_stride;
    for (int q = threadIdx.x; q < kc * n_s; q += blockDim.x) {
        const int p = q / n_s, c = q - p * n_s;
        x0_out[(int64_t)j * kc * n_s + q] = Xs[mem[p] * n_s + c];
        xf_out[(int64_t)j * kc * n_s + q] = xfs[mem[p] * n_s + c];
    }
    const double* Us = U + (int64_t)s * T * k * n_c;
    for (int q = threadIdx.x; q < T * kc * n_c; q += blockDim.x) {
        const int t = q / (kc * n_c), r = q - t * kc * n_c, p = r / n_c, c = r - p * n_c;
        U_out[(int64_t)j * T * kc * n_c + q] = Us[(int64_t)t * k * n_c + mem[p] * n_c + c];
    }
    if (members)
        for (int p = threadIdx.x; p < kc; p += blockDim.x) members[(int64_t)j * kc + p] = mem[p];
}

// owner_lookup over n_words words: the lower members are counted across the words
__device__ __forceinline__ bool owner_lookup_wide(int k, int n_words, const unsigned long long* bits, const int32_t* rep,
                                                  const int32_t* size, const int32_t* slot, int64_t e, int& kc, int& sl, int& pos) {
    const int i = (int)(e % k);
    const int r = rep[e];
    if (r < 0) return false;
    const int64_t er = e - i + r;
    kc = size[er];
    sl = slot[er];
    const unsigned long long* m = bits + e * n_words;
    int p = 0;
    for (int w = 0; w < (i >> 6); ++w) p += __popcll(m[w]);
    pos = p + __popcll(m[i >> 6] & ((1ull << (i & 63)) - 1ull));
    return true;
}

static __global__ void k_stitch_wide(int S, int k, int n_s, int n_c, int T, int n_words, const unsigned long long* __restrict__ bits,
                                     const int32_t* __restrict__ rep, const int32_t* __restrict__ size,
                                     const int32_t* __restrict__ slot, BucketResults R, double* __restrict__ X_dec,
                                     double* __restrict__ U_dec) {
    const int64_t e = blockIdx.x;             // (s, i)
    if (e >= (int64_t)S * k) return;
    int kc, sl, pos;
    if (!owner_lookup_wide(k, n_words, bits, rep, size, slot, e, kc, sl, pos)) return;
    if (kc > kFrontMaxAgents) return;         // no such bucket was solved (the caller refuses the team)
    sl -= R.first[kc];
    if (sl < 0 || sl >= R.count[kc]) return;
    const int s = (int)(e / k), i = (int)(e % k);
    const double* Xb = R.X[kc] + (int64_t)sl * (T + 1) * kc * n_s;
    const double* Ub = R.U[kc] + (int64_t)sl * T * kc * n_c;
    for (int q = threadIdx.x; q < (T + 1) * n_s; q += blockDim.x) {
        const int t = q / n_s, c = q - t * n_s;
        X_dec[((int64_t)s * (T + 1) + t) * k * n_s + i * n_s + c] = Xb[(int64_t)t * kc * n_s + pos * n_s + c];
    }
    for (int q = threadIdx.x; q < T * n_c; q += blockDim.x) {
        const int t = q / n_c, c = q - t * n_c;
        U_dec[((int64_t)s * T + t) * k * n_c + i * n_c + c] = Ub[(int64_t)t * kc * n_c + pos * n_c + c];
    }
}

// k_stitch_policy (frontend.hpp: the definition of Kc and U_ff is the comment above it, unchanged) over n_words words: the owner
// looked up across the words, the member list (at most kFrontMaxAgents members, ascending) built from them; kc_max <=
// kFrontMaxAgents (the launcher holds it).  With n_words = 1 Kc and U_ff equal k_stitch_policy's bit for bit.
static __global__ void k_stitch_policy_wide(int S, int k, int n_s, int n_c, int T, int kc_max, int n_words,
                                            const unsigned long long* __restrict__ bits, const int32_t* __restrict__ rep,
                                            const int32_t* __restrict__ size, const int32_t* __restrict__ slot, BucketResults R,
                                            BucketGains G, const double* __restrict__ X_dec, double* __restrict__ Kc,
                                            double* __restrict__ U_ff) {
    const int64_t e = blockIdx.x;             // (s, i)
    if (e >= (int64_t)S * k) return;
    int kc, sl, pos;
    if (!owner_lookup_wide(k, n_words, bits, rep, size, slot, e, kc, sl, pos)) return;
    if (kc > kc_max || kc > kFrontMaxAgents) return;      // no such bucket was solved (the caller refuses the team)
    sl -= R.first[kc];
    if (sl < 0 || sl >= R.count[kc]) return;
    const int s = (int)(e / k), i = (int)(e % k);
    __shared__ int mem[kFrontMaxAgents];
    if (threadIdx.x == 0) {
        for (int p = 0; p < kFrontMaxAgents; ++p) mem[p] = i;      // (a mask with bits at or past k has fewer members than its size)
        mask_members(bits + e * n_words, k, n_words, mem);
    }
    __syncthreads();
    const int nx = kc * n_s, nu = kc * n_c, kw = kc_max * n_s;
    const double* Xb = R.X[kc] + (int64_t)sl * (T + 1) * nx;
    const double* Ub = R.U[kc] + (int64_t)sl * T * nu;
    const double* Kb = G.K[kc] + (int64_t)sl * T * nu * nx;
    for (int q = threadIdx.x; q < T * n_c * kw; q += blockDim.x) {
        const int t = q / (n_c * kw), r = q - t * n_c * kw, c = r / kw, col = r - c * kw;
        Kc[(((int64_t)s * T + t) * k + i) * n_c * kw + r] = col < nx ? Kb[((int64_t)t * nu + pos * n_c + c) * nx + col] : 0.0;
    }
    for (int q = threadIdx.x; q < T * n_c; q += blockDim.x) {
        const int t = q / n_c, c = q - t * n_c;
        const double* Krow = Kb + ((int64_t)t * nu + pos * n_c + c) * nx;
        const double* Xd = X_dec + ((int64_t)s * (T + 1) + t) * k * n_s;
        double sum = 0.0;
        for (int col = 0; col < nx; ++col) {
            const int p = col / n_s;
            sum += Krow[col] * (Xd[mem[p] * n_s + (col - p * n_s)] - Xb[(int64_t)t * nx + col]);
        }
        U_ff[((int64_t)s * T + t) * k * n_c + i * n_c + c] = Ub[(int64_t)t * nu + pos * n_c + c] + sum;
    }
}

}  // namespace dpilqr

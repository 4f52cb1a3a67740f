// lds_sync.hpp -- the workgroup-wide LDS hand-off and the in-order sum of the stage costs, shared by the forward passes
// (forward.hpp) and the closed-loop policy rollout (policy.hpp).
#pragma once
#include <hip/hip_runtime.h>

namespace dpilqr {

// Workgroup-wide LDS hand-off.  A single-wave workgroup executes its LDS operations in order, so a
// compiler fence is enough; larger workgroups use a bare s_barrier behind an LDS-only wait (NOT
// __syncthreads(), whose vmcnt(0) would drain the global prefetches that are meant to stay in flight).
__device__ __forceinline__ void lds_handoff(bool single_wave) {
    if (single_wave) asm volatile("" ::: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// p[0] + p[1] + ... + p[count - 1] added in that order (the reference's stage-cost sums).  One thread per candidate walks 190 pair
// costs at cfg5's size while the rest of its wavefront waits: the loads sixteen at a time and a set AHEAD of the additions (a
// load -> add -> load chain is an LDS round trip per term; eight at a time without the look-ahead: 7 k of a step's 135 k clocks)
template <typename R>
__device__ __forceinline__ R sum_in_order(const R* p, int count) {
    constexpr int W = 16;
    R s = 0.0;
    int i = 0;
    if (count >= 2 * W) {
        R va[W], vb[W];
#pragma unroll
        for (int q = 0; q < W; ++q) va[q] = p[q];
        for (; i + 2 * W <= count; i += 2 * W) {
#pragma unroll
            for (int q = 0; q < W; ++q) vb[q] = p[i + W + q];
#pragma unroll
            for (int q = 0; q < W; ++q) s += va[q];
            // (the set after next; beyond the end it re-reads the array's last full set -- never used)
            const int nx = i + 3 * W <= count ? i + 2 * W : count - W;
#pragma unroll
            for (int q = 0; q < W; ++q) va[q] = p[nx + q];
#pragma unroll
            for (int q = 0; q < W; ++q) s += vb[q];
        }
        if (i + W <= count) {      // va holds p[i .. i + W)
#pragma unroll
            for (int q = 0; q < W; ++q) s += va[q];
            i += W;
        }
    }
    for (; i + 8 <= count; i += 8) {
        R v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = p[i + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; i < count; ++i) s += p[i];
    return s;
}

}  // namespace dpilqr

// wave_util.hpp -- small device helpers shared by the wavefront kernels (riccati_mfma.hpp, riccati_wg.hpp, forward_wave.hpp,
// tiles_wave.hpp): 16-byte values, cross-lane reads, global stores hidden from the wait-count pass, the diagnostic stamp buffer.
#pragma once
#include <hip/hip_runtime.h>

namespace dpilqr {

typedef double v2d __attribute__((ext_vector_type(2)));

#define DPILQR_LDS_FENCE() asm volatile("" ::: "memory")

__device__ __forceinline__ double readlane_f64(double v, int src_lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}

// Global stores issued through inline asm, on purpose.  hipcc's wait-count pass treats a vmcnt with both
// loads and stores pending as out of order and answers every wait on a prefetched load with vmcnt(0),
// which would also wait for loads issued a few instructions earlier.  gfx950 retires vector-memory
// operations in issue order (MI355X guide, s_waitcnt notes), so hiding these fire-and-forget stores from
// the pass keeps its counted vmcnt(N) waits: they merely become conservative by the number of stores
// in flight.  Nothing ever reads the stored data back inside the kernel.
// The trailing s_nop covers the "VMEM store data > 64 bit, then a VALU write of the data VGPRs" hazard: the
// compiler's hazard recogniser does not look inside inline assembly, and the data registers are read a few
// cycles after issue.
__device__ __forceinline__ void store_v2d_nt(double* p, v2d v) {
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 2" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_f64_nt(double* p, double v) {
    asm volatile("global_store_dwordx2 %0, %1, off\n\ts_nop 0" ::"v"(p), "v"(v) : "memory");
}

// Diagnostic stamps (dpilqr_debug_stamps): when a buffer is registered, lane 0 of every sweep workgroup
// records {start, end} of s_memrealtime (100 MHz) and its XCC / CU / SIMD ids.  Never read by any kernel.
static __device__ unsigned long long* g_stamp_buf = nullptr;   // one copy per translation unit (launch.hpp)

constexpr int round_up(int x, int q) { return (x + q - 1) / q * q; }

}  // namespace dpilqr

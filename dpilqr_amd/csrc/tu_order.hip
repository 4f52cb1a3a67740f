// tu_order.hip -- the active list ordered by sweep cost (admit_order.hpp): the key and order kernels and their launchers.
#include <hip/hip_runtime.h>

#define DPILQR_ADMIT_ORDER_KERNELS
#include "admit_order.hpp"
#include "launch.hpp"
#include "riccati_mfma.hpp"   // MfmaCfg: the fused sweep's LDS per wavefront decides its tier

namespace dpilqr {

// Wavefronts per workgroup of the sweep launch_riccati_fused (tu_riccati.hip) makes for grid_items items of this batch, where that
// is the fused four-state wavefront sweep above the team tier; 0 for every other launch (their lists keep their order).
int fused_sweep_tier(const dpilqr_batch_desc& D, int grid_items) {
    if (!fused_wavefront_sweep_applies(D) || grid_items <= kOrderMinLive) return 0;
    const int n = D.k * D.n_s, m = D.k * D.n_c;
#define DPILQR_TIER(NN, MM) \
    if (n == NN && m == MM) return sweep_waves(grid_items, sweep_max_waves(), sizeof(double) * MfmaCfg<NN, MM, true>::total, true);
    DPILQR_TIER(4, 2) DPILQR_TIER(8, 4) DPILQR_TIER(12, 6) DPILQR_TIER(16, 8) DPILQR_TIER(20, 10)
#undef DPILQR_TIER
    return 0;
}

int32_t launch_cost_keys(const dpilqr_batch_desc& D, const double* X, const int32_t* list, const int32_t* count, int grid_items,
                         int min_live, int32_t* key, int32_t* key_dense, hipStream_t st) {
    if (grid_items <= 0) return DPILQR_OK;
    hipLaunchKernelGGL(k_cost_keys, dim3((grid_items + 3) / 4), dim3(256), 0, st, X, D.radius, D.radius_bstride, list, count, D.B, D.T,
                       D.k, min_live, key, key_dense);
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

int32_t launch_order_list(const int32_t* src, int32_t* dst, const int32_t* count, const int32_t* key, int T, int cus, int waves,
                          int order, int min_live, hipStream_t st) {
    hipLaunchKernelGGL(k_order_list, dim3(1), dim3(1024), 0, st, src, dst, count, key, T, cus, waves, order, min_live);
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // namespace dpilqr

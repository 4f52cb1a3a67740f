// tu_bike.hip -- K2 for the five-state family (BikeDynamics5D): the wavefront sweep with in-sweep production
// (riccati_mfma.hpp, PNS = 5) for clusters of at most four bikes, padded into the next instantiated size like CarDynamics3D's
// (tu_inprod.hip delegates n_s = 5 here).  Larger bike clusters (n_x 25..60) take the family-5 tile producer and the record-fed
// sweep of launch_riccati.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "launch.hpp"
#include "riccati_mfma.hpp"

namespace dpilqr {

// (n_rec, m_rec) = k (5, 2) padded into (N, M): A = 1 on the diagonal of the padded states, unit L_uu on the padded controls
template <int N, int M, int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void k_riccati_bike_inprod(
    int B, int T, const double* __restrict__ mu_arr, double* __restrict__ Kout, double* __restrict__ dout,
    int32_t* __restrict__ singular, const int32_t* __restrict__ items, const int32_t* __restrict__ n_items, int gains_by_item,
    int n_cus, FusedArgs F, int n_rec, int m_rec) {
    riccati_mfma_sweep<N, M, WAVES, 0, 0, 0, true, false, 5>(B, T, nullptr, mu_arr, Kout, dout, singular, items, n_items,
                                                             gains_by_item, n_cus, F, n_rec, m_rec);
}

int32_t launch_riccati_bike(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K, double* d,
                            int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items, int gains_by_item,
                            hipStream_t st) {
    if (grid_items <= 0 || D.n_s != 5 || D.n_c != 2 || !fused_wavefront_inprod_applies(D)) return DPILQR_EUNSUPPORTED;
    const int n = D.k * D.n_s, m = D.k * D.n_c;
    const int cus = device_cus();
#define DPILQR_TRY_BIKE(NN, MM)                                                                                    \
    if (n <= NN && m <= MM) {                                                                                      \
        static_assert(MfmaCfg<NN, MM>::supported, "MFMA sweep not available for this size");                       \
        static_assert(NN % 5 != 0 || MM * 5 != NN * InprodCfg<NN, MM, 5>::PNC, "every bike cluster is padded");    \
        constexpr size_t per_wave = sizeof(double) * (MfmaCfg<NN, MM>::total + InprodCfg<NN, MM, 5>::total);       \
        return launch_wave_sweep(k_riccati_bike_inprod<NN, MM, 4>, k_riccati_bike_inprod<NN, MM, 8>, nullptr, per_wave, \
                                 grid_items, cus, st, D.B, D.T, mu, K, d, singular, items, n_items, gains_by_item, cus, \
                                 FusedArgs{D, X, U}, n, m);                                                        \
    }
    // one bike (5, 2) -> (8, 4); two (10, 4) -> (12, 6); three (15, 6) -> (16, 8); four (20, 8) -> (20, 10)
    DPILQR_TRY_BIKE(8, 4) DPILQR_TRY_BIKE(12, 6) DPILQR_TRY_BIKE(16, 8) DPILQR_TRY_BIKE(20, 10)
#undef DPILQR_TRY_BIKE
    return DPILQR_EUNSUPPORTED;
}

}  // namespace dpilqr

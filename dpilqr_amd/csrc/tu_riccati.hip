// tu_riccati.hip -- K2, the Riccati sweeps for n_x <= 60 (riccati_mfma.hpp, riccati_wg.hpp, riccati.hpp), and their launcher.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "launch.hpp"
#include "riccati.hpp"
#include "riccati_mfma.hpp"
#include "riccati_wg.hpp"

namespace dpilqr {

static int riccati_threads(int n) { return n <= 24 ? 64 : (n <= 36 ? 128 : 256); }

// sizes of the wavefront sweeps (one wavefront per sub-problem); everything else takes the workgroup sweep or the generic kernel
#define DPILQR_WAVE_SIZES(X) X(4, 2) X(8, 4) X(12, 6) X(16, 8) X(20, 10)

// Sizes of the workgroup sweep (riccati_wg.hpp), as X(agents, n_s, n_c).  Both forms: four-state models (DoubleInt4D,
// Unicycle4D), 6..15 agents; six-state models (DoubleInt6D, Quadcopter6D, Human6D, HumanLin6D), 2..10 agents
#define DPILQR_WG_SIZES(X)                                                                                      \
    X(6, 4, 2) X(7, 4, 2) X(8, 4, 2) X(9, 4, 2) X(10, 4, 2) X(11, 4, 2) X(12, 4, 2) X(13, 4, 2) X(14, 4, 2) X(15, 4, 2) \
    X(2, 6, 3) X(3, 6, 3) X(4, 6, 3) X(5, 6, 3) X(6, 6, 3) X(7, 6, 3) X(8, 6, 3) X(9, 6, 3) X(10, 6, 3)
// ... and the record-fed form only: Quadcopter12D / the padded human, 2..5 agents; single six- and twelve-state agents (cfg4's
// k = 1 bucket, selfish_warmstart); CarDynamics3D pairs (n_x even)
#define DPILQR_WG_RECORD_SIZES(X) \
    X(2, 12, 4) X(3, 12, 4) X(4, 12, 4) X(5, 12, 4) X(1, 6, 3) X(1, 12, 4) X(2, 3, 2) X(4, 3, 2) X(6, 3, 2)

thread_local int g_sweep_waves = 0;

// one workgroup per sub-problem, record-fed or FUSED; `args` are k_riccati_wg's.  DPILQR_EUNSUPPORTED, without an error text,
// for a size outside the tables above.
template <bool FUSED, typename... Args>
static int32_t launch_riccati_wg(int n, int m, int ns, int nc, int grid_items, hipStream_t st, const Args&... args) {
#define DPILQR_TRY_WG(KK, NS_, NC_)                                                                                 \
    if (ns == NS_ && nc == NC_ && n == KK * NS_ && m == KK * NC_) {                                                 \
        using WC = WgCfg<KK * NS_, KK * NC_, NS_, NC_, FUSED>;                                                      \
        static_assert(WC::supported, "workgroup sweep not available for this size");                                \
        const size_t lds_w = sizeof(double) * WC::total;                                                            \
        auto kern = k_riccati_wg<KK * NS_, KK * NC_, NS_, NC_, FUSED>;                                              \
        int32_t rc_w = allow_lds(kern, lds_w);                                                                      \
        if (rc_w) return rc_w;                                                                                      \
        hipLaunchKernelGGL(kern, dim3(grid_items), dim3(kWgThreads), lds_w, st, args...);                           \
        HIP_TRY(hipGetLastError());                                                                                 \
        return DPILQR_OK;                                                                                           \
    }
    DPILQR_WG_SIZES(DPILQR_TRY_WG)
    if constexpr (!FUSED) {
        DPILQR_WG_RECORD_SIZES(DPILQR_TRY_WG)
    }
#undef DPILQR_TRY_WG
    return DPILQR_EUNSUPPORTED;
}

int32_t launch_riccati(int B, int T, int n, int m, const double* tiles, const double* mu, double* K, double* d,
                       int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items,
                       int gains_by_item, int block_ns, int block_nc, hipStream_t st) {
    g_sweep_waves = 0;
    if (grid_items <= 0) return DPILQR_OK;
    // block_ns > 0: the caller guarantees that [A|B] is block diagonal with block_ns x (block_ns + block_nc) blocks
    // (tiles made by k_make_tiles from a MultiDynamicalModel); 0: arbitrary dense tiles (the plugin boundary).
    static const bool no_bd = route_flag("DPILQR_RICCATI_DENSE");   // A/B switch
    const bool bd = !no_bd && block_ns == 4 && block_nc == 2 && n == 4 * (m / 2) && m % 2 == 0;
    // sweep selection: the matrix-pipe wavefront sweep where instantiated, then the workgroup sweep, else the generic kernel
    // (DPILQR_RICCATI=generic pins the last for A/B measurements)
    static const char* pick_env = route_env("DPILQR_RICCATI");
    static const bool generic = route_flag("DPILQR_FORCE_GENERIC_RICCATI") || (pick_env && !strcmp(pick_env, "generic"));
    // k_riccati_mfma's instantiations for 4 / 8 / 12 wavefronts and its LDS per wavefront, in doubles
    auto wave_sweep = [&](auto k4, auto k8, auto k12, int lds_per_wave) {
        const int cus = device_cus();
        return launch_wave_sweep(k4, k8, k12, sizeof(double) * lds_per_wave, grid_items, cus, st, B, T, tiles, mu, K, d, singular,
                                 items, n_items, gains_by_item, cus, FusedArgs{});
    };
    if (!generic) {
        // three wavefronts per SIMD for block-diagonal tiles only
#define DPILQR_TRY_MFMA(NN, MM)                                                                                    \
    if (n == NN && m == MM) {                                                                                      \
        static_assert(MfmaCfg<NN, MM>::supported, "MFMA sweep not available for this size");                       \
        return bd ? wave_sweep(k_riccati_mfma<NN, MM, 4, 4, 2>, k_riccati_mfma<NN, MM, 8, 4, 2>,                    \
                               k_riccati_mfma<NN, MM, 12, 4, 2>, MfmaCfg<NN, MM>::total)                           \
                  : wave_sweep(k_riccati_mfma<NN, MM, 4, 0, 0>, k_riccati_mfma<NN, MM, 8, 0, 0>, nullptr,          \
                               MfmaCfg<NN, MM>::total);                                                            \
    }
        DPILQR_WAVE_SIZES(DPILQR_TRY_MFMA)
#undef DPILQR_TRY_MFMA
        // n_x = 24 (four six-state or six four-state agents): 19 KB of LDS per wavefront, two per SIMD; the workgroup sweep
        // costs 2.2 ms per 2048 items there, a wavefront per item 0.7 (profiles/r03_small_clusters.txt)
        if (n == 24 && m == 12) {   // the all-MFMA (dense) instantiation only: the block-diagonal lane mapping stops at five agents
            static_assert(MfmaCfg<24, 12>::supported, "MFMA sweep not available for this size");
            return wave_sweep(k_riccati_mfma<24, 12, 4, 0, 0>, k_riccati_mfma<24, 12, 8, 0, 0>, nullptr, MfmaCfg<24, 12>::total);
        }
    }
    // Cluster sizes without a wavefront instantiation of their own (n_x not a multiple of 4: three six-state agents,
    // CarDynamics3D; tiny: one six-state agent; a user plugin's odd sizes): the dense wavefront sweep of the next larger
    // instantiated size, which pads the records while loading them and stores the real block of the gains
    // (riccati_mfma.hpp, PAD).  Before: the workgroup sweep or the generic kernel -- slower than clusters twice the size
    // (profiles/r03_small_clusters.txt: three quadcopters 1.85 ms per 2048 items against 0.89 ms for four).
    static const bool no_pad = route_flag("DPILQR_RICCATI_NO_PAD");   // A/B switch
    // (not two twelve-state agents: n_u = 8 padded to 12 is slower than their workgroup sweep, 1.72 against 1.51 ms per 512 items)
    if (!generic && !no_pad && n <= 24 && m <= 12 && !(block_ns == 12 && n == 24)) {
        const int cus = device_cus();
#define DPILQR_TRY_PAD(NN, MM)                                                                                     \
    if (n <= NN && m <= MM) {                                                                                      \
        static_assert(MfmaCfg<NN, MM>::supported, "MFMA sweep not available for this size");                       \
        return launch_wave_sweep(k_riccati_mfma_pad<NN, MM, 4>, k_riccati_mfma_pad<NN, MM, 8>, nullptr,            \
                                 sizeof(double) * MfmaCfg<NN, MM>::total, grid_items, cus, st, B, T, tiles, mu, K, d, \
                                 singular, items, n_items, gains_by_item, cus, n, m);                              \
    }
        DPILQR_WAVE_SIZES(DPILQR_TRY_PAD)
        DPILQR_TRY_PAD(24, 12)
#undef DPILQR_TRY_PAD
    }
    // larger clusters of the library's own (block-diagonal) tiles: one workgroup per sub-problem, riccati_wg.hpp
    static const bool no_wg = route_flag("DPILQR_RICCATI_NO_WG");   // A/B switch
    if (!generic && !no_wg && block_ns > 0) {
        const int32_t rc_w = launch_riccati_wg<false>(n, m, block_ns, block_nc, grid_items, st, B, T, tiles, mu, K, d, singular,
                                                      items, n_items, gains_by_item, FusedArgs{});
        if (rc_w != DPILQR_EUNSUPPORTED) return rc_w;
    }
    const size_t lds = riccati_lds_bytes(n, m);
    int32_t rc = allow_lds(k_riccati_generic, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_riccati_generic, dim3(grid_items), dim3(riccati_threads(n)), lds, st, B, T, n, m, tiles, mu, K,
                       d, singular, items, n_items, gains_by_item);
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

// The fused sweep (riccati_mfma.hpp, FUSED): no tile records; for batches of DoubleIntDynamics4D agents with one Q, R, Q_f
// for all agents and items and a planar proximity cost (the caller checks the descriptor's hints).  Returns
// DPILQR_EUNSUPPORTED without touching the error text when the shape has no fused instantiation.
int32_t launch_riccati_fused(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K,
                             double* d, int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items,
                             int gains_by_item, hipStream_t st) {
    g_sweep_waves = 0;
    if (grid_items <= 0) return DPILQR_OK;
    const int n = D.k * D.n_s, m = D.k * D.n_c;
    // the six-state family up to four agents, CarDynamics3D up to six: in-sweep production (tu_inprod.hip)
    {
        const int32_t rc_ip = launch_riccati_inprod(D, X, U, mu, K, d, singular, items, n_items, grid_items, gains_by_item, st);
        if (rc_ip != DPILQR_EUNSUPPORTED) return rc_ip;
    }
    // launches of at most one item per SIMD: a team of two wavefronts per item (tu_team.hip)
    if (grid_items <= 1024 && sweep_max_waves() >= 4 && (fused_wavefront_sweep_applies(D) || fused_wavefront_general_applies(D))) {
        const int32_t rc_team = launch_riccati_team(D, X, U, mu, K, d, singular, items, n_items, grid_items, gains_by_item, st);
        if (rc_team != DPILQR_EUNSUPPORTED) return rc_team;
    }
    const int cus = device_cus();
    static const bool no_dec = route_flag("DPILQR_NO_DECOUPLED");   // A/B switch: every step of the DoubleInt4D form densely
#define DPILQR_TRY_FUSED(NN, MM)                                                                                   \
    if (n == NN && m == MM)                                                                                        \
        return launch_wave_sweep(k_riccati_mfma<NN, MM, 4, 4, 2, true>, k_riccati_mfma<NN, MM, 8, 4, 2, true>,     \
                                 k_riccati_mfma<NN, MM, 12, 4, 2, true>, sizeof(double) * MfmaCfg<NN, MM, true>::total, \
                                 grid_items, cus, st, D.B, D.T, nullptr, mu, K, d, singular, items, n_items, gains_by_item, \
                                 cus, FusedArgs{D, X, U, no_dec ? 1 : 0});
    if (fused_wavefront_sweep_applies(D)) {
        DPILQR_WAVE_SIZES(DPILQR_TRY_FUSED)
    }
#undef DPILQR_TRY_FUSED
    // the general form for the four-state family (FUSED == 2): UnicycleDynamics4D, per-agent / per-item weights
#define DPILQR_TRY_FUSED2(NN, MM)                                                                                  \
    if (n == NN && m == MM)                                                                                        \
        return launch_wave_sweep(k_riccati_mfma_general<NN, MM, 4>, k_riccati_mfma_general<NN, MM, 8>, nullptr,    \
                                 sizeof(double) * MfmaCfg<NN, MM, 2>::total, grid_items, cus, st, D.B, D.T, mu, K, d, \
                                 singular, items, n_items, gains_by_item, cus, FusedArgs{D, X, U});
    if (fused_wavefront_general_applies(D)) {
        DPILQR_WAVE_SIZES(DPILQR_TRY_FUSED2)
    }
#undef DPILQR_TRY_FUSED2
    // larger clusters: the workgroup sweep, fused (riccati_wg.hpp): any models of the four- or six-state family
    if (fused_workgroup_sweep_applies(D))
        return launch_riccati_wg<true>(n, m, D.n_s, D.n_c, grid_items, st, D.B, D.T, nullptr, mu, K, d, singular, items, n_items,
                                       gains_by_item, FusedArgs{D, X, U});
    return DPILQR_EUNSUPPORTED;
}

int32_t set_stamp_buffer_riccati(void* buf) {
    void* p = buf;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &p, sizeof(p)));
    return DPILQR_OK;
}

}  // namespace dpilqr

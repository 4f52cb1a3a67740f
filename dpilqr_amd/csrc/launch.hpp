// launch.hpp -- host-side declarations shared by the translation units of libdpilqr_hip.so.
//
// The library is built from several .hip files so that they compile in parallel (one file with every kernel
// instantiation took over two minutes): tu_tiles.hip (K1), tu_riccati.hip (K2), tu_forward.hip (K3, rollouts, the small
// batched entry points), tu_big.hip (the sweep for n_x > 60 and the fp32 arm), tu_bigfwd.hip (their forward passes),
// tu_team.hip (the fused wavefront sweeps with a helper wavefront per item), tu_inprod.hip (the wavefront sweeps with in-sweep
// production), tu_bike.hip (the same for the five-state family, BikeDynamics5D), tu_lsteam.hip (the line search with two
// wavefronts per item), tu_frontend.hip (the device-side dispatch front / back end), tu_policy.hip (the closed-loop ensemble rollouts),
// tu_policy_large.hip (the same for n_x > 60), tu_policy_dec_team.hip (a distributed solution's closed loop for teams of up to
// 64 agents), tu_policy_dec_wide.hip (the same for teams of up to 256), tu_policy_advance.hip (the receding-horizon advance),
// tu_policy_advance_large.hip (the same for n_x > 60), tu_rollout_wide.hip (the
// full-team rollout for up to 256 agents), tu_order.hip (the active list ordered by sweep cost) and dpilqr_hip.hip (the C ABI and
// the solve loop).
// No device code crosses a file boundary.
// The closed-loop units (tu_policy*.hip) share the section "the closed loop" below: the routes' limits as named constants and one
// argument record per kind of entry (PolicyRolloutArgs, PolicyAdvanceArgs) -- the places to change when a limit or an argument does.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "dpilqr_hip.h"
#include "solve_state.hpp"

namespace dpilqr {

int32_t fail(int32_t code, const char* fmt, ...);   // records the calling thread's error message, returns `code`
const char* last_error();

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return ::dpilqr::fail(DPILQR_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int kMaxLds = 160 * 1024;  // gfx950: 160 KiB per workgroup

template <typename Kern>
inline int32_t allow_lds(Kern kern, size_t bytes) {
    if (bytes > (size_t)kMaxLds) return fail(DPILQR_EUNSUPPORTED, "needs %zu B of LDS per workgroup (> %d)", bytes, kMaxLds);
    if (bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return DPILQR_OK;
}

// run `body` with the (NS,NC) family as compile-time constants.  DISPATCH_FAMILY: the families of the large-cluster path
// (tu_big.hip, tu_bigfwd.hip); DISPATCH_FAMILY_ALL adds the five-state family (BikeDynamics5D), which that path does not serve
// (dpilqr_hip.hip rejects bike clusters with n_x > 60 and the fp32 arm for them before any launcher is reached).
#define DISPATCH_FAMILY_CASE(NS_, NC_, ...) case NS_: { constexpr int NS = NS_, NC = NC_; __VA_ARGS__ } break;
#define DISPATCH_FAMILY_CASES(ns, ...)                                                    \
    DISPATCH_FAMILY_CASE(3, 2, __VA_ARGS__)                                               \
    DISPATCH_FAMILY_CASE(4, 2, __VA_ARGS__)                                               \
    DISPATCH_FAMILY_CASE(6, 3, __VA_ARGS__)                                               \
    DISPATCH_FAMILY_CASE(12, 4, __VA_ARGS__)                                              \
    default: return ::dpilqr::fail(DPILQR_EINVAL, "unsupported per-agent state dim %d", (int)(ns));
#define DISPATCH_FAMILY(ns, BODY) switch (ns) { DISPATCH_FAMILY_CASES(ns, BODY) }
#define DISPATCH_FAMILY_ALL(ns, BODY) switch (ns) { DISPATCH_FAMILY_CASE(5, 2, BODY) DISPATCH_FAMILY_CASES(ns, BODY) }

// compute units of the current device (256 on MI355X): the sweep deals its items over rounds of this many workgroups
int device_cus();

// A/B route switches and tuning knobs (DPILQR_NO_FUSED, DPILQR_MFMA_WAVES, DPILQR_BIG_TEAM, ...) exist for experiments and
// tests.  They are honoured only in a process that sets DPILQR_DEBUG_ROUTES=1: without that gate route_env answers null for
// every name, so a stray variable in a production process's environment cannot change which kernel serves a batch.  The gate and
// the library's only getenv live in dpilqr_hip.hip.
const char* route_env(const char* name);
inline bool route_flag(const char* name) { return route_env(name) != nullptr; }
inline int route_int(const char* name, int dflt) { const char* e = route_env(name); return (e && *e) ? atoi(e) : dflt; }

// hints packed into dpilqr_batch_desc::uniform_model (include/dpilqr_hip.h): -1 = unknown / mixed
inline int hint_model(const dpilqr_batch_desc& D) { return (D.uniform_model & 0xff) - 1; }
inline int hint_n_dims(const dpilqr_batch_desc& D) { return ((D.uniform_model >> 8) & 0xff) - 1; }
inline bool hint_shared_weights(const dpilqr_batch_desc& D) { return ((D.uniform_model >> 16) & 1) != 0; }
inline bool hint_planar4(const dpilqr_batch_desc& D) { return ((D.uniform_model >> 17) & 1) != 0 || hint_model(D) == 0 || hint_model(D) == 3; }
// The fused sweeps (no tile records: linearize / quadraticize evaluated inside the sweep).
// Wavefront sweep (n_x <= 20, riccati_mfma.hpp): DoubleIntDynamics4D agents only, planar proximity cost, one Q / R / Q_f for
// every agent of every item (the descriptor's hints), at most five agents.
inline bool fused_wavefront_sweep_applies(const dpilqr_batch_desc& D) {
    static const bool off = route_flag("DPILQR_NO_FUSED");   // A/B switch: the record-fed sweep
    return !off && hint_model(D) == 0 && hint_n_dims(D) == 2 && hint_shared_weights(D) && D.Q_bstride == 0 && D.R_bstride == 0 &&
           D.Qf_bstride == 0 && D.n_s == 4 && D.n_c == 2 && D.k <= 5;
}
// ... and its general form (k_riccati_mfma_general, FUSED == 2): at most five agents of the planar four-state models --
// DoubleIntDynamics4D and UnicycleDynamics4D, mixed or not (the descriptor's hints) -- with any per-agent, per-item Q / R / Q_f,
// planar proximity cost.  Two wavefronts per SIMD at most (the per-agent weights take the LDS the third one needs).
inline bool fused_wavefront_general_applies(const dpilqr_batch_desc& D) {
    static const bool off = route_flag("DPILQR_NO_FUSED") || route_flag("DPILQR_NO_FUSED_GENERAL");
    return !off && hint_planar4(D) && hint_n_dims(D) == 2 && D.n_s == 4 && D.n_c == 2 && D.k <= 5;
}
// Workgroup sweep (riccati_wg.hpp): 6..15 agents of the four-state family or 2..10 of the six-state family -- any models of
// the family, any per-agent weights, any n_dims.
inline bool fused_workgroup_sweep_applies(const dpilqr_batch_desc& D) {
    static const bool off = route_flag("DPILQR_NO_FUSED") || route_flag("DPILQR_NO_FUSED_WG");
    return !off && ((D.n_s == 4 && D.n_c == 2 && D.k >= 6 && D.k <= 15) || (D.n_s == 6 && D.n_c == 3 && D.k >= 2 && D.k <= 10));
}
// Wavefront sweep with in-sweep production (riccati_mfma.hpp, PNS; tu_inprod.hip, tu_bike.hip): at most four agents of the
// six-state family (n_x <= 24), at most six CarDynamics3D agents (n_x <= 18) or at most four BikeDynamics5D agents (n_x <= 20)
// -- any models of the family, any per-agent weights, any n_dims -- padded into the next instantiated size.
inline bool fused_wavefront_inprod_applies(const dpilqr_batch_desc& D) {
    static const bool off = route_flag("DPILQR_NO_FUSED") || route_flag("DPILQR_NO_INPROD");
    static const bool no4 = route_flag("DPILQR_NO_INPROD4");   // A/B switch: the four-state clusters' previous routes
    if (off) return false;
    // ... and what is left of the four-state family at n_x <= 20: at most five agents WITHOUT the hints the forms above need (a
    // proximity cost over three dimensions, mixed models unannounced).  (Six agents, n_x = 24, keep the producer + the
    // record-fed wavefront sweep: a full 2048-item pass is 2.18 ms in-sweep against 1.94 + 1.22, but a whole solve 81.5 against
    // 72.6 ms -- fifteen pairs' derivatives at the top of each of T = 100 steps of a lone wavefront in the solve's long tail;
    // profiles/r04_inprod_four_state.txt)
    if (D.n_s == 4 && D.n_c == 2 && D.k <= 5 && !no4)
        return !fused_wavefront_sweep_applies(D) && !fused_wavefront_general_applies(D);
    return (D.n_s == 6 && D.n_c == 3 && D.k <= 4) || (D.n_s == 3 && D.n_c == 2 && D.k <= 6) || (D.n_s == 5 && D.n_c == 2 && D.k <= 4);
}
inline bool fused_sweep_applies(const dpilqr_batch_desc& D) {
    return fused_wavefront_sweep_applies(D) || fused_wavefront_general_applies(D) || fused_workgroup_sweep_applies(D) ||
           fused_wavefront_inprod_applies(D);
}
// The solve loop's choice where both a record-free workgroup sweep and a record-fed WAVEFRONT sweep serve a batch: at
// n_x = 12 and 24 (two / four six-state agents: cfg4's small clusters; six four-state agents: cfg3's smallest) a wavefront
// per item beats a workgroup per item by more than the tile producer costs.  2048 items, one sweep (profiles/
// r03_small_clusters.txt): n_x = 12 fused workgroup sweep 1.74 ms against producer 0.36 + wavefront sweep 0.26 ms; n_x = 24
// (four quadcopters) 2.67 against 1.01 + 0.88.  Whole solves of 2048 items: two quadcopters 24.3 -> 13.4 ms, four 26.7 -> 20.6,
// six unicycles 86.2 -> 80.6, six double integrators 23.8 -> 21.3.  DPILQR_NO_WAVE_PREF: A/B switch.
inline bool solve_prefers_records(const dpilqr_batch_desc& D) {
    static const bool off = route_flag("DPILQR_NO_WAVE_PREF");
    // round 4: three six-state agents (n_x = 18: 16 % of cfg4's sub-problems) through the (20, 10) wavefront sweep, padded
    // while loading (riccati_mfma.hpp, PAD; DPILQR_RICCATI_NO_PAD switches it off in the launcher)
    // (two .. four six-state agents: records unless the in-sweep producer serves them)
    // (one or two BikeDynamics5D: the producer + the record-fed padded sweep; whole solves of 4096 items 14.6 / 18.8 ms against
    // 17.5 / 20.8 in-sweep -- four bikes the other way, 42.4 against 33.9; profiles/bike_solves.txt)
    if (fused_wavefront_inprod_applies(D)) {
        static const bool rec = route_flag("DPILQR_INPROD_RECORDS");
        return rec || (!off && D.n_s == 5 && D.k <= 2);
    }
    return !off && ((D.n_s == 6 && D.n_c == 3 && (D.k == 2 || D.k == 3 || D.k == 4)) || (D.n_s == 4 && D.n_c == 2 && D.k == 6));
}

// ---- tu_tiles.hip
int32_t launch_make_tiles(const dpilqr_batch_desc& D, const double* X, const double* U, double* tiles,
                          const int32_t* items, const int32_t* n_items, int grid_items, bool sparse, bool dyn_only,
                          hipStream_t st);
int32_t tile_layout_host(int32_t n_x, int32_t n_u, int64_t offsets[7], int64_t row_strides[7], int64_t* stride);

// ---- tu_riccati.hip
extern thread_local int g_sweep_waves;   // wavefronts per workgroup of the last launch_riccati (0: not the wavefront sweep)
int32_t launch_riccati(int B, int T, int n, int m, const double* tiles, const double* mu, double* K, double* d,
                       int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items,
                       int gains_by_item, int block_ns, int block_nc, hipStream_t st);
int32_t launch_riccati_fused(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K,
                             double* d, int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items,
                             int gains_by_item, hipStream_t st);
int32_t set_stamp_buffer_riccati(void* device_buffer);

// ---- the launch of a wavefront sweep (riccati_mfma.hpp), for tu_riccati.hip, tu_inprod.hip, tu_bike.hip and tu_team.hip.
// Wavefronts per workgroup = per CU: 4 (one per SIMD), or 8 / 12 (two / three per SIMD) when the launch has the items for them,
// DPILQR_MFMA_WAVES (max_wv) allows them and they fit the CU's LDS.  tier12: the kernel family has a 12-wavefront
// instantiation for this launch (the record-fed sweep: for block-diagonal tiles only).
constexpr int sweep_waves(int grid_items, int max_wv, size_t lds_per_wave, bool tier12) {
    return (tier12 && grid_items > 2048 && max_wv >= 12 && lds_per_wave * 12 <= (size_t)kMaxLds) ? 12
           : (grid_items > 1024 && max_wv >= 8 && lds_per_wave * 8 <= (size_t)kMaxLds) ? 8 : 4;
}
// whole rounds of one workgroup per CU; the kernel deals the live items over them (riccati_mfma.hpp)
constexpr int sweep_grid(int grid_items, int cus, int wv) {
    return grid_items <= cus ? grid_items : (grid_items + cus * wv - 1) / (cus * wv) * cus;
}
inline int sweep_max_waves() { static const int v = route_int("DPILQR_MFMA_WAVES", 12); return v; }
// one instantiation, `wv` sweeping wavefronts per workgroup of `threads`; `args` are the kernel's, `cus` among them
template <typename Kern, typename... Args>
int32_t launch_sweep_kernel(Kern kern, int wv, int threads, size_t lds, int grid_items, int cus, hipStream_t st, const Args&... args) {
    const int32_t rc = allow_lds(kern, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(sweep_grid(grid_items, cus, wv)), dim3(threads), lds, st, args...);
    HIP_TRY(hipGetLastError());
    g_sweep_waves = wv;
    return DPILQR_OK;
}
// a kernel family's instantiations for 4, 8 and 12 wavefronts (k12 = nullptr: none); lds_per_wave in bytes
template <typename T> struct same_type { using type = T; };
template <typename Kern, typename... Args>
int32_t launch_wave_sweep(Kern k4, typename same_type<Kern>::type k8, typename same_type<Kern>::type k12, size_t lds_per_wave,
                          int grid_items, int cus, hipStream_t st, const Args&... args) {
    const int wv = sweep_waves(grid_items, sweep_max_waves(), lds_per_wave, k12 != nullptr);
    return launch_sweep_kernel(wv == 12 ? k12 : (wv == 8 ? k8 : k4), wv, 64 * wv, lds_per_wave * wv, grid_items, cus, st, args...);
}
// ---- tu_team.hip: the fused wavefront sweeps with a helper wavefront per item, for launches of at most 1024 items
int32_t launch_riccati_team(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K, double* d,
                            int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items, int gains_by_item,
                            hipStream_t st);

// ---- tu_inprod.hip: the wavefront sweeps with in-sweep production (six-state family up to four agents, CarDynamics3D up to six)
int32_t launch_riccati_inprod(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K, double* d,
                              int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items, int gains_by_item,
                              hipStream_t st);

// ---- tu_bike.hip: the wavefront sweep with in-sweep production for at most four BikeDynamics5D agents (tu_inprod.hip delegates
// n_s = 5 to it); DPILQR_EUNSUPPORTED, without an error text, for any other batch
int32_t launch_riccati_bike(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K, double* d,
                            int32_t* singular, const int32_t* items, const int32_t* n_items, int grid_items, int gains_by_item,
                            hipStream_t st);

// ---- tu_order.hip: the active list ordered by sweep cost (admit_order.hpp), for the fused four-state wavefront sweep above the
// team tier.  fused_sweep_tier: wavefronts per workgroup of the sweep launch_riccati_fused makes for grid_items items, 0 for every
// launch whose list keeps its order.  cost_keys: key[pos] = near-step count of the item at list position pos (list / count null:
// the batch in index order), key_dense[pos] = its last near step + 1 (either may be null); order_list: dst = src sorted by key class, heaviest first, dealt by `order` (CostOrder); both leave
// lists of at most min_live items as they are (order_list copies them).
int fused_sweep_tier(const dpilqr_batch_desc& D, int grid_items);
int32_t launch_cost_keys(const dpilqr_batch_desc& D, const double* X, const int32_t* list, const int32_t* count, int grid_items,
                         int min_live, int32_t* key, int32_t* key_dense, hipStream_t st);
int32_t launch_order_list(const int32_t* src, int32_t* dst, const int32_t* count, const int32_t* key, int T, int cus, int waves,
                          int order, int min_live, hipStream_t st);

// ---- tu_lsteam.hip: the line search with two wavefronts per item (rollout / costs), for launches of at most 1024 items
int32_t launch_linesearch_team(const dpilqr_batch_desc& D, double* X, double* U, const double* K, const double* d,
                               const double* alphas, double* Xc, double* Uc, const SolveState& S, const int32_t* items,
                               const int32_t* n_items, int grid_items, hipStream_t st);

// ---- tu_forward.hip
int32_t launch_forward(const dpilqr_batch_desc& D, int mode, const double* x0, double* X, double* U, const double* K,
                       const double* d, const double* alphas, int ngrp, double* Xc, double* Uc, double* Jc,
                       const SolveState& S, const int32_t* items, const int32_t* n_items, int grid_items,
                       hipStream_t st);
int32_t set_stamp_buffer_forward(void* device_buffer);
int32_t launch_model_op(int op, int32_t n, int32_t ns, const int32_t* model, const double* x, const double* u, double dt,
                        double* o1, double* o2, hipStream_t st);
int32_t launch_cost_eval(const dpilqr_batch_desc& D, int32_t n_pts, const double* x, const double* u, int32_t terminal,
                         double* cost, hipStream_t st);
int32_t launch_pairwise_graph(int32_t S, int32_t N, int32_t k, int32_t n_s, const double* X, const double* radius,
                              int32_t* adj, hipStream_t st);


// ---- the closed loop (include/dpilqr_policy.h): the ensemble rollouts and the receding-horizon advances.  This section is the
// C side's one statement of the routes and of the argument lists -- a further entry, or another limit, is made here and in the
// route table of dpilqr_amd/batch.py (ROUTES), which tests/test_closed_loop_routes_host.py holds to the launchers' answers.
// The routes: small -- n_x <= kRouteSmallMaxNx and k <= kRouteSmallMaxK (tu_policy.hip, tu_policy_advance.hip); large --
// kRouteSmallMaxNx < n_x <= kRouteLargeMaxNx, k <= kRouteLargeMaxK, the (4, 2), (6, 3), (12, 4) families (tu_policy_large.hip,
// tu_policy_advance_large.hip, whose kernels are built for these bounds: policy_large.hpp); team -- k <= kPolicyTeamAgents
// (policy_dec_team.hpp: one mask word), whatever n_x is.
constexpr int kRouteSmallMaxNx = 60, kRouteSmallMaxK = 20, kRouteLargeMaxNx = 240, kRouteLargeMaxK = 20;

// The plan an entry executes: X, U and the gains.  Dense gains K[B][T][n_u][n_x]: kc_max = 0, nbr_bits null; neighbourhood gains
// Kc[B][T][k][n_c][kc_max * n_s] with the masks nbr_bits[B][k] (policy_dec.hpp).
struct PolicyPlan {
    const double *X, *U, *K;
    int32_t kc_max;
    const uint64_t* nbr_bits;
};
// One record per kind, filled once by the extern "C" entry and unpacked at the kernel launch: a rollout's ...
struct PolicyRolloutArgs {
    PolicyPlan plan;
    int32_t n_samples;
    const double *x0s, *W, *u_lim;                   // W, u_lim may be null
    double *Xs, *Us, *J, *min_sep, *goal_dist;       // all but J may be null
};
// ... and an advance's (K, scen, W, u_lim may be null)
struct PolicyAdvanceArgs {
    PolicyPlan plan;
    int32_t h;
    const int32_t* scen;
    int32_t n_scen, L, n_d;
    const double *W, *u_lim;
    double* x_cur;
    int32_t* n_done;
    double *X_exec, *U_exec, *J_exec, *min_sep, *dist_left, *U_next, *X_next;
};
inline int32_t check_kc_max(const char* who, const dpilqr_batch_desc& D, int32_t kc_max) {
    return kc_max >= 1 && kc_max <= D.k ? DPILQR_OK
                                        : fail(DPILQR_EUNSUPPORTED, "%s: kc_max=%d, a neighbourhood has 1 .. k = %d members", who, kc_max, D.k);
}

// tu_policy.hip: S closed-loop samples per item under u = U + K (x - X) (policy.hpp); the small route, enqueue only
int32_t launch_policy_rollout(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st);
// ... and of a distributed solution: u_i = U_ff_i + Kc_i (x - X_dec) over agent i's neighbourhood nbr_bits[b][i] (policy_dec.hpp)
int32_t launch_policy_rollout_dec(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st);
// tu_policy_dec_team.hip: the same closed loop for a whole team of up to 64 agents at any n_x, a thread per (sample, agent), the
// gains read straight from global memory (policy_dec_team.hpp); enqueue only
int32_t launch_policy_rollout_dec_team(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st);
// tu_policy_dec_wide.hip: the same closed loop for a team of up to 256 agents, the masks nbr_bits[B][k][n_words] of
// n_words = ceil(k / 64) words, a neighbourhood of at most 64 members (policy_dec_team.hpp at four mask words); enqueue only
int32_t launch_policy_rollout_dec_wide(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, int32_t n_words, hipStream_t st);
// tu_policy_large.hip: the dense rollout on the large route, K[t] dx on the matrix pipe (policy_large.hpp); enqueue only
int32_t launch_policy_rollout_large(const dpilqr_batch_desc& D, const PolicyRolloutArgs& a, hipStream_t st);
// tu_policy_advance.hip: the step between two solves of a receding-horizon loop (policy_advance.hpp): h steps of every running
// scenario's plan, floor(256 / k) items per workgroup, with the loop's bookkeeping; dense or neighbourhood gains; enqueue only
int32_t launch_policy_advance(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, hipStream_t st);
// tu_policy_advance_dec_team.hip: the same step under a distributed solution's policy for a whole team of up to 64 agents at
// any n_x, a thread per (item, agent), the team rollout's arithmetic (policy_advance_dec_team.hpp); Kc null: open loop; enqueue only
int32_t launch_policy_advance_dec_team(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, hipStream_t st);
// tu_policy_advance_dec_wide.hip: the same step for a team of up to 256 agents, the masks nbr_bits[B][k][n_words] of
// n_words = ceil(k / 64) words, a neighbourhood of at most 64 members (policy_advance_dec_team.hpp at four mask words); Kc null:
// open loop; enqueue only
int32_t launch_policy_advance_dec_wide(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, int32_t n_words, hipStream_t st);
// tu_policy_advance_large.hip: the advance on the large route, dense gains, one workgroup per item, K[i] dx on the matrix pipe
// (policy_advance_large.hpp); enqueue only
int32_t launch_policy_advance_large(const dpilqr_batch_desc& D, const PolicyAdvanceArgs& a, hipStream_t st);

// ---- tu_rollout_wide.hip: dpilqr_rollout's definition for a full team of up to 256 agents, one workgroup per item
// (rollout_wide.hpp); X, min_sep, goal_dist may be null; enqueue only
int32_t launch_rollout_wide(const dpilqr_batch_desc& D, const double* x0, const double* U, double* X, double* J, double* min_sep,
                            double* goal_dist, hipStream_t st);

// ---- tu_big.hip: large clusters (n_x > 60) in fp64, any size in fp32 (BASELINE config 5's tolerance study)
int64_t riccati_big_scratch_elems(int n, int m);   // per sub-problem in flight, in elements of the arithmetic type
int32_t launch_riccati_big_f64(const dpilqr_batch_desc& D, const double* X, const double* U, const double* mu, double* K,
                               double* d, int32_t* singular, const int32_t* items, const int32_t* n_items,
                               int grid_items, int gains_by_item, void* scratch, hipStream_t st);
int32_t launch_riccati_big_f32(const dpilqr_batch_desc& D, const float* X, const float* U, const double* mu, float* K,
                               float* d, int32_t* singular, const int32_t* items, const int32_t* n_items,
                               int grid_items, int gains_by_item, void* scratch, hipStream_t st);
int32_t launch_forward_big_f64(const dpilqr_batch_desc& D, int mode, const double* x0, double* X, double* U, const double* K,
                               const double* d, const double* alphas, int ngrp, double* Xc, double* Uc, double* Jc,
                               const SolveState& S, const int32_t* items, const int32_t* n_items, int grid_items,
                               hipStream_t st);
int32_t launch_forward_big_f32(const dpilqr_batch_desc& D, int mode, const float* x0, float* X, float* U, const float* K,
                               const float* d, const double* alphas, int ngrp, float* Xc, float* Uc, double* Jc,
                               const SolveState& S, const int32_t* items, const int32_t* n_items, int grid_items,
                               hipStream_t st);
// the sweep's choice: clusters beyond the wavefront / workgroup sweeps (n_x > 60) take the fused big kernel
inline bool uses_big_path(int n_x) {
    static const bool force = route_flag("DPILQR_FORCE_BIG");   // test / A-B switch: every size through tu_big.hip
    return force || n_x > 60;
}

}  // namespace dpilqr

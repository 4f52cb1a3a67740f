// tu_trial_inputs.hip -- C ABI of the Monte-Carlo study's input generator (trial_inputs.hpp): dpilqr_trial_inputs.
#include <hip/hip_runtime.h>

#include <vector>

#include "dpilqr_hip.h"
#define DPILQR_TRIAL_INPUTS_KERNELS
#include "trial_inputs.hpp"
#include "launch.hpp"

using namespace dpilqr;

static_assert(DPILQR_MAX_TEAM == kTrialMaxAgents, "the generator serves the teams the wide entries serve");
static_assert(DPILQR_TRIAL_INPUTS_LDS == kTrialLdsBytes, "the LDS the header states");

extern "C" {

int32_t dpilqr_trial_inputs(int32_t S, int64_t seed0, const int64_t* seeds, int32_t k, int32_t n_s, int32_t n_d, double var,
                            double energy, int32_t n_warm, int32_t N, int32_t n_u, double warm_scale, double* x0, double* xf,
                            double* U_a, double* U_b, void* stream) {
    if (S < 0) return fail(DPILQR_EINVAL, "trial_inputs: S=%d", S);
    if (k < 1 || k > kTrialMaxAgents) return fail(DPILQR_EINVAL, "trial_inputs: k=%d, the generator serves 1 .. %d agents", k, kTrialMaxAgents);
    if (n_d < 1 || n_d > kTrialMaxDims || n_d > n_s)
        return fail(DPILQR_EINVAL, "trial_inputs: n_d=%d, positions have 1 .. %d coordinates and at most n_s = %d", n_d, kTrialMaxDims, n_s);
    if (n_warm < 0 || n_warm > 2) return fail(DPILQR_EINVAL, "trial_inputs: n_warm=%d, a trial draws 0, 1 or 2 warm starts", n_warm);
    if (n_warm > 0 && (N < 1 || n_u < 1)) return fail(DPILQR_EINVAL, "trial_inputs: a warm start of N=%d by n_u=%d", N, n_u);
    if (!x0 || !xf || (n_warm >= 1 && !U_a) || (n_warm >= 2 && !U_b))
        return fail(DPILQR_EINVAL, "trial_inputs: a NULL output (x0, xf, and U_a / U_b as n_warm=%d requires)", n_warm);
    if (!seeds && (seed0 < 0 || seed0 + (int64_t)S > 0x100000000ll))
        return fail(DPILQR_EINVAL, "trial_inputs: seeds %lld .. %lld, np.random.seed takes [0, 2^32)", (long long)seed0,
                    (long long)(seed0 + S - 1));
    if (S == 0) return DPILQR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (seeds) {      // the caller's seeds are device memory: read them back once, this form of the call is not enqueue-only
        std::vector<int64_t> h((size_t)S);
        HIP_TRY(hipMemcpyAsync(h.data(), seeds, sizeof(int64_t) * (size_t)S, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int32_t s = 0; s < S; ++s)
            if (h[s] < 0 || h[s] > 0xffffffffll)
                return fail(DPILQR_EINVAL, "trial_inputs: seeds[%d]=%lld, np.random.seed takes [0, 2^32)", s, (long long)h[s]);
    }
    hipLaunchKernelGGL(k_trial_inputs, dim3((unsigned)((S + kTrialWaves - 1) / kTrialWaves)), dim3(kTrialThreads), 0, st, S, seed0, seeds,
                       k, n_s, n_d, var, energy, n_warm, N, n_u, warm_scale, x0, xf, U_a, U_b);
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // extern "C"

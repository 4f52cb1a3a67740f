// tu_separated_setup.hip -- C ABI of the separated scenarios (separated_setup.hpp): dpilqr_setup_separate.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dpilqr_hip.h"
#define DPILQR_SEPARATED_SETUP_KERNELS
#include "separated_setup.hpp"
#include "launch.hpp"

using namespace dpilqr;

static_assert(DPILQR_MAX_TEAM == kTrialMaxAgents, "the loop serves the teams the generator serves");
static_assert(DPILQR_SETUP_SEPARATE_MAX_ITER == kSepMaxIter, "the cap the header states");
static_assert(DPILQR_SETUP_SEPARATE_LDS == (int)sizeof(SepLds), "the LDS the header states");

extern "C" {

int32_t dpilqr_setup_separate(int32_t S, int32_t k, int32_t n_s, int32_t n_d, double rel_dist, double energy, int32_t max_iter,
                              double* x0, double* xf, int32_t* n_iter, void* stream) {
    if (S < 0) return fail(DPILQR_EINVAL, "setup_separate: S=%d", S);
    if (k < kSepMinAgents || k > kTrialMaxAgents)
        return fail(DPILQR_EINVAL, "setup_separate: k=%d, the loop serves %d .. %d agents (no pairwise distance for one agent)", k,
                    kSepMinAgents, kTrialMaxAgents);
    if (n_d < 1 || n_d > kTrialMaxDims || n_d > n_s)
        return fail(DPILQR_EINVAL, "setup_separate: n_d=%d, positions have 1 .. %d coordinates and at most n_s = %d", n_d, kTrialMaxDims, n_s);
    if (max_iter < 1 || max_iter > kSepMaxIter) return fail(DPILQR_EINVAL, "setup_separate: max_iter=%d, expected 1 .. %d", max_iter, kSepMaxIter);
    if (!x0 || !xf || !n_iter) return fail(DPILQR_EINVAL, "setup_separate: a NULL pointer (x0, xf, n_iter)");
    if (std::isnan(rel_dist)) return fail(DPILQR_EINVAL, "setup_separate: rel_dist is NaN");
    if (S == 0) return DPILQR_OK;
    hipLaunchKernelGGL(k_setup_separate, dim3((unsigned)S, 2u), dim3(kSepThreads), 0, reinterpret_cast<hipStream_t>(stream), k, n_s, n_d,
                       rel_dist, energy, max_iter, x0, xf, n_iter);
    HIP_TRY(hipGetLastError());
    return DPILQR_OK;
}

}  // extern "C"

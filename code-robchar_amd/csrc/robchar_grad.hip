// librobchar_hip.so, third translation unit: the fidelity-gradient kernels (k_fidelity_grad.inc.h, N = 2 .. RC_MAX_NSPIN_GRAD)
// and the noise-sensitivity kernels (k_fidelity_sens.inc.h; k_fidelity_sens_philox.inc.h: the same with the counter-based draws
// generated inside the kernel; same range), the gradient kernel that generates its draws (k_fidelity_grad_philox.inc.h) and
// that kernel on a grid of readout times (k_fidelity_grad_times_philox.inc.h),
// compiled in parallel with robchar_hip.hip and robchar_large.hip (`make -j`).  The host side and the C ABI are in
// robchar_hip.hip, which reaches the launches below through hidden entry points.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/robchar_hip.h"
#include "kernel_params.h"
#include "grad_core.h"
#include "grad_times_core.h"
#include "sens_core.h"

namespace {

using rckp::GradParams;
using rckp::GradPhiloxParams;
using rckp::GradListedParams;
using rckp::GradTimesParams;
using rckp::SensParams;
using rckp::SensPhiloxParams;
#include "tile_stage.inc.h"

// tiles in which some sample's QL hit the sweep cap and took the textbook routine (diagnostic; rare path only); counted by
// mc_fid_grad_kernel, mc_fid_grad_philox_kernel, mc_fid_grad_times_philox_kernel and mc_fid_grad_listed_kernel
__device__ unsigned long long g_grad_general_tiles = 0;

// the same for mc_fid_sens_kernel and mc_fid_sens_philox_kernel
__device__ unsigned long long g_sens_general_tiles = 0;

#include "k_fidelity_grad.inc.h"
#include "k_fidelity_sens.inc.h"
#include "philox_core.inc.h"
#include "k_fidelity_sens_philox.inc.h"
#include "k_fidelity_grad_philox.inc.h"
#include "k_fidelity_grad_times_philox.inc.h"
#include "k_fidelity_grad_listed.inc.h"

}  // namespace

// Defines  hipError_t NAME(int N, hipStream_t s, const PARAMS& p):  enqueues KERNEL<N>, N = 2 .. RC_MAX_NSPIN_GRAD, one wave per tile.
static_assert(RC_MAX_NSPIN_GRAD == 12, "RC_LAUNCH_2_TO_12 instantiates every kernel of this unit for every N up to RC_MAX_NSPIN_GRAD");
#define RC_LAUNCH_CASE(KERNEL, n) \
    case n: hipLaunchKernelGGL(KERNEL<n>, dim3((unsigned)p.ntiles), dim3(64), 0, s, p); break;
#define RC_LAUNCH_2_TO_12(NAME, KERNEL, PARAMS)                                                                                    \
    static hipError_t NAME(int N, hipStream_t s, const PARAMS& p) {                                                               \
        switch (N) {                                                                                                              \
            RC_LAUNCH_CASE(KERNEL, 2) RC_LAUNCH_CASE(KERNEL, 3) RC_LAUNCH_CASE(KERNEL, 4) RC_LAUNCH_CASE(KERNEL, 5)               \
            RC_LAUNCH_CASE(KERNEL, 6) RC_LAUNCH_CASE(KERNEL, 7) RC_LAUNCH_CASE(KERNEL, 8) RC_LAUNCH_CASE(KERNEL, 9)               \
            RC_LAUNCH_CASE(KERNEL, 10) RC_LAUNCH_CASE(KERNEL, 11) RC_LAUNCH_CASE(KERNEL, 12)                                      \
            default: return hipErrorInvalidValue;                                                                                 \
        }                                                                                                                         \
        return hipGetLastError();                                                                                                 \
    }
RC_LAUNCH_2_TO_12(launch_grad, mc_fid_grad_kernel, rckp::GradParams)
RC_LAUNCH_2_TO_12(launch_sens, mc_fid_sens_kernel, rckp::SensParams)
RC_LAUNCH_2_TO_12(launch_sens_philox, mc_fid_sens_philox_kernel, rckp::SensPhiloxParams)
RC_LAUNCH_2_TO_12(launch_grad_philox, mc_fid_grad_philox_kernel, rckp::GradPhiloxParams)
RC_LAUNCH_2_TO_12(launch_grad_listed, mc_fid_grad_listed_kernel, rckp::GradListedParams)
RC_LAUNCH_2_TO_12(launch_grad_times_philox, mc_fid_grad_times_philox_kernel, rckp::GradTimesParams)
#undef RC_LAUNCH_2_TO_12
#undef RC_LAUNCH_CASE

// The second pass behind a launch that went well (`first`): the row means of the `nent` entries of the part rows into `mean`
// [C][nent], or - `moments`: the part rows carry the moment sums too - into `mean` and / or `moment`.  Nothing without `part`.
static int launch_row_means(hipError_t first, hipStream_t s, const double* part, double* mean, double* moment, bool moments, int nent,
                            long long tiles_per_ctrl, long long K, long long C) {
    if (first != hipSuccess || !part || !(moments || mean)) return (int)first;
    if (moments)
        hipLaunchKernelGGL(mc_fid_grad_moment_mean_kernel, dim3((unsigned)C), dim3(64), 0, s, part, mean, moment, tiles_per_ctrl, nent,
                           K);
    else
        hipLaunchKernelGGL(mc_fid_grad_mean_kernel, dim3((unsigned)C), dim3(64), 0, s, part, mean, tiles_per_ctrl, nent, K);
    return (int)hipGetLastError();
}

extern "C" {

// Each enqueues its kernel and - when p->part is set - the second pass of the row means: [C][N+2] for the gradients, [C][3N+2] for
// the sensitivities.  They return the hipError_t of the launches.
__attribute__((visibility("hidden"))) int rc_grad_launch(int N, void* s, const rckp::GradParams* p, double* mean) {
    return launch_row_means(launch_grad(N, (hipStream_t)s, *p), (hipStream_t)s, p->part, mean, nullptr, false, N + 2,
                            p->tiles_per_ctrl, p->K, p->C);
}
__attribute__((visibility("hidden"))) int rc_sens_launch(int N, void* s, const rckp::SensParams* p, double* mean) {
    return launch_row_means(launch_sens(N, (hipStream_t)s, *p), (hipStream_t)s, p->part, mean, nullptr, false, 3 * N + 2,
                            p->tiles_per_ctrl, p->K, p->C);
}
__attribute__((visibility("hidden"))) int rc_sens_philox_launch(int N, void* s, const rckp::SensPhiloxParams* p, double* mean) {
    return launch_row_means(launch_sens_philox(N, (hipStream_t)s, *p), (hipStream_t)s, p->part, mean, nullptr, false, 3 * N + 2,
                            p->tiles_per_ctrl, p->K, p->C);
}
// (p->moments: the part rows also carry the sums of F^2 and F dF/dx, for `moment`)
__attribute__((visibility("hidden"))) int rc_grad_philox_launch(int N, void* s, const rckp::GradPhiloxParams* p, double* mean,
                                                                double* moment) {
    return launch_row_means(launch_grad_philox(N, (hipStream_t)s, *p), (hipStream_t)s, p->part, mean, moment, p->moments != 0,
                            N + 2, p->tiles_per_ctrl, p->K, p->C);
}
// (the same second pass: the part rows carry the sums of W, dW/dx and - p->moments - of W^2, W dW/dx)
__attribute__((visibility("hidden"))) int rc_grad_times_philox_launch(int N, void* s, const rckp::GradTimesParams* p, double* mean,
                                                                      double* moment) {
    return launch_row_means(launch_grad_times_philox(N, (hipStream_t)s, *p), (hipStream_t)s, p->part, mean, moment, p->moments != 0,
                            N + 2, p->tiles_per_ctrl, p->K, p->C);
}

// (the part rows carry the WEIGHTED sums over the listed slots; `sum` [C][N+2] is their row sum: the second pass with K = 1, whose
// division by 1.0 is exact)
__attribute__((visibility("hidden"))) int rc_grad_listed_launch(int N, void* s, const rckp::GradListedParams* p, double* sum) {
    return launch_row_means(launch_grad_listed(N, (hipStream_t)s, *p), (hipStream_t)s, p->part, sum, nullptr, false, N + 2,
                            p->tiles_per_ctrl, 1, p->C);
}

// device address of g_grad_general_tiles
__attribute__((visibility("hidden"))) int rc_grad_counter_addr(void** addr) {
    return (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_grad_general_tiles));
}
__attribute__((visibility("hidden"))) int rc_sens_counter_addr(void** addr) {
    return (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_sens_general_tiles));
}

}  // extern "C"

// librobchar_hip.so, third translation unit: the fidelity-gradient kernels (k_fidelity_grad.inc.h, N = 2 .. RC_MAX_NSPIN_GRAD)
// and the noise-sensitivity kernels (k_fidelity_sens.inc.h; k_fidelity_sens_philox.inc.h: the same with the counter-based draws
// generated inside the kernel; same range), and the gradient kernel that generates its draws (k_fidelity_grad_philox.inc.h),
// compiled in parallel with robchar_hip.hip and robchar_large.hip (`make -j`).  The host side and the C ABI are in
// robchar_hip.hip, which reaches the launches below through hidden entry points.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/robchar_hip.h"
#include "kernel_params.h"
#include "grad_core.h"
#include "sens_core.h"

namespace {

using rckp::GradParams;
using rckp::GradPhiloxParams;
using rckp::SensParams;
using rckp::SensPhiloxParams;
typedef __attribute__((address_space(1))) const void* rc_gptr_t;
typedef __attribute__((address_space(3))) void* rc_lptr_t;

// tiles in which some sample's QL hit the sweep cap and took the textbook routine (diagnostic; rare path only); counted by
// mc_fid_grad_kernel and mc_fid_grad_philox_kernel
__device__ unsigned long long g_grad_general_tiles = 0;

// the same for mc_fid_sens_kernel and mc_fid_sens_philox_kernel
__device__ unsigned long long g_sens_general_tiles = 0;

#include "k_fidelity_grad.inc.h"
#include "k_fidelity_sens.inc.h"
#include "philox_core.inc.h"
#include "k_fidelity_sens_philox.inc.h"
#include "k_fidelity_grad_philox.inc.h"

}  // namespace

extern "C" {

// Enqueues mc_fid_grad_kernel<N> and - when p.part is set - the second pass of the row means into `mean`.  Returns the
// hipError_t of the launches.
__attribute__((visibility("hidden"))) int rc_grad_launch(int N, void* stream, const rckp::GradParams* pp, double* mean) {
    const GradParams& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.ntiles);
    switch (N) {
#define RC_GRAD_CASE(n) \
    case n: hipLaunchKernelGGL(mc_fid_grad_kernel<n>, grid, dim3(64), 0, s, p); break;
        RC_GRAD_CASE(2) RC_GRAD_CASE(3) RC_GRAD_CASE(4) RC_GRAD_CASE(5) RC_GRAD_CASE(6) RC_GRAD_CASE(7) RC_GRAD_CASE(8)
        RC_GRAD_CASE(9) RC_GRAD_CASE(10) RC_GRAD_CASE(11) RC_GRAD_CASE(12)
#undef RC_GRAD_CASE
        default: return (int)hipErrorInvalidValue;
    }
    static_assert(RC_MAX_NSPIN_GRAD == 12, "instantiate mc_fid_grad_kernel for every N up to RC_MAX_NSPIN_GRAD");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (p.part && mean) {
        hipLaunchKernelGGL(mc_fid_grad_mean_kernel, dim3((unsigned)p.C), dim3(64), 0, s, (const double*)p.part, mean,
                           p.tiles_per_ctrl, N + 2, p.K);
        e = hipGetLastError();
    }
    return (int)e;
}

// Enqueues mc_fid_sens_kernel<N> and - when p.part is set - the second pass of the row means into `mean` [C][3N+2].
__attribute__((visibility("hidden"))) int rc_sens_launch(int N, void* stream, const rckp::SensParams* pp, double* mean) {
    const SensParams& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.ntiles);
    switch (N) {
#define RC_SENS_CASE(n) \
    case n: hipLaunchKernelGGL(mc_fid_sens_kernel<n>, grid, dim3(64), 0, s, p); break;
        RC_SENS_CASE(2) RC_SENS_CASE(3) RC_SENS_CASE(4) RC_SENS_CASE(5) RC_SENS_CASE(6) RC_SENS_CASE(7) RC_SENS_CASE(8)
        RC_SENS_CASE(9) RC_SENS_CASE(10) RC_SENS_CASE(11) RC_SENS_CASE(12)
#undef RC_SENS_CASE
        default: return (int)hipErrorInvalidValue;
    }
    static_assert(RC_MAX_NSPIN_GRAD == 12, "instantiate mc_fid_sens_kernel for every N up to RC_MAX_NSPIN_GRAD");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (p.part && mean) {
        hipLaunchKernelGGL(mc_fid_grad_mean_kernel, dim3((unsigned)p.C), dim3(64), 0, s, (const double*)p.part, mean,
                           p.tiles_per_ctrl, 3 * N + 2, p.K);
        e = hipGetLastError();
    }
    return (int)e;
}

// Enqueues mc_fid_sens_philox_kernel<N> and - when p.part is set - the same second pass of the row means.
__attribute__((visibility("hidden"))) int rc_sens_philox_launch(int N, void* stream, const rckp::SensPhiloxParams* pp, double* mean) {
    const SensPhiloxParams& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.ntiles);
    switch (N) {
#define RC_SENS_CASE(n) \
    case n: hipLaunchKernelGGL(mc_fid_sens_philox_kernel<n>, grid, dim3(64), 0, s, p); break;
        RC_SENS_CASE(2) RC_SENS_CASE(3) RC_SENS_CASE(4) RC_SENS_CASE(5) RC_SENS_CASE(6) RC_SENS_CASE(7) RC_SENS_CASE(8)
        RC_SENS_CASE(9) RC_SENS_CASE(10) RC_SENS_CASE(11) RC_SENS_CASE(12)
#undef RC_SENS_CASE
        default: return (int)hipErrorInvalidValue;
    }
    static_assert(RC_MAX_NSPIN_GRAD == 12, "instantiate mc_fid_sens_philox_kernel for every N up to RC_MAX_NSPIN_GRAD");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (p.part && mean) {
        hipLaunchKernelGGL(mc_fid_grad_mean_kernel, dim3((unsigned)p.C), dim3(64), 0, s, (const double*)p.part, mean,
                           p.tiles_per_ctrl, 3 * N + 2, p.K);
        e = hipGetLastError();
    }
    return (int)e;
}

// Enqueues mc_fid_grad_philox_kernel<N> and - when p.part is set - the second pass: mc_fid_grad_mean_kernel into `mean` for the
// row means alone, mc_fid_grad_moment_mean_kernel into `mean` and / or `moment` when the part rows carry the moment sums.
__attribute__((visibility("hidden"))) int rc_grad_philox_launch(int N, void* stream, const rckp::GradPhiloxParams* pp, double* mean,
                                                                double* moment) {
    const GradPhiloxParams& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.ntiles);
    switch (N) {
#define RC_GRAD_CASE(n) \
    case n: hipLaunchKernelGGL(mc_fid_grad_philox_kernel<n>, grid, dim3(64), 0, s, p); break;
        RC_GRAD_CASE(2) RC_GRAD_CASE(3) RC_GRAD_CASE(4) RC_GRAD_CASE(5) RC_GRAD_CASE(6) RC_GRAD_CASE(7) RC_GRAD_CASE(8)
        RC_GRAD_CASE(9) RC_GRAD_CASE(10) RC_GRAD_CASE(11) RC_GRAD_CASE(12)
#undef RC_GRAD_CASE
        default: return (int)hipErrorInvalidValue;
    }
    static_assert(RC_MAX_NSPIN_GRAD == 12, "instantiate mc_fid_grad_philox_kernel for every N up to RC_MAX_NSPIN_GRAD");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (p.part && p.moments) {
        hipLaunchKernelGGL(mc_fid_grad_moment_mean_kernel, dim3((unsigned)p.C), dim3(64), 0, s, (const double*)p.part, mean, moment,
                           p.tiles_per_ctrl, N + 2, p.K);
        e = hipGetLastError();
    } else if (p.part && mean) {
        hipLaunchKernelGGL(mc_fid_grad_mean_kernel, dim3((unsigned)p.C), dim3(64), 0, s, (const double*)p.part, mean,
                           p.tiles_per_ctrl, N + 2, p.K);
        e = hipGetLastError();
    }
    return (int)e;
}

// device address of g_grad_general_tiles
__attribute__((visibility("hidden"))) int rc_grad_counter_addr(void** addr) {
    return (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_grad_general_tiles));
}
__attribute__((visibility("hidden"))) int rc_sens_counter_addr(void** addr) {
    return (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_sens_general_tiles));
}

}  // extern "C"

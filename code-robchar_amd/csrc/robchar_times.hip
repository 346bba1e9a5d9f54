// librobchar_hip.so, fourth translation unit: the kernels of the fidelity on a grid of readout times (k_fidelity_times.inc.h,
// N = 2 .. RC_MAX_NSPIN_FAST: the tensor kernel and the one that generates its draws), compiled in parallel with robchar_hip.hip,
// robchar_large.hip and robchar_grad.hip (`make -j`).  The host side and the C ABI are in robchar_hip.hip, which reaches the
// launches below through hidden entry points.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/robchar_hip.h"
#include "kernel_params.h"
#include "times_core.h"

namespace {

using rckp::TimesParams;
#include "tile_stage.inc.h"

// tiles in which some sample's QL hit the sweep cap and took the textbook routine (diagnostic; rare path only); counted by
// mc_fid_times_kernel and mc_fid_times_philox_kernel
__device__ unsigned long long g_times_general_tiles = 0;

#include "philox_core.inc.h"
#include "k_fidelity_times.inc.h"

}  // namespace

// Defines  hipError_t NAME(int N, hipStream_t s, const TimesParams& p):  enqueues KERNEL<N>, N = 2 .. RC_MAX_NSPIN_FAST, one wave per tile.
static_assert(RC_MAX_NSPIN_FAST == 16, "RC_LAUNCH_2_TO_16 instantiates both kernels of this unit for every N up to RC_MAX_NSPIN_FAST");
#define RC_LAUNCH_CASE(KERNEL, n) \
    case n: hipLaunchKernelGGL(KERNEL<n>, dim3((unsigned)p.ntiles), dim3(64), 0, s, p); break;
#define RC_LAUNCH_2_TO_16(NAME, KERNEL)                                                                                          \
    static hipError_t NAME(int N, hipStream_t s, const rckp::TimesParams& p) {                                                   \
        switch (N) {                                                                                                             \
            RC_LAUNCH_CASE(KERNEL, 2) RC_LAUNCH_CASE(KERNEL, 3) RC_LAUNCH_CASE(KERNEL, 4) RC_LAUNCH_CASE(KERNEL, 5)              \
            RC_LAUNCH_CASE(KERNEL, 6) RC_LAUNCH_CASE(KERNEL, 7) RC_LAUNCH_CASE(KERNEL, 8) RC_LAUNCH_CASE(KERNEL, 9)              \
            RC_LAUNCH_CASE(KERNEL, 10) RC_LAUNCH_CASE(KERNEL, 11) RC_LAUNCH_CASE(KERNEL, 12) RC_LAUNCH_CASE(KERNEL, 13)          \
            RC_LAUNCH_CASE(KERNEL, 14) RC_LAUNCH_CASE(KERNEL, 15) RC_LAUNCH_CASE(KERNEL, 16)                                     \
            default: return hipErrorInvalidValue;                                                                                \
        }                                                                                                                        \
        return hipGetLastError();                                                                                                \
    }
RC_LAUNCH_2_TO_16(launch_times, mc_fid_times_kernel)
RC_LAUNCH_2_TO_16(launch_times_philox, mc_fid_times_philox_kernel)
#undef RC_LAUNCH_2_TO_16
#undef RC_LAUNCH_CASE

extern "C" {

// Each enqueues its kernel and returns the hipError_t of the launch.
__attribute__((visibility("hidden"))) int rc_times_launch(int N, void* s, const rckp::TimesParams* p) {
    return (int)launch_times(N, (hipStream_t)s, *p);
}
__attribute__((visibility("hidden"))) int rc_times_philox_launch(int N, void* s, const rckp::TimesParams* p) {
    return (int)launch_times_philox(N, (hipStream_t)s, *p);
}
// device address of g_times_general_tiles
__attribute__((visibility("hidden"))) int rc_times_counter_addr(void** addr) {
    return (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_times_general_tiles));
}
}  // extern "C"

// librobchar_hip.so, sixth translation unit: the variance indices - the pick-freeze fidelity kernel that generates its two draw
// vectors itself (k_fidelity_pickfreeze.inc.h, N = 2 .. RC_MAX_NSPIN_PICKFREEZE) and the second pass of its row means, compiled
// in parallel with the other units (`make -j`).  The host side and the C ABI are in robchar_hip.hip, which reaches the launch
// below through a hidden entry point.  Device globals (tables, the diagnostic tile counters) exist once per unit:
// rc_stats_general_tiles / rc_stats_polish_tiles add this unit's copies.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/robchar_hip.h"
#include "kernel_params.h"
#include "tridiag_core.h"
#include "hermitian_core.h"

namespace {

using rckp::StaticH;
using rckp::FidParams;
using rckp::RingRepairList;
using rckp::PickFreezeParams;
#include "tile_stage.inc.h"

#include "k_fidelity_chain.inc.h"                  // LdsVec, the counters, philox_core.inc.h (the generator and its tables)
#include "k_fidelity_pickfreeze.inc.h"

}  // namespace

static_assert(RC_MAX_NSPIN_PICKFREEZE == 13, "the switch below instantiates mc_fid_pickfreeze_philox_kernel for N = 2 .. 13");
static_assert(3 * RC_MAX_NSPIN_PICKFREEZE <= 64, "a group is a 64-bit mask over the 3 N coordinates");

extern "C" {

// Enqueues the kernel and - when p->part is set - the second pass of the row means into mean [C][3 + 2 G]; returns the hipError_t
// of the launches.  ends: the end-to-end weights mode (the same choice as enqueue_fidelity's, so that the slabs stay bit-identical
// to the tensor route)
__attribute__((visibility("hidden"))) int rc_vidx_pickfreeze_launch(int N, int ends, void* stream, const rckp::PickFreezeParams* pp,
                                                                    double* mean) {
    const PickFreezeParams& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.ntiles);
    switch (N) {
#define RC_CASE(n)                                                                                                          \
    case n:                                                                                                                 \
        if (ends) hipLaunchKernelGGL((mc_fid_pickfreeze_philox_kernel<n, rc::kWeightsEnds>), grid, dim3(64), 0, s, p);      \
        else hipLaunchKernelGGL((mc_fid_pickfreeze_philox_kernel<n, rc::kWeightsAdjugate>), grid, dim3(64), 0, s, p);       \
        break;
        RC_CASE(2) RC_CASE(3) RC_CASE(4) RC_CASE(5) RC_CASE(6) RC_CASE(7) RC_CASE(8) RC_CASE(9)
        RC_CASE(10) RC_CASE(11) RC_CASE(12) RC_CASE(13)
#undef RC_CASE
        default: return (int)hipErrorInvalidValue;
    }
    const hipError_t first = hipGetLastError();
    if (first != hipSuccess || !p.part || !mean) return (int)first;
    hipLaunchKernelGGL(mc_fid_pickfreeze_mean_kernel, dim3((unsigned)p.C), dim3(64), 0, s, p.part, mean, p.tiles_per_ctrl, 3 + 2 * p.G,
                       p.K);
    return (int)hipGetLastError();
}

// device address of this unit's copy of a diagnostic counter: 0 = g_general_tiles, 1 = g_polish_tiles
__attribute__((visibility("hidden"))) int rc_vidx_counter_addr(int which, void** addr) {
    return which == 0 ? (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_general_tiles))
                      : (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_polish_tiles));
}

}  // extern "C"

// librobchar_hip.so, fifth translation unit: randomised quasi-Monte Carlo - the scrambled Sobol generator (k_draws_sobol.inc.h)
// and the chain fidelity kernel that generates its Sobol normals itself (k_fidelity_sobol.inc.h, N = 2 .. RC_MAX_NSPIN_SOBOL),
// compiled in parallel with the other units (`make -j`).  The host side and the C ABI are in robchar_hip.hip, which reaches the
// launches below through hidden entry points.  Device globals (tables, the diagnostic tile counters) exist once per unit:
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
#include "tile_stage.inc.h"

#include "k_fidelity_chain.inc.h"                  // fid_min_waves, LdsVec, the counters, philox_core.inc.h (ln_table, the tables)
#include "sobol_core.h"
#include "k_draws_sobol.inc.h"
#include "k_fidelity_sobol.inc.h"

}  // namespace

static_assert(RC_MAX_NSPIN_SOBOL == 13, "the switch below instantiates mc_fid_chain_sobol_kernel for N = 2 .. 13");
static_assert(3 * RC_MAX_NSPIN_SOBOL <= 64, "sobol_tile_base: one lane per dimension in the fidelity kernel");

extern "C" {

// Each enqueues its kernel and returns the hipError_t of the launch.
__attribute__((visibility("hidden"))) int rc_qmc_draws_launch(void* stream, const rckp::SobolDraws* qp, long long C, long long K,
                                                              double* draws, unsigned int* bits) {
    const SobolDraws& q = *qp;
    const long long tiles_per_row = (K + 63) / 64;
    hipLaunchKernelGGL(sobol_draws_kernel, dim3((unsigned)(C * tiles_per_row)), dim3(64), 0, (hipStream_t)stream, q, K, tiles_per_row,
                       draws, bits);
    return (int)hipGetLastError();
}

// ends: the end-to-end weights mode (the same choice as enqueue_fidelity's, so that the two routes stay bit-identical)
__attribute__((visibility("hidden"))) int rc_qmc_fidelity_launch(int N, int ends, void* stream, const rckp::FidParams* pp,
                                                                 const rckp::SobolDraws* qp) {
    const FidParams& p = *pp;
    const SobolDraws& q = *qp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.ntiles);
    switch (N) {
#define RC_CASE(n)                                                                                                     \
    case n:                                                                                                            \
        if (ends) hipLaunchKernelGGL((mc_fid_chain_sobol_kernel<n, rc::kWeightsEnds>), grid, dim3(64), 0, s, p, q);    \
        else hipLaunchKernelGGL((mc_fid_chain_sobol_kernel<n, rc::kWeightsAdjugate>), grid, dim3(64), 0, s, p, q);     \
        break;
        RC_CASE(2) RC_CASE(3) RC_CASE(4) RC_CASE(5) RC_CASE(6) RC_CASE(7) RC_CASE(8) RC_CASE(9)
        RC_CASE(10) RC_CASE(11) RC_CASE(12) RC_CASE(13)
#undef RC_CASE
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

// device address of this unit's copy of a diagnostic counter: 0 = g_general_tiles, 1 = g_polish_tiles
__attribute__((visibility("hidden"))) int rc_qmc_counter_addr(int which, void** addr) {
    return which == 0 ? (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_general_tiles))
                      : (int)hipGetSymbolAddress(addr, HIP_SYMBOL(g_polish_tiles));
}

}  // extern "C"

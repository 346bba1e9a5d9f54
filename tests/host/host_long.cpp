// Host build of the long-chain arithmetic (code-robchar_amd/csrc/tridiag_core.h) for CPU unit tests: ONE chain length per
// library, chosen with -DRC_HOST_N=<17 .. 24>, in the general adjugate mode - what mc_fid_chain_kernel<N, kWeightsAdjugate>
// (robchar_large.hip) runs for every (in, out) pair.  One translation unit per N so that the test can compile them in parallel.
// TEST HARNESS ONLY: the product never loads this library.
#include "../../code-robchar_amd/csrc/tridiag_core.h"

#ifndef RC_HOST_N
#error "compile with -DRC_HOST_N=<chain length>"
#endif

static long long g_general_calls = 0;
static const double g_sctab[128] = {RC_SINCOS_TABLE_VALUES};

extern "C" int rc_host_long_n(void) { return RC_HOST_N; }
extern "C" long long rc_host_long_general_calls(void) { return g_general_calls; }

// same contract as rc_host_chain_fidelity (host_core.cpp) for N = RC_HOST_N; a sample the fast path rejects takes the general
// per-sample routine (the kernel's last resort at N >= 17: there is no in-register rows-mode repair there) and is counted
extern "C" int rc_host_long_chain_fidelity(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                           long long C, long long K, int in, int out, double* fid) {
    constexpr int kN = RC_HOST_N;
    if (N != kN) return -1;
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* g = draws + (c * K + k) * 3 * kN;
            auto lg = [g](int j) { return g[j]; };
            double f;
            if (!rc::chain_fidelity_fast<kN, rc::kWeightsAdjugate>(ctrl + c * (kN + 1), h0d, h0o, lg, in, out, g_sctab, f)) {
                double w[4][32];
                f = rc::chain_fidelity_general<double*>(kN, ctrl + c * (kN + 1), h0d, h0o, g, in, out, w[0], w[1], w[2], w[3]);
                ++g_general_calls;
            }
            fid[c * K + k] = f;
        }
    return 0;
}

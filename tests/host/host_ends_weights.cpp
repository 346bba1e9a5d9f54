// Host build of chain_fidelity_fast<N, kWeightsEnds, AMPLITUDE> for both values of AMPLITUDE: true = the fidelity without
// weights (rc::ends_amplitude, what the chain kernels run up to N = 13), false = the weights + phase loop (rc::ends_weights,
// what the directional kernel and N >= 14 keep).  TEST HARNESS ONLY: the product never loads this library.
#include "../../code-robchar_amd/csrc/tridiag_core.h"

static const double g_sctab[128] = {RC_SINCOS_TABLE_VALUES};

template <int N, bool AMPLITUDE>
static long long run(const double* ctrl, const double* h0d, const double* h0o, const double* draws, long long C, long long K,
                     double* fid) {
    long long left = 0;                            // samples that reported "not ok" (the kernels would repair them)
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* g = draws + (c * K + k) * 3 * N;
            double f;
            const bool ok = rc::chain_fidelity_fast<N, rc::kWeightsEnds, AMPLITUDE>(ctrl + c * (N + 1), h0d, h0o,
                                                                                    [g](int j) { return g[j]; }, 0, N - 1, g_sctab, f);
            left += ok ? 0 : 1;
            fid[c * K + k] = f;
        }
    return left;
}

// returns the number of samples that left the fast path, -1 for an N without an instantiation
extern "C" long long rc_host_ends_fidelity(int N, int amplitude, const double* ctrl, const double* h0d, const double* h0o,
                                           const double* draws, long long C, long long K, double* fid) {
    switch (N) {
#define CASE(n) case n: return amplitude ? run<n, true>(ctrl, h0d, h0o, draws, C, K, fid) : run<n, false>(ctrl, h0d, h0o, draws, C, K, fid);
        CASE(3) CASE(5) CASE(7) CASE(8) CASE(9) CASE(10) CASE(13)
#undef CASE
    }
    return -1;
}

// Host build of the per-sample arithmetic of the readout-time kernels (code-robchar_amd/csrc/times_core.h) for CPU unit tests,
// beside the rows mode of chain_fidelity_fast it must agree with bit for bit.  TEST HARNESS ONLY: the product never loads this
// library.
#include "../../code-robchar_amd/csrc/times_core.h"

static const double g_tab[128] = {RC_SINCOS_TABLE_VALUES};
static long long g_general_calls = 0;
extern "C" long long rc_host_times_general_calls(void) { return g_general_calls; }

// force_general: 0 = the kernels' order (fast QL, textbook routine for a sample whose QL hit the sweep cap), 1 = the textbook
// routine for every sample.  fid [M][C][K], wsum [C][K], fmin [C][K]; tscale / tshift / weights [M] or NULL.
template <int N>
static void run(const double* ctrl, const double* h0d, const double* h0o, const double* draws, long long cstride, long long C,
                long long K, int in, int out, int force_general, int M, const double* tscale, const double* tshift,
                const double* weights, double* fid, double* wsum, double* fmin) {
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* x = ctrl + c * (N + 1);
            const double* g = draws + c * cstride + k * 3 * N;
            double* slab0 = fid + c * K + k;
            const long long slab = C * K;
            auto store = [slab0, slab](int j, double f) { slab0[j * slab] = f; };
            rc::TimesAcc acc{0.0, 0.0};
            double dl[N], w[N];
            bool ok = false;
            if (!force_general) ok = rc::times_eigen_fast<N>(x, h0d, h0o, [g](int j) { return g[j]; }, in, out, dl, w);
            if (ok) {
                rc::times_loop_fast<N>(dl, w, x[N], M, tscale, tshift, weights, g_tab, store, acc);
            } else {
                double d[N], e[N], za[N], zb[N];
                rc::times_general(N, x, h0d, h0o, g, in, out, (double*)d, (double*)e, (double*)za, (double*)zb, M, tscale, tshift,
                                  weights, store, acc);
                ++g_general_calls;
            }
            wsum[c * K + k] = acc.wsum;
            fmin[c * K + k] = acc.fmin;
        }
}

// chain_fidelity_fast<N, kWeightsRows> (what mc_fid_chain_kernel runs for kernel = RC_KERNEL_TRIDIAG_QL) with x[N] = the row's time
template <int N>
static int run_rows(const double* ctrl, const double* h0d, const double* h0o, const double* draws, long long cstride, long long C,
                    long long K, int in, int out, double* fid) {
    int bad = 0;
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* g = draws + c * cstride + k * 3 * N;
            double f = 0.0;
            if (!rc::chain_fidelity_fast<N, rc::kWeightsRows>(ctrl + c * (N + 1), h0d, h0o, [g](int j) { return g[j]; }, in, out, g_tab, f))
                ++bad;
            fid[c * K + k] = f;
        }
    return bad;
}

#define ALL_N CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)

extern "C" int rc_host_chain_fidelity_times(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                            long long cstride, long long C, long long K, int in, int out, int force_general, int M,
                                            const double* tscale, const double* tshift, const double* weights, double* fid,
                                            double* wsum, double* fmin) {
    switch (N) {
#define CASE(n) case n: run<n>(ctrl, h0d, h0o, draws, cstride, C, K, in, out, force_general, M, tscale, tshift, weights, fid, wsum, fmin); return 0;
        ALL_N
#undef CASE
    }
    return -1;
}

// returns the number of samples whose fast path reported failure (0 expected), -1 for an N outside 2 .. 16
extern "C" int rc_host_chain_fidelity_rows(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                           long long cstride, long long C, long long K, int in, int out, double* fid) {
    switch (N) {
#define CASE(n) case n: return run_rows<n>(ctrl, h0d, h0o, draws, cstride, C, K, in, out, fid);
        ALL_N
#undef CASE
    }
    return -1;
}

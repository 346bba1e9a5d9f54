// Host build of the per-sample time loop of the gradient kernel on a grid of readout times
// (code-robchar_amd/csrc/grad_times_core.h) for CPU unit tests, beside the single-time host arithmetic of host_grad.cpp
// (rc_host_chain_fidelity_grad), which the tests evaluate per grid time as the yardstick.  TEST HARNESS ONLY.
#include "host_grad.cpp"
#include "../../code-robchar_amd/csrc/grad_times_core.h"

// rc_host_chain_fidelity_grad with the call of gradient_from_eigensystem replaced by the loop over the grid: wfid [C][K],
// wgrad [C][K][N + 1].  tscale / tshift may be NULL.
template <int N>
static void run_times(const double* ctrl, const double* h0d, const double* h0o, const double* draws, long long cstride, long long C,
                      long long K, int in, int out, int force_general, int M, const double* tscale, const double* tshift,
                      const double* weights, double* fid, double* grad) {
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* x = ctrl + c * (N + 1);
            const double* g = draws + c * cstride + k * 3 * N;
            constexpr int R = rc::grad_batch_rows(N);
            double d0[N], e0[N];
            rc::grad_load_matrix<N>(x, h0d, h0o, [g](int j) { return g[j]; }, d0, e0);
            for (int pass = 0; pass < rc::grad_passes(N); ++pass) {
                int site[R];
                rc::grad_pass_rows<N>(in, out, pass, site);
                rc::TriEig<N, R> s;
                bool ok = false;
                if (!force_general) ok = rc::grad_eigensystem_fast<N, R>(d0, e0, site, s);
                if (!ok) {
                    double d[N], e[N], z[N * N];
                    rc::grad_eigensystem_general<N, R>(x, h0d, h0o, g, site, (double*)d, (double*)e, HostMat{z, N}, s);
                }
                rc::GradTimesRegs<R> acc;
                rc::gradient_times_from_eigensystem<N, R, true>(s, x[N], in == out, rc::GridPointers{M, tscale, tshift, weights}, acc);
                double* gout = grad + (c * K + k) * (N + 1);
                for (int l = 0; l <= R; ++l) {
                    const int col = rc::grad_result_column<N>(site, pass, l);
                    if (col >= 0) gout[col] = acc.get(l);
                }
                if (pass == 0) fid[c * K + k] = acc.get(R + 1);
            }
        }
}

extern "C" int rc_host_chain_fidelity_grad_times(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                                 long long cstride, long long C, long long K, int in, int out, int force_general,
                                                 int M, const double* tscale, const double* tshift, const double* weights,
                                                 double* fid, double* grad) {
    switch (N) {
#define CASE(n) \
    case n: run_times<n>(ctrl, h0d, h0o, draws, cstride, C, K, in, out, force_general, M, tscale, tshift, weights, fid, grad); return 0;
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12)
#undef CASE
    }
    return -1;
}

// Host build of the per-sample arithmetic of the fidelity-gradient kernel (code-robchar_amd/csrc/grad_core.h) for CPU unit
// tests.  TEST HARNESS ONLY: the product never loads this library.
#include "../../code-robchar_amd/csrc/grad_core.h"

static long long g_general_calls = 0;
extern "C" long long rc_host_grad_general_calls(void) { return g_general_calls; }

namespace {
struct HostMat {            // z(q, i) of tridiag_qln_general on a plain array
    double* base;
    int n;
    double& operator()(int q, int i) const { return base[q * n + i]; }
};
}  // namespace

// force_general: 0 = the kernel's order (fast QL, textbook routine for a sample whose QL hit the sweep cap), 1 = the textbook
// routine for every sample
template <int N>
static void run(const double* ctrl, const double* h0d, const double* h0o, const double* draws, long long cstride, long long C,
                long long K, int in, int out, int force_general, double* fid, double* grad) {
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* x = ctrl + c * (N + 1);
            const double* g = draws + c * cstride + k * 3 * N;
            constexpr int R = rc::grad_batch_rows(N);
            double d0[N], e0[N];
            rc::grad_load_matrix<N>(x, h0d, h0o, [g](int j) { return g[j]; }, d0, e0);
            bool counted = false;
            for (int pass = 0; pass < rc::grad_passes(N); ++pass) {
                int site[R];
                rc::grad_pass_rows<N>(in, out, pass, site);
                rc::TriEig<N, R> s;
                bool ok = false;
                if (!force_general) ok = rc::grad_eigensystem_fast<N, R>(d0, e0, site, s);
                if (!ok) {
                    double d[N], e[N], z[N * N];
                    rc::grad_eigensystem_general<N, R>(x, h0d, h0o, g, site, (double*)d, (double*)e, HostMat{z, N}, s);
                    if (!counted) ++g_general_calls;
                    counted = true;
                }
                double f, gr[R + 1];
                rc::gradient_from_eigensystem<N, R>(s, x[N], in == out, f, gr);
                double* gout = grad + (c * K + k) * (N + 1);
                for (int l = 0; l <= R; ++l) {
                    const int col = rc::grad_result_column<N>(site, pass, l);
                    if (col >= 0) gout[col] = gr[l];
                }
                if (pass == 0) fid[c * K + k] = f;
            }
        }
}

extern "C" int rc_host_chain_fidelity_grad(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                           long long cstride, long long C, long long K, int in, int out, int force_general,
                                           double* fid, double* grad) {
    switch (N) {
#define CASE(n) case n: run<n>(ctrl, h0d, h0o, draws, cstride, C, K, in, out, force_general, fid, grad); return 0;
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12)
#undef CASE
    }
    return -1;
}

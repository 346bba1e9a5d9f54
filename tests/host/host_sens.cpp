// Host build of the per-sample arithmetic of the noise-sensitivity kernel (code-robchar_amd/csrc/sens_core.h) for CPU unit
// tests.  TEST HARNESS ONLY: the product never loads this library.
#include "../../code-robchar_amd/csrc/sens_core.h"

static long long g_general_calls = 0;
extern "C" long long rc_host_sens_general_calls(void) { return g_general_calls; }

namespace {
struct HostMat {            // z(q, i) of tridiag_qln_general on a plain array
    double* base;
    int n;
    double& operator()(int q, int i) const { return base[q * n + i]; }
};
}  // namespace

// The kernel's order of work on one sample at a time.  force_general: 0 = fast QL (textbook routine for a sample whose QL hit the
// sweep cap), 1 = the textbook routine for every sample.  writes[c][k][N][3] counts how many passes produced every entry.
template <int N>
static void run(const double* ctrl, const double* h0d, const double* h0o, const double* draws, long long cstride, long long C,
                long long K, int in, int out, int force_general, double* fid, double* sens, double* rho, int* writes) {
    constexpr int R = rc::sens_batch_rows(N);
    for (long long c = 0; c < C; ++c)
        for (long long k = 0; k < K; ++k) {
            const double* x = ctrl + c * (N + 1);
            const double* g = draws + c * cstride + k * 3 * N;
            double* so = sens + (c * K + k) * 3 * N;
            int* wr = writes + (c * K + k) * 3 * N;
            double d0[N], e0[N];
            rc::grad_load_matrix<N>(x, h0d, h0o, [g](int j) { return g[j]; }, d0, e0);
            so[1] = so[2] = 0.0;
            double r = 0.0;
            bool counted = false;
            for (int pass = 0; pass < rc::sens_passes(N); ++pass) {
                int site[R];
                rc::sens_pass_rows<N>(in, out, pass, site);
                rc::TriEig<N, R> s;
                bool ok = false;
                if (!force_general) ok = rc::grad_eigensystem_fast<N, R>(d0, e0, site, s);
                if (!ok) {
                    double d[N], e[N], z[N * N];
                    rc::grad_eigensystem_general<N, R>(x, h0d, h0o, g, site, (double*)d, (double*)e, HostMat{z, N}, s);
                    if (!counted) ++g_general_calls;
                    counted = true;
                }
                double f, ds[R], dr[R];
                rc::sens_from_eigensystem<N, R>(s, site, in, out, x[N], f, ds, dr);
                for (int q = 0; q < R; ++q) {
                    bool wsite, wbond;
                    rc::sens_row_writes<N>(site, pass, q, wsite, wbond);
                    const int i = site[q];
                    if (wsite) {
                        so[3 * i] = ds[q];
                        ++wr[3 * i];
                        r = fma(g[3 * i], ds[q], r);
                    }
                    if (wbond) {
                        double cr, ci;
                        rc::sens_unit_phase(h0o[i - 1] + g[3 * i + 1], g[3 * i + 2], cr, ci);
                        so[3 * i + 1] = cr * dr[q];
                        so[3 * i + 2] = ci * dr[q];
                        ++wr[3 * i + 1];
                        ++wr[3 * i + 2];
                        r = fma(g[3 * i + 1], so[3 * i + 1], fma(g[3 * i + 2], so[3 * i + 2], r));
                    }
                }
                if (pass == 0) fid[c * K + k] = f;
            }
            rho[c * K + k] = r;
        }
}

extern "C" int rc_host_chain_fidelity_sens(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                           long long cstride, long long C, long long K, int in, int out, int force_general,
                                           double* fid, double* sens, double* rho, int* writes) {
    switch (N) {
#define CASE(n) case n: run<n>(ctrl, h0d, h0o, draws, cstride, C, K, in, out, force_general, fid, sens, rho, writes); return 0;
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12)
#undef CASE
    }
    return -1;
}

extern "C" int rc_host_sens_passes(int N) {
    switch (N) {
#define CASE(n) case n: return rc::sens_passes(n);
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12)
#undef CASE
    }
    return -1;
}

// Per-sample arithmetic of the chain-topology fidelity GRADIENT kernel (one sample per lane): the fidelity
//   F = |phi|^2,  phi = [exp(-i T H)]_{out,in},  T = |x_N|,  H = HH + Z(draws) + diag(x_0 .. x_{N-1})
// and its derivatives with respect to the N biases and the time entry x_N of the controller.
//
// Route.  After the diagonal gauge of tridiag_core.h, H is real symmetric tridiagonal (d, e) and dH/dx_l = |l><l| is
// untouched by the gauge.  With H = V diag(lam) V^T (rows of V accumulated through the all-fp64 implicit QL,
// tridiag_ql2_fast<N, R>: genuine eigenvectors, so no condition on the eigenvalue gaps and none on cut bonds),
// p_k = exp(-i T lam_k):
//     phi        = sum_k V[out,k] V[in,k] p_k
//     dphi/dx_l  = sum_{j,k} V[out,j] V[l,j] Gam_jk V[l,k] V[in,k]
//                = sum_k  vo_k vi_k Gam_kk V[l,k]^2  +  sum_{j<k} (vo_j vi_k + vo_k vi_j) Gam_jk V[l,j] V[l,k]
//     Gam_jk     = -i T exp(-i T (lam_j + lam_k)/2) sinc(T (lam_j - lam_k)/2),       Gam_kk = -i T p_k
//     dphi/dT    = -i sum_k lam_k vo_k vi_k p_k
//     dF/dx_l    = 2 Re(conj(phi) dphi/dx_l),   dF/dx_N = sign(x_N) 2 Re(conj(phi) dphi/dT)   (0 at x_N = 0).
// The divided difference (p_j - p_k)/(lam_j - lam_k) is never formed: the sinc form is exact down to lam_j = lam_k.
// Cost per sample beyond the QL: N half-angle sincos (exp(-i T lam_k / 2): the pair phases are their products), one sine
// per pair, and 2 N operations per pair for the N bias entries (the real scalar 2 Re(conj(phi) Gam_jk (..)) times
// V[l,j] V[l,k]).
// The matrix is shifted by the mean of its diagonal before the QL: F and every derivative are unchanged by H -> H - c
// (a global phase; the time entry picks up 2 Re(conj(phi) i c phi) = 0), and the eigenvalues' absolute rounding error -
// which T multiplies - then scales with the SPREAD of the spectrum instead of its offset (biases of 1e3).
//
// Registers.  The N^2 doubles of V do not fit beside the rest from N = 10 (512 VGPRs = 256 doubles per lane at one wave per
// SIMD), and dF/dx_l needs only ROW l of V beside the rows `out` and `in`.  So the QL runs in passes over batches of
// R = grad_batch_rows(N) rows: every pass carries the rows out, in and R - 2 further sites through the same sweeps (the
// rotations are recomputed: 17 of the 17 + 4 R operations of a rotation) and is self-contained - its own eigenvalues, its own
// rows -, so nothing has to agree between passes.  N <= 9: one pass with all rows.
//
// A lane whose QL runs into the sweep cap of the fast path (not observed) reports false; the kernel then recomputes the
// eigensystem of such lanes with the textbook per-sample routine (eigensystem_general: per-sample window, runtime
// loops, vectors in LDS) and every lane goes through the same gradient arithmetic (gradient_from_eigensystem).
//
// Plain C++ like tridiag_core.h: tests/host/host_grad.cpp compiles exactly this for the CPU.
#pragma once
#include "tridiag_core.h"

// -DRC_GRAD_FORCE_GENERAL=1 (scripts/build_variant.sh): the fast QL reports failure for EVERY sample, so that every tile takes
// the kernel's sweep-cap fallback (textbook routine, vectors in LDS) - results stay correct, the kernel is an order of
// magnitude slower.  The only way to run that path on a device: no input is known that hits the sweep cap.  Off.
#ifndef RC_GRAD_FORCE_GENERAL
#define RC_GRAD_FORCE_GENERAL 0
#endif

namespace rc {

// sin(x)/x; below 0.03 the Taylor series to x^6 (truncation 2e-18), above sin(x) * (1/x)
RC_HD double sinc_taylor(double x) {
    const double z = x * x;
    const bool small = fabs(x) < 0.03;
    double s, c;
    sincos_reduced(x, s, c);
    const double big = s * rcp_full(small ? 1.0 : x);
    const double ser = fma(z, fma(z, fma(z, -1.0 / 5040.0, 1.0 / 120.0), -1.0 / 6.0), 1.0);
    return small ? ser : big;
}

// Rows of V carried per QL pass (see "Registers" above) and the number of passes.  Chosen from the ISA listing: no
// instantiation may spill (tests/test_asm_resources.py).
constexpr int grad_batch_rows(int n) { return n <= 9 ? n : (n == 10 ? 6 : (n == 11 ? 5 : 4)); }
constexpr int grad_passes(int n) { return grad_batch_rows(n) == n ? 1 : (n - 2 + grad_batch_rows(n) - 3) / (grad_batch_rows(n) - 2); }

// The sites in the order the passes take them: rank 0 = out, rank 1 = in (when in != out), then the other sites ascending.
// Returns -1 beyond the last site.  Wave-uniform integer arithmetic.
RC_HD int grad_site_of_rank(int n, int in, int out, int r) {
    if (r == 0) return out;
    int left = r - 1;
    if (in != out) {
        if (r == 1) return in;
        left = r - 2;
    }
    for (int i = 0; i < n; ++i) {
        if (i == in || i == out) continue;
        if (left == 0) return i;
        --left;
    }
    return -1;
}
// site of row q in pass b: rows 0, 1 are ranks 0, 1 in every pass
template <int N>
RC_HD void grad_pass_rows(int in, int out, int pass, int (&site)[grad_batch_rows(N)]) {
    constexpr int R = grad_batch_rows(N);
#pragma unroll
    for (int q = 0; q < R; ++q) site[q] = grad_site_of_rank(N, in, out, q < 2 ? q : 2 + pass * (R - 2) + (q - 2));
}

// Where entry l of a pass's result (gradient_from_eigensystem: l < R the bias of the site of row l, l = R the time entry) goes
// in the sample's gradient [N + 1], or -1 when this pass does not write it: rows 0 and 1 (out, in) ride in every pass and the
// time entry is the same in every pass - the first pass writes them -, and a row beyond the last site has nothing to write.
template <int N>
RC_HD int grad_result_column(const int (&site)[grad_batch_rows(N)], int pass, int l) {
    constexpr int R = grad_batch_rows(N);
    const bool first_only = l < 2 || l == R;
    if (first_only && pass > 0) return -1;
    return l == R ? N : site[l];
}

// (d, e) of the gauged, mean-shifted matrix of one sample.  loadg as in chain_fidelity_fast.
template <int N, typename LoadG>
RC_HD void grad_load_matrix(const double* x, const double* h0d, const double* h0o, LoadG loadg, double (&d)[N], double (&e)[N]) {
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        d[i] = x[i] + h0d[i] + loadg(3 * i);
        c += d[i];
    }
    c *= 1.0 / N;
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] -= c;
#pragma unroll
    for (int i = 1; i < N; ++i) {
        const double re = h0o[i - 1] + loadg(3 * i + 1);
        const double im = loadg(3 * i + 2);
        // (an exactly cancelled coupling becomes 1e-150: see chain_fidelity_fast)
        const double h = fma(re, re, fma(im, im, 1e-300));
        double r, rinv;
        sqrt_rsqrt(h, r, rinv);
        e[i - 1] = r;
    }
    e[N - 1] = 0.0;
}

// Fast path, one pass: eigenvalues in s.d, V[site[q]][k] in s.z[q][k] (a row with site < 0 is zero).  Returns false - per
// lane - on the sweep cap.  FREEZE: tridiag_ql2_fast's - every lane performs exactly the sweeps it would perform alone, so its
// result does not depend on which other samples share its wave (mc_fid_grad_listed_kernel, whose waves are packed from a list).
template <int N, int R, bool FREEZE = false>
RC_HD bool grad_eigensystem_fast(const double (&d)[N], const double (&e)[N], const int (&site)[R], TriEig<N, R>& s) {
    // (the unit rows are wave-uniform: left alone the compiler keeps all R N of them in SCALAR registers until the first rotation
    // touches them and spills ~200 of those; two opaque per-lane constants put them where they end up anyway)
    double one = 1.0, zero = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(one), "+v"(zero));
#endif
#pragma unroll
    for (int i = 0; i < N; ++i) {
        s.d[i] = d[i];
        s.e[i] = e[i];
#pragma unroll
        for (int q = 0; q < R; ++q) s.z[q][i] = (site[q] == i) ? one : zero;
    }
#if RC_GRAD_FORCE_GENERAL
    (void)tridiag_ql2_fast<N, R, FREEZE>(s);
    return false;
#else
    return tridiag_ql2_fast<N, R, FREEZE>(s);
#endif
}

// Textbook implicit QL with a per-sample window and ALL rows of the eigenvector matrix: tridiag_ql2_general with n rows
// instead of two.  `Vec` d, e: n entries each; `Mat` z(q, i): row q, column i, identity on entry.
template <typename Vec, typename Mat>
RC_HD void tridiag_qln_general(int n, Vec d, Vec e, Mat z) {
    for (int l = 0; l < n - 1; ++l) {
        for (int iter = 0; iter < kMaxSweepsPerEig; ++iter) {
            int m = l;
            for (; m < n - 1; ++m) {
                const double dd = fabs(d[m]) + fabs(d[m + 1]);
                if (fabs(e[m]) <= kEps * dd) break;
            }
            if (m == l) break;
            const double delta = 0.5 * (d[l + 1] - d[l]);
            const double e2 = e[l] * e[l];
            const double rho = sqrt_fast(fma(delta, delta, e2) + 1e-300);
            double g = d[m] - d[l] + e2 * rcp_fast(delta + copysign(rho, delta));
            double sn = 1.0, cs = 1.0, p = 0.0;
            for (int i = m - 1; i >= l; --i) {
                const double f = sn * e[i];
                const double b = cs * e[i];
                const double gn = g + 1e-150;
                double r, rinv;
                sqrt_rsqrt(fma(f, f, gn * gn), r, rinv);
                e[i + 1] = r;
                sn = f * rinv;
                cs = gn * rinv;
                g = d[i + 1] - p;
                r = fma(d[i] - g, sn, 2.0 * cs * b);
                p = sn * r;
                d[i + 1] = g + p;
                g = fma(cs, r, -b);
                for (int q = 0; q < n; ++q) {
                    const double a1 = z(q, i + 1), a0 = z(q, i);
                    z(q, i + 1) = fma(sn, a0, cs * a1);
                    z(q, i) = fma(cs, a0, -sn * a1);
                }
            }
            d[l] = d[l] - p;
            e[l] = g;
            e[m] = 0.0;
        }
    }
}

// General path (rare): the whole eigensystem of one sample through tridiag_qln_general, then the rows of this pass; the work
// vectors (2 N + N^2 doubles) are the caller's (lane-strided LDS views on the device, plain arrays on the host).  g: this
// sample's 3 N draws.
template <int N, int R, typename Vec, typename Mat>
RC_HD void grad_eigensystem_general(const double* x, const double* h0d, const double* h0o, const double* g, const int (&site)[R],
                                    Vec d, Vec e, Mat z, TriEig<N, R>& s) {
    double c = 0.0;
    for (int i = 0; i < N; ++i) {
        d[i] = x[i] + h0d[i] + g[3 * i];
        c += d[i];
        e[i] = 0.0;
        for (int q = 0; q < N; ++q) z(q, i) = (q == i) ? 1.0 : 0.0;
    }
    c *= 1.0 / N;
    for (int i = 0; i < N; ++i) d[i] = d[i] - c;
    for (int i = 1; i < N; ++i) {
        const double re = h0o[i - 1] + g[3 * i + 1];
        const double im = g[3 * i + 2];
        const double h = fma(re, re, im * im);
        double r, rinv;
        sqrt_rsqrt(h, r, rinv);
        e[i - 1] = (h > 0.0) ? r : 0.0;
    }
    tridiag_qln_general(N, d, e, z);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        s.d[i] = d[i];
#pragma unroll
        for (int q = 0; q < R; ++q) s.z[q][i] = (site[q] >= 0) ? z(site[q] >= 0 ? site[q] : 0, i) : 0.0;
    }
}

// Fidelity and gradient from the eigensystem of one pass (s.d, s.z: row 0 = out, row 1 = in unless `same`: in == out).
// xT = x_N (signed).  grad[q], q < R: the derivative with respect to the bias of the site of row q; grad[R]: time.
template <int N, int R>
RC_HD void gradient_from_eigensystem(const TriEig<N, R>& s, double xT, bool same, double& fid, double (&grad)[R + 1]) {
    const double T = fabs(xT);
    const double (&vo)[N] = s.z[0];
    // (a select per use on a wave-uniform flag: a reference picked at run time would put the matrix into scratch memory)
    const auto VI = [&s, same](int k) { return same ? s.z[0][k] : s.z[1][k]; };
    // h_k = exp(-i T lam_k / 2) = ch_k - i sh_k;  p_k = h_k^2
    double ch[N], sh[N];
    double fr = 0.0, fi = 0.0, sr = 0.0, si = 0.0;       // phi and S = sum_k lam_k w_k p_k
    const double hT = 0.5 * T;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sincos_reduced(hT * s.d[k], sh[k], ch[k]);
        const double pr = fma(ch[k], ch[k], -sh[k] * sh[k]);
        const double pi = -2.0 * ch[k] * sh[k];
        const double w = vo[k] * VI(k);
        fr = fma(w, pr, fr);
        fi = fma(w, pi, fi);
        const double lw = s.d[k] * w;
        sr = fma(lw, pr, sr);
        si = fma(lw, pi, si);
    }
    fid = fma(fr, fr, fi * fi);
    // 2 Re(conj(phi) (-i S)) = 2 (phi_r S_i - phi_i S_r)
    const double sg = (xT > 0.0) ? 1.0 : ((xT < 0.0) ? -1.0 : 0.0);
    grad[R] = sg * 2.0 * fma(fr, si, -fi * sr);
#pragma unroll
    for (int l = 0; l < R; ++l) grad[l] = 0.0;
    const double T2 = 2.0 * T;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        // Gam_kk = -i T p_k = T (p_i - i p_r):  2 Re(conj(phi) Gam_kk) = 2 T (phi_r p_i - phi_i p_r)
        const double pr = fma(ch[k], ch[k], -sh[k] * sh[k]);
        const double pi = -2.0 * ch[k] * sh[k];
        const double q = T2 * fma(fr, pi, -fi * pr) * (vo[k] * VI(k));
#pragma unroll
        for (int l = 0; l < R; ++l) grad[l] = fma(q * s.z[l][k], s.z[l][k], grad[l]);
#pragma unroll
        for (int j = 0; j < k; ++j) {
            // exp(-i T (lam_j + lam_k)/2) = h_j h_k = a + i b;  Gam_jk = T sinc (b - i a)
            const double a = fma(ch[j], ch[k], -sh[j] * sh[k]);
            const double b = -fma(sh[j], ch[k], ch[j] * sh[k]);
            const double sc = sinc_taylor(hT * (s.d[j] - s.d[k]));
            const double qq = (T2 * sc) * fma(fr, b, -fi * a) * fma(vo[j], VI(k), vo[k] * VI(j));
#pragma unroll
            for (int l = 0; l < R; ++l) grad[l] = fma(qq * s.z[l][j], s.z[l][k], grad[l]);
            }
    }
}

}  // namespace rc

// Per-sample arithmetic of the chain-topology fidelity on a GRID OF READOUT TIMES (one sample per lane):
//   F_j = |<out| exp(-i H t_j) |in>|^2,   t_j = | T * tscale_j + tshift_j |,   j = 0 .. M - 1,   T = x_N,
// from ONE eigen decomposition of the sample's matrix H = HH + Z(draws) + diag(x_0 .. x_{N-1}).
//
// Route.  The gauged real tridiagonal matrix is built exactly as chain_fidelity_fast<N, kWeightsRows> builds it and goes
// through the same all-fp64 implicit QL with the two unit rows `in` and `out` (tridiag_ql2_fast<N, 2>): genuine eigenvector
// rows, so the weights w_k = z_out,k z_in,k carry no condition on eigenvalue gaps, cut bonds or sum rules and ONE
// decomposition is valid for every t - there are no guards to re-argue per time.  What depends on the time is the phase sum
//   phi_j = sum_k w_k exp(-i t_j (lam_k - lam_0)),   F_j = |phi_j|^2,
// N - 1 table-driven sines / cosines and two fma chains per time: the `!AMP` branch of chain_fidelity_fast, operation for
// operation, so that slab j is bit for bit what the rows kernel gives for a controller whose time entry is t_j.
//
// The time.  The product T * tscale_j is rounded first, the sum second (no fused multiply-add: the product is opaque to the
// optimiser), the absolute value last - NumPy's np.abs(T * a + b), bit for bit.  tscale / tshift / the quadrature weights are
// wave-uniform: the loop over j is rolled and reads them through the scalar path.
//
// Outputs of the loop (TimesAcc): every F_j goes to the caller's `store(j, F)`; wsum = w_0 F_0, then fma(w_j, F_j, wsum) in
// the order of j; fmin = min_j F_j in the order of j.
//
// A lane whose QL runs into the sweep cap of the fast path reports false; the kernel then recomputes such lanes with the
// textbook per-sample routine (times_general: tridiag_ql2_general, vectors in LDS, the time loop inside).  One input is known
// to do that: H = 0 exactly (every bond cut, every bias zero) - no coupling, 1e-150 after the exact cancellation, is negligible
// against |d_l| + |d_l+1| = 0 (tests/test_host_times.py, tests/test_gpu_times.py run it); nothing else has been observed.
//
// sincos_table's domain: |t_j (lam_k - lam_0)| < 2.1e8 (the turn count must fit an int32), as everywhere on the fast path.
//
// Plain C++ like tridiag_core.h: tests/host/host_times.cpp compiles exactly this for the CPU.
#pragma once
#include "tridiag_core.h"

// -DRC_TIMES_FORCE_GENERAL=1 (scripts/build_variant.sh): the fast QL reports failure for EVERY sample, so that every tile takes
// the kernels' sweep-cap fallback (textbook routine, vectors in LDS) - results stay correct, the kernels are an order of magnitude
// slower.  Runs that path on every input (the product build takes it for H = 0 only, see above).  Off.
#ifndef RC_TIMES_FORCE_GENERAL
#define RC_TIMES_FORCE_GENERAL 0
#endif

namespace rc {

// t = | T a + b |: the product rounded, then the sum, then the absolute value
RC_HD double readout_time(double T, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    double prod = T * a;
    asm volatile("" : "+v"(prod));                 // (opaque: the compiler otherwise contracts product and sum into one fma)
#else
    volatile double prod = T * a;
#endif
    return fabs(prod + b);
}

// What the time loop accumulates besides the slabs.
struct TimesAcc {
    double wsum, fmin;
    RC_HD void take(int j, double f, double omega) {
        const double first = omega * f;
        wsum = (j == 0) ? first : fma(omega, f, wsum);
        fmin = (j == 0) ? f : ::fmin(fmin, f);
    }
};

// Fast path, the part that does not depend on the time: eigenvalue differences dl[k] = lam_k - lam_0 (dl[0] = 0) and weights
// w[k] of one sample.  loadg as in chain_fidelity_fast.  Returns false - per lane - on the sweep cap.
template <int N, typename LoadG>
RC_HD bool times_eigen_fast(const double* x, const double* h0d, const double* h0o, LoadG loadg, int in, int out, double (&dl)[N],
                            double (&w)[N]) {
    TriEig<N, 2> s;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        s.d[i] = x[i] + h0d[i] + loadg(3 * i);
        s.z[0][i] = (i == in) ? 1.0 : 0.0;
        s.z[1][i] = (i == out) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 1; i < N; ++i) {
        const double re = h0o[i - 1] + loadg(3 * i + 1);
        const double im = loadg(3 * i + 2);
        // (an exactly cancelled coupling becomes 1e-150: see chain_fidelity_fast)
        const double h = fma(re, re, fma(im, im, 1e-300));
        double r, rinv;
        sqrt_rsqrt(h, r, rinv);
        s.e[i - 1] = r;
    }
    s.e[N - 1] = 0.0;
    const bool ok = tridiag_ql2_fast(s);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        w[k] = s.z[1][k] * s.z[0][k];
        dl[k] = s.d[k] - s.d[0];
    }
#if RC_TIMES_FORCE_GENERAL
    return false;
#else
    return ok;
#endif
}

// F at one time from (dl, w): the phase sum of chain_fidelity_fast (global phase exp(i t lam_0) dropped: N - 1 sincos)
template <int N>
RC_HD double times_phase_fid(const double (&dl)[N], const double (&w)[N], double t, const double* sctab) {
    const double Tk = t * kTurnsPerRadian;
    double re = w[0], im = 0.0;
#pragma unroll
    for (int k = 1; k < N; ++k) {
        double sk, ck;
        sincos_table(Tk * dl[k], sctab, sk, ck);
        re = fma(w[k], ck, re);
        im = fma(-w[k], sk, im);
    }
    return fma(re, re, im * im);
}

// The loop over the grid, fast path.  tscale / tshift / weights: [M] or NULL (1, 0, and no weighted sum: acc.wsum is then
// not meaningful).  store(j, F) receives every F_j.
template <int N, typename Store>
RC_HD void times_loop_fast(const double (&dl)[N], const double (&w)[N], double T, int M, const double* tscale, const double* tshift,
                           const double* weights, const double* sctab, Store store, TimesAcc& acc) {
#pragma unroll 1
    for (int j = 0; j < M; ++j) {
        const double t = readout_time(T, tscale ? tscale[j] : 1.0, tshift ? tshift[j] : 0.0);
        const double f = times_phase_fid<N>(dl, w, t, sctab);
        store(j, f);
        acc.take(j, f, weights ? weights[j] : 0.0);
    }
}

// General path (rare; runtime n): the textbook QL of chain_fidelity_general on the caller's work vectors (n entries each:
// lane-strided LDS views on the device, plain arrays on the host), then the same loop over the grid with the phase sum of
// chain_fidelity_general.  g: this sample's 3 n draws.
template <typename Vec, typename Store>
RC_HD void times_general(int n, const double* x, const double* h0d, const double* h0o, const double* g, int in, int out, Vec d,
                         Vec e, Vec za, Vec zb, int M, const double* tscale, const double* tshift, const double* weights,
                         Store store, TimesAcc& acc) {
    for (int i = 0; i < n; ++i) {
        d[i] = x[i] + h0d[i] + g[3 * i];
        za[i] = (i == in) ? 1.0 : 0.0;
        zb[i] = (i == out) ? 1.0 : 0.0;
        e[i] = 0.0;
    }
    for (int i = 1; i < n; ++i) {
        const double re = h0o[i - 1] + g[3 * i + 1];
        const double im = g[3 * i + 2];
        const double h = fma(re, re, im * im);
        double r, rinv;
        sqrt_rsqrt(h, r, rinv);
        e[i - 1] = (h > 0.0) ? r : 0.0;
    }
    tridiag_ql2_general(n, d, e, za, zb);
    for (int k = 0; k < n; ++k) za[k] = zb[k] * za[k];           // the weights
    const double T = x[n];
    for (int j = 0; j < M; ++j) {
        const double t = readout_time(T, tscale ? tscale[j] : 1.0, tshift ? tshift[j] : 0.0);
        double re = 0.0, im = 0.0;
        for (int k = 0; k < n; ++k) {
            double sk, ck;
            sincos_reduced(t * d[k], sk, ck);
            const double wk = za[k];
            re = fma(wk, ck, re);
            im = fma(-wk, sk, im);
        }
        const double f = fma(re, re, im * im);
        store(j, f);
        acc.take(j, f, weights ? weights[j] : 0.0);
    }
}

}  // namespace rc

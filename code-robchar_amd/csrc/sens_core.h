// Per-sample arithmetic of the chain-topology noise-SENSITIVITY kernel (one sample per lane): the fidelity F of grad_core.h and
// its derivatives with respect to the 3 N - 2 structured perturbation directions, i.e. the sample's own draws
//   g0_i (site energies, i = 0 .. N-1),   g1_i, g2_i (real and imaginary part of the coupling of sites i-1 and i, i = 1 .. N-1).
//
// Route.  The eigensystem and the real pair scalars are those of gradient_from_eigensystem (grad_core.h):
//     q_kk = 2 Re(conj(phi) Gam_kk) vo_k vi_k,        q_jk = 2 Re(conj(phi) Gam_jk) (vo_j vi_k + vo_k vi_j)   (j < k)
// and every derivative is a contraction of them with a pattern of two rows of V:
//     dF/dg0_i = sum_{j<=k} q_jk V_ij V_ik                                    (= dF/dx_i of the gradient kernel)
//     dF/dr_i  = sum_{j<k} q_jk (V_ij V_{i-1,k} + V_{i-1,j} V_ik)  +  sum_k q_kk 2 V_ik V_{i-1,k}
// r_i = |re_i + i im_i| is the gauged coupling: F depends on the complex coupling through its modulus only, hence
//     dF/dg1_i = (re_i / r_i) dF/dr_i,      dF/dg2_i = (im_i / r_i) dF/dr_i,
// both exactly 0 at an exactly cut bond (F is even in r_i; sens_unit_phase gives 0 * finite there).
//
// Registers.  A bond needs the rows i-1 and i of V in the same QL pass.  N <= 9: one pass with all rows in site order (the
// rows `out` and `in` are picked out of them by wave-uniform selects).  From N = 10 the QL runs in passes of
// R = sens_batch_rows(N) rows: rows 0, 1 = out, in (every pass needs them for the pair scalars) and a window of R - 2
// consecutive sites; consecutive windows overlap by one row, so that every bond has both its rows in exactly one pass
// (sens_row_writes).  Every pass is self-contained like the gradient kernel's.
//
// The eigensystem comes from grad_eigensystem_fast / grad_eigensystem_general of grad_core.h unchanged.
// Plain C++: tests/host/host_sens.cpp compiles exactly this for the CPU.
#pragma once
#include "grad_core.h"

namespace rc {

// Rows of V per QL pass, sites per window and passes.  Chosen from the ISA listing: no instantiation may spill.
constexpr int sens_batch_rows(int n) { return n <= 9 ? n : (n <= 11 ? 6 : 5); }
constexpr bool sens_single_pass(int n) { return sens_batch_rows(n) == n; }
constexpr int sens_first_window_row(int n) { return sens_single_pass(n) ? 0 : 2; }
constexpr int sens_window(int n) { return sens_batch_rows(n) - sens_first_window_row(n); }
constexpr int sens_passes(int n) { return sens_single_pass(n) ? 1 : (n - 1 + sens_window(n) - 2) / (sens_window(n) - 1); }

// site of row q in pass b (-1: none).  Wave-uniform integer arithmetic.
template <int N>
RC_HD void sens_pass_rows(int in, int out, int pass, int (&site)[sens_batch_rows(N)]) {
    constexpr int R = sens_batch_rows(N), Q0 = sens_first_window_row(N), W = sens_window(N);
    if (Q0 == 2) {
        site[0] = out;
        site[1] = in;
    }
#pragma unroll
    for (int q = Q0; q < R; ++q) {
        const int i = pass * (W - 1) + (q - Q0);
        site[q] = i < N ? i : -1;
    }
}

// What row q of pass b writes: `wsite` the site entry dF/dg0 of site[q], `wbond` the two coupling entries of the bond
// (site[q] - 1, site[q]).  The first window row of a later pass is the overlap: the pass before has written its site, and the
// bond below it belongs to that pass too.  Rows 0, 1 of a multi-pass schedule (out, in) write nothing.
template <int N>
RC_HD void sens_row_writes(const int (&site)[sens_batch_rows(N)], int pass, int q, bool& wsite, bool& wbond) {
    constexpr int Q0 = sens_first_window_row(N);
    const bool row = q >= Q0 && site[q] >= 0;
    wsite = row && !(pass > 0 && q == Q0);
    wbond = row && q > Q0;
}

// (re, im) / |re + i im|; (0, 0) at re = im = 0 (the nudge keeps the reciprocal root finite: 0 * 1e150)
RC_HD void sens_unit_phase(double re, double im, double& cr, double& ci) {
    const double h = fma(re, re, fma(im, im, 1e-300));
    double r, rinv;
    sqrt_rsqrt(h, r, rinv);
    cr = re * rinv;
    ci = im * rinv;
}

// Fidelity and the two contractions from the eigensystem of one pass (s.d, s.z: row q = site[q]).  ds[q]: dF/dg0 of site[q];
// dr[q], q > Q0: dF/dr of the bond between the rows q - 1 and q.  Entries below Q0 (and dr[Q0]) are left 0.
// The pair loop is gradient_from_eigensystem's, duplicated so that the gradient kernel's code stays as it is.
template <int N, int R>
RC_HD void sens_from_eigensystem(const TriEig<N, R>& s, const int (&site)[R], int in, int out, double xT, double& fid,
                                 double (&ds)[R], double (&dr)[R]) {
    constexpr int Q0 = sens_first_window_row(N);
    const double T = fabs(xT);
    // rows out, in: rows 0, 1 of a multi-pass schedule; picked by wave-uniform selects out of all rows otherwise (a row
    // indexed at run time would put the matrix into scratch memory)
    double vo[N], vi[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (Q0 == 2) {
            vo[k] = s.z[0][k];
            vi[k] = s.z[1][k];
        } else {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                a = (site[q] == out) ? s.z[q][k] : a;
                b = (site[q] == in) ? s.z[q][k] : b;
            }
            vo[k] = a;
            vi[k] = b;
        }
    }
    // h_k = exp(-i T lam_k / 2) = ch_k - i sh_k;  p_k = h_k^2
    double ch[N], sh[N];
    double fr = 0.0, fi = 0.0;
    const double hT = 0.5 * T;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sincos_reduced(hT * s.d[k], sh[k], ch[k]);
        const double pr = fma(ch[k], ch[k], -sh[k] * sh[k]);
        const double pi = -2.0 * ch[k] * sh[k];
        const double w = vo[k] * vi[k];
        fr = fma(w, pr, fr);
        fi = fma(w, pi, fi);
    }
    fid = fma(fr, fr, fi * fi);
#pragma unroll
    for (int l = 0; l < R; ++l) ds[l] = dr[l] = 0.0;
    const double T2 = 2.0 * T;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double pr = fma(ch[k], ch[k], -sh[k] * sh[k]);
        const double pi = -2.0 * ch[k] * sh[k];
        const double q = T2 * fma(fr, pi, -fi * pr) * (vo[k] * vi[k]);
#pragma unroll
        for (int l = Q0; l < R; ++l) {
            const double qz = q * s.z[l][k];
            ds[l] = fma(qz, s.z[l][k], ds[l]);
            if (l > Q0) dr[l] = fma(2.0 * qz, s.z[l - 1][k], dr[l]);
        }
#pragma unroll
        for (int j = 0; j < k; ++j) {
            const double a = fma(ch[j], ch[k], -sh[j] * sh[k]);
            const double b = -fma(sh[j], ch[k], ch[j] * sh[k]);
            const double sc = sinc_taylor(hT * (s.d[j] - s.d[k]));
            const double qq = (T2 * sc) * fma(fr, b, -fi * a) * fma(vo[j], vi[k], vo[k] * vi[j]);
#pragma unroll
            for (int l = Q0; l < R; ++l) {
                ds[l] = fma(qq * s.z[l][j], s.z[l][k], ds[l]);
                if (l > Q0) dr[l] = fma(qq, fma(s.z[l][j], s.z[l - 1][k], s.z[l - 1][j] * s.z[l][k]), dr[l]);
            }
        }
    }
}

}  // namespace rc

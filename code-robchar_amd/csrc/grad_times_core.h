// Per-sample arithmetic of the fidelity GRADIENT on a GRID OF READOUT TIMES (one sample per lane): for controller row c with
// time entry T = x_N (signed, as stored) and a grid of M times,
//   u_j = T * tscale_j + tshift_j      (product rounded first, sum second, no fused multiply-add; |u_j| = backend.readout_times),
//   W        = sum_j w_j F(u_j),
//   dW/dx_l  = sum_j w_j dF/dx_l(u_j)                                  for the N biases,
//   dW/dx_N  = sum_j w_j tscale_j sgn(u_j) F'(|u_j|)                   (0 from a time with u_j = 0: F is even in t),
// from ONE eigen decomposition of the sample's matrix.  After the QL gradient_from_eigensystem (grad_core.h) depends on the time
// only through N half-angle sines / cosines, one sinc per pair and the pair contraction, so the loop below calls it once per grid
// time on the same eigensystem - unchanged: its time entry already carries sgn(u) - and accumulates.
//
// Fixed arithmetic (the result is testable bit for bit against M single-time evaluations):
//   per time j    f_j, g_j = gradient_from_eigensystem(s, u_j, same);  g_j[R] = tscale_j * g_j[R], rounded once (opaque);
//   accumulation  acc = w_0 v_0;  acc = fma(w_j, v_j, acc), j = 1 .. M - 1  (times_core.h's wsum order) for W and each of the
//                 R + 1 gradient entries of the pass.
// The loop is rolled and wave-uniform.  The grid comes through `Grid` - anything with  int M,  double scale(int j),
// double shift(int j),  double weight(int j)  -: GridPointers below on the host; on the device the kernel's view on the constant
// address space, so that the three values of a grid time are scalar loads (k_fidelity_grad_times_philox.inc.h).
//
// Where the accumulators live is the caller's: `Acc` is anything with  double get(int l) const  and  void set(int l, double v),
// l = 0 .. R + 1 (l <= R: the gradient entries, l = R + 1: W) - GradTimesRegs below (an array: registers on the device), or a
// lane-strided view on LDS (k_fidelity_grad_times_philox.inc.h).
//
// Plain C++ like grad_core.h: tests/host/host_grad_times.cpp compiles exactly this for the CPU.
#pragma once
#include "grad_core.h"

namespace rc {

// u = T a + b: the product rounded, then the sum (fabs(u) is readout_time of times_core.h, bit for bit)
RC_HD double grid_time_signed(double T, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    double prod = T * a;
    asm volatile("" : "+v"(prod));                 // (opaque: the compiler otherwise contracts product and sum into one fma)
#else
    volatile double prod = T * a;
#endif
    return prod + b;
}

// a * g rounded once, never contracted into what consumes it
RC_HD double opaque_product(double a, double g) {
#if defined(__HIP_DEVICE_COMPILE__)
    double prod = a * g;
    asm volatile("" : "+v"(prod));
    return prod;
#else
    volatile double prod = a * g;
    return prod;
#endif
}

// The grid behind plain pointers.  tscale / tshift: [M] or NULL (all 1 / all 0); weights: [M].
struct GridPointers {
    int M;
    const double *tscale, *tshift, *weights;
    RC_HD double scale(int j) const { return tscale ? tscale[j] : 1.0; }
    RC_HD double shift(int j) const { return tshift ? tshift[j] : 0.0; }
    RC_HD double weight(int j) const { return weights[j]; }
};

template <int R>
struct GradTimesRegs {
    double v[R + 2];
    RC_HD double get(int l) const { return v[l]; }
    RC_HD void set(int l, double x) { v[l] = x; }
};

// Keeps the eigenvalues and the rows out and in opaque to the optimiser at the head of every grid time (no instruction is
// emitted).  Without it the compiler hoists everything of gradient_from_eigensystem that does not depend on the time - the weights
// vo_k vi_k, the N (N - 1) / 2 pair factors vo_j vi_k + vo_k vi_j, the eigenvalue differences: all functions of these 3 N values
// alone - out of the rolled loop and holds it in registers across the loop: 130 registers more than the single-time kernel at
// N = 11 and spills from N = 5.  Fenced, a grid time costs what a single-time evaluation costs and needs the registers of one.
// (The other rows enter only through products with time-dependent factors; fencing them too would pin the whole matrix into
// architectural registers at once, which from N = 8 - where part of it lives in accumulation registers - costs spill copies.)
template <int N, int R>
RC_HD void eigensystem_fence(TriEig<N, R>& s) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int k = 0; k < N; ++k) {
        asm volatile("" : "+v"(s.d[k]));
#pragma unroll
        for (int q = 0; q < (R < 2 ? R : 2); ++q) asm volatile("" : "+v"(s.z[q][k]));
    }
#else
    (void)s;
#endif
}

// The loop over the grid on the eigensystem of one pass.
// On return acc(l), l < R: dW/dx of the site of row l; acc(R): dW/dx_N; acc(R + 1): W.
// FENCE: eigensystem_fence at the head of every grid time (the caller's choice per N, from the listing).
template <int N, int R, bool FENCE, typename Grid, typename Acc>
RC_HD void gradient_times_from_eigensystem(TriEig<N, R>& s, double xT, bool same, const Grid& grid, Acc& acc) {
#pragma unroll 1
    for (int j = 0; j < grid.M; ++j) {
        if (FENCE) eigensystem_fence(s);
        const double a = grid.scale(j);
        const double u = grid_time_signed(xT, a, grid.shift(j));
        const double om = grid.weight(j);
        double f, g[R + 1];
        gradient_from_eigensystem<N, R>(s, u, same, f, g);
        g[R] = opaque_product(a, g[R]);
        if (j == 0) {                               // (wave-uniform)
#pragma unroll
            for (int l = 0; l <= R; ++l) acc.set(l, om * g[l]);
            acc.set(R + 1, om * f);
        } else {
#pragma unroll
            for (int l = 0; l <= R; ++l) acc.set(l, fma(om, g[l], acc.get(l)));
            acc.set(R + 1, fma(om, f, acc.get(R + 1)));
        }
    }
}

}  // namespace rc

// Scrambled Sobol points -> normals, per element: the device side of code-robchar_amd/sobol.py (the definition; read its module
// text first).  Shared by the generator kernel (k_draws_sobol.inc.h) and by the fidelity kernel that generates its own points
// (k_fidelity_sobol.inc.h): both produce the same bits for the same element.
//
// A tile is 64 consecutive samples of ONE controller row, and the contract (skip % 64 == 0, P % 64 == 0 whenever R > 1) puts all
// of them in one replicate at the points n = n0 + lane, n0 a multiple of 64.  gray() is linear over GF(2) and n0 + lane = n0 ^ lane,
// so per dimension d
//     x = [ shift[d] ^ XOR over the set bits j >= 5 of gray(n0) of v[d][j] ]  ^  XOR over the set bits j < 6 of gray(lane) of v[d][j]
// with a wave-uniform first part (bit 5 of gray(n0) is bit 6 of n0).  sobol_tile_base forms it once per tile, lane d doing dimension
// d, into LDS; sobol_point folds in the six low direction numbers - wave-uniform words, so scalar loads - with one a ^ (b & c) each
// (v_bitop3_b32; the compiler forms it from the plain expression).
//
// #included INSIDE the anonymous namespace of robchar_qmc.hip, after philox_core.inc.h (ln_table) and tridiag_core.h (sqrt_rsqrt).
#pragma once

using rckp::SobolDraws;

// what a tile's lanes share: its replicate's table, its shift row, and the first point's Gray code
struct SobolTile {
    const unsigned int* v;            // dirnum[r]: [D][32]
    const unsigned int* sh;           // shift[c or 0][r]: [D]
    unsigned int g0;                  // gray(n0)
};

__device__ __forceinline__ SobolTile sobol_tile(const SobolDraws& q, long long c, long long kb) {
    const long long r = kb / q.P;                                    // wave-uniform
    const unsigned int n0 = (unsigned int)(q.skip + (unsigned long long)(kb - r * q.P));
    SobolTile t;
    t.v = q.dirnum + r * (long long)q.D * 32;
    t.sh = q.shift + c * q.shift_cstride + r * (long long)q.D;
    t.g0 = n0 ^ (n0 >> 1);
    return t;
}

// base[d], d < D: the wave-uniform part of every coordinate.  The caller puts a barrier between this and the first sobol_point.
__device__ __forceinline__ void sobol_tile_base(const SobolTile& t, int D, int lane, unsigned int* base) {
    for (int d = lane; d < D; d += 64) {
        unsigned int b = t.sh[d];
#pragma unroll 1
        for (int j = 5; j < 32; ++j)
            if ((t.g0 >> j) & 1u) b ^= t.v[d * 32 + j];
        base[d] = b;
    }
}

// the scrambled point of this lane in dimension d; gl = gray(lane)
__device__ __forceinline__ unsigned int sobol_point(const SobolTile& t, const unsigned int* base, unsigned int gl, int d) {
    unsigned int x = base[d];
    const unsigned int* v = t.v + d * 32;
#pragma unroll
    for (int j = 0; j < 6; ++j) x ^= (unsigned int)(-(int)((gl >> j) & 1u)) & v[j];
    return x;
}

// Phi^-1 by Wichura's AS 241 (PPND16), coefficients in ascending order.  sobol.py (normal_from_bits) restates this routine.
#define RC_PPND_POLY(r, c0, c1, c2, c3, c4, c5, c6, c7) \
    fma(fma(fma(fma(fma(fma(fma(c7, r, c6), r, c5), r, c4), r, c3), r, c2), r, c1), r, c0)

// z = Phi^-1((x + 0.5) 2^-32).  The word is folded to the lower half, xm = x < 2^31 ? x : ~x, so p = (xm + 0.5) 2^-32 <= 1/2 and
// |u - 1/2| = 1/2 - p are exact; |z| comes from p alone and the sign from the word's top bit: z(~x) == -z(x) bit for bit.
// p >= 2^-33, so sqrt(-ln p) <= 4.79 and AS 241's far-tail branch (beyond 5) does not exist here.  One division serves both branches.
__device__ __forceinline__ double sobol_normal(unsigned int x, const double* lntab) {
    const bool upper = (x >> 31) != 0u;
    const unsigned int xm = upper ? ~x : x;
    const double p = ((double)xm + 0.5) * 0x1.0p-32;
    const double qa = 0.5 - p;
    double num, den;
    if (qa <= 0.425) {
        const double r = fma(-qa, qa, 0.180625);
        num = RC_PPND_POLY(r, 3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                           4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3) * qa;
        den = RC_PPND_POLY(r, 1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
                           2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3);
    } else {
        const double nl = -ln_table(p, lntab);
        double root, rinv;
        rc::sqrt_rsqrt(nl, root, rinv);
        const double r = fma(nl, rinv, -1.6);                        // sqrt(-ln p) - 1.6, the root's last product inside the fma
        num = RC_PPND_POLY(r, 1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                           1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4);
        den = RC_PPND_POLY(r, 1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1,
                           1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9);
    }
    const double z = num / den;
    return upper ? z : -z;
}

// draw = fl(sigma z): the product is rounded once and made opaque, as in philox_lane_draws - left to the compiler it would be
// contracted into the fma that forms the consumer's matrix entry, another rounding than the tensor route's.
__device__ __forceinline__ double sobol_draw(unsigned int x, double sigma, const double* lntab) {
    double v = sigma * sobol_normal(x, lntab);
    asm volatile("" : "+v"(v));
    return v;
}

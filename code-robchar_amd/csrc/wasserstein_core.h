// Per-element pieces of the pairwise Wasserstein matrix (wasserstein_tile_kernel, wasserstein_finish_kernel: k_wasserstein.inc.h)
// - plain C++ so that the CPU unit test runs the exact term, summation order, split plan and argument checks
// (tests/host/host_wasserstein.cpp); the product only ever runs them inside the kernels and the entry.  The definition in NumPy
// is wasserstein.py.
//
// Summation order of one element (a_i, b_j), a function of K and p alone: the K terms are cut at multiples of kChunk (256),
// kGroup1 (1024) and kGroup2 (4096).  A chunk is summed term by term in the order of k; a kGroup1 block is the sum, in order, of
// its chunk sums; a kGroup2 block the sum, in order, of its kGroup1 sums; the element the sum, in order, of its kGroup2 sums.
// Every partial sum starts from +0, and the terms are non-negative, so a block that is cut short by K (or is missing) adds +0 and
// changes no bit.  A workgroup therefore may own the whole of K, or one aligned block of any of the three sizes: the finishing
// pass adds the levels above the block (combine_parts) and the bits are the same whichever split the launch chose.
#pragma once
#include <math.h>

#ifndef RC_HD
#if defined(__HIPCC__)
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif
#endif

namespace rcwd {

constexpr int kTile = 64;                 // a workgroup owns kTile x kTile elements (i, j)
constexpr int kReg = 4;                   // a thread owns kReg x kReg of them
constexpr int kThreads = (kTile / kReg) * (kTile / kReg);   // 256
constexpr int kStep = 32;                 // k values staged in LDS at a time
constexpr int kLdsStride = kTile + 2;     // doubles per k of an LDS image: rows stay 16-byte aligned, and the staging stores of
                                          // 16 consecutive lanes (8 k x 2 rows: 132 k + 2 row dwords) fall on 32 distinct banks
constexpr long long kChunk = 256, kGroup1 = 1024, kGroup2 = 4096;
constexpr long long kWholeK = 0;          // Plan::unit of a launch that is not split
constexpr long long kFillWorkgroups = 1024;   // a launch is split until it has this many workgroups (256 CUs, 4 waves each, x 4)

template <int P>
RC_HD double add_term(double acc, double a, double b) {
    const double d = a - b;
    if (P == 1) return acc + fabs(d);
    return fma(d, d, acc);
}

template <int P>
RC_HD double finish(double sum, long long K) {
    const double m = sum / (double)K;
    if (P == 1) return m;
    return sqrt(m);
}

// which of the kTile rows of a tile thread coordinate t (0 .. 15) owns: r = 0 .. 3 -> 2 t, 2 t + 1, 32 + 2 t, 33 + 2 t (two 16-byte
// pairs: the 16 lanes of a ds_read_b128 group read 256 contiguous bytes)
RC_HD int owned_row(int t, int r) { return (r >> 1) * (kTile / 2) + 2 * t + (r & 1); }

// Split of K over workgroups: every part but the last covers `unit` values of k, part q the range [q unit, min(K, (q + 1) unit)).
struct Plan {
    long long unit;     // kWholeK, kGroup2, kGroup1 or kChunk
    long long nparts;   // 1: the tile kernel writes the result; above 1: partial sums [nparts][CA][CB], then the finishing pass
    RC_HD long long begin(long long q) const { return unit == kWholeK ? 0 : q * unit; }
    RC_HD long long end(long long q, long long K) const {
        if (unit == kWholeK) return K;
        const long long e = (q + 1) * unit;
        return e < K ? e : K;
    }
};

// The coarsest split that gives kFillWorkgroups workgroups, else the finest.  `tiles`: tiles of the launch (those on or above the
// diagonal in symmetric mode).  The result's bits do not depend on the choice.
RC_HD Plan choose_plan(long long tiles, long long K) {
    const long long units[3] = {kGroup2, kGroup1, kChunk};
    if (tiles >= kFillWorkgroups || K <= kChunk) return Plan{kWholeK, 1};
    for (int l = 0; l < 3; ++l) {
        const long long n = (K + units[l] - 1) / units[l];
        if (l == 2 || tiles * n >= kFillWorkgroups) return n > 1 ? Plan{units[l], n} : Plan{kWholeK, 1};
    }
    return Plan{kWholeK, 1};
}

// what the two kernels are given
struct Params {
    const double* a;    // [CA][K]
    const double* b;    // [CB][K]; = a in symmetric mode
    long long CA, CB, K;
    long long nti, ntj; // tiles along i and j
    long long tiles;    // tiles of the launch: nti ntj, or nti (nti + 1) / 2 in symmetric mode
    int sym;
    Plan plan;
    double* out;        // [CA][CB]
    double* part;       // [plan.nparts][CA][CB] when plan.nparts > 1
};

// What a workgroup's thread carries for one element: the running sums of the four levels.
struct Levels {
    double s0, s1, s2, s3;
};
RC_HD void levels_init(Levels& v) { v.s0 = v.s1 = v.s2 = v.s3 = 0.0; }
// after the term of index k (next = k + 1): close the blocks that end there (`last`: the range of the workgroup ends)
RC_HD void levels_close(Levels& v, long long next, bool last) {
    if (last || next % kChunk == 0) {
        v.s1 += v.s0;
        v.s0 = 0.0;
        if (last || next % kGroup1 == 0) {
            v.s2 += v.s1;
            v.s1 = 0.0;
            if (last || next % kGroup2 == 0) {
                v.s3 += v.s2;
                v.s2 = 0.0;
            }
        }
    }
}

// The sum of the terms k0 <= k < k1 in the order above; k0 is 0 or a multiple of the plan's unit.  (The kernel runs the same
// recurrence kStep terms at a time, with +0 terms beyond k1.)
template <int P>
RC_HD double range_sum(const double* a, const double* b, long long k0, long long k1) {
    Levels v;
    levels_init(v);
    for (long long k = k0; k < k1; ++k) {
        v.s0 = add_term<P>(v.s0, a[k], b[k]);
        levels_close(v, k + 1, k + 1 == k1);
    }
    return v.s3;
}

// The levels above a split: part q of `nparts` (each the range_sum of `unit` values of k) is at part[q * stride].
RC_HD double combine_parts(const double* part, long long stride, long long nparts, long long unit) {
    Levels v;
    levels_init(v);
    for (long long q = 0; q < nparts; ++q) {
        const long long next = (q + 1) * unit;
        const bool last = q + 1 == nparts;
        const double x = part[q * stride];
        if (unit == kChunk) {
            v.s1 += x;
            if (last || next % kGroup1 == 0) {
                v.s2 += v.s1;
                v.s1 = 0.0;
            }
        } else if (unit == kGroup1) {
            v.s2 += x;
        }
        if (unit == kGroup2) {
            v.s3 += x;
        } else if (last || next % kGroup2 == 0) {
            v.s3 += v.s2;
            v.s2 = 0.0;
        }
    }
    return v.s3;
}

// one element from its two sorted rows, as the launch computes it under plan `pl`
template <int P>
inline double element(const double* a, const double* b, long long K, Plan pl) {
    if (pl.nparts == 1) return finish<P>(range_sum<P>(a, b, 0, K), K);
    double part[64];
    double total;
    if (pl.nparts <= 64) {
        for (long long q = 0; q < pl.nparts; ++q) part[q] = range_sum<P>(a, b, pl.begin(q), pl.end(q, K));
        total = combine_parts(part, 1, pl.nparts, pl.unit);
    } else {
        double* big = new double[pl.nparts];
        for (long long q = 0; q < pl.nparts; ++q) big[q] = range_sum<P>(a, b, pl.begin(q), pl.end(q, K));
        total = combine_parts(big, 1, pl.nparts, pl.unit);
        delete[] big;
    }
    return finish<P>(total, K);
}

// Argument checks of rc_wasserstein_matrix_f64(_async), in the entry's order, before any HIP call: NULL, or the message.
inline const char* check_args(int p, long long CA, long long CB, long long K) {
    if (p != 1 && p != 2) return "p must be 1 or 2";
    if (CA < 0 || CB < 0 || K < 0) return "CA, CB and K must be non-negative";
    return nullptr;
}
inline const char* check_sizes(long long CA, long long CB, long long K) {
    (void)K;
    if (CA > 0x7fffffffLL || CB > 0x7fffffffLL) return "too many rows for one launch";
    return nullptr;
}

}  // namespace rcwd

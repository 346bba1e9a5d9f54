// Per-lane pieces of the on-device bootstrap (bootstrap_replicates_kernel, bootstrap_summary_kernel: k_bootstrap.inc.h) - plain
// C++ so that the CPU unit test runs the exact counter layout, index rule, accumulation order and argument checks
// (tests/host/host_bootstrap.cpp); the product only ever runs them inside the kernels and the entry.  The definition in NumPy is
// bootstrap.py.
//
// Index stream: Philox4x32-10 keyed by the seed, counter high words 0.  With Q = ceil(K / 4), draw t of replicate b of row c is
// word (t & 3) of counter offset + (c B + b) Q + (t >> 2), and idx = (word * K) >> 32: no rejection step (the bias, below
// K / 2^32, is part of the definition).  One WAVE owns one replicate: lane l takes the quads l, l + 64, ... in turn, the four
// draws of a quad in order, and the 64 partial results meet in a fixed butterfly (lane_xor 32, 16, ... 1): the summation order
// depends on K alone.
#pragma once
#include <math.h>

#ifndef RC_HD
#if defined(__HIPCC__)
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif
#endif

namespace rcboot {

constexpr int kMaxQ = 8;                  // thresholds, as in the reduce entry
constexpr int kThreads = 1024;            // one workgroup: 16 waves, each on a replicate of its own
constexpr int kWaves = kThreads / 64;
// the LDS route keeps the row in LDS: 18 432 doubles = 144 KiB of a CU's 160 KiB, the rest for the row pass's partial sums
constexpr long long kLdsMaxK = 18432;
constexpr long long kMaxB = 16384;        // the summary sorts a replicate row with the one-launch merge sort (kSortChunk)
constexpr int kFixedMetrics = 3;          // rim1, std, min; then q[0 .. nq)
constexpr int kSummaryFields = 4;         // mean, standard error, lower, upper

RC_HD long long quads(long long K) { return (K + 3) >> 2; }

// first counter of replicate b of row c
RC_HD unsigned long long replicate_counter(unsigned long long offset, unsigned long long c, unsigned long long B, unsigned long long b,
                                           unsigned long long Q) {
    return offset + (c * B + b) * Q;
}

RC_HD unsigned int draw_index(unsigned int word, unsigned int K) { return (unsigned int)(((unsigned long long)word * K) >> 32); }

// Philox4x32-10 in plain C++ (the device runs philox_core.inc.h's, which is the same function)
RC_HD void philox4x32_10_plain(unsigned long long ctr, unsigned long long seed, unsigned int (&o)[4]) {
    unsigned int c0 = (unsigned int)ctr, c1 = (unsigned int)(ctr >> 32), c2 = 0u, c3 = 0u;
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned int)p1;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned int)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
struct PlainPhilox {
    unsigned long long seed;
    RC_HD void operator()(unsigned long long ctr, unsigned int (&o)[4]) const { philox4x32_10_plain(ctr, seed, o); }
};

// what a lane carries through a replicate: sums of g = f - m and g^2, the minimum, the threshold counts
template <int NQ>
struct Acc {
    double s1, s2, mn;
    unsigned int cnt[NQ > 0 ? NQ : 1];
};

template <int NQ>
RC_HD void acc_init(Acc<NQ>& a) {
    a.s1 = 0.0;
    a.s2 = 0.0;
    a.mn = __builtin_inf();
    for (int i = 0; i < NQ; ++i) a.cnt[i] = 0u;
}

template <int NQ>
RC_HD void acc_add(Acc<NQ>& a, double f, double m, const double* thr) {
    const double g = f - m;
    a.s1 += g;
    a.s2 = fma(g, g, a.s2);
    a.mn = fmin(a.mn, f);
    for (int i = 0; i < NQ; ++i) a.cnt[i] += (f >= thr[i]) ? 1u : 0u;
}

// one butterfly step: `a` takes in its partner's partial results (addition and min commute: both partners end up equal)
template <int NQ>
RC_HD void acc_merge(Acc<NQ>& a, const Acc<NQ>& o) {
    a.s1 += o.s1;
    a.s2 += o.s2;
    a.mn = fmin(a.mn, o.mn);
    for (int i = 0; i < NQ; ++i) a.cnt[i] += o.cnt[i];
}

// Lane `lane` of the wave that owns the replicate whose first counter is `base`: its quads in turn.  `row(idx)` reads a value,
// `rng(ctr, words)` is Philox4x32-10 of the call's seed.  The last quad of a row whose length is no multiple of four is cut.
template <int NQ, class Row, class Rng>
RC_HD void lane_accumulate(Acc<NQ>& a, const Row& row, const Rng& rng, unsigned long long base, int lane, int K, double m,
                           const double* thr) {
    const int full = K >> 2;
    unsigned int w[4];
    for (int q = lane; q < full; q += 64) {
        rng(base + (unsigned long long)q, w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 4; ++j) acc_add<NQ>(a, row(draw_index(w[j], (unsigned int)K)), m, thr);
    }
    if ((K & 3) != 0 && lane == (full & 63)) {
        rng(base + (unsigned long long)full, w);
        for (int j = 0; j < (K & 3); ++j) acc_add<NQ>(a, row(draw_index(w[j], (unsigned int)K)), m, thr);
    }
}

// the replicate's rim1 and std from the wave's totals
RC_HD void replicate_finish(double s1, double s2, double m, int K, double* rim1, double* stdv) {
    const double mg = s1 / (double)K;
    *rim1 = 1.0 - (m + mg);
    *stdv = sqrt(fmax(0.0, fma(-mg, mg, s2 / (double)K)));
}

// standard error of B replicates from ss = sum (x - mean)^2: their std with ddof = 1, NaN for one replicate
RC_HD double standard_error(double ss, long long B) { return B > 1 ? sqrt(ss / (double)(B - 1)) : __builtin_nan(""); }

// Argument checks of rc_bootstrap_metrics_f64(_async), in the entry's order, before any HIP call: NULL, or the message.
inline const char* check_args(long long C, long long K, long long B, int nq, bool thr_null, long long rank_lo, long long rank_hi,
                              int route, unsigned long long offset, bool fid_null) {
    if (C < 0) return "C must be non-negative";
    if (K < 1) return "K must be positive";
    if (K > 0x7fffffffLL) return "K must be at most 2^31 - 1";
    if (B < 1) return "B must be positive";
    if (B > kMaxB) return "B must be at most 16384 (the row sort behind the summary)";
    if (nq < 0 || nq > kMaxQ) return "nq must be in [0, 8]";
    if (nq > 0 && thr_null) return "q_thresholds is NULL";
    if (rank_lo < 0 || rank_lo > rank_hi || rank_hi >= B) return "ranks must satisfy 0 <= rank_lo <= rank_hi < B";
    if (route < 0 || route > 2) return "route must be 0 (auto), 1 (LDS) or 2 (global)";
    if (route == 1 && K > kLdsMaxK) return "route 1 (LDS) holds rows of at most 18432 values";
    if (C > 0x7fffffffLL / 16) return "too many rows for one launch";
    const unsigned __int128 span = (unsigned __int128)(unsigned long long)C * (unsigned long long)B * (unsigned long long)quads(K);
    if ((unsigned __int128)offset + span > ((unsigned __int128)1 << 64)) return "offset + C * B * ceil(K / 4) wraps 2^64";
    if (C > 0 && fid_null) return "NULL fid pointer";
    return nullptr;
}

// Workgroups per row: the replicates of a row are spread over `splits` workgroups so that few rows still fill the device
// (256 CUs, one workgroup each).  Among 1 .. 1024 / C (and no more than there are groups of kWaves replicates) the count that
// wastes least of the last round of workgroups; the results do not depend on it.
inline int choose_splits(long long C, long long B) {
    const long long cus = 256, most_b = (B + kWaves - 1) / kWaves;
    long long most = C > 0 ? 1024 / C : 1;
    if (most > most_b) most = most_b;
    if (most < 1) most = 1;
    long long best = 1;
    double best_score = -1.0;
    for (long long s = 1; s <= most; ++s) {
        const long long blocks = C * s, rounds = (blocks + cus - 1) / cus;
        const double score = (double)blocks / (double)(rounds * cus);
        if (score > best_score + 1e-9) {
            best_score = score;
            best = s;
        }
    }
    return (int)best;
}

}  // namespace rcboot

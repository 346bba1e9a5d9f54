// The per-lane functions of csrc/bootstrap_core.h - counter layout, index rule, accumulation, butterfly, finish, argument checks -
// run on the CPU the way bootstrap_replicates_kernel and bootstrap_summary_kernel run them (64 lanes of a wave in a loop), on the
// cases of tests/bootstrap_checks.py read from a file, against the values of bootstrap.py (NumPy) in the same file.
// Stand-alone: g++ -std=c++17 host_bootstrap.cpp; also built with -fsanitize=address,undefined (tests/test_host_bootstrap.py).
//
// file: int64 ncases, then per case: int64 C, K, B; uint64 seed, offset; int64 nq; double thr[nq]; int64 rank_lo, rank_hi;
// double fid[C][K]; double rep[M][C][B]; double summary[M][4][C]  (M = 3 + nq; the last two are NumPy's).
// min and q K must be equal; 1 - rim1 within K 2^-52, std^2 within 4 K 2^-52 (two summation orders of values in [0, 1], each
// inside half of that); the summary's mean and picks within the metric's bound, SE^2 within 4 B 2^-52 + the metric's bound.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../code-robchar_amd/csrc/bootstrap_core.h"

namespace {

bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

// the 64 partial results of a wave meet as in boot_wave_merge: lane l takes in lane l ^ off, off = 32 .. 1
template <class T, class Merge>
void butterfly(T (&lane)[64], Merge merge) {
    for (int off = 32; off >= 1; off >>= 1) {
        T next[64];
        for (int l = 0; l < 64; ++l) {
            next[l] = lane[l];
            merge(next[l], lane[l ^ off]);
        }
        for (int l = 0; l < 64; ++l) lane[l] = next[l];
    }
}

// the row pass: 1024 thread partial sums, wave butterflies, the 16 waves in index order
double row_mean(const double* row, long long K, bool* bad) {
    double part[rcboot::kWaves];
    *bad = false;
    for (int w = 0; w < rcboot::kWaves; ++w) {
        double lane[64];
        for (int l = 0; l < 64; ++l) {
            lane[l] = 0.0;
            for (long long k = 64 * w + l; k < K; k += rcboot::kThreads) {
                lane[l] += row[k];
                *bad |= row[k] != row[k];
            }
        }
        butterfly(lane, [](double& a, const double& b) { a += b; });
        part[w] = lane[0];
    }
    double m = part[0];
    for (int w = 1; w < rcboot::kWaves; ++w) m += part[w];
    return m / (double)K;
}

template <int NQ>
void replicate(const double* row, int K, double m, unsigned long long seed, unsigned long long base, const double* thr, int nq,
               double* out /*[3 + nq]*/) {
    rcboot::Acc<NQ> lane[64];
    const rcboot::PlainPhilox rng{seed};
    for (int l = 0; l < 64; ++l) {
        rcboot::acc_init<NQ>(lane[l]);
        rcboot::lane_accumulate<NQ>(lane[l], [&](unsigned int i) { return row[i]; }, rng, base, l, K, m, thr);
    }
    butterfly(lane, [](rcboot::Acc<NQ>& a, const rcboot::Acc<NQ>& b) { rcboot::acc_merge<NQ>(a, b); });
    rcboot::replicate_finish(lane[0].s1, lane[0].s2, m, K, &out[0], &out[1]);
    out[2] = lane[0].mn;
    for (int i = 0; i < nq; ++i) out[3 + i] = (double)lane[0].cnt[i] / (double)K;
}

bool same_nan(double a, double b) { return (a != a) == (b != b); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ncases = 0;
    if (!read_all(f, &ncases, 8)) return 2;
    const double U = std::ldexp(1.0, -52);
    for (int64_t id = 0; id < ncases; ++id) {
        int64_t C, K, B, nq, rank_lo, rank_hi;
        uint64_t seed, offset;
        double thr[rcboot::kMaxQ];
        for (double& t : thr) t = INFINITY;
        if (!read_all(f, &C, 8) || !read_all(f, &K, 8) || !read_all(f, &B, 8) || !read_all(f, &seed, 8) || !read_all(f, &offset, 8) ||
            !read_all(f, &nq, 8) || nq < 0 || nq > rcboot::kMaxQ || !read_all(f, thr, 8 * nq) || !read_all(f, &rank_lo, 8) ||
            !read_all(f, &rank_hi, 8))
            return 2;
        if (const char* msg = rcboot::check_args(C, K, B, (int)nq, false, rank_lo, rank_hi, 0, offset, false)) {
            printf("case %lld: refused: %s\n", (long long)id, msg);
            return 1;
        }
        const int64_t M = 3 + nq;
        std::vector<double> fid(C * K), want_rep(M * C * B), want_sum(M * 4 * C), rep(M * C * B), sum(M * 4 * C);
        if (!read_all(f, fid.data(), 8 * fid.size()) || !read_all(f, want_rep.data(), 8 * want_rep.size()) ||
            !read_all(f, want_sum.data(), 8 * want_sum.size()))
            return 2;
        const unsigned long long Q = (unsigned long long)rcboot::quads(K);
        for (int64_t c = 0; c < C; ++c) {
            bool bad;
            const double m = row_mean(&fid[c * K], K, &bad);
            for (int64_t b = 0; b < B; ++b) {
                double out[3 + rcboot::kMaxQ];
                if (bad)
                    for (double& v : out) v = NAN;
                else if (nq <= 2)
                    replicate<2>(&fid[c * K], (int)K, m, seed, rcboot::replicate_counter(offset, c, B, b, Q), thr, (int)nq, out);
                else
                    replicate<rcboot::kMaxQ>(&fid[c * K], (int)K, m, seed, rcboot::replicate_counter(offset, c, B, b, Q), thr, (int)nq, out);
                for (int64_t j = 0; j < M; ++j) rep[(j * C + c) * B + b] = out[j];
            }
        }
        // the summary as bootstrap_summary_kernel forms it
        for (int64_t r = 0; r < M * C; ++r) {
            const double* x = &rep[r * B];
            double lane[64];
            for (int l = 0; l < 64; ++l) {
                lane[l] = 0.0;
                for (int64_t b = l; b < B; b += 64) lane[l] += x[b];
            }
            butterfly(lane, [](double& a, const double& b) { a += b; });
            const double mean = lane[0] / (double)B;
            for (int l = 0; l < 64; ++l) {
                lane[l] = 0.0;
                for (int64_t b = l; b < B; b += 64) lane[l] = fma(x[b] - mean, x[b] - mean, lane[l]);
            }
            butterfly(lane, [](double& a, const double& b) { a += b; });
            std::vector<double> srt(x, x + B);
            if (!(x[0] != x[0])) std::sort(srt.begin(), srt.end());
            double* o = &sum[(r / C) * 4 * C + r % C];
            o[0] = mean;
            o[C] = rcboot::standard_error(lane[0], B);
            o[2 * C] = srt[rank_lo];
            o[3 * C] = srt[rank_hi];
        }
        // comparison
        int bad_at = -1;
        double worst = 0.0;
        auto differs = [&](int what, double err, double bound) {
            if (!(err <= bound)) {
                bad_at = what;
                worst = err;
            }
        };
        const double bm = (double)K * U, bv = 4.0 * (double)K * U;
        for (int64_t j = 0; j < M; ++j)
            for (int64_t i = 0; i < C * B; ++i) {
                const double a = rep[j * C * B + i], w = want_rep[j * C * B + i];
                if (!same_nan(a, w)) differs((int)j, INFINITY, 0.0);
                else if (a != a) continue;
                else if (j == 0) differs(0, std::fabs(a - w), bm);
                else if (j == 1) differs(1, std::fabs(a * a - w * w), bv);
                else differs((int)j, std::fabs(a - w), 0.0);
            }
        for (int64_t j = 0; j < M; ++j)
            for (int64_t c = 0; c < C; ++c) {
                const double bound = j == 0 ? bm : (j == 1 ? std::sqrt(bv) : 0.0);           // |a - w| <= sqrt|a^2 - w^2| for a, w >= 0
                for (int fld = 0; fld < 4; ++fld) {
                    const double a = sum[(j * 4 + fld) * C + c], w = want_sum[(j * 4 + fld) * C + c];
                    if (!same_nan(a, w)) differs(100 + fld, INFINITY, 0.0);
                    else if (a != a) continue;
                    else if (fld == 1) differs(101, std::fabs(a * a - w * w), 4.0 * (double)B * U + 4.0 * bound);
                    else differs(100 + fld, std::fabs(a - w), bound + (fld == 0 ? (double)B * U : 0.0));
                }
            }
        if (bad_at >= 0) {
            printf("case %lld (C %lld K %lld B %lld): differs at %d by %.3e\n", (long long)id, (long long)C, (long long)K, (long long)B,
                   bad_at, worst);
            return 1;
        }
        printf("case %lld ok\n", (long long)id);
    }
    fclose(f);
    printf("OK\n");
    return 0;
}

// Bootstrap of the per-controller metrics, resampled on the device (rc_bootstrap_metrics_f64_async; the definition is
// bootstrap.py, the per-lane arithmetic bootstrap_core.h).
//
// Part of ONE translation unit: this file is #included by robchar_hip.hip INSIDE its anonymous namespace, behind
// k_reduce_sort.inc.h and philox_core.inc.h; it is not a stand-alone header.
//
// bootstrap_replicates_kernel<NQ, LDS>: 1024 threads.  Workgroup (c, part) stages row c once - LDS route: into LDS, 80 KB for the
// paper's K = 10^4, which fits a gfx950 CU's 160 KiB; global route (rows beyond kLdsMaxK): the row stays where it is, in L2 - and
// forms the row's mean m in a fixed order (thread partial sums, wave butterfly, the 16 waves in index order; the same order in both
// routes and in every workgroup of the row).  Then its waves take the replicates part * 16 + wave, + splits * 16, ...: ONE WAVE owns
// one replicate.  A lane makes one Philox call per four draws, then 4 x (mul_hi, read, subtract, two accumulations, min, NQ compares);
// the 64 partial results meet in a fixed butterfly.  No atomics, no workspace: same inputs, same bits, whatever `splits` is.
// A row holding a NaN gives NaN in every output.
// CONTROL FLOW: the barriers sit in the row pass, which every thread runs; behind it a wave only returns or loops on its own.
struct BootParams {
    const double* fid;     // [C][K]
    long long C, K, B;
    unsigned long long seed, offset;
    int nq, splits;
    double thr[rcboot::kMaxQ];
    double* rep;           // [3 + nq][C][B]
};

struct BootPhilox {
    unsigned int k0, k1;
    __device__ __forceinline__ void operator()(unsigned long long ctr, unsigned int (&o)[4]) const {
        philox4x32_10((unsigned int)ctr, (unsigned int)(ctr >> 32), 0u, 0u, k0, k1, o);
    }
};

template <int NQ>
__device__ __forceinline__ void boot_wave_merge(rcboot::Acc<NQ>& a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        rcboot::Acc<NQ> o;
        o.s1 = __shfl_xor(a.s1, off, 64);
        o.s2 = __shfl_xor(a.s2, off, 64);
        o.mn = __shfl_xor(a.mn, off, 64);
#pragma unroll
        for (int i = 0; i < NQ; ++i) o.cnt[i] = __shfl_xor(a.cnt[i], off, 64);
        rcboot::acc_merge<NQ>(a, o);
    }
}

template <int NQ, bool LDS>
__global__ __launch_bounds__(rcboot::kThreads) void bootstrap_replicates_kernel(const BootParams p) {
    constexpr int kWaves = rcboot::kWaves;
    __shared__ double srow[LDS ? rcboot::kLdsMaxK : 1];
    __shared__ double part[kWaves];
    const long long c = blockIdx.x / p.splits;
    const int piece = (int)(blockIdx.x % p.splits);
    const int K = (int)p.K;
    const double* row = p.fid + c * p.K;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

    // row pass
    double sum = 0.0;
    int bad = 0;
    for (int k = threadIdx.x; k < K; k += rcboot::kThreads) {
        const double v = row[k];
        if (LDS) srow[k] = v;
        sum += v;
        bad |= (v != v);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) part[wave] = sum;
    bad = __syncthreads_or(bad);                           // (the row in LDS and the wave sums are visible behind it)
    double m = part[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m += part[w];
    m /= (double)K;

    const int M = rcboot::kFixedMetrics + p.nq;
    const long long CB = p.C * p.B;
    const long long stride = (long long)p.splits * kWaves;
    if (bad) {
        const double nan = __builtin_nan("");
        for (long long b = (long long)piece * kWaves + wave; b < p.B; b += stride)
            for (int j = lane; j < M; j += 64) p.rep[j * CB + c * p.B + b] = nan;
        return;
    }
    const unsigned long long Q = (unsigned long long)rcboot::quads(p.K);
    const BootPhilox rng{(unsigned int)p.seed, (unsigned int)(p.seed >> 32)};
    for (long long b = (long long)piece * kWaves + wave; b < p.B; b += stride) {
        const unsigned long long base = rcboot::replicate_counter(p.offset, (unsigned long long)c, (unsigned long long)p.B,
                                                                  (unsigned long long)b, Q);
        rcboot::Acc<NQ> a;
        rcboot::acc_init<NQ>(a);
        if (LDS)
            rcboot::lane_accumulate<NQ>(a, [&](unsigned int i) { return srow[i]; }, rng, base, lane, K, m, p.thr);
        else
            rcboot::lane_accumulate<NQ>(a, [&](unsigned int i) { return row[i]; }, rng, base, lane, K, m, p.thr);
        boot_wave_merge<NQ>(a);
        if (lane == 0) {
            double rim1, stdv;
            rcboot::replicate_finish(a.s1, a.s2, m, K, &rim1, &stdv);
            double* out = p.rep + c * p.B + b;
            out[0] = rim1;
            out[CB] = stdv;
            out[2 * CB] = a.mn;
#pragma unroll
            for (int i = 0; i < NQ; ++i)
                if (i < p.nq) out[(rcboot::kFixedMetrics + i) * CB] = (double)a.cnt[i] / (double)K;
        }
    }
}

// Summary of the replicates: one wave per (metric, row), four per workgroup.  rep [R][B] as the replicate kernel wrote it, sorted
// [R][B] the same rows in ascending order (sort_rows_merge_kernel; a NaN row is copied through, so its picks are NaN).  Mean and
// the centred sum of squares in a fixed order (lane partial sums over b = lane, lane + 64, ..., butterfly), two passes.
// out [M][4][C]: row r = metric * C + c goes to out[(metric * 4 + field) * C + c].
__global__ __launch_bounds__(256) void bootstrap_summary_kernel(const double* rep, const double* sorted, long long R, long long C,
                                                                long long B, long long rank_lo, long long rank_hi, double* out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + wave;
    if (r >= R) return;                                     // wave-uniform (the kernel has no barrier)
    const double* x = rep + r * B;
    double sum = 0.0;
    for (long long b = lane; b < B; b += 64) sum += x[b];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const double mean = sum / (double)B;
    double ss = 0.0;
    for (long long b = lane; b < B; b += 64) {
        const double d = x[b] - mean;
        ss = fma(d, d, ss);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (lane == 0) {
        const long long metric = r / C, c = r % C;
        double* o = out + metric * rcboot::kSummaryFields * C + c;
        o[0] = mean;
        o[C] = rcboot::standard_error(ss, B);
        o[2 * C] = sorted[r * B + rank_lo];
        o[3 * C] = sorted[r * B + rank_hi];
    }
}

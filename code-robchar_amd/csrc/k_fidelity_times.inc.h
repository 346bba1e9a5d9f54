// Lane-per-sample kernels of the chain fidelity on a GRID OF READOUT TIMES from one eigen decomposition per sample (times_core.h):
// mc_fid_times_kernel<N> reads the (C, K, N, 3) draw tensor, mc_fid_times_philox_kernel<N> generates the counter-based draws where
// they are consumed; N = 2 .. RC_MAX_NSPIN_FAST.
//
// Included by robchar_times.hip inside its anonymous namespace (after philox_core.inc.h); not a stand-alone header.
// Same tiling as mc_fid_chain_kernel (k_fidelity_chain.inc.h): one wave per 64-sample tile of ONE controller, the controller row
// wave-uniform.  The tensor kernel brings the tile's draws in by LDS-DMA in phases with the streaming load policy and reads them
// back transposed (stage_tile_draws); the other one regenerates them with philox_lane_draws (philox_core.inc.h; stream element
// offset + ((c K + k) N + i) 3 + s), so its outputs are bit-identical to philox_normal followed by the tensor kernel.
//
// Outputs (each optional): fid[M][C][K] - M slabs, each an ordinary [C][K] fidelity tensor: a wave stores 64 consecutive doubles
// per time -, wsum[C][K] and fmin[C][K] (TimesAcc).  A NaN controller row gives NaN in every output; its draws are not read.
// The grid (tscale, tshift, weights: [M] each or NULL) is wave-uniform and read through the scalar path inside the rolled loop.
//
// Registers: the QL phase holds what the rows mode of mc_fid_chain_kernel holds (4 N doubles); the time loop holds 2 N doubles
// (weights, eigenvalue differences) and the two accumulators.  Launch bounds below are chosen from the listing (`make asm`;
// tests/test_asm_times.py fails on any spill; DESIGN.md has the table).

constexpr int times_min_waves(int n) { return n <= 8 ? 5 : (n <= 12 ? 3 : 2); }
constexpr int times_philox_min_waves(int n) { return n >= 14 ? 1 : (times_min_waves(n) > 3 ? 3 : times_min_waves(n)); }
constexpr int times_phases(int n) { return n <= 2 ? 1 : (n <= 8 ? 2 : 4); }

struct TimesLdsVec {
    double* base;
    int stride;
    __device__ __forceinline__ double& operator[](int i) const { return base[i * stride]; }
};

// where a lane writes its F_j: slab j of fid at sdst[j * slab] (the `store` of times_core.h's loops)
struct TimesDst {
    double* sdst;          // fid + c K + kb + lane, or NULL
    long long slab;        // C K
    __device__ __forceinline__ void operator()(int j, double f) const {
        if (sdst) sdst[j * slab] = f;
    }
};

// NaN-padded controller row: NaN in every output of the tile
__device__ __forceinline__ void times_fill_nan(const TimesParams& p, long long at, int lane, int nk) {
    const double nan = __builtin_nan("");
    if (lane >= nk) return;
    if (p.fid) {
#pragma unroll 1
        for (int j = 0; j < p.M; ++j) p.fid[j * (p.C * p.K) + at + lane] = nan;
    }
    if (p.wsum) p.wsum[at + lane] = nan;
    if (p.fmin) p.fmin[at + lane] = nan;
}

template <int N>
__global__ __launch_bounds__(64, times_min_waves(N)) void mc_fid_times_kernel(const TimesParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int PH = times_phases(N);
    constexpr int SP = 64 / PH;                    // samples per staging phase
    constexpr int CH = (SP * G) / (4 * N);         // samples of the textbook routine that fit the staging buffer at a time
    static_assert(CH >= 1, "staging buffer too small for the textbook routine");
    __shared__ __attribute__((aligned(16))) double stage[SP * G];
    __shared__ __attribute__((aligned(16))) double sctab[128];   // sincos_table's table, one copy per wave (1 KiB)

    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;             // wave-uniform
    reinterpret_cast<double2*>(sctab)[lane] = reinterpret_cast<const double2*>(g_sincos_table)[lane];
    __builtin_amdgcn_s_setprio(3);                 // (the staging phase at raised priority: see mc_fid_chain_kernel)
    const long long c = tile / p.tiles_per_ctrl;
    const long long kb = (tile - c * p.tiles_per_ctrl) * 64;
    const int nk = (int)((p.K - kb < 64) ? (p.K - kb) : 64);

    const double* xg = p.ctrl + c * (N + 1);       // controller row: wave-uniform -> scalar registers
    double x[N + 1];
    bool pad = false;
#pragma unroll
    for (int i = 0; i <= N; ++i) {
        x[i] = xg[i];
        pad |= (x[i] != x[i]);
    }
    const long long at = c * p.K + kb;
    if (pad) {                                     // no draws read
        times_fill_nan(p, at, lane, nk);
        return;
    }

    // HBM -> LDS -> registers (see mc_fid_chain_kernel): the tile's draws are one contiguous run of nk * G doubles
    const char* src = (const char*)(p.draws + c * p.draw_cstride + kb * G);
    double gl[G];
    stage_tile_draws<G, PH>(src, nk, lane, p.align16, stage, gl);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();                               // the table copy has landed (one wave per workgroup: no wait)

    const TimesDst dst{p.fid ? p.fid + at + lane : nullptr, p.C * p.K};
    rc::TimesAcc acc{0.0, 0.0};
    bool ok = true;
    {
        double dl[N], w[N];
        if (lane < nk) ok = rc::times_eigen_fast<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, p.in, p.out, dl, w);
        if (lane < nk && ok) rc::times_loop_fast<N>(dl, w, x[N], p.M, p.tscale, p.tshift, p.weights, sctab, dst, acc);
    }
    const unsigned long long badmask = __ballot(lane < nk && !ok);
    if (badmask != 0ull) {
        // Rare (H = 0 exactly; times_core.h): some lane's QL ran into the sweep cap.  Those lanes take the textbook routine, CH at
        // a time, work vectors (4 N doubles per sample) in the staging buffer, which is free now; draws re-read from HBM; the time
        // loop inside.
        if (lane == 0) atomicAdd(&g_times_general_tiles, 1ull);
        const bool bad = (badmask >> lane) & 1ull;
        const int rank = __popcll(badmask & ((1ull << lane) - 1ull));     // position among the bad lanes
        const int nbad = __popcll(badmask);
#pragma unroll 1
        for (int c0 = 0; c0 < nbad; c0 += CH) {
            const int rel = rank - c0;
            if (bad && rel >= 0 && rel < CH) {
                const TimesLdsVec vd{stage + rel, CH}, ve{stage + N * CH + rel, CH}, va{stage + 2 * N * CH + rel, CH},
                    vb{stage + 3 * N * CH + rel, CH};
                rc::times_general(N, xg, p.h0.diag, p.h0.off, (const double*)src + (long long)lane * G, p.in, p.out, vd, ve, va, vb,
                                  p.M, p.tscale, p.tshift, p.weights, dst, acc);
            }
        }
    }
    if (lane < nk) {
        if (p.wsum) p.wsum[at + lane] = acc.wsum;
        if (p.fmin) p.fmin[at + lane] = acc.fmin;
    }
}

template <int N>
__global__ __launch_bounds__(64, times_philox_min_waves(N)) void mc_fid_times_philox_kernel(const TimesParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int CH = 4;                          // lanes per pass of the textbook routine (draws and work vectors in LDS)
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ __attribute__((aligned(16))) double work[(4 * N + G) * CH];

    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;             // wave-uniform
    philox_stage_tables(lane, sctab, lntab);
    const long long c = tile / p.tiles_per_ctrl;
    const long long kb = (tile - c * p.tiles_per_ctrl) * 64;
    const int nk = (int)((p.K - kb < 64) ? (p.K - kb) : 64);

    const double* xg = p.ctrl + c * (N + 1);       // controller row: wave-uniform -> scalar registers
    double x[N + 1];
    bool pad = false;
#pragma unroll
    for (int i = 0; i <= N; ++i) {
        x[i] = xg[i];
        pad |= (x[i] != x[i]);
    }
    const long long at = c * p.K + kb;
    if (pad) {                                     // its draws are not generated
        times_fill_nan(p, at, lane, nk);
        return;
    }
    const double sigma = p.sigma_rows ? p.sigma_rows[c] : p.sigma;
    // this lane's G elements start at stream element E
    const unsigned long long E = p.offset + (unsigned long long)(at + lane) * (unsigned long long)G;
    double gl[G];
    if (lane < nk) philox_lane_draws<G>(p.seed, E, sigma, lntab, sctab, gl);

    const TimesDst dst{p.fid ? p.fid + at + lane : nullptr, p.C * p.K};
    rc::TimesAcc acc{0.0, 0.0};
    bool ok = true;
    {
        double dl[N], w[N];
        if (lane < nk) ok = rc::times_eigen_fast<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, p.in, p.out, dl, w);
        if (lane < nk && ok) rc::times_loop_fast<N>(dl, w, x[N], p.M, p.tscale, p.tshift, p.weights, sctab, dst, acc);
    }
    const unsigned long long badmask = __ballot(lane < nk && !ok);
    if (badmask != 0ull) {
        // rare: the textbook routine, CH lanes at a time; their draws are regenerated element by element into LDS
        if (lane == 0) atomicAdd(&g_times_general_tiles, 1ull);
        const bool bad = (badmask >> lane) & 1ull;
        const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
        const int nbad = __popcll(badmask);
#pragma unroll 1
        for (int c0 = 0; c0 < nbad; c0 += CH) {
            const int rel = rank - c0;
            if (bad && rel >= 0 && rel < CH) {
                double* g = work + 4 * N * CH + rel * G;
                for (int i = 0; i < G; ++i) g[i] = philox_element(p.seed, E + (unsigned long long)i, sigma, lntab, sctab);
                const TimesLdsVec vd{work + rel, CH}, ve{work + N * CH + rel, CH}, va{work + 2 * N * CH + rel, CH},
                    vb{work + 3 * N * CH + rel, CH};
                rc::times_general(N, xg, p.h0.diag, p.h0.off, g, p.in, p.out, vd, ve, va, vb, p.M, p.tscale, p.tshift, p.weights,
                                  dst, acc);
            }
        }
    }
    if (lane < nk) {
        if (p.wsum) p.wsum[at + lane] = acc.wsum;
        if (p.fmin) p.fmin[at + lane] = acc.fmin;
    }
}

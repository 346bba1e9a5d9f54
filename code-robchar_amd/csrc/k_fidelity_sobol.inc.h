// mc_fid_chain_sobol_kernel<N, MODE>: the chain fidelity kernel with scrambled Sobol normals generated WHERE THEY ARE CONSUMED.
// It is mc_fid_chain_philox_kernel (k_fidelity_philox.inc.h) with philox_lane_draws replaced by the Sobol leaf of sobol_core.h:
// the same tiling (one sample per lane, one 64-sample tile of ONE controller per wave), the same NaN-row rule, the same
// chain_fidelity_fast call, rows-mode repair, last-resort routine and counters.  Lane (c, k) makes its D = 3 N coordinates -
// dimension 3 i + s for site i, slot s - of point skip + (k mod P) of replicate k / P, exactly what sobol_draws_kernel stores
// there, so the fidelities are BIT-IDENTICAL to rc_draws_sobol_f64_async followed by the tensor kernel
// (tests/test_gpu_sobol.py).  The repair lanes regenerate their coordinates element by element from the same leaf.
//
// Part of ONE translation unit: #included by robchar_qmc.hip inside its anonymous namespace, after sobol_core.h.
constexpr int fid_sobol_min_waves(int n, int mode) {
    const int w = fid_min_waves(n, mode);
    return w > 3 ? 3 : w;                          // (as the Philox kernel: the coordinates live beside the matrix being formed)
}

template <int N, int MODE>
__global__ __launch_bounds__(64, fid_sobol_min_waves(N, MODE)) void mc_fid_chain_sobol_kernel(const FidParams p, const SobolDraws q) {
    constexpr int G = 3 * N;                       // doubles per sample = dimensions
    constexpr int CH = 4;                          // lanes per pass of the last-resort routine (work vectors in LDS)
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ __attribute__((aligned(16))) double work[(4 * N + G) * CH];
    __shared__ unsigned int base[64];              // G <= 39

    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;             // wave-uniform
    const long long c = tile / p.tiles_per_ctrl;
    const long long kb = (tile - c * p.tiles_per_ctrl) * 64;
    const int nk = (int)((p.K - kb < 64) ? (p.K - kb) : 64);
    const SobolTile t = sobol_tile(q, c, kb);
    sobol_tile_base(t, G, lane, base);
    philox_stage_tables(lane, sctab, lntab);       // (its barrier also covers `base`)

    const double* xg = p.ctrl + c * (N + 1);       // controller row: wave-uniform -> scalar registers
    double x[N + 1];
    bool pad = false;
#pragma unroll
    for (int i = 0; i <= N; ++i) {
        x[i] = xg[i];
        pad |= (x[i] != x[i]);
    }
    double* dst = p.fid + c * p.K + kb;
    if (pad) {                                     // NaN-padded controller: its points are not generated
        if (lane < nk) dst[lane] = __builtin_nan("");
        return;
    }
    const double sigma = q.sigma_rows ? q.sigma_rows[c] : q.sigma;
    const unsigned int gray = (unsigned int)(lane ^ (lane >> 1));
    const double* lt = lntab;
    const unsigned int* bs = base;
    const auto element = [t, bs, gray, sigma, lt](int i) { return sobol_draw(sobol_point(t, bs, gray, i), sigma, lt); };
    double gl[G];
    if (lane < nk) {
#pragma unroll
        for (int i = 0; i < G; ++i) gl[i] = element(i);
    }

    double f = 0.0;
    bool ok = true;
    int extra = 0;
    if (lane < nk)
        ok = rc::chain_fidelity_fast<N, MODE>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, p.in, p.out, sctab, f, nullptr,
                                              &extra);
    if (extra && lane == 0) atomicAdd(&g_polish_tiles[blockIdx.x & 63u], 1ull);
    unsigned long long badmask = __ballot(lane < nk && !ok);
    if (badmask) {
        if (lane == 0) atomicAdd(&g_general_tiles, 1ull);
        // rare: the eigenvector-rows route for the lanes the eigenvalue-only weights cannot take; their coordinates are regenerated
        // element by element (nothing of the fast path has to stay alive)
        const bool bad = (badmask >> lane) & 1ull;
        bool ok2 = true;
        if (bad) {
            double f2;
            ok2 = rc::chain_fidelity_fast<N, rc::kWeightsRows>(xg, p.h0.diag, p.h0.off, element, p.in, p.out, sctab, f2);
            if (ok2) f = f2;
        }
        badmask = __ballot(bad && !ok2);
    }
    if (badmask) {
        // last resort (the rows-mode QL at its sweep cap): the textbook per-sample routine, CH lanes at a time, coordinates and
        // work vectors in LDS
        const bool bad = (badmask >> lane) & 1ull;
        const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
        const int nbad = __popcll(badmask);
#pragma unroll 1
        for (int c0 = 0; c0 < nbad; c0 += CH) {
            const int rel = rank - c0;
            if (bad && rel >= 0 && rel < CH) {
                double* g = work + 4 * N * CH + rel * G;
                for (int i = 0; i < G; ++i) g[i] = element(i);
                const LdsVec vd{work + rel, CH}, ve{work + N * CH + rel, CH}, va{work + 2 * N * CH + rel, CH}, vb{work + 3 * N * CH + rel, CH};
                f = rc::chain_fidelity_general(N, xg, p.h0.diag, p.h0.off, g, p.in, p.out, vd, ve, va, vb);
            }
        }
    }
    if (lane < nk) dst[lane] = f;
}

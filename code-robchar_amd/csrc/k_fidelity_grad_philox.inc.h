// mc_fid_grad_philox_kernel<N> (N = 2 .. RC_MAX_NSPIN_GRAD): mc_fid_grad_kernel (k_fidelity_grad.inc.h) with the counter-based
// draws generated WHERE THEY ARE CONSUMED, as mc_fid_sens_philox_kernel does for the noise sensitivity, plus - on request - the
// second-moment sums from which the gradient of the row's variance follows.  No draw tensor exists: lane (c, k) makes its 3 N
// normals with philox_lane_draws (philox_core.inc.h: the bits philox_normal_kernel stores).  Two draw modes (p.shared):
//     per-controller draws:  sample (c, k), site i, slot s is element  offset + ((c K + k) N + i) 3 + s  of stream `seed`;
//     shared draws (common random numbers, the fidelity_ss_av objective):  element  offset + (k N + i) 3 + s,  the same for every c;
// in both scaled by sigma or by the wave-uniform sigma_rows[c].
// Tiling, NaN-row rule, per-sample arithmetic (grad_core.h), the row batches from N = 10, the order of the wave sums and the
// second pass of the row means are mc_fid_grad_kernel's: fid, grad and mean are bit-identical to philox_normal_kernel followed by
// mc_fid_grad_kernel (on the [C][K][N][3] tensor, or on the one [1][K][N][3] set in the shared mode).
//
// The draws are dead once (d, e) are built - from N = 10 d0, e0 live across the passes anyway -, so nothing of the generator is
// held across the QL, in registers or in LDS.
//
// Moment sums (p.moments, wave-uniform): every tile also writes the wave sum of F^2 and, for every gradient column a pass writes,
// the wave sum of F dF/dx_col behind its N + 2 mean sums: part[tile][2N + 4].  F is the fidelity of THAT pass (rows out and in and
// the eigenvalues are the same in every pass, so it is pass 0's value; no register is held for it).  Each product is rounded once
// (opaque: never contracted into the first addition of the tree), same grad_wave_sum tree, lanes beyond the row's end add zeros.
// mc_fid_grad_moment_mean_kernel reduces both halves of the row with mc_fid_grad_mean_kernel's order over the tiles.  No atomics.
//
// Sweep-cap fallback (rare; -DRC_GRAD_FORCE_GENERAL=1 forces it): the textbook QL of grad_core.h, CH lanes at a time, work
// vectors and the lane's 3 N draws - regenerated element by element with philox_element (through a call) - in LDS; counted in
// g_grad_general_tiles.
// LDS: the ln and sin/cos tables (3 KiB) + that work space; no staging buffer, no DMA.
//
// Included by robchar_grad.hip inside its anonymous namespace after philox_core.inc.h; not a stand-alone header.

// from the listing (DESIGN.md has the table): the register counts are mc_fid_grad_kernel's or a few more, same residency
constexpr int grad_philox_min_waves(int n) { return grad_min_waves(n); }

// philox_element as a CALL (22 registers of its own, no stack): inlined into the fallback its temporaries sit on top of the
// eigenvector rows that are live there, and N = 10 .. 12 need 385 - 400 registers and 2 - 8 VGPR -> AGPR spill copies instead of
// 360 - 380 and none.  Rare path only.
__device__ __attribute__((noinline)) double grad_philox_element(unsigned long long seed, unsigned long long e, double scale,
                                                                const double* lntab, const double* sctab) {
    return philox_element(seed, e, scale, lntab, sctab);
}

template <int N>
__global__ __launch_bounds__(64, grad_philox_min_waves(N)) void mc_fid_grad_philox_kernel(const GradPhiloxParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int kWork = 2 * N + N * N;           // doubles per sample of the textbook routine
    constexpr int CH = N <= 8 ? 8 : 4;             // lanes of it at a time
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ __attribute__((aligned(16))) double work[(kWork + G) * CH];

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
    const bool moments = p.moments != 0;           // wave-uniform
    const int nent = moments ? 2 * (N + 2) : N + 2;
    double* fdst = p.fid ? p.fid + c * p.K + kb : nullptr;
    double* gdst = p.grad ? p.grad + (c * p.K + kb) * (N + 1) : nullptr;
    double* pdst = p.part ? p.part + tile * nent : nullptr;
    double* mdst = (pdst && moments) ? pdst + (N + 2) : nullptr;
    if (pad) {                                     // NaN-padded controller row: NaN everywhere, its draws are not generated
        const double nan = __builtin_nan("");
        if (fdst && lane < nk) fdst[lane] = nan;
        if (gdst) {
            for (int i = lane; i < nk * (N + 1); i += 64) gdst[i] = nan;
        }
        if (pdst && lane < nent) pdst[lane] = nan;
        return;
    }
    const bool live = lane < nk;
    const double sigma = p.sigma_rows ? p.sigma_rows[c] : p.sigma;
    // this lane's G elements start at stream element E
    const unsigned long long E =
        p.offset + (unsigned long long)((p.shared ? 0ll : c * p.K) + kb + lane) * (unsigned long long)G;
    double gl[G];
    if (live) philox_lane_draws<G>(p.seed, E, sigma, lntab, sctab, gl);

    constexpr int R = rc::grad_batch_rows(N);      // rows of the eigenvector matrix per QL pass (grad_core.h)
    constexpr int NP = rc::grad_passes(N);
    double d0[NP > 1 ? N : 1], e0[NP > 1 ? N : 1];  // the matrix, kept for the later passes
    if constexpr (NP > 1) {
        if (live) rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, d0, e0);
    }
    const bool same = p.in == p.out;
#pragma unroll 1
    for (int pass = 0; pass < NP; ++pass) {
        int site[R];                               // wave-uniform: the site of every row of this pass (-1: none)
        rc::grad_pass_rows<N>(p.in, p.out, pass, site);
        rc::TriEig<N, R> s;
        bool ok = true;
        if constexpr (NP > 1) {
            if (live) ok = rc::grad_eigensystem_fast<N, R>(d0, e0, site, s);
        } else {
            if (live) {
                rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, s.d, s.e);
                ok = rc::grad_eigensystem_fast<N, R>(s.d, s.e, site, s);
            }
        }
        const unsigned long long badmask = __ballot(live && !ok);
        if (badmask != 0ull) {
            // Rare (not observed): some lane's QL ran into the sweep cap - the textbook routine as in mc_fid_grad_kernel, the
            // lane's draws made again element by element
            if (lane == 0 && pass == 0) atomicAdd(&g_grad_general_tiles, 1ull);
            const bool bad = (badmask >> lane) & 1ull;
            const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
            const int nbad = __popcll(badmask);
#pragma unroll 1
            for (int b0 = 0; b0 < nbad; b0 += CH) {
                const int rel = rank - b0;
                if (bad && rel >= 0 && rel < CH) {
                    double* g = work + kWork * CH + rel * G;
                    // (E again from an opaque copy of the lane number: hoisted out of the pass loop it would be one more
                    // live pair across gradient_from_eigensystem, and from N = 10 that pair is the one that spills)
                    int ln = lane;
                    asm volatile("" : "+v"(ln));
                    const unsigned long long Eb =
                        p.offset + (unsigned long long)((p.shared ? 0ll : c * p.K) + kb + ln) * (unsigned long long)G;
                    for (int i = 0; i < G; ++i) g[i] = grad_philox_element(p.seed, Eb + (unsigned long long)i, sigma, lntab, sctab);
                    const GradLdsVec vd{work + rel, CH}, ve{work + N * CH + rel, CH};
                    const GradLdsMat vz{work + 2 * N * CH + rel, CH, N};
                    rc::grad_eigensystem_general<N, R>(xg, p.h0.diag, p.h0.off, g, site, vd, ve, vz, s);
                }
            }
        }

        double f = 0.0, g[R + 1];
#pragma unroll
        for (int l = 0; l <= R; ++l) g[l] = 0.0;
        if (live) rc::gradient_from_eigensystem<N, R>(s, x[N], same, f, g);
        // (grad_result_column: rows out, in and the time entry are written by the first pass only, like the fidelity)
#pragma unroll
        for (int l = 0; l <= R; ++l) {
            const int col = rc::grad_result_column<N>(site, pass, l);     // wave-uniform
            if (col < 0) continue;
            if (gdst && live) gdst[lane * (N + 1) + col] = g[l];
            if (pdst) {
                const double sg = grad_wave_sum(g[l]);
                if (lane == 0) pdst[1 + col] = sg;
            }
            if (mdst) {
                double fg = f * g[l];
                asm volatile("" : "+v"(fg));
                const double sm = grad_wave_sum(fg);
                if (lane == 0) mdst[1 + col] = sm;
            }
        }
        if (pass == 0) {
            if (fdst && live) fdst[lane] = f;
            if (pdst) {
                const double sf = grad_wave_sum(f);
                if (lane == 0) pdst[0] = sf;
            }
            if (mdst) {
                double ff = f * f;
                asm volatile("" : "+v"(ff));
                const double sm = grad_wave_sum(ff);
                if (lane == 0) mdst[0] = sm;
            }
        }
    }
}

// The second pass when the moment sums are wanted: mc_fid_grad_mean_kernel's arithmetic per entry (lane t adds the tiles t,
// t + 64, ... in order, then the fixed shuffle tree, then / K) over part rows of 2 nent entries: the first nent go to `mean`
// [C][nent], the second nent to `moment` [C][nent]; either may be NULL.
__global__ __launch_bounds__(64) void mc_fid_grad_moment_mean_kernel(const double* part, double* mean, double* moment,
                                                                     long long tiles_per_ctrl, int nent, long long K) {
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;
    const double* row = part + c * tiles_per_ctrl * (2 * nent);
    for (int j = (mean ? 0 : nent); j < (moment ? 2 * nent : nent); ++j) {
        double acc = 0.0;
        for (long long t = lane; t < tiles_per_ctrl; t += 64) acc += row[t * (2 * nent) + j];
        acc = grad_wave_sum(acc);
        if (lane == 0) {
            if (j < nent) mean[c * nent + j] = acc / (double)K;
            else moment[c * nent + (j - nent)] = acc / (double)K;
        }
    }
}

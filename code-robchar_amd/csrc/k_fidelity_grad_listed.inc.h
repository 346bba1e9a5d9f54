// mc_fid_grad_listed_kernel<N> (N = 2 .. RC_MAX_NSPIN_GRAD): mc_fid_grad_philox_kernel (k_fidelity_grad_philox.inc.h) over a
// caller-chosen LIST of a row's K draws, with caller-chosen weights on the row sums - the primitive behind tail objectives
// (CVaR: the worst alpha K draws with tail weights; entropic risk; smoothed yield; bootstrap resamples).  Only a counter-based
// generator allows it: a lane makes the draws of whatever (c, k) it is handed.  Three changes against that kernel:
//
// 1. Sample choice.  Lane j of tile t of row c handles slot s = 64 t + j < L and reads k = list[c][s] (int32, coalesced).  A value
//    outside 0 .. K - 1 is an EMPTY slot: NaN in fid / grad, +0.0 in the sums, no draws generated.  The sample's stream element is
//    the family's convention with that k:  offset + ((c K + k) N + i) 3 + s',  shared draws:  offset + (k N + i) 3 + s'.  sigma /
//    sigma_rows[c], the NaN-row rule, the static terms, the row batches from N = 10 and the sweep-cap fallback (counted in
//    g_grad_general_tiles; -DRC_GRAD_FORCE_GENERAL=1 forces it) are unchanged.
//
// 2. Per-lane sweeps.  grad_eigensystem_fast<N, R, true>: tridiag_ql2_fast's FREEZE, for the reason the ring repair kernel has it -
//    the waves are packed from a list.  A sample's fid and grad bits depend on (c, k) and the other arguments only: not on L, not on
//    the slot, not on what else is listed.  Against the full launch (mc_fid_grad_philox_kernel, where the wave votes the sweep count
//    and a lane may run sweeps beyond its own convergence) a sample agrees to rounding, not bit for bit.
//
// 3. Weighted row sums (p.part): every tile writes the grad_wave_sum of w F and, for every gradient column a pass writes, of
//    w dF/dx_col to part[tile][N + 2].  Each product is rounded once (opaque: never contracted into the first addition of the tree),
//    empty and out-of-row lanes add +0.0; p.weight == NULL: w = 1 and no multiplication.  mc_fid_grad_mean_kernel with K = 1 adds a
//    row's tiles in its fixed order (the division by 1.0 is exact).  No atomics.
//
// Registers: neither k nor w lives across the QL.  The set of live lanes is a ballot (a scalar pair), k is read again where the
// fallback regenerates a lane's draws, w is read after the gradient arithmetic of each pass.
//
// Included by robchar_grad.hip inside its anonymous namespace after k_fidelity_grad_philox.inc.h; not a stand-alone header.

// from the listing (DESIGN.md has the table)
constexpr int grad_listed_min_waves(int n) { return grad_philox_min_waves(n); }

template <int N>
__global__ __launch_bounds__(64, grad_listed_min_waves(N)) void mc_fid_grad_listed_kernel(const GradListedParams p) {
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
    const long long sb = (tile - c * p.tiles_per_ctrl) * 64;       // first slot of this tile
    const int nl = (int)((p.L - sb < 64) ? (p.L - sb) : 64);

    const double* xg = p.ctrl + c * (N + 1);       // controller row: wave-uniform -> scalar registers
    double x[N + 1];
    bool pad = false;
#pragma unroll
    for (int i = 0; i <= N; ++i) {
        x[i] = xg[i];
        pad |= (x[i] != x[i]);
    }
    constexpr int nent = N + 2;
    const int* lsrc = p.list + c * p.L + sb;
    const double* wsrc = p.weight ? p.weight + c * p.L + sb : nullptr;
    double* fdst = p.fid ? p.fid + c * p.L + sb : nullptr;
    double* gdst = p.grad ? p.grad + (c * p.L + sb) * (N + 1) : nullptr;
    double* pdst = p.part ? p.part + tile * nent : nullptr;
    const double nan = __builtin_nan("");
    if (pad) {                                     // NaN-padded controller row: NaN everywhere, its draws are not generated
        if (fdst && lane < nl) fdst[lane] = nan;
        if (gdst) {
            for (int i = lane; i < nl * (N + 1); i += 64) gdst[i] = nan;
        }
        if (pdst && lane < nent) pdst[lane] = nan;
        return;
    }
    const double sigma = p.sigma_rows ? p.sigma_rows[c] : p.sigma;
    const long long rowk = p.shared ? 0ll : c * p.K;
    unsigned long long livemask;                   // wave-uniform: the slots of this tile that hold a sample
    double gl[G];
    {
        const int k = lane < nl ? lsrc[lane] : -1;
        const bool lv = k >= 0 && (long long)k < p.K;
        livemask = __ballot(lv);
        if (lv) {
            // this lane's G elements start at E
            const unsigned long long E = p.offset + (unsigned long long)(rowk + k) * (unsigned long long)G;
            philox_lane_draws<G>(p.seed, E, sigma, lntab, sctab, gl);
        }
    }
    const bool live = (livemask >> lane) & 1ull;
    if (!live) {                                   // empty slots of the row: NaN, written once
        if (fdst && lane < nl) fdst[lane] = nan;
        if (gdst && lane < nl) {
            for (int i = 0; i <= N; ++i) gdst[lane * (N + 1) + i] = nan;
        }
    }

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
            if (live) ok = rc::grad_eigensystem_fast<N, R, true>(d0, e0, site, s);
        } else {
            if (live) {
                rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, s.d, s.e);
                ok = rc::grad_eigensystem_fast<N, R, true>(s.d, s.e, site, s);
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
                    // (k again from the list, through an opaque copy of the lane number: see mc_fid_grad_philox_kernel)
                    int ln = lane;
                    asm volatile("" : "+v"(ln));
                    const unsigned long long Eb = p.offset + (unsigned long long)(rowk + lsrc[ln]) * (unsigned long long)G;
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
        // the weight, read here and not before the QL; 1.0 for an empty lane, whose f and g are +0.0
        double w = 1.0;
        if (pdst && wsrc && live) w = wsrc[lane];
        // (grad_result_column: rows out, in and the time entry are written by the first pass only, like the fidelity)
#pragma unroll
        for (int l = 0; l <= R; ++l) {
            const int col = rc::grad_result_column<N>(site, pass, l);     // wave-uniform
            if (col < 0) continue;
            if (gdst && live) gdst[lane * (N + 1) + col] = g[l];
            if (pdst) {
                double wg = g[l];
                if (wsrc) {
                    wg = w * g[l];
                    asm volatile("" : "+v"(wg));
                }
                const double sg = grad_wave_sum(wg);
                if (lane == 0) pdst[1 + col] = sg;
            }
        }
        if (pass == 0) {
            if (fdst && live) fdst[lane] = f;
            if (pdst) {
                double wf = f;
                if (wsrc) {
                    wf = w * f;
                    asm volatile("" : "+v"(wf));
                }
                const double sf = grad_wave_sum(wf);
                if (lane == 0) pdst[0] = sf;
            }
        }
    }
}

// Lane-per-sample kernel for the fidelity AND its derivatives with respect to the sample's own draws (the 3 N - 2 structured
// noise directions), chain topology: mc_fid_sens_kernel<N> (N = 2 .. RC_MAX_NSPIN_GRAD).
//
// Included by robchar_grad.hip inside its anonymous namespace after k_fidelity_grad.inc.h; not a stand-alone header.
// Tiling, LDS-DMA staging, NaN-row rule and the fast / textbook QL routes are mc_fid_grad_kernel's (the staging block is
// written out here: through stage_tile_draws<G, PH, 0> the listing stays within every resource bound, but the kernel with all
// outputs measured 1.1 - 1.4 % slower at N = 5, 9 - profiles/shared_leaves_listing.txt).  Per lane: sens_core.h.  The
// sample's draws are needed again after the QL - for the unit phases re/r, im/r of the couplings and for the radial
// derivative rho = sum g dF/dg - and are re-read from global memory then (every lane its own 24 N contiguous bytes, hot in
// L2 from the staging) instead of being held in 6 N registers across the QL.
//
// Row means (`part` != nullptr): every tile writes the wave sums of (F, rho, dF/dg [N][3]) over its samples - fixed shuffle
// tree, lanes beyond the row's end add zeros - to part[tile][3 N + 2]; mc_fid_grad_mean_kernel adds a row's tiles in a
// fixed order.  No atomics on results: the same inputs give the same bits on every run.

constexpr int sens_min_waves(int n) { return n <= 3 ? 4 : (n <= 7 ? 2 : 1); }

template <int N>
__global__ __launch_bounds__(64, sens_min_waves(N)) void mc_fid_sens_kernel(const SensParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int PH = grad_phases(N);
    constexpr int SP = 64 / PH;                    // samples per staging phase
    constexpr int kPhaseBytes = SP * G * 8;
    constexpr int kWork = 2 * N + N * N;           // doubles per sample of the textbook routine
    constexpr int CH = (SP * G) / kWork;           // samples of it that fit the staging buffer at a time
    static_assert(CH >= 1, "staging buffer too small for the textbook routine");
    __shared__ __attribute__((aligned(16))) double stage[SP * G];

    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;             // wave-uniform
    __builtin_amdgcn_s_setprio(3);
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
    double* fdst = p.fid ? p.fid + c * p.K + kb : nullptr;
    double* sdst = p.sens ? p.sens + (c * p.K + kb) * G : nullptr;
    double* pdst = p.part ? p.part + tile * (G + 2) : nullptr;
    if (pad) {                                     // NaN-padded controller row: NaN everywhere, no draws read
        const double nan = __builtin_nan("");
        if (fdst && lane < nk) fdst[lane] = nan;
        if (sdst) {
            for (int i = lane; i < nk * G; i += 64) sdst[i] = nan;
        }
        if (pdst && lane < G + 2) pdst[lane] = nan;
        return;
    }

    // HBM -> LDS -> registers (see mc_fid_chain_kernel)
    const char* src = (const char*)(p.draws + c * p.draw_cstride + kb * G);
    double gl[G];
#pragma unroll
    for (int ph = 0; ph < PH; ++ph) {
        const int first = ph * SP;
        if (first < nk) {                          // wave-uniform
            const int cnt = (nk - first < SP) ? (nk - first) : SP;
            const int bytes = cnt * G * 8;
            const char* ps = src + (long long)first * G * 8;
            if (p.align16 && !(cnt & 1)) {
#pragma unroll
                for (int it = 0; it < (kPhaseBytes + 1023) / 1024; ++it) {
                    const int off = it * 1024 + lane * 16;
                    if (off < bytes)
                        __builtin_amdgcn_global_load_lds((rc_gptr_t)(ps + off), (rc_lptr_t)((char*)stage + it * 1024), 16, 0, 0);
                }
            } else {
#pragma unroll 2
                for (int it = 0; it < (kPhaseBytes + 255) / 256; ++it) {
                    const int off = it * 256 + lane * 4;
                    if (off < bytes)
                        __builtin_amdgcn_global_load_lds((rc_gptr_t)(ps + off), (rc_lptr_t)((char*)stage + it * 256), 4, 0, 0);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // DMA landed
            int rel = lane - first;
            asm volatile("" : "+v"(rel));                             // one base address + immediate offsets
            if (rel >= 0 && rel < cnt) {
#pragma unroll
                for (int i = 0; i < G; ++i) gl[i] = stage[rel * G + i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // reads done before the buffer is refilled
        }
    }
    __builtin_amdgcn_s_setprio(0);

    constexpr int R = rc::sens_batch_rows(N);      // rows of the eigenvector matrix per QL pass (sens_core.h)
    constexpr int NP = rc::sens_passes(N);
    double d0[NP > 1 ? N : 1], e0[NP > 1 ? N : 1];  // the matrix, kept for the later passes
    if constexpr (NP > 1) {
        if (lane < nk) rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, d0, e0);
    }
    const bool live = lane < nk;
    const double* gs = (const double*)src + (long long)(live ? lane : 0) * G;     // this sample's draws, re-read below
    // site 0 has no bond below it: its two coupling entries are 0
    if (sdst && live) sdst[lane * G + 1] = sdst[lane * G + 2] = 0.0;
    if (pdst && lane == 0) pdst[2 + 1] = pdst[2 + 2] = 0.0;
    double rho = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < NP; ++pass) {
        int site[R];                               // wave-uniform: the site of every row of this pass (-1: none)
        rc::sens_pass_rows<N>(p.in, p.out, pass, site);
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
            // Rare (not observed): some lane's QL ran into the sweep cap - the textbook routine as in mc_fid_grad_kernel
            if (lane == 0 && pass == 0) atomicAdd(&g_sens_general_tiles, 1ull);
            const bool bad = (badmask >> lane) & 1ull;
            const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
            const int nbad = __popcll(badmask);
#pragma unroll 1
            for (int c0 = 0; c0 < nbad; c0 += CH) {
                const int rel = rank - c0;
                if (bad && rel >= 0 && rel < CH) {
                    const GradLdsVec vd{stage + rel, CH}, ve{stage + N * CH + rel, CH};
                    const GradLdsMat vz{stage + 2 * N * CH + rel, CH, N};
                    rc::grad_eigensystem_general<N, R>(xg, p.h0.diag, p.h0.off, gs, site, vd, ve, vz, s);
                }
            }
        }

        double f = 0.0, ds[R], dr[R];
#pragma unroll
        for (int l = 0; l < R; ++l) ds[l] = dr[l] = 0.0;
        if (live) rc::sens_from_eigensystem<N, R>(s, site, p.in, p.out, x[N], f, ds, dr);
#pragma unroll
        for (int q = 0; q < R; ++q) {
            bool wsite, wbond;                     // wave-uniform (sens_row_writes: every entry comes from exactly one pass)
            rc::sens_row_writes<N>(site, pass, q, wsite, wbond);
            if (!wsite && !wbond) continue;
            const int i = site[q];
            if (wsite) {
                const double g0 = live ? gs[3 * i] : 0.0;
                rho = fma(g0, ds[q], rho);
                if (sdst && live) sdst[lane * G + 3 * i] = ds[q];
                if (pdst) {
                    const double sg = grad_wave_sum(ds[q]);
                    if (lane == 0) pdst[2 + 3 * i] = sg;
                }
            }
            if (wbond) {
                const double g1 = live ? gs[3 * i + 1] : 0.0, g2 = live ? gs[3 * i + 2] : 0.0;
                double cr, ci;
                rc::sens_unit_phase(p.h0.off[i - 1] + g1, g2, cr, ci);
                const double s1 = cr * dr[q], s2 = ci * dr[q];
                rho = fma(g1, s1, fma(g2, s2, rho));
                if (sdst && live) {
                    sdst[lane * G + 3 * i + 1] = s1;
                    sdst[lane * G + 3 * i + 2] = s2;
                }
                if (pdst) {
                    const double a1 = grad_wave_sum(s1), a2 = grad_wave_sum(s2);
                    if (lane == 0) {
                        pdst[2 + 3 * i + 1] = a1;
                        pdst[2 + 3 * i + 2] = a2;
                    }
                }
            }
        }
        if (pass == 0) {
            if (fdst && live) fdst[lane] = f;
            if (pdst) {
                const double sf = grad_wave_sum(f);
                if (lane == 0) pdst[0] = sf;
            }
        }
    }
    if (pdst) {
        const double sr = grad_wave_sum(rho);
        if (lane == 0) pdst[1] = sr;
    }
}

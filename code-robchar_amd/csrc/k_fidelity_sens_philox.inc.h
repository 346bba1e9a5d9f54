// mc_fid_sens_philox_kernel<N> (N = 2 .. RC_MAX_NSPIN_GRAD): mc_fid_sens_kernel (k_fidelity_sens.inc.h) with the counter-based
// draws generated WHERE THEY ARE CONSUMED, as mc_fid_chain_philox_kernel does for the fidelities.  No draw tensor exists: lane
// (c, k) makes its 3 N normals from the stream of rc_draws_philox_f64,
//     element  offset + ((c K + k) N + i) 3 + s   of stream `seed`, scaled by sigma or by sigma_rows[c] (wave-uniform: all sigma
//     levels of an algorithm go through one launch with the controller rows tiled L times),
// with philox_lane_draws (philox_core.inc.h: the bits philox_normal_kernel stores).  Tiling, NaN-row rule, per-sample arithmetic
// (sens_core.h / grad_core.h), the order of the wave sums and the second pass of the row means (mc_fid_grad_mean_kernel) are
// mc_fid_sens_kernel's: fid, sens and mean are bit-identical to philox_normal_kernel followed by mc_fid_sens_kernel.
//
// The draws are needed twice: for the matrix, and after the QL for the unit phases and rho = sum g dF/dg (from N = 10 once per
// pass, for the sites that pass writes).  mc_fid_sens_kernel re-reads them from global memory; here, from the listing
// (DESIGN.md has the table of every variant that was built):
//   N <= 9   one pass, every index a compile-time constant: the 3 N values stay in REGISTERS across the QL (the compiler parks
//            them in accumulation registers where the eigenvector rows need the architectural ones); no spill up to N = 9.
//   N >= 10  the site of a row is a run-time (wave-uniform) number, and the pair loop of sens_from_eigensystem alone needs more
//            than the 256 architectural registers.  Held in registers (picked by select chains): 415 - 455 registers and 2 - 8
//            VGPR -> AGPR spill copies in that loop.  Generated again - by pair inside the passes, or in one rolled loop behind
//            them with dF/dg0, dF/dr parked in LDS -: 372 - 402 registers and still 2 - 10 spill copies: the generator's
//            constants compete with the pair loop's for scalar registers.  So the lane's 3 N draws are HELD IN LDS, lane-strided
//            (24 N bytes x 64 lanes: 18 KiB at N = 12, with one wave per SIMD the CU has 40 KiB per wave): the passes read the
//            three values of a site at a run-time index, the fallback copies its lane's run, nothing of the generator lives
//            across the passes, and the register numbers are mc_fid_sens_kernel's (336 / 372 / 366, no spill).
//
// Sweep-cap fallback (rare; -DRC_GRAD_FORCE_GENERAL=1 forces it): the textbook QL of grad_core.h, CH lanes at a time, work
// vectors and the lane's draws in LDS - N <= 9: element by element from philox_element; N >= 10: copied from the held draws -;
// counted in g_sens_general_tiles.
// LDS: the ln and sin/cos tables (3 KiB) + that work space + from N = 10 the held draws; no staging buffer, no DMA.
//
// Included by robchar_grad.hip inside its anonymous namespace after k_fidelity_sens.inc.h; not a stand-alone header.

// (single-pass sizes above 9 hold their draws in LDS too; with 6 here, N = 7 fits two waves per SIMD, 256 registers - the A/B
// against the registers: DESIGN.md, the sensitivity kernels)
constexpr bool sens_philox_hold_in_registers(int n) { return rc::sens_passes(n) == 1 && n <= 9; }
// from the listing: 58 / 108 registers at N = 2, 3 (four waves), 152 / 196 / 252 at N = 4 .. 6 (two), from N = 7
// (294: the 42 held values beside mc_fid_sens_kernel's 256) one wave
constexpr int sens_philox_min_waves(int n) { return n <= 3 ? 4 : ((n <= 6 || (n == 7 && !sens_philox_hold_in_registers(7))) ? 2 : 1); }

template <int N>
__global__ __launch_bounds__(64, sens_philox_min_waves(N)) void mc_fid_sens_philox_kernel(const SensPhiloxParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int kWork = 2 * N + N * N;           // doubles per sample of the textbook routine
    constexpr int CH = N <= 8 ? 8 : 4;             // lanes of it at a time
    constexpr bool HOLD = sens_philox_hold_in_registers(N);
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ __attribute__((aligned(16))) double work[(kWork + G) * CH];
    __shared__ double drw[HOLD ? 1 : G * 64];      // N >= 10: the draws, element i of lane l at [i * 64 + l]

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
    double* fdst = p.fid ? p.fid + c * p.K + kb : nullptr;
    double* sdst = p.sens ? p.sens + (c * p.K + kb) * G : nullptr;
    double* pdst = p.part ? p.part + tile * (G + 2) : nullptr;
    if (pad) {                                     // NaN-padded controller row: NaN everywhere, its draws are not generated
        const double nan = __builtin_nan("");
        if (fdst && lane < nk) fdst[lane] = nan;
        if (sdst) {
            for (int i = lane; i < nk * G; i += 64) sdst[i] = nan;
        }
        if (pdst && lane < G + 2) pdst[lane] = nan;
        return;
    }
    const bool live = lane < nk;
    const double sigma = p.sigma_rows ? p.sigma_rows[c] : p.sigma;
    // this lane's G elements start at stream element E
    const unsigned long long E = p.offset + (unsigned long long)(c * p.K + kb + lane) * (unsigned long long)G;
    double gl[G];
    if (live) philox_lane_draws<G>(p.seed, E, sigma, lntab, sctab, gl);

    constexpr int R = rc::sens_batch_rows(N);      // rows of the eigenvector matrix per QL pass (sens_core.h)
    constexpr int NP = rc::sens_passes(N);
    double d0[NP > 1 ? N : 1], e0[NP > 1 ? N : 1];  // the matrix, kept for the later passes
    if constexpr (!HOLD) {
        if (live) {
#pragma unroll
            for (int i = 0; i < G; ++i) drw[i * 64 + lane] = gl[i];
        }
    }
    if constexpr (NP > 1) {
        if (live) {
            rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, d0, e0);
        }
    }
    // site 0 has no bond below it: its two coupling entries are 0
    if (sdst && live) sdst[lane * G + 1] = sdst[lane * G + 2] = 0.0;
    if (pdst && lane == 0) pdst[2 + 1] = pdst[2 + 2] = 0.0;
    double rho = 0.0;
    // What site i contributes once its draws (g0, g1, g2) are at hand again: rho, the two coupling entries through the unit
    // phase, the stores and the wave sums - in mc_fid_sens_kernel's order (sites ascending).  dsi = dF/dg0_i, dri = dF/dr_i.
    auto finish_site = [&](int i, bool bond, double dsi, double dri, double g0, double g1, double g2) {
        rho = fma(g0, dsi, rho);
        if (sdst && live) sdst[lane * G + 3 * i] = dsi;
        if (pdst) {
            const double sg = grad_wave_sum(dsi);
            if (lane == 0) pdst[2 + 3 * i] = sg;
        }
        if (bond) {
            double cr, ci;
            rc::sens_unit_phase(p.h0.off[i - 1] + g1, g2, cr, ci);
            const double s1 = cr * dri, s2 = ci * dri;
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
    };
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
            // Rare (not observed): some lane's QL ran into the sweep cap - the textbook routine as in mc_fid_sens_kernel
            if (lane == 0 && pass == 0) atomicAdd(&g_sens_general_tiles, 1ull);
            const bool bad = (badmask >> lane) & 1ull;
            const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
            const int nbad = __popcll(badmask);
#pragma unroll 1
            for (int c0 = 0; c0 < nbad; c0 += CH) {
                const int rel = rank - c0;
                if (bad && rel >= 0 && rel < CH) {
                    double* g = work + kWork * CH + rel * G;
                    for (int i = 0; i < G; ++i) {
                        if constexpr (HOLD) g[i] = philox_element(p.seed, E + (unsigned long long)i, sigma, lntab, sctab);
                        else g[i] = drw[i * 64 + lane];
                    }
                    const GradLdsVec vd{work + rel, CH}, ve{work + N * CH + rel, CH};
                    const GradLdsMat vz{work + 2 * N * CH + rel, CH, N};
                    rc::grad_eigensystem_general<N, R>(xg, p.h0.diag, p.h0.off, g, site, vd, ve, vz, s);
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
            if constexpr (HOLD) {                  // one pass: row q is site q - constant indices into the held draws
                const bool lv = live;
                finish_site(q, wbond, ds[q], dr[q], lv ? gl[3 * q] : 0.0, lv ? gl[3 * q + 1] : 0.0, lv ? gl[3 * q + 2] : 0.0);
            } else {                               // the site is a run-time number: an index into the draws held in LDS
                const int i = (NP == 1) ? q : site[q];
                const double* gi = drw + (3 * i) * 64 + lane;
                const bool lv = live;
                finish_site(i, wbond, ds[q], dr[q], lv ? gi[0] : 0.0, lv ? gi[64] : 0.0, lv ? gi[128] : 0.0);
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

// mc_fid_pickfreeze_philox_kernel<N, MODE> (N = 2 .. RC_MAX_NSPIN_PICKFREEZE, the two eigenvalue-only weight modes): the
// pick-freeze scheme of the variance indices (code-robchar_amd/variance_indices.py is the definition) in the frame of
// mc_fid_chain_philox_kernel (k_fidelity_philox.inc.h) - one sample per lane, one 64-sample tile of ONE controller per wave, the
// controller row in scalar registers, the same NaN-row rule, sigma or the wave-uniform sigma_rows[c], the same repair routes and
// counters.  Lane (c, k) makes TWO draw vectors with philox_lane_draws,
//     a: elements  offset_a + ((c K + k) N + i) 3 + s,   b: the same at offset_b,   of stream `seed`, scaled by sigma,
// once, and then runs ONE ROLLED LOOP over the evaluations e = 0 .. G + 1: the wave-uniform mask is 0 (e = 0: A), all ones (e = 1:
// B) or groups[e - 2], and the draw accessor handed to chain_fidelity_fast picks coordinate j from b where bit j of the mask is
// set and from a elsewhere - a select on a scalar condition, a copy of bits.  There is one inlined copy of the fidelity routine
// whatever G is.  Slab e of fid_out [G + 2][C][K] is therefore bit for bit what the tensor kernel gives on the materialised
// hybrid tensor (same tiles, same MODE choice), and slabs 0 and 1 are mc_fid_chain_philox_kernel's at the two offsets
// (tests/test_gpu_variance.py).
//
// Sums (p.part [ntiles][3 + 2 G]): behind e = 1 the wave sums of fA, fB and (fA - fB)^2, behind e >= 2 those of (fA - f)^2 and
// (fB - f)^2 - a difference rounded once, a square rounded once and kept opaque (never contracted into the first addition of the
// tree), lanes beyond the row's end add +0.0, pickfreeze_wave_sum is grad_wave_sum's tree.  mc_fid_pickfreeze_mean_kernel reduces
// a row's tiles with mc_fid_grad_mean_kernel's arithmetic.  No atomics on results.
//
// Where a and b (6 N doubles) live across the loop, from the listing (DESIGN.md has the table and the variants that were built):
// the first pickfreeze_reg_a(n) coordinates of a and the first pickfreeze_reg_b(n) of b stay in REGISTERS, the others are held in
// LDS, lane-strided (slot t of lane l at [t * 64 + l]: a's coordinates, then b's).  A coordinate with both values in LDS costs ONE
// read at a selected address; with one value in LDS that value is read whatever the bit says.
//   N <= 6       a and b in registers (N = 2, 3: three waves per SIMD, 4 .. 6: two)
//   N == 7       a in registers, b in LDS: 15 KiB, two waves (in registers the general adjugate mode needs 264)
//   N = 8 .. 11  both in LDS (29 .. 39 KiB), one wave: 4 waves per compute unit share 160 KiB
//   N = 12, 13   both in LDS but the first 4 / 10 coordinates of a, which is what 40 KiB per wave leave room for
//
// Part of ONE translation unit: #included by robchar_vidx.hip inside its anonymous namespace, after k_fidelity_chain.inc.h.
constexpr int pickfreeze_reg_a(int n) { return n <= 7 ? 3 * n : (n <= 11 ? 0 : (n == 12 ? 4 : 10)); }
constexpr int pickfreeze_reg_b(int n) { return n <= 6 ? 3 * n : 0; }
constexpr int pickfreeze_min_waves(int n, int mode) { return n <= 3 ? 3 : (n <= 7 ? 2 : 1); }

__device__ __forceinline__ double pickfreeze_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                              // valid in lane 0
}

// wave sum of (u - v)^2 over the live lanes
__device__ __forceinline__ double pickfreeze_sq_sum(double u, double v, bool live) {
    const double d = u - v;
    double sq = d * d;
    asm volatile("" : "+v"(sq));                   // the rounded square, never contracted into the tree's first addition
    return pickfreeze_wave_sum(live ? sq : 0.0);
}

template <int N, int MODE>
__global__ __launch_bounds__(64, pickfreeze_min_waves(N, MODE)) void mc_fid_pickfreeze_philox_kernel(const PickFreezeParams p) {
    constexpr int G = 3 * N;                       // doubles per draw vector
    constexpr int CH = 4;                          // lanes per pass of the last-resort routine (work vectors in LDS)
    constexpr int RA = pickfreeze_reg_a(N), RB = pickfreeze_reg_b(N);     // coordinates of a, b held in registers
    constexpr int SB = G - RA;                     // first LDS slot of b
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ __attribute__((aligned(16))) double work[(4 * N + G) * CH];
    __shared__ double drw[(2 * G - RA - RB) * 64 + 1];

    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;             // wave-uniform
    philox_stage_tables(lane, sctab, lntab);
    const long long c = tile / p.tiles_per_ctrl;
    const long long kb = (tile - c * p.tiles_per_ctrl) * 64;
    const int nk = (int)((p.K - kb < 64) ? (p.K - kb) : 64);
    const int NG = p.G;
    const int nent = 3 + 2 * NG;
    const long long slab = p.C * p.K;

    const double* xg = p.ctrl + c * (N + 1);       // controller row: wave-uniform -> scalar registers
    double x[N + 1];
    bool pad = false;
#pragma unroll
    for (int i = 0; i <= N; ++i) {
        x[i] = xg[i];
        pad |= (x[i] != x[i]);
    }
    double* fdst = p.fid ? p.fid + c * p.K + kb : nullptr;
    double* pdst = p.part ? p.part + tile * nent : nullptr;
    const bool live = lane < nk;
    if (pad) {                                     // NaN-padded controller row: NaN everywhere, its draws are not generated
        const double nan = __builtin_nan("");
        if (fdst && live) {
            for (int e = 0; e < NG + 2; ++e) fdst[e * slab + lane] = nan;
        }
        if (pdst) {
            for (int j = lane; j < nent; j += 64) pdst[j] = nan;
        }
        return;
    }
    const double sigma = p.sigma_rows ? p.sigma_rows[c] : p.sigma;
    // this lane's two draw vectors start at stream elements Ea, Eb
    const unsigned long long rel = (unsigned long long)(c * p.K + kb + lane) * (unsigned long long)G;
    const unsigned long long Ea = p.offset_a + rel, Eb = p.offset_b + rel;
    double* dl = drw + lane;                       // LDS slot t of this lane at dl[t * 64]
    double a[G], b[G];
    if (live) {
        philox_lane_draws<G>(p.seed, Ea, sigma, lntab, sctab, a);
#pragma unroll
        for (int j = RA; j < G; ++j) dl[(j - RA) * 64] = a[j];
        philox_lane_draws<G>(p.seed, Eb, sigma, lntab, sctab, b);
#pragma unroll
        for (int j = RB; j < G; ++j) dl[(SB + j - RB) * 64] = b[j];
    }

    double fA = 0.0, fB = 0.0;
#pragma unroll 1
    for (int e = 0; e < NG + 2; ++e) {
        const unsigned long long mask = e == 0 ? 0ull : (e == 1 ? ~0ull : p.groups[e - 2]);     // wave-uniform
        double f = 0.0;
        bool ok = true;
        int extra = 0;
        if (live)
            ok = rc::chain_fidelity_fast<N, MODE>(
                x, p.h0.diag, p.h0.off,
                [dl, &a, &b, mask](int j) {        // (j is a compile-time index once the routine's loops are unrolled)
                    const bool bit = (mask >> j) & 1ull;
                    if (j < RA && j < RB) return bit ? b[j] : a[j];
                    if (j >= RA && j >= RB) return dl[(bit ? SB + j - RB : j - RA) * 64];
                    // one of the two in LDS: read whatever the bit says (a load under the condition becomes a load from a
                    // selected ADDRESS and the register array goes to scratch - philox_lane_draws has the same note)
                    double v = dl[(j < RA ? SB + j - RB : j - RA) * 64];
                    asm volatile("" : "+v"(v));
                    return j < RA ? (bit ? v : a[j]) : (bit ? b[j] : v);
                },
                p.in, p.out, sctab, f, nullptr, &extra);
        if (extra && lane == 0) atomicAdd(&g_polish_tiles[blockIdx.x & 63u], 1ull);
        unsigned long long badmask = __ballot(live && !ok);
        if (badmask) {
            if (lane == 0) atomicAdd(&g_general_tiles, 1ull);
            // rare: the eigenvector-rows route for the lanes the eigenvalue-only weights cannot take; the coordinates of their
            // hybrid are regenerated element by element (nothing of the fast path has to stay alive)
            const bool bad = (badmask >> lane) & 1ull;
            bool ok2 = true;
            if (bad) {
                double f2;
                const unsigned long long seed = p.seed;
                const double* lt = lntab;
                const double* st = sctab;
                ok2 = rc::chain_fidelity_fast<N, rc::kWeightsRows>(
                    xg, p.h0.diag, p.h0.off,
                    [seed, Ea, Eb, mask, sigma, lt, st](int j) {
                        return philox_element(seed, (((mask >> j) & 1ull) ? Eb : Ea) + (unsigned long long)j, sigma, lt, st);
                    },
                    p.in, p.out, sctab, f2);
                if (ok2) f = f2;
            }
            badmask = __ballot(bad && !ok2);
        }
        if (badmask) {
            // last resort (the rows-mode QL at its sweep cap): the textbook per-sample routine, CH lanes at a time, the hybrid and
            // work vectors in LDS
            const bool bad = (badmask >> lane) & 1ull;
            const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
            const int nbad = __popcll(badmask);
#pragma unroll 1
            for (int c0 = 0; c0 < nbad; c0 += CH) {
                const int rl = rank - c0;
                if (bad && rl >= 0 && rl < CH) {
                    double* g = work + 4 * N * CH + rl * G;
                    for (int j = 0; j < G; ++j)
                        g[j] = philox_element(p.seed, (((mask >> j) & 1ull) ? Eb : Ea) + (unsigned long long)j, sigma, lntab, sctab);
                    const LdsVec vd{work + rl, CH}, ve{work + N * CH + rl, CH}, va{work + 2 * N * CH + rl, CH}, vb{work + 3 * N * CH + rl, CH};
                    f = rc::chain_fidelity_general(N, xg, p.h0.diag, p.h0.off, g, p.in, p.out, vd, ve, va, vb);
                }
            }
        }
        if (fdst && live) fdst[e * slab + lane] = f;
        if (e == 0) {
            fA = f;
        } else if (e == 1) {
            fB = f;
            if (pdst) {
                const double sa = pickfreeze_wave_sum(fA), sb = pickfreeze_wave_sum(fB), sd = pickfreeze_sq_sum(fA, fB, live);
                if (lane == 0) {
                    pdst[0] = sa;
                    pdst[1] = sb;
                    pdst[2] = sd;
                }
            }
        } else if (pdst) {
            const double st = pickfreeze_sq_sum(fA, f, live), su = pickfreeze_sq_sum(fB, f, live);
            if (lane == 0) {
                pdst[3 + 2 * (e - 2)] = st;
                pdst[4 + 2 * (e - 2)] = su;
            }
        }
    }
}

// mean[c][j] = (sum over the row's tiles of part[tile][j]) / K, one wave per controller row: mc_fid_grad_mean_kernel's arithmetic
// (lane t adds the tiles t, t + 64, ... in order, then the fixed shuffle tree).
__global__ __launch_bounds__(64) void mc_fid_pickfreeze_mean_kernel(const double* part, double* mean, long long tiles_per_ctrl, int nent,
                                                                    long long K) {
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;
    const double* row = part + c * tiles_per_ctrl * nent;
    for (int j = 0; j < nent; ++j) {
        double acc = 0.0;
        for (long long t = lane; t < tiles_per_ctrl; t += 64) acc += row[t * nent + j];
        acc = pickfreeze_wave_sum(acc);
        if (lane == 0) mean[c * nent + j] = acc / (double)K;
    }
}

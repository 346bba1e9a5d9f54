// Lane-per-sample kernel for the fidelity AND its gradient with respect to the controller, chain topology:
// mc_fid_grad_kernel<N> (N = 2 .. RC_MAX_NSPIN_GRAD) and the second pass of the row means, mc_fid_grad_mean_kernel.
//
// Included by robchar_grad.hip inside its anonymous namespace; not a stand-alone header.
// Same tiling and staging as mc_fid_chain_kernel (k_fidelity_chain.inc.h): one wave per 64-sample tile of ONE controller,
// the controller row wave-uniform, the tile's draws one contiguous run brought in by LDS-DMA in phases and read back
// transposed.  Per lane: grad_core.h (all-fp64 QL with eigenvector rows in registers, then the spectral formulas), in
// passes over batches of rows from N = 10 (grad_batch_rows).  The eigenvector rows are the register budget: grad_min_waves
// below is chosen from the listing (`make asm`; DESIGN.md has the VGPR counts per N).
//
// Row means (`part` != nullptr): every tile writes the wave sums of (F, dF/dx_0 .. dF/dx_N) over its samples - a fixed
// shuffle tree, lanes beyond the row's end add zeros - to part[tile][N + 2]; mc_fid_grad_mean_kernel adds a row's tiles in
// a fixed order.  No atomics: the same inputs give the same bits on every run.

constexpr int grad_min_waves(int n) { return n <= 3 ? 4 : (n <= 5 ? 3 : (n <= 7 ? 2 : 1)); }
constexpr int grad_phases(int n) { return n <= 2 ? 1 : (n <= 8 ? 2 : 4); }

struct GradLdsVec {
    double* base;
    int stride;
    __device__ __forceinline__ double& operator[](int i) const { return base[i * stride]; }
};
struct GradLdsMat {         // z(q, i) of tridiag_qln_general, lane-strided
    double* base;
    int stride, n;
    __device__ __forceinline__ double& operator()(int q, int i) const { return base[(q * n + i) * stride]; }
};

__device__ __forceinline__ double grad_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                              // valid in lane 0
}

template <int N>
__global__ __launch_bounds__(64, grad_min_waves(N)) void mc_fid_grad_kernel(const GradParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int PH = grad_phases(N);
    constexpr int SP = 64 / PH;                    // samples per staging phase
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
    double* gdst = p.grad ? p.grad + (c * p.K + kb) * (N + 1) : nullptr;
    double* pdst = p.part ? p.part + tile * (N + 2) : nullptr;
    if (pad) {                                     // NaN-padded controller row: NaN everywhere, no draws read
        const double nan = __builtin_nan("");
        if (fdst && lane < nk) fdst[lane] = nan;
        if (gdst) {
            for (int i = lane; i < nk * (N + 1); i += 64) gdst[i] = nan;
        }
        if (pdst && lane < N + 2) pdst[lane] = nan;
        return;
    }

    // HBM -> LDS -> registers, with the default cache policy (AUX = 0)
    const char* src = (const char*)(p.draws + c * p.draw_cstride + kb * G);
    double gl[G];
    stage_tile_draws<G, PH, 0>(src, nk, lane, p.align16, stage, gl);
    __builtin_amdgcn_s_setprio(0);

    constexpr int R = rc::grad_batch_rows(N);      // rows of the eigenvector matrix per QL pass (grad_core.h)
    constexpr int NP = rc::grad_passes(N);
    double d0[NP > 1 ? N : 1], e0[NP > 1 ? N : 1];  // the matrix, kept for the later passes
    if constexpr (NP > 1) {
        if (lane < nk) rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, d0, e0);
    }
    const bool same = p.in == p.out;
#pragma unroll 1
    for (int pass = 0; pass < NP; ++pass) {
        int site[R];                               // wave-uniform: the site of every row of this pass (-1: none)
        rc::grad_pass_rows<N>(p.in, p.out, pass, site);
        rc::TriEig<N, R> s;
        bool ok = true;
        if constexpr (NP > 1) {
            if (lane < nk) ok = rc::grad_eigensystem_fast<N, R>(d0, e0, site, s);
        } else {
            if (lane < nk) {
                rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, s.d, s.e);
                ok = rc::grad_eigensystem_fast<N, R>(s.d, s.e, site, s);
            }
        }
        const unsigned long long badmask = __ballot(lane < nk && !ok);
        if (badmask != 0ull) {
            // Rare (not observed): some lane's QL ran into the sweep cap.  Those lanes recompute their eigensystem with the
            // textbook routine, CH at a time, vectors in the staging buffer (free now), draws re-read from HBM.
            if (lane == 0 && pass == 0) atomicAdd(&g_grad_general_tiles, 1ull);
            const bool bad = (badmask >> lane) & 1ull;
            const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
            const int nbad = __popcll(badmask);
#pragma unroll 1
            for (int c0 = 0; c0 < nbad; c0 += CH) {
                const int rel = rank - c0;
                if (bad && rel >= 0 && rel < CH) {
                    const GradLdsVec vd{stage + rel, CH}, ve{stage + N * CH + rel, CH};
                    const GradLdsMat vz{stage + 2 * N * CH + rel, CH, N};
                    rc::grad_eigensystem_general<N, R>(xg, p.h0.diag, p.h0.off, (const double*)src + (long long)lane * G, site, vd,
                                                       ve, vz, s);
                }
            }
        }

        double f = 0.0, g[R + 1];
#pragma unroll
        for (int l = 0; l <= R; ++l) g[l] = 0.0;
        if (lane < nk) rc::gradient_from_eigensystem<N, R>(s, x[N], same, f, g);
        // (grad_result_column: rows out, in and the time entry are written by the first pass only, like the fidelity)
#pragma unroll
        for (int l = 0; l <= R; ++l) {
            const int col = rc::grad_result_column<N>(site, pass, l);     // wave-uniform
            if (col < 0) continue;
            if (gdst && lane < nk) gdst[lane * (N + 1) + col] = g[l];
            if (pdst) {
                const double sg = grad_wave_sum(g[l]);
                if (lane == 0) pdst[1 + col] = sg;
            }
        }
        if (pass == 0) {
            if (fdst && lane < nk) fdst[lane] = f;
            if (pdst) {
                const double sf = grad_wave_sum(f);
                if (lane == 0) pdst[0] = sf;
            }
        }
    }
}

// mean[c][j] = (sum over the row's tiles of part[tile][j]) / K, one wave per controller row: lane t adds the tiles t, t + 64,
// ... in order, then the fixed shuffle tree.
__global__ __launch_bounds__(64) void mc_fid_grad_mean_kernel(const double* part, double* mean, long long tiles_per_ctrl, int nent,
                                                              long long K) {
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;
    const double* row = part + c * tiles_per_ctrl * nent;
    for (int j = 0; j < nent; ++j) {
        double acc = 0.0;
        for (long long t = lane; t < tiles_per_ctrl; t += 64) acc += row[t * nent + j];
        acc = grad_wave_sum(acc);
        if (lane == 0) mean[c * nent + j] = acc / (double)K;
    }
}

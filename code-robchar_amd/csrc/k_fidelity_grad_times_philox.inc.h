// mc_fid_grad_times_philox_kernel<N> (N = 2 .. RC_MAX_NSPIN_GRAD): mc_fid_grad_philox_kernel (k_fidelity_grad_philox.inc.h) on a
// GRID OF READOUT TIMES: per sample the weighted fidelity W = sum_j w_j F(u_j), u_j = T tscale_j + tshift_j, and its gradient with
// respect to the controller row, from ONE eigen decomposition (grad_times_core.h has the definition and the fixed arithmetic).
// The call of gradient_from_eigensystem is replaced by the loop over the grid around it; everything else is that kernel's:
// tiling and the NaN-row rule, philox_lane_draws with the two draw modes and sigma / sigma_rows, grad_load_matrix,
// grad_eigensystem_fast and the row batches from N = 10 (the loop sits inside every QL pass; rows out and in ride in every pass,
// so W is pass 0's value; grad_result_column decides what a pass writes), the sweep-cap fallback (textbook QL in LDS,
// grad_philox_element; counted in g_grad_general_tiles, forced by -DRC_GRAD_FORCE_GENERAL=1), grad_wave_sum and the part rows
// [tile][N + 2] ([2N + 4] with the moment sums: mean W^2 and mean W dW/dx_l, each product rounded once).  The second pass is
// mc_fid_grad_mean_kernel / mc_fid_grad_moment_mean_kernel, unchanged.
//
// fid and grad are bit for bit what M launches of mc_fid_grad_philox_kernel on controllers with the time entry replaced by u_j
// give when the time column is multiplied by tscale_j and the slabs are combined by the fma sequence; with M = 1, the unit grid
// and w = 1 all four outputs are that kernel's bits.
//
// Registers.  The loop adds R + 2 accumulators that live across the inlined pair loop of gradient_from_eigensystem.  Where the
// parent kernel has the room they are registers (GradTimesRegs); where it has not (grad_times_acc_in_lds) they sit lane-strided
// in LDS - (R + 2) 64 doubles, one read and one write per entry and grid time, against N (N - 1) / 2 sincs per time - and the
// kernel keeps the parent's launch bound.  DESIGN.md has the listing table; no instantiation may spill or use scratch
// (tests/test_asm_grad_times.py).
//
// Included by robchar_grad.hip inside its anonymous namespace after k_fidelity_grad_philox.inc.h; not a stand-alone header.

// from the listing (DESIGN.md has the table)
constexpr int grad_times_min_waves(int n) { return grad_philox_min_waves(n); }
constexpr bool grad_times_acc_in_lds(int n) { return n >= 5; }
// eigensystem_fence (grad_times_core.h) at the head of every grid time: on for N <= 8 and N = 12, off for N = 9, 10, 11, whose
// listings have no spill without it (the time-independent factors hoisted out of the loop fit the 512 registers of one wave
// per SIMD) and spill copies with it
constexpr bool grad_times_fence(int n) { return n <= 8 || n == 12; }
// the matrix (d0, e0) that the later QL passes start from sits lane-strided in LDS instead of 4 N registers held across every pass
constexpr bool grad_times_matrix_in_lds(int n) { return rc::grad_passes(n) > 1; }

// The grid of grad_times_core.h's loop read through the CONSTANT address space: the arrays are inputs that nothing writes while
// the kernel runs, and the index is wave-uniform, so every value is a scalar load into scalar registers (through a plain global
// pointer the compiler cannot prove the arrays unclobbered - the kernel stores and has an atomic - and issues vector loads).
typedef const __attribute__((address_space(4))) double* rc_cptr_t;
struct GradTimesScalarGrid {
    int M;
    rc_cptr_t tscale, tshift, weights;
    __device__ __forceinline__ GradTimesScalarGrid(const GradTimesParams& p)
        : M(p.M), tscale((rc_cptr_t)p.tscale), tshift((rc_cptr_t)p.tshift), weights((rc_cptr_t)p.weights) {}
    // (the loaded value is moved to a vector register at once: as scalar operands the three values change the allocation of the
    // loop body enough to spill at N = 5, 6 and 9 - the listing -, and every use is a vector instruction anyway)
    static __device__ __forceinline__ double in_vgpr(double v) {
        asm volatile("" : "+v"(v));
        return v;
    }
    __device__ __forceinline__ double scale(int j) const { return in_vgpr(tscale ? tscale[j] : 1.0); }
    __device__ __forceinline__ double shift(int j) const { return in_vgpr(tshift ? tshift[j] : 0.0); }
    __device__ __forceinline__ double weight(int j) const { return in_vgpr(weights[j]); }
};

struct GradTimesLdsAcc {    // entry l of this lane's accumulators, lane-strided
    double* base;
    __device__ __forceinline__ double get(int l) const { return base[l * 64]; }
    __device__ __forceinline__ void set(int l, double v) { base[l * 64] = v; }
};

template <int N>
__global__ __launch_bounds__(64, grad_times_min_waves(N)) void mc_fid_grad_times_philox_kernel(const GradTimesParams p) {
    constexpr int G = 3 * N;                       // doubles per sample
    constexpr int kWork = 2 * N + N * N;           // doubles per sample of the textbook routine
    constexpr int CH = N <= 8 ? 8 : 4;             // lanes of it at a time
    constexpr int R = rc::grad_batch_rows(N);      // rows of the eigenvector matrix per QL pass (grad_core.h)
    constexpr int NP = rc::grad_passes(N);
    constexpr bool kLdsAcc = grad_times_acc_in_lds(N);
    constexpr bool kFence = grad_times_fence(N);
    constexpr bool kLdsMat = grad_times_matrix_in_lds(N);
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ __attribute__((aligned(16))) double work[(kWork + G) * CH];
    __shared__ __attribute__((aligned(16))) double accs[kLdsAcc ? (R + 2) * 64 : 1];
    __shared__ __attribute__((aligned(16))) double mat[kLdsMat ? 2 * N * 64 : 1];

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

    // the matrix, kept for the later passes: mat[i][lane] = d0[i], mat[N + i][lane] = e0[i] (every lane reads back what it wrote)
    if constexpr (NP > 1) {
        static_assert(kLdsMat, "the multi-pass sizes keep the matrix in LDS");
        double d0[N] = {}, e0[N] = {};             // (zeros in a lane beyond the row's end)
        if (live) rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, d0, e0);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            mat[i * 64 + lane] = d0[i];
            mat[(N + i) * 64 + lane] = e0[i];
        }
    }
    const bool same = p.in == p.out;
    const GradTimesScalarGrid grid(p);
#pragma unroll 1
    for (int pass = 0; pass < NP; ++pass) {
        int site[R];                               // wave-uniform: the site of every row of this pass (-1: none)
        rc::grad_pass_rows<N>(p.in, p.out, pass, site);
        rc::TriEig<N, R> s;
        bool ok = true;
        if constexpr (NP > 1) {
            double d0[N], e0[N];
            asm volatile("" ::: "memory");         // (read back in every pass: nothing of the matrix is carried in registers)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                d0[i] = mat[i * 64 + lane];
                e0[i] = mat[(N + i) * 64 + lane];
            }
            if (live) ok = rc::grad_eigensystem_fast<N, R>(d0, e0, site, s);
        } else {
            if (live) {
                rc::grad_load_matrix<N>(x, p.h0.diag, p.h0.off, [&gl](int i) { return gl[i]; }, s.d, s.e);
                ok = rc::grad_eigensystem_fast<N, R>(s.d, s.e, site, s);
            }
        }
        const unsigned long long badmask = __ballot(live && !ok);
        if (badmask != 0ull) {
            // Rare: some lane's QL ran into the sweep cap - the textbook routine as in mc_fid_grad_philox_kernel
            if (lane == 0 && pass == 0) atomicAdd(&g_grad_general_tiles, 1ull);
            const bool bad = (badmask >> lane) & 1ull;
            const int rank = __popcll(badmask & ((1ull << lane) - 1ull));
            const int nbad = __popcll(badmask);
#pragma unroll 1
            for (int b0 = 0; b0 < nbad; b0 += CH) {
                const int rel = rank - b0;
                if (bad && rel >= 0 && rel < CH) {
                    double* g = work + kWork * CH + rel * G;
                    // (E again from an opaque copy of the lane number: see mc_fid_grad_philox_kernel)
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

        // the loop over the grid: W and the R + 1 gradient entries of this pass (a lane beyond the row's end: zeros)
        double f, g[R + 1];
        if constexpr (kLdsAcc) {
            GradTimesLdsAcc acc{accs + lane};
#pragma unroll
            for (int l = 0; l <= R + 1; ++l) acc.set(l, 0.0);
            if (live) rc::gradient_times_from_eigensystem<N, R, kFence>(s, x[N], same, grid, acc);
#pragma unroll
            for (int l = 0; l <= R; ++l) g[l] = acc.get(l);
            f = acc.get(R + 1);
        } else {
            rc::GradTimesRegs<R> acc;
#pragma unroll
            for (int l = 0; l <= R + 1; ++l) acc.set(l, 0.0);
            if (live) rc::gradient_times_from_eigensystem<N, R, kFence>(s, x[N], same, grid, acc);
#pragma unroll
            for (int l = 0; l <= R; ++l) g[l] = acc.get(l);
            f = acc.get(R + 1);
        }
        // (grad_result_column: rows out, in and the time entry are written by the first pass only, like W)
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

// Pairwise Wasserstein distances between sorted rows (ABI 18): out[i][j] = W_p(A[i], B[j]) = (mean_k |a_ik - b_jk|^p)^(1/p),
// p = 1, 2.  An "L1 GEMM": there is no MFMA form of |a - b|, so this is fp64 VALU work, 2 instructions per term (p = 1: v_add_f64
// d = a - b, v_add_f64 acc += |d| with the source modifier; p = 2: v_add_f64, v_fma_f64).
//
// A workgroup of 256 threads owns a 64 x 64 tile of (i, j) and the range of k that the launch's plan gives it
// (wasserstein_core.h); each thread keeps a 4 x 4 block of elements in registers.  kStep = 32 values of k of the 64 + 64 rows are
// staged in LDS transposed, [k][row] with kLdsStride = 66 doubles per k, while the next 32 wait in registers: global reads run
// along k (8 consecutive doubles per row and 16 lanes), and the staging stores of 16 consecutive lanes (ds_write_b64's conflict
// group) go to 32 distinct banks.  Per k a thread reads its rows {2 ty, 2 ty + 1} and {32 + 2 ty, 33 + 2 ty} and the columns of tx
// likewise, four ds_read_b128: the 16 lanes of a b128 group hold all 16 tx and two ty, so the B reads cover 256 contiguous bytes
// and the A reads two 16-byte slots beside each other - conflict-free.  16 LDS cycles against 32 fp64 instructions (128 issue
// cycles) per k and wave.
// Rows past CA / CB and values of k past the range are staged as +0: their terms are +0 and change no bit of a sum.
// The summation order (Levels) is that of rcwd::range_sum, so an element's bits depend on its two rows, K and p alone.

// tile (ti, tj), ti <= tj, number `t` of the nt (nt + 1) / 2 tiles on or above the diagonal, row by row
__device__ __forceinline__ void wd_sym_tile(long long t, long long nt, long long* ti, long long* tj) {
    const long long rev = nt * (nt + 1) / 2 - 1 - t;          // counted from the last tile: row r from the end holds r + 1 tiles
    long long r = (long long)((sqrt(8.0 * (double)rev + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > rev) --r;
    while ((r + 1) * (r + 2) / 2 <= rev) ++r;
    *ti = nt - 1 - r;
    *tj = nt - 1 - (rev - r * (r + 1) / 2);
}

template <int P>
__global__ __launch_bounds__(rcwd::kThreads, 2) void wasserstein_tile_kernel(const rcwd::Params p) {
    using namespace rcwd;
    constexpr int kPasses = 2 * kTile * kStep / kThreads;     // 16 values per thread and step
    __shared__ __attribute__((aligned(16))) double s_a[kStep * kLdsStride];
    __shared__ __attribute__((aligned(16))) double s_b[kStep * kLdsStride];
    const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
    const long long tile = (long long)blockIdx.x % p.tiles, q = (long long)blockIdx.x / p.tiles;
    long long ti, tj;
    if (p.sym) {
        wd_sym_tile(tile, p.nti, &ti, &tj);
    } else {
        ti = tile / p.ntj;
        tj = tile % p.ntj;
    }
    const long long i0 = ti * kTile, j0 = tj * kTile;
    const long long k0 = p.plan.begin(q), k1 = p.plan.end(q, p.K);

    // staging: pass s of a thread takes k = 8 (s & 3) + (t & 7) of tile row 32 (s >> 2) + (t >> 3); rows 0 .. 63 are A's, 64 .. 127 B's
    const int sk = t & 7, srow = t >> 3;
    const double* grow[4];
    bool gok[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const long long row = (rb < 2 ? i0 : j0) + (rb & 1) * 32 + srow, rows = rb < 2 ? p.CA : p.CB;
        gok[rb] = row < rows;
        grow[rb] = (rb < 2 ? p.a : p.b) + (gok[rb] ? row : 0) * p.K;
    }
    double stage[kPasses];
    auto load = [&](long long s0) {
#pragma unroll
        for (int s = 0; s < kPasses; ++s) {
            const long long k = s0 + 8 * (s & 3) + sk;
            stage[s] = (gok[s >> 2] && k < k1) ? grow[s >> 2][k] : 0.0;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int s = 0; s < kPasses; ++s) {
            double* img = (s >> 2) < 2 ? s_a : s_b;
            img[(8 * (s & 3) + sk) * kLdsStride + ((s >> 2) & 1) * 32 + srow] = stage[s];
        }
    };

    double a0[kReg][kReg], a1[kReg][kReg], a2[kReg][kReg], a3[kReg][kReg];   // the four levels of rcwd::Levels
#pragma unroll
    for (int r = 0; r < kReg; ++r)
#pragma unroll
        for (int c = 0; c < kReg; ++c) a0[r][c] = a1[r][c] = a2[r][c] = a3[r][c] = 0.0;

    load(k0);
    for (long long s0 = k0; s0 < k1; s0 += kStep) {
        __syncthreads();                                       // the previous step's reads are done
        store();
        __syncthreads();
        const long long next = s0 + kStep;
        const bool last = next >= k1;
        if (!last) load(next);
#pragma unroll 8
        for (int kk = 0; kk < kStep; ++kk) {
            const double2 al = *(const double2*)&s_a[kk * kLdsStride + 2 * ty], ah = *(const double2*)&s_a[kk * kLdsStride + 32 + 2 * ty];
            const double2 bl = *(const double2*)&s_b[kk * kLdsStride + 2 * tx], bh = *(const double2*)&s_b[kk * kLdsStride + 32 + 2 * tx];
            const double av[kReg] = {al.x, al.y, ah.x, ah.y}, bv[kReg] = {bl.x, bl.y, bh.x, bh.y};
#pragma unroll
            for (int r = 0; r < kReg; ++r)
#pragma unroll
                for (int c = 0; c < kReg; ++c) a0[r][c] = add_term<P>(a0[r][c], av[r], bv[c]);
        }
        // rcwd::levels_close for the 16 elements (kChunk is a multiple of kStep; the branches are uniform)
        if (last || next % kChunk == 0) {
            const bool c1 = last || next % kGroup1 == 0, c2 = last || next % kGroup2 == 0;
#pragma unroll
            for (int r = 0; r < kReg; ++r)
#pragma unroll
                for (int c = 0; c < kReg; ++c) {
                    a1[r][c] += a0[r][c];
                    a0[r][c] = 0.0;
                    if (c1) {
                        a2[r][c] += a1[r][c];
                        a1[r][c] = 0.0;
                    }
                    if (c2) {
                        a3[r][c] += a2[r][c];
                        a2[r][c] = 0.0;
                    }
                }
        }
    }

    const bool direct = p.plan.nparts == 1, mirror = p.sym && ti != tj;
    double* dst = direct ? p.out : p.part + q * p.CA * p.CB;
#pragma unroll
    for (int r = 0; r < kReg; ++r) {
        const long long i = i0 + owned_row(ty, r);
        if (i >= p.CA) continue;
#pragma unroll
        for (int c = 0; c < kReg; ++c) {
            const long long j = j0 + owned_row(tx, c);
            if (j >= p.CB) continue;
            const double v = direct ? finish<P>(a3[r][c], p.K) : a3[r][c];
            dst[i * p.CB + j] = v;
            if (direct && mirror) dst[j * p.CB + i] = v;
        }
    }
}

// The levels above the split (rcwd::combine_parts), the division and the root: one thread per element of out.  In symmetric mode
// the partial sums exist for tiles on or above the diagonal only; an element below takes its mirror image's.
template <int P>
__global__ __launch_bounds__(256) void wasserstein_finish_kernel(const rcwd::Params p) {
    using namespace rcwd;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n = p.CA * p.CB;
    if (e >= n) return;
    const long long i = e / p.CB, j = e % p.CB;
    const long long src = (p.sym && i / kTile > j / kTile) ? j * p.CB + i : e;
    p.out[e] = finish<P>(combine_parts(p.part + src, n, p.plan.nparts, p.plan.unit), p.K);
}

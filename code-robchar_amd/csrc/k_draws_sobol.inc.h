// sobol_draws_kernel: the scrambled Sobol points of code-robchar_amd/sobol.py and their normals as tensors, bits[C][K][D] (uint32,
// the points x) and draws[C][K][D] (fp64, sigma_c Phi^-1((x + 0.5) 2^-32)); either may be NULL.  Any D up to RC_SOBOL_MAX_DIM.
// One wave per tile of 64 consecutive samples of one controller row (sobol_core.h: the tile's wave-uniform part of every
// coordinate is formed once, in LDS).  The tile's 64 D elements are one contiguous run of both tensors: the lanes walk it element
// by element, so every store is coalesced; element e is (sample e / D, dimension e % D), kept by increments.  No atomics: same
// inputs, same bits.
//
// Part of ONE translation unit: #included by robchar_qmc.hip inside its anonymous namespace, after sobol_core.h.
__global__ __launch_bounds__(64) void sobol_draws_kernel(const SobolDraws q, const long long K, const long long tiles_per_row,
                                                         double* __restrict__ draws, unsigned int* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) double lntab[256];
    __shared__ unsigned int base[RC_SOBOL_MAX_DIM];

    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;             // wave-uniform
    const long long c = tile / tiles_per_row;
    const long long kb = (tile - c * tiles_per_row) * 64;
    const int nk = (int)((K - kb < 64) ? (K - kb) : 64);
    const int D = q.D;

    reinterpret_cast<double2*>(lntab)[lane] = reinterpret_cast<const double2*>(g_ln_table)[lane];
    reinterpret_cast<double2*>(lntab)[lane + 64] = reinterpret_cast<const double2*>(g_ln_table)[lane + 64];
    const SobolTile t = sobol_tile(q, c, kb);
    sobol_tile_base(t, D, lane, base);
    __syncthreads();

    const double sigma = q.sigma_rows ? q.sigma_rows[c] : q.sigma;
    const long long row0 = (c * K + kb) * D;       // the tile's first element
    const int total = nk * D;
    const int ds = 64 / D, dd = 64 % D;
    int s = lane / D, d = lane % D;
    for (int e = lane; e < total; e += 64) {
        const unsigned int x = sobol_point(t, base, (unsigned int)(s ^ (s >> 1)), d);
        if (bits) bits[row0 + e] = x;
        if (draws) draws[row0 + e] = sobol_draw(x, sigma, lntab);
        s += ds;
        d += dd;
        if (d >= D) {
            d -= D;
            ++s;
        }
    }
}

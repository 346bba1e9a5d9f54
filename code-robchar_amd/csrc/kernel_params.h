// Parameter blocks of the fidelity kernels, shared by the two translation units of librobchar_hip.so (robchar_hip.hip: host side,
// C ABI and most kernels; robchar_large.hip: the largest instantiations - chains of 17 .. 24 spins, rings of 11 .. 16 - compiled in
// parallel).  Passed by value in the kernarg segment.
#pragma once
#include "../../include/robchar_hip.h"

namespace rckp {

struct StaticH {          // passed by value in the kernarg segment: no device allocation for 2N doubles
    double diag[RC_MAX_NSPIN];
    double off[RC_MAX_NSPIN];
};

// Cache policy of the draw stream: the `aux` operand of the LDS-DMA loads (__builtin_amdgcn_global_load_lds) of
// mc_fid_chain_kernel and stage_tile_draws.  The draws are read exactly once per launch and are larger than L2 (168 MB at
// 100 x 10 000, N = 7), so they stream: 2 = the `nt` bit (global_load_lds_dword[x4] ... nt), 0 = the default policy.
// Changes no arithmetic (profiles/launch_boundary_ab.txt: the A/B against the default policy).
constexpr int kDrawLoadAux = 2;

struct FidParams {
    const double* ctrl;    // [C][N+1]
    const double* draws;   // [C][K][N][3]
    double* fid;           // [C][K]
    long long C, K;
    long long draw_cstride;     // elements between consecutive controllers' draw blocks (K*3N; 0 = shared set)
    long long tiles_per_ctrl;   // ceil(K / 64)
    long long ntiles;           // C * tiles_per_ctrl
    int in, out;
    int align16;                // draws base and every controller's run of K*3N doubles are 16-byte aligned
    int nt_store;               // mc_fid_chain_kernel: the fidelities leave with a non-temporal store (host rule: launch_chain)
    StaticH h0;
    long long* stamps;          // diagnostic builds only (-DRC_STAMPS): [ntiles][kStampSlots] stamps, indexed by tile
};
constexpr int kStampSlots = 12; // (RC_STAMPS) slots of one tile's record: mc_fid_chain_kernel lists them where it writes them

// repair list of the ring-topology route (mc_fid_ring_mixed_kernel -> mc_fid_ring_repair_kernel)
struct RingRepairList {
    unsigned long long* count;        // [1] number of listed samples of THIS call (zero on entry)
    unsigned long long* clear;        // [1] the counter the NEXT call on this stream will use: zeroed by this call's first wave
    long long* samples;               // [>= C * K] flat sample indices c * K + k
};

// fidelity + gradient kernel (k_fidelity_grad.inc.h): FidParams' geometry, three optional outputs
struct GradParams {
    const double* ctrl;    // [C][N+1]
    const double* draws;   // [C][K][N][3]
    double* fid;           // [C][K] or NULL
    double* grad;          // [C][K][N+1] or NULL
    double* part;          // [ntiles][N+2] per-tile sums for the row means, or NULL
    long long C, K;
    long long draw_cstride;
    long long tiles_per_ctrl;
    long long ntiles;
    int in, out;
    int align16;
    StaticH h0;
};

// fidelity + noise-sensitivity kernel (k_fidelity_sens.inc.h): the same geometry, derivatives in the draws' own layout
struct SensParams {
    const double* ctrl;    // [C][N+1]
    const double* draws;   // [C][K][N][3]
    double* fid;           // [C][K] or NULL
    double* sens;          // [C][K][N][3] or NULL
    double* part;          // [ntiles][3N+2] per-tile sums for the row means, or NULL
    long long C, K;
    long long draw_cstride;
    long long tiles_per_ctrl;
    long long ntiles;
    int in, out;
    int align16;
    StaticH h0;
};

// fidelity + noise-sensitivity kernel with the counter-based draws generated inside it (k_fidelity_sens_philox.inc.h): SensParams'
// geometry without a draw tensor; sample (c, k), site i, slot s is element  offset + ((c K + k) N + i) 3 + s  of stream `seed`
struct SensPhiloxParams {
    const double* ctrl;    // [C][N+1]
    double* fid;           // [C][K] or NULL
    double* sens;          // [C][K][N][3] or NULL
    double* part;          // [ntiles][3N+2] per-tile sums for the row means, or NULL
    long long C, K;
    long long tiles_per_ctrl;
    long long ntiles;
    int in, out;
    unsigned long long seed;
    unsigned long long offset;        // stream element of sample (c = 0, k = 0), site 0, slot 0
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    StaticH h0;
};

// fidelity + gradient kernel with the counter-based draws generated inside it (k_fidelity_grad_philox.inc.h): GradParams' geometry
// without a draw tensor.  Sample (c, k), site i, slot s is element  offset + ((c K + k) N + i) 3 + s  of stream `seed`, or - with
// `shared` (common random numbers) - element  offset + (k N + i) 3 + s  for every c.
struct GradPhiloxParams {
    const double* ctrl;    // [C][N+1]
    double* fid;           // [C][K] or NULL
    double* grad;          // [C][K][N+1] or NULL
    double* part;          // [ntiles][N+2] per-tile sums for the row means ([ntiles][2N+4] with `moments`), or NULL
    long long C, K;
    long long tiles_per_ctrl;
    long long ntiles;
    int in, out;
    int shared;                       // 1: one draw set for every controller row
    int moments;                      // 1: the part rows also carry the sums of F^2 and F dF/dx
    unsigned long long seed;
    unsigned long long offset;        // stream element of sample (c = 0, k = 0), site 0, slot 0
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    StaticH h0;
};

// GradPhiloxParams on a grid of M readout times (k_fidelity_grad_times_philox.inc.h): u_cj = T_c tscale_j + tshift_j; `fid` and
// `grad` carry the weighted sums W = sum_j weights_j F_j and dW/dx, the part rows their tile sums (and, with `moments`, those of
// W^2 and W dW/dx).
struct GradTimesParams {
    const double* ctrl;    // [C][N+1]
    double* fid;           // [C][K] or NULL: W
    double* grad;          // [C][K][N+1] or NULL: dW/dx
    double* part;          // [ntiles][N+2] per-tile sums for the row means ([ntiles][2N+4] with `moments`), or NULL
    long long C, K;
    long long tiles_per_ctrl;
    long long ntiles;
    int in, out;
    int shared;                       // 1: one draw set for every controller row
    int moments;                      // 1: the part rows also carry the sums of W^2 and W dW/dx
    unsigned long long seed;
    unsigned long long offset;        // stream element of sample (c = 0, k = 0), site 0, slot 0
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    const double* tscale;  // [M] or NULL: 1
    const double* tshift;  // [M] or NULL: 0
    const double* weights; // [M]
    int M;
    StaticH h0;
};

// GradPhiloxParams over a list of each row's draws (k_fidelity_grad_listed.inc.h): slot s of row c is sample (c, list[c][s]) of
// the same stream convention - a value outside 0 .. K - 1 is an empty slot -; the tiles cover the L slots of a row, the outputs
// are per slot and the part rows carry the sums weighted by weight[c][s].
struct GradListedParams {
    const double* ctrl;    // [C][N+1]
    double* fid;           // [C][L] or NULL
    double* grad;          // [C][L][N+1] or NULL
    double* part;          // [ntiles][N+2] per-tile weighted sums for the row sums, or NULL
    long long C, K;
    long long tiles_per_ctrl;         // ceil(L / 64)
    long long ntiles;                 // C * tiles_per_ctrl
    int in, out;
    int shared;                       // 1: one draw set for every controller row
    unsigned long long seed;
    unsigned long long offset;        // stream element of sample (c = 0, k = 0), site 0, slot 0
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    const int* list;       // [C][L]
    const double* weight;  // [C][L], or NULL: 1 for every slot
    long long L;
    StaticH h0;
};

// fidelity on a grid of M readout times (k_fidelity_times.inc.h): FidParams' geometry, t_cj = |T_c tscale_j + tshift_j|, three
// optional outputs.  mc_fid_times_kernel reads `draws`; mc_fid_times_philox_kernel generates sample (c, k), site i, slot s as
// element  offset + ((c K + k) N + i) 3 + s  of stream `seed` and ignores `draws`, `draw_cstride` and `align16`.
struct TimesParams {
    const double* ctrl;    // [C][N+1]
    const double* draws;   // [C][K][N][3]
    double* fid;           // [M][C][K] or NULL
    double* wsum;          // [C][K] or NULL (needs `weights`)
    double* fmin;          // [C][K] or NULL
    const double* tscale;  // [M] or NULL: 1
    const double* tshift;  // [M] or NULL: 0
    const double* weights; // [M] or NULL
    int M;
    long long C, K;
    long long draw_cstride;     // elements between consecutive controllers' draw blocks (K*3N; 0 = shared set)
    long long tiles_per_ctrl;   // ceil(K / 64)
    long long ntiles;           // C * tiles_per_ctrl
    int in, out;
    int align16;
    unsigned long long seed;
    unsigned long long offset;        // stream element of sample (c = 0, k = 0), site 0, slot 0
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    StaticH h0;
};

// scrambled Sobol points (sobol_core.h; the definition: code-robchar_amd/sobol.py): sample k of controller row c is point
// skip + (k mod P) of replicate k / P; its D coordinates read dirnum[r][d][0..31] and shift[c or 0][r][d]
struct SobolDraws {
    const unsigned int* dirnum;       // [R][D][32]
    const unsigned int* shift;        // [Cs][R][D]
    long long shift_cstride;          // R D (a row per controller) or 0 (row 0 for all)
    long long P;                      // points per replicate
    unsigned long long skip;          // first point of every replicate
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    int R, D;
};

// pick-freeze kernel of the variance indices (k_fidelity_pickfreeze.inc.h; the definition: code-robchar_amd/variance_indices.py):
// FidParams' geometry without a draw tensor and TWO draw vectors per sample - coordinate j = 3 i + s of sample (c, k) is element
// offset_a (offset_b) + (c K + k) 3 N + j  of stream `seed` -; evaluation e = 0 takes a, e = 1 takes b, e = 2 + g takes b where
// groups[g] has bit j set and a elsewhere.
struct PickFreezeParams {
    const double* ctrl;    // [C][N+1]
    double* fid;           // [G+2][C][K] or NULL
    double* part;          // [ntiles][3+2G] per-tile sums for the row means, or NULL
    long long C, K;
    long long tiles_per_ctrl;
    long long ntiles;
    int in, out;
    int G;                            // number of groups, 0 .. RC_PICKFREEZE_MAX_GROUPS
    unsigned long long seed;
    unsigned long long offset_a, offset_b;
    const double* sigma_rows;         // [C] scale per controller row, or NULL: `sigma` for all
    double sigma;
    StaticH h0;
    unsigned long long groups[RC_PICKFREEZE_MAX_GROUPS];   // by value: no device copy, no lifetime obligation for the caller
};

}  // namespace rckp

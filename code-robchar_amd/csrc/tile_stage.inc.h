// Bringing a tile's draws in from the draw tensor (stage_tile_draws): the one leaf that the ring, rows, gradient and
// readout-time kernels share.  Each kernel keeps its own prologue, NaN-row rule, outputs, pass loop and sweep-cap fallback
// (the walk over the bad lanes stays written out in every kernel: as a function it cost instructions, an occupancy step or
// a spill in each of them - profiles/shared_leaves_listing.txt).
//
// #included INSIDE the anonymous namespace of every device translation unit (robchar_hip.hip, robchar_large.hip,
// robchar_grad.hip, robchar_times.hip), after kernel_params.h; not a stand-alone header.
#pragma once

// operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(1))) const void* rc_gptr_t;
typedef __attribute__((address_space(3))) void* rc_lptr_t;

// HBM -> LDS -> registers for one tile (see mc_fid_chain_kernel, which keeps its own hand-placed copy, as mc_fid_sens_kernel
// does: k_fidelity_sens.inc.h says why): the nk * G doubles at `src` through the `stage` buffer in PH phases; lane l < nk ends
// with its G values in gl.  AUX is the cache-policy operand of the loads (kernel_params.h): the streaming policy unless the
// kernel says otherwise; the gradient kernel passes 0, the default policy.
template <int G, int PH, int AUX = rckp::kDrawLoadAux>
__device__ __forceinline__ void stage_tile_draws(const char* src, int nk, int lane, int align16, double* stage, double (&gl)[G]) {
    constexpr int SP = 64 / PH;
    constexpr int kPhaseBytes = SP * G * 8;
#pragma unroll
    for (int ph = 0; ph < PH; ++ph) {
        const int first = ph * SP;
        if (first < nk) {                          // wave-uniform
            const int cnt = (nk - first < SP) ? (nk - first) : SP;
            const int bytes = cnt * G * 8;
            const char* ps = src + (long long)first * G * 8;
            if (align16 && !(cnt & 1)) {
#pragma unroll
                for (int it = 0; it < (kPhaseBytes + 1023) / 1024; ++it) {
                    const int off = it * 1024 + lane * 16;
                    if (off < bytes)
                        __builtin_amdgcn_global_load_lds((rc_gptr_t)(ps + off), (rc_lptr_t)((char*)stage + it * 1024), 16, 0, AUX);
                }
            } else {
#pragma unroll 2
                for (int it = 0; it < (kPhaseBytes + 255) / 256; ++it) {
                    const int off = it * 256 + lane * 4;
                    if (off < bytes)
                        __builtin_amdgcn_global_load_lds((rc_gptr_t)(ps + off), (rc_lptr_t)((char*)stage + it * 256), 4, 0, AUX);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // DMA landed
            int rel = lane - first;
            asm volatile("" : "+v"(rel));                             // one base address + immediate offsets (see chain kernel)
            if (rel >= 0 && rel < cnt) {
#pragma unroll
                for (int i = 0; i < G; ++i) gl[i] = stage[rel * G + i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // reads done before the buffer is refilled
        }
    }
}

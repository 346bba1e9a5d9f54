// librobchar_hip.so - HIP kernels (gfx950 / MI355X) and the C ABI declared in include/robchar_hip.h.
//
// One translation unit: the kernels live in k_fidelity_chain.inc.h, k_fidelity_dense.inc.h, k_reduce_sort.inc.h and
// k_draws.inc.h (included below, inside this file's anonymous namespace); this file holds the shared parameter structs,
// the host side (per-device state, launch logic, the multi-device and legacy-stream drivers) and the extern "C" entries.
//
// Kernels
//   mc_fid_chain_kernel<N,M> one (controller, perturbation) sample per LANE, one wave per workgroup.  A wave
//                            owns tiles of 64 consecutive samples of ONE controller: the controller row is
//                            wave-uniform (scalar loads); a tile's 64*3N draws are one contiguous HBM run that
//                            is copied to LDS by LDS-DMA (global_load_lds_dwordx4: no staging VGPRs, every HBM
//                            byte fetched exactly once, fully coalesced) and read back transposed (lane l
//                            takes its own 3N values).  Per lane: real symmetric tridiagonal implicit QL in
//                            registers with wave-uniform control flow (tridiag_core.h).
//   mc_fid_ring_kernel<N>    ring topology, N = 3..10: lane per sample, complex Hermitian matrix in registers ->
//                            Householder tridiagonalisation (hermitian_core.h) -> the same QL with two complex rows.
//   mc_fid_chain_anyn_kernel chains of 16 < N <= 32 spins: the general per-sample routine, work vectors in dynamic LDS.
//   mc_fid_jacobi_kernel     general complex Hermitian path (ring topology, cross-check): 8 or 4 samples per WAVE,
//                            dense matrix in LDS, round-robin cyclic Jacobi with the rotations of a round
//                            spread over the 64 lanes.
//   mc_fid_expm_kernel       dense complex, possibly non-Hermitian H (directional_perturbation): one WAVE per sample,
//                            Pade scaling-and-squaring expm in LDS - the reference's own algorithm shape on the device.
//   reduce_kernel            one workgroup per controller: RIM_1, std, min, Q(thr) for the centre / DKW-upper /
//                            DKW-lower variants in two passes over the K fidelities (fixed summation order).
//   sort_*_kernel            row sort for the ECDF: merge sort in LDS (K <= 16384), chunked bitonic network above.
//   lbfgs_advance_kernel     one LANE per controller row: the batched L-BFGS state machine (lbfgs_core.h), state [field][C]
//   lbfgs_advance_box_kernel the same machine with box bounds: projected steps, active set in registers
//   tail_select_kernel       one workgroup per row: list, CVaR weights and value at risk of the row's lower tail by a radix
//                            select over an order-preserving key (no sort), compacted in index order.
//   philox_normal_kernel     counter-based Gaussian draws for sample spaces too large to draw on the host.
//
// Roofline: algorithmic HBM traffic is 24 N + 8 bytes per sample; the kernel is bound by
// fp64 VALU issue under the socket power cap, not by HBM.  See DESIGN.md.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <unordered_map>
#include <thread>
#include <string>
#include <vector>

#include "../../include/robchar_hip.h"
#include "kernel_params.h"
#include "tridiag_core.h"
#include "hermitian_core.h"
#include "csym_core.h"
#include "sort_core.h"
#include "select_core.h"
#include "bootstrap_core.h"
#include "wasserstein_core.h"
#include "lbfgs_core.h"
#include "legacy_rng_core.h"
#include "mt19937_jump_poly.h"
#include "ws_plan.h"
#include "sobol_joe_kuo_96.h"

// The largest instantiations live in a second translation unit (robchar_large.hip) that compiles in parallel with this one:
// chains of 17 .. 24 spins (general adjugate mode), rings of 11 .. 16 spins (mixed route + repair, all-fp64 route).  Each
// returns the hipError_t of its launch; the unit keeps its own copies of the diagnostic tile counters (rc_large_counter_addr).
extern "C" {
__attribute__((visibility("hidden"))) int rc_large_chain_launch(int N, void* stream, const rckp::FidParams* p);
__attribute__((visibility("hidden"))) int rc_large_ring_launch(int N, int mixed, void* stream, const rckp::FidParams* p, double corner,
                                                               const rckp::RingRepairList* rl, unsigned grid, unsigned rgrid);
__attribute__((visibility("hidden"))) int rc_large_counter_addr(int which, void** addr);
// third translation unit (robchar_grad.hip): the fidelity-gradient kernels
__attribute__((visibility("hidden"))) int rc_grad_launch(int N, void* stream, const rckp::GradParams* p, double* mean);
__attribute__((visibility("hidden"))) int rc_grad_philox_launch(int N, void* stream, const rckp::GradPhiloxParams* p, double* mean,
                                                                double* moment);
__attribute__((visibility("hidden"))) int rc_grad_times_philox_launch(int N, void* stream, const rckp::GradTimesParams* p, double* mean,
                                                                      double* moment);
__attribute__((visibility("hidden"))) int rc_grad_listed_launch(int N, void* stream, const rckp::GradListedParams* p, double* sum);
__attribute__((visibility("hidden"))) int rc_grad_counter_addr(void** addr);
__attribute__((visibility("hidden"))) int rc_sens_launch(int N, void* stream, const rckp::SensParams* p, double* mean);
__attribute__((visibility("hidden"))) int rc_sens_counter_addr(void** addr);
__attribute__((visibility("hidden"))) int rc_sens_philox_launch(int N, void* stream, const rckp::SensPhiloxParams* p, double* mean);
// fourth translation unit (robchar_times.hip): the fidelity on a grid of readout times
__attribute__((visibility("hidden"))) int rc_times_launch(int N, void* stream, const rckp::TimesParams* p);
__attribute__((visibility("hidden"))) int rc_times_philox_launch(int N, void* stream, const rckp::TimesParams* p);
__attribute__((visibility("hidden"))) int rc_times_counter_addr(void** addr);
// fifth translation unit (robchar_qmc.hip): the scrambled Sobol generator and the fidelity kernel that generates its Sobol normals
__attribute__((visibility("hidden"))) int rc_qmc_draws_launch(void* stream, const rckp::SobolDraws* q, long long C, long long K,
                                                              double* draws, unsigned int* bits);
__attribute__((visibility("hidden"))) int rc_qmc_fidelity_launch(int N, int ends, void* stream, const rckp::FidParams* p,
                                                                 const rckp::SobolDraws* q);
__attribute__((visibility("hidden"))) int rc_qmc_counter_addr(int which, void** addr);
// sixth translation unit (robchar_vidx.hip): the pick-freeze fidelity kernel of the variance indices and its row means
__attribute__((visibility("hidden"))) int rc_vidx_pickfreeze_launch(int N, int ends, void* stream, const rckp::PickFreezeParams* p,
                                                                    double* mean);
__attribute__((visibility("hidden"))) int rc_vidx_counter_addr(int which, void** addr);
}

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define RC_HIP_CHECK(expr)                                                                       \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(RC_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

using rckp::StaticH;
using rckp::FidParams;
using rckp::RingRepairList;

#include "tile_stage.inc.h"

#include "k_fidelity_chain.inc.h"
#include "k_fidelity_dense.inc.h"
#include "k_reduce_sort.inc.h"
#include "k_tail_select.inc.h"
#include "k_bootstrap.inc.h"
#include "k_wasserstein.inc.h"
#include "k_lbfgs.inc.h"
#include "k_draws.inc.h"
#include "k_fidelity_philox.inc.h"
#include "k_directional.inc.h"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
std::mutex g_cfg_mu;                 // guards g_default_kernel only
int g_default_kernel = RC_KERNEL_AUTO;
long long* g_stamps = nullptr;      // diagnostic builds only

// Per-device state.  The C ABI takes a `device` argument everywhere, so nothing here is process-wide: the blocking
// entry points serialise PER DEVICE (two devices run concurrently, e.g. from the threads of
// rc_mc_metrics_sharded_f64), and the kernel attributes that must be raised before a launch
// (hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property) are tracked per device.
constexpr int kMaxDevices = 64;
enum { kAttrExpm = 0, kAttrAnyN, kAttrSortMerge, kAttrSortChunk, kAttrMtJump, kAttrMtJumpWide, kAttrCount };
// repair list of the ring-topology route (k_fidelity_chain.inc.h: RingRepairList), one per (device, stream): two counters
// used in turns + C*K sample slots.  Persistent - no allocation, no memset per call: every call's first wave zeroes the
// counter of the NEXT call - and per STREAM, so that launches on different streams of one device never share a list.
// Everything that touches the buffer is ordered on ITS stream (round 4): it is allocated with hipMallocAsync, zeroed with
// hipMemsetAsync and - when a larger problem arrives, or in rc_release_stream - released with hipFreeAsync on that stream,
// behind the kernels that still read it.  An `_async` entry therefore never synchronises the device (round 3: hipFree +
// hipMalloc + a null-stream hipMemset on first use).  rc_reserve_ring pre-sizes it outside a latency-critical region.
struct RingBuf {
    char* mem = nullptr;
    long long cap = 0;               // sample slots
    int turn = 0;                    // which of the two counters the next call uses
    unsigned long long last_use = 0; // ring_buf_for's clock: the least recently used entry is evicted beyond kMaxRingBufs
};
// Streams that ran a ring launch and were never handed back with rc_release_stream keep their buffer; the map is capped so that
// a caller cycling through short-lived streams cannot grow it without bound: the entry used longest ago is freed with a plain
// (device-synchronising, stream-agnostic: its stream may be gone) hipFree when a 17th stream arrives.  Leak bound per device:
// kMaxRingBufs x (256 + 10 bytes per sample of the largest launch on that stream).
constexpr size_t kMaxRingBufs = 16;
struct DeviceCtx {
    std::mutex mu;                   // blocking entry points: one at a time per device (they share `stream` and `ws`)
    hipStream_t stream = nullptr;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    std::mutex ring_mu;
    std::unordered_map<hipStream_t, RingBuf> ring_bufs;
    unsigned long long ring_clock = 0;
    std::atomic<bool> attr[kAttrCount];
    DeviceCtx() {
        for (auto& a : attr) a.store(false);
    }
};
DeviceCtx g_ctx[kMaxDevices];

int device_in_range(int device) {
    int n = 0;
    RC_HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n || device >= kMaxDevices) return fail(RC_EINVAL, "device index out of range");
    return RC_OK;
}

// caller holds g_ctx[device].mu
int get_ctx(int device, DeviceCtx** out) {
    if (int rc = device_in_range(device)) return rc;
    RC_HIP_CHECK(hipSetDevice(device));
    if (!g_ctx[device].stream) RC_HIP_CHECK(hipStreamCreateWithFlags(&g_ctx[device].stream, hipStreamNonBlocking));
    *out = &g_ctx[device];
    return RC_OK;
}

// Raises a kernel's dynamic-LDS limit once per DEVICE (the current one).  Racing callers may both set it: idempotent.
int ensure_func_attr(int which, const void* func, int bytes) {
    int dev = 0;
    RC_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return fail(RC_EINVAL, "device index out of range");
    if (g_ctx[dev].attr[which].load(std::memory_order_acquire)) return RC_OK;
    RC_HIP_CHECK(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    g_ctx[dev].attr[which].store(true, std::memory_order_release);
    return RC_OK;
}

int ensure_ws(DeviceCtx* ctx, size_t bytes) {
    if (ctx->ws_bytes >= bytes) return RC_OK;
    if (ctx->ws) RC_HIP_CHECK(hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    RC_HIP_CHECK(hipMalloc(&ctx->ws, bytes));
    ctx->ws_bytes = bytes;
    return RC_OK;
}

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // plain host memory: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

// The device workspace of one blocking call (caller holds the device's `mu`): the call declares its arrays in order - either
// input and any output may be a host or a device pointer - and ws_plan.h derives the carving.  stage_in(): grows the workspace
// to the plan's total, then copies the staged inputs in; ptr(): what the kernel is given; stage_out(): copies the staged outputs
// back behind the launch and waits for the stream.
struct Staging {
    DeviceCtx* ctx = nullptr;
    rcws::Plan plan;
    int in(const void* p, size_t bytes) { return plan.in(p, bytes, is_device_ptr(p)); }
    int out(void* p, size_t bytes, bool always = false) { return plan.out(p, bytes, p && !always && is_device_ptr(p), always); }
    double* ptr(int slot) const { return (double*)plan.ptr(slot, ctx->ws); }
    int stage_in() {
        if (int rc = ensure_ws(ctx, plan.total)) return rc;
        for (int i = 0; i < plan.n; ++i)
            if (const rcws::Slot& s = plan.s[i]; s.input && s.staged)
                RC_HIP_CHECK(hipMemcpyAsync(ptr(i), s.user, s.bytes, hipMemcpyHostToDevice, ctx->stream));
        return RC_OK;
    }
    int stage_out() {
        for (int i = 0; i < plan.n; ++i)
            if (const rcws::Slot& s = plan.s[i]; !s.input && s.staged && s.user)
                RC_HIP_CHECK(hipMemcpyAsync((void*)s.user, ptr(i), s.bytes, s.always ? hipMemcpyDefault : hipMemcpyDeviceToHost,
                                            ctx->stream));
        RC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return RC_OK;
    }
};

// stream-ordered release of a hipMallocAsync block at scope exit
struct StreamFree {
    void* p;
    hipStream_t s;
    ~StreamFree() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

// the static Hamiltonian of a parameter block: the first N diagonal entries (default 0) and N - 1 couplings (default 1), zeros beyond
void fill_h0(StaticH& h0, int N, const double* h0_diag, const double* h0_offdiag) {
    for (int i = 0; i < RC_MAX_NSPIN; ++i) {
        h0.diag[i] = (h0_diag && i < N) ? h0_diag[i] : 0.0;
        h0.off[i] = (i < N - 1) ? (h0_offdiag ? h0_offdiag[i] : 1.0) : 0.0;
    }
}

int check_common(int N, int in, int out, long long C, long long K) {
    if (N < 2 || N > RC_MAX_NSPIN) return fail(RC_EINVAL, "N must be in [2, 32]");
    if (in < 0 || in >= N || out < 0 || out >= N) return fail(RC_EINVAL, "in/out spin index out of range");
    if (C < 0 || K < 0) return fail(RC_EINVAL, "C and K must be non-negative");
    return RC_OK;
}

// caller holds the device's ring_mu.  Grow-only; stream-ordered (see RingBuf).
int ring_buf_reserve(RingBuf& rb, hipStream_t s, long long samples) {
    if (rb.cap >= samples && rb.mem) return RC_OK;
    if (rb.mem) RC_HIP_CHECK(hipFreeAsync(rb.mem, s));        // behind whatever on `s` still reads the old list
    rb.mem = nullptr;
    rb.cap = 0;
    const long long cap = samples + (samples >> 2);
    RC_HIP_CHECK(hipMallocAsync((void**)&rb.mem, 256 + (size_t)cap * sizeof(long long), s));
    RC_HIP_CHECK(hipMemsetAsync(rb.mem, 0, 256, s));           // both counters: ordered before the kernels that add to them
    rb.cap = cap;
    rb.turn = 0;
    return RC_OK;
}

// caller holds the device's ring_mu.  The stream's entry, created on first use; evicts the least recently used one beyond the cap.
RingBuf& ring_buf_for(DeviceCtx& ctx, hipStream_t s) {
    auto it = ctx.ring_bufs.find(s);
    if (it == ctx.ring_bufs.end()) {
        if (ctx.ring_bufs.size() >= kMaxRingBufs) {
            auto old = ctx.ring_bufs.begin();
            for (auto j = ctx.ring_bufs.begin(); j != ctx.ring_bufs.end(); ++j)
                if (j->second.last_use < old->second.last_use) old = j;
            if (old->second.mem) (void)hipFree(old->second.mem);
            ctx.ring_bufs.erase(old);
        }
        it = ctx.ring_bufs.emplace(s, RingBuf{}).first;
    }
    it->second.last_use = ++ctx.ring_clock;
    return it->second;
}

// Store rule of mc_fid_chain_kernel: launches of fewer than this many tiles write their fidelities with non-temporal stores.
// scripts/nt_store_sweep.py (N = 7, K = 10 000, rule forced on / off, interleaved; profiles/launch_boundary_ab.txt section 3),
// non-temporal / plain time per launch, end-to-end pair | general pair:
//     3 925 tiles 0.970 | 0.976      15 700 (the benchmark's launch) 0.987 | 0.991      62 800 tiles 0.997 | 0.996
//     157 000 .. 1 570 000 tiles 0.995 .. 1.0015, every one inside the two sides' own spread (0.2 .. 1.7 %)
// The gain belongs to the launch boundary and is gone where the boundary is: from 62 800 tiles on nothing is measurable, and an
// earlier trial read +1.6 % on a launch of 10^8 evaluations (NOTEBOOK.md 12 (i)).  The threshold sits between the last size with a
// measured gain and the first one without: 32 768 tiles = eight rounds of the chip's 4 096 wave slots.
constexpr long long kNtStoreTiles = 32768;
std::atomic<long long> g_nt_store_tiles{kNtStoreTiles};      // (tests move it: rc_debug_nt_store_tiles)

template <int N, int MODE>
int launch_chain(hipStream_t s, const FidParams& p0, long long nt_store_tiles) {
    const long long blocks = p0.ntiles;
    if (blocks > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
    FidParams p = p0;
    p.nt_store = (blocks < nt_store_tiles) ? 1 : 0;
    hipLaunchKernelGGL((mc_fid_chain_kernel<N, MODE>), dim3((unsigned)blocks), dim3(64), 0, s, p);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int enqueue_expm(hipStream_t s, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, int ring,
                 const double* ctrl, const double* draws, long long draw_cstride, const double* diag_imag,
                 long long imag_cstride, long long C, long long K, double* fid, bool fast_complex_diagonal = false) {
    if (N > RC_MAX_NSPIN_FAST) return fail(RC_EINVAL, "the dense kernels (ring topology, expm) support N <= 16");
    ExpmParams p{};
    p.ctrl = ctrl;
    p.draws = draws;
    p.diag_imag = diag_imag;
    p.fid = fid;
    p.C = C;
    p.K = K;
    p.draw_cstride = draw_cstride;
    p.imag_cstride = imag_cstride;
    p.N = N;
    p.in = in;
    p.out = out;
    p.ring = ring ? 1 : 0;
    fill_h0(p.h0, N, h0_diag, h0_offdiag);
    const size_t lds = (size_t)kExpmWaves * kExpmBufs * N * N * sizeof(cplx);
    if (int rc = ensure_func_attr(kAttrExpm, (const void*)mc_fid_expm_kernel,
                                  kExpmWaves * kExpmBufs * RC_MAX_NSPIN_FAST * RC_MAX_NSPIN_FAST * (int)sizeof(cplx)))
        return rc;
    const long long total = C * K;
    long long blocks = (total + kExpmWaves - 1) / kExpmWaves;
    if (blocks > 256LL * 16) blocks = 256LL * 16;              // grid-stride loop inside; every wave exits
    if (fast_complex_diagonal && !ring && N <= kCsymMaxN) {
        // chain with a complex diagonal: the lane-per-sample complex symmetric QL route, then the expm kernel over the
        // samples it marked (normally none: the waves of that pass find nothing and end)
        const long long cblocks = (total + 63) / 64;
        if (cblocks > 0x7fffffffLL) return fail(RC_EINVAL, "too many samples for one launch");
        switch (N) {
#define RC_CSYM_CASE(n) \
    case n: hipLaunchKernelGGL(mc_fid_csym_kernel<n>, dim3((unsigned)cblocks), dim3(64), 0, s, p); break;
            RC_CSYM_CASE(2) RC_CSYM_CASE(3) RC_CSYM_CASE(4) RC_CSYM_CASE(5) RC_CSYM_CASE(6) RC_CSYM_CASE(7) RC_CSYM_CASE(8)
            RC_CSYM_CASE(9) RC_CSYM_CASE(10) RC_CSYM_CASE(11) RC_CSYM_CASE(12)
#undef RC_CSYM_CASE
        }
        p.only_marked = 1;
    }
    hipLaunchKernelGGL(mc_fid_expm_kernel, dim3((unsigned)blocks), dim3(64 * kExpmWaves), lds, s, p);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

// FidParams::align16 and its like: the draws base and every controller's run of K * 3N doubles are 16-byte aligned
int draws_align16(const double* draws, long long draw_cstride) {
    return (((uintptr_t)draws & 15) == 0 && (((size_t)draw_cstride * 8) & 15) == 0) ? 1 : 0;
}
// bytes of a draw tensor whose controllers are `stride` doubles apart (0: one set shared by all)
size_t draws_bytes(long long C, long long K, int N, long long stride) {
    return (stride == 0 ? (size_t)K * N * 3 : ((size_t)(C - 1) * stride + (size_t)K * N * 3)) * sizeof(double);
}

int enqueue_fidelity(hipStream_t s, int kernel, int N, int in, int out, const double* h0_diag,
                     const double* h0_offdiag, int ring, const double* ctrl, const double* draws,
                     long long draw_cstride, long long C, long long K, double* fid) {
    if (draw_cstride < 0) draw_cstride = K * N * 3;          // default: private draws per controller
    if (draw_cstride != 0 && draw_cstride < K * N * 3) return fail(RC_EINVAL, "draws_ctrl_stride overlaps controllers");
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (C == 0 || K == 0) return RC_OK;
    if (!ctrl || !draws || !fid) return fail(RC_EINVAL, "NULL array pointer");
    const bool ends = (in == 0 && out == N - 1) || (in == N - 1 && out == 0);
    if (ring && N == 2) ring = 0;               // the closure of a 2-ring IS the chain bond (noise_model.py:83-85 re-assigns 1)
    // ring: AUTO = the mixed-precision route (round 3; N = 11 .. 16 since round 5: folded band reduction instead of the dense
    // Householder); RC_KERNEL_RING_HH asks for the all-fp64 route explicitly
    const bool mixed_ring = (kernel == RC_KERNEL_AUTO) && ring && N <= kRingMaxN;
    if (kernel == RC_KERNEL_AUTO)
        kernel = ring ? (N <= kRingMaxN ? RC_KERNEL_RING_HH : RC_KERNEL_JACOBI) : RC_KERNEL_TRIDIAG_ADJ;
    if (kernel == RC_KERNEL_RING_HH) {
        if (!ring) return fail(RC_EINVAL, "RC_KERNEL_RING_HH is the ring-topology kernel (chains: the tridiagonal kernels)");
        if (N > kRingMaxN) return fail(RC_EINVAL, "the lane-per-sample ring kernels support N <= 16");
        FidParams p{};
        p.ctrl = ctrl;
        p.draws = draws;
        p.fid = fid;
        p.C = C;
        p.K = K;
        p.draw_cstride = draw_cstride;
        p.tiles_per_ctrl = (K + 63) / 64;
        p.ntiles = C * p.tiles_per_ctrl;
        p.in = in;
        p.out = out;
        p.align16 = draws_align16(draws, draw_cstride);
        fill_h0(p.h0, N, h0_diag, h0_offdiag);
        if (p.ntiles > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
        const dim3 grid((unsigned)p.ntiles);
        if (mixed_ring) {
            // mixed-precision route + the repair launch right behind it on the same stream: the route lists the samples it
            // does not trust itself with, the repair kernel recomputes them lane per sample (a few hundred waves that end
            // at once when the list is empty).  List and counters: the stream's persistent RingBuf.
            RingRepairList rl{};
            {
                int dev = 0;
                RC_HIP_CHECK(hipGetDevice(&dev));
                if (dev < 0 || dev >= kMaxDevices) return fail(RC_EINVAL, "device index out of range");
                std::lock_guard<std::mutex> lk(g_ctx[dev].ring_mu);
                RingBuf& rb = ring_buf_for(g_ctx[dev], s);
                if (int rc = ring_buf_reserve(rb, s, C * K)) return rc;      // (first use of this stream, or a larger problem: rare)
                rl.count = (unsigned long long*)(rb.mem + 64 * rb.turn);
                rl.clear = (unsigned long long*)(rb.mem + 64 * (rb.turn ^ 1));
                rl.samples = (long long*)(rb.mem + 256);
                rb.turn ^= 1;
            }
            // the repair kernel walks the list with a grid-stride loop; its width only matters when MANY samples are listed
            // (a translation-invariant ring lists every sample).  RC_RING_REPAIR_GRID (environment, read once): A/B knob.
            static const long long kRepairGrid = [] {
                const char* e = getenv("RC_RING_REPAIR_GRID");
                const long long v = e ? atoll(e) : 0;
                return v > 0 ? v : 1024LL;
            }();
            const long long nwaves = (C * K + 63) / 64;
            const dim3 rgrid((unsigned)(nwaves < kRepairGrid ? nwaves : kRepairGrid));
            if (N > 10) {                              // 11 .. 16: instantiated in robchar_large.hip
                RC_HIP_CHECK((hipError_t)rc_large_ring_launch(N, 1, (void*)s, &p, 1.0, &rl, grid.x, rgrid.x));
                return RC_OK;
            }
            switch (N) {
#define RC_RING_CASE(n)                                                                         \
    case n:                                                                                     \
        hipLaunchKernelGGL(mc_fid_ring_mixed_kernel<n>, grid, dim3(64), 0, s, p, 1.0, rl);      \
        hipLaunchKernelGGL(mc_fid_ring_repair_kernel<n>, rgrid, dim3(64), 0, s, p, 1.0, rl);    \
        break;
                RC_RING_CASE(3) RC_RING_CASE(4) RC_RING_CASE(5) RC_RING_CASE(6) RC_RING_CASE(7) RC_RING_CASE(8) RC_RING_CASE(9)
                RC_RING_CASE(10)
#undef RC_RING_CASE
            }
            RC_HIP_CHECK(hipGetLastError());
            return RC_OK;
        }
        if (N > 10) {                                   // 11 .. 16: instantiated in robchar_large.hip
            RC_HIP_CHECK((hipError_t)rc_large_ring_launch(N, 0, (void*)s, &p, 1.0, nullptr, grid.x, 0u));
            return RC_OK;
        }
        switch (N) {
#define RC_RING_CASE(n) \
    case n: hipLaunchKernelGGL(mc_fid_ring_kernel<n>, grid, dim3(64), 0, s, p, 1.0); break;
            RC_RING_CASE(3) RC_RING_CASE(4) RC_RING_CASE(5) RC_RING_CASE(6) RC_RING_CASE(7) RC_RING_CASE(8) RC_RING_CASE(9)
            RC_RING_CASE(10)
#undef RC_RING_CASE
        }
        RC_HIP_CHECK(hipGetLastError());
        return RC_OK;
    }
    if (kernel == RC_KERNEL_TRIDIAG_QL || kernel == RC_KERNEL_TRIDIAG_ADJ) {
        // (N = 15, 16: the end-to-end instantiation needs more than 256 registers - one wave per SIMD - and is slower than the
        // general adjugate one, which covers the pair (0, N - 1) as well and fits two: 338 / 395 us against 310 / 342 us per 1e6)
        const int mode = (kernel == RC_KERNEL_TRIDIAG_QL) ? rc::kWeightsRows
                                                          : ((ends && N <= 14) ? rc::kWeightsEnds : rc::kWeightsAdjugate);
        if (ring) return fail(RC_EINVAL, "the tridiagonal QL kernel handles chain topology only");
        FidParams p{};
        p.ctrl = ctrl;
        p.draws = draws;
        p.fid = fid;
        p.C = C;
        p.K = K;
        p.draw_cstride = draw_cstride;
        p.tiles_per_ctrl = (K + 63) / 64;
        p.ntiles = C * p.tiles_per_ctrl;
        p.in = in;
        p.out = out;
        p.align16 = draws_align16(draws, draw_cstride);
        p.stamps = g_stamps;
        fill_h0(p.h0, N, h0_diag, h0_offdiag);
        // chains of 17 .. 24 spins (round 5): the register-resident general-adjugate instantiation (one wave per SIMD) for the
        // eigenvalue-only kernels; the rows mode keeps the LDS kernel there (its 4N more doubles of state do not fit)
        if (N > RC_MAX_NSPIN_CHAIN || (N > RC_MAX_NSPIN_FAST && mode == rc::kWeightsRows)) {
            const long long blocks = p.ntiles;
            if (blocks > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
            const size_t lds = (size_t)4 * N * 64 * sizeof(double);
            if (int rc = ensure_func_attr(kAttrAnyN, (const void*)mc_fid_chain_anyn_kernel, 4 * RC_MAX_NSPIN * 64 * (int)sizeof(double)))
                return rc;
            hipLaunchKernelGGL(mc_fid_chain_anyn_kernel, dim3((unsigned)blocks), dim3(64), lds, s, p, N);
            RC_HIP_CHECK(hipGetLastError());
            return RC_OK;
        }
        if (N > RC_MAX_NSPIN_FAST) {                   // 17 .. 24: instantiated in robchar_large.hip
            if (p.ntiles > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
            RC_HIP_CHECK((hipError_t)rc_large_chain_launch(N, (void*)s, &p));
            return RC_OK;
        }
        const long long nt_tiles = g_nt_store_tiles.load(std::memory_order_relaxed);
        switch (N) {
#define RC_CASE(n)                                                                        \
    case n:                                                                               \
        return mode == rc::kWeightsRows ? launch_chain<n, rc::kWeightsRows>(s, p, nt_tiles)         \
               : (mode == rc::kWeightsEnds ? launch_chain<n, rc::kWeightsEnds>(s, p, nt_tiles)      \
                                           : launch_chain<n, rc::kWeightsAdjugate>(s, p, nt_tiles));
/* N = 15, 16: no end-to-end instantiation (never dispatched: see above) */
#define RC_CASE_ADJ_ROWS(n)                                                               \
    case n:                                                                               \
        return mode == rc::kWeightsRows ? launch_chain<n, rc::kWeightsRows>(s, p, nt_tiles) : launch_chain<n, rc::kWeightsAdjugate>(s, p, nt_tiles);
#ifdef RC_DEV_FEW_N      /* kernel-tuning builds only (scripts/): the three BASELINE sizes, a third of the compile time */
            RC_CASE(5) RC_CASE(7) RC_CASE(10)
#else
            RC_CASE(2) RC_CASE(3) RC_CASE(4) RC_CASE(5) RC_CASE(6) RC_CASE(7) RC_CASE(8) RC_CASE(9)
            RC_CASE(10) RC_CASE(11) RC_CASE(12) RC_CASE(13) RC_CASE(14) RC_CASE_ADJ_ROWS(15) RC_CASE_ADJ_ROWS(16)
#endif
#undef RC_CASE
#undef RC_CASE_ADJ_ROWS
        }
        return fail(RC_EINVAL, "unsupported N");
    }
    if (N > RC_MAX_NSPIN_FAST) return fail(RC_EINVAL, "the dense kernels (ring topology, expm) support N <= 16");
    if (kernel == RC_KERNEL_EXPM)
        return enqueue_expm(s, N, in, out, h0_diag, h0_offdiag, ring, ctrl, draws, draw_cstride, nullptr, 0, C, K, fid);
    if (kernel == RC_KERNEL_JACOBI) {
        JacParams p{};
        p.ctrl = ctrl;
        p.draws = draws;
        p.fid = fid;
        p.C = C;
        p.K = K;
        p.draw_cstride = draw_cstride;
        p.N = N;
        p.in = in;
        p.out = out;
        p.ring = ring ? 1 : 0;
        fill_h0(p.h0, N, h0_diag, h0_offdiag);
        const long long total = C * K;
        const int spw = (N <= 8) ? 8 : 4;                       // samples per wave
        long long blocks = (total + kJacWaves * spw - 1) / (kJacWaves * spw);
        if (blocks > 256LL * 16) blocks = 256LL * 16;          // grid-stride loop inside; every wave exits
        if (N <= 8)
            hipLaunchKernelGGL((mc_fid_jacobi_kernel<8, 8>), dim3((unsigned)blocks), dim3(64 * kJacWaves), 0, s, p);
        else
            hipLaunchKernelGGL((mc_fid_jacobi_kernel<16, 16>), dim3((unsigned)blocks), dim3(64 * kJacWaves), 0, s, p);
        RC_HIP_CHECK(hipGetLastError());
        return RC_OK;
    }
    return fail(RC_EINVAL, "unknown kernel id");
}

int enqueue_reduce(hipStream_t s, const double* fid, long long C, long long K, const double* thr, int nq,
                   double eps, double* rim1, double* stdv, double* minf, double* q, double* sorted_out, bool standalone = false) {
    if (C < 0 || K < 0) return fail(RC_EINVAL, "C and K must be non-negative");
    if (nq < 0 || nq > kMaxQ) return fail(RC_EINVAL, "nq must be in [0, 8]");
    if (nq > 0 && !thr) return fail(RC_EINVAL, "q_thresholds is NULL");
    if (C == 0) return RC_OK;
    if (K == 0) return fail(RC_EINVAL, "K must be positive for a reduction");
    if (!fid) return fail(RC_EINVAL, "NULL fid pointer");
    if (C > 0x7fffffffLL) return fail(RC_EINVAL, "too many controllers for one launch");
    RedParams p{};
    p.fid = fid;
    p.C = C;
    p.K = K;
    p.nq = nq;
    for (int j = 0; j < nq; ++j) p.thr[j] = thr[j];
    p.eps = eps;
    p.rim1 = rim1;
    p.stdv = stdv;
    p.minf = minf;
    p.q = q;
    if (rim1 || stdv || minf || q) {
        if (K <= kWaveRowMaxK && C >= 64) {                   // many short rows: one wave per row
            const dim3 grid((unsigned)((C + 3) / 4));
            if (nq == 0)
                hipLaunchKernelGGL(reduce_rows_wave_kernel<0>, grid, dim3(256), 0, s, p);
            else if (nq <= 2)
                hipLaunchKernelGGL(reduce_rows_wave_kernel<2>, grid, dim3(256), 0, s, p);
            else
                hipLaunchKernelGGL(reduce_rows_wave_kernel<kMaxQ>, grid, dim3(256), 0, s, p);
        } else if (nq <= 2 && K > kWaveRowMaxK && K <= 32LL * 128) {      // rows of up to 4096 / 8192 values: narrower workgroups,
            if (nq == 0) hipLaunchKernelGGL((reduce_kernel<0, 128>), dim3((unsigned)C), dim3(128), 0, s, p);      // more rows in flight
            else hipLaunchKernelGGL((reduce_kernel<2, 128>), dim3((unsigned)C), dim3(128), 0, s, p);
        } else if (nq <= 2 && K > kWaveRowMaxK && K <= 32LL * 256) {
            if (nq == 0) hipLaunchKernelGGL((reduce_kernel<0, 256>), dim3((unsigned)C), dim3(256), 0, s, p);
            else hipLaunchKernelGGL((reduce_kernel<2, 256>), dim3((unsigned)C), dim3(256), 0, s, p);
        } else if (standalone && nq <= 2 && K > 32LL * 256 && K <= 40LL * 256) {
            // Rows of 8193 .. 10 240 values (BASELINE's K = 10 000) with NOTHING running beside the reduction (RC_REDUCE_STANDALONE:
            // the product's cold calls, the blocking and multi-device entries): 256 threads x 40 cached values - five rows in flight
            // per CU instead of two: 11 000 rows 440 -> 208 us, 1 000 rows 46 -> 29.5 us (profiles/r04_reduce_sweep.txt).  A caller
            // that OVERLAPS the reduction with fidelity launches (bench.py's side stream in steady state) keeps the 512-thread
            // version below: latency-bound, it fills issue slots the fidelity kernel leaves idle, where this one displaces its
            // waves (steady-state step +1.5 %, round 4).  The hint picks the route, and with it the summation order of these rows.
            if (nq == 0) hipLaunchKernelGGL((reduce_kernel<0, 256, 40>), dim3((unsigned)C), dim3(256), 0, s, p);
            else hipLaunchKernelGGL((reduce_kernel<2, 256, 40>), dim3((unsigned)C), dim3(256), 0, s, p);
        } else if (nq == 0)
            hipLaunchKernelGGL(reduce_kernel<0>, dim3((unsigned)C), dim3(kRedThreads), 0, s, p);
        else if (nq <= 2)
            hipLaunchKernelGGL(reduce_kernel<2>, dim3((unsigned)C), dim3(kRedThreads), 0, s, p);
        else
            hipLaunchKernelGGL(reduce_kernel<kMaxQ>, dim3((unsigned)C), dim3(kRedThreads), 0, s, p);
        RC_HIP_CHECK(hipGetLastError());
    }
    if (sorted_out) {
        long long P = 2;
        while (P < K) P <<= 1;
        if (C * P > (1LL << 34)) return fail(RC_EINVAL, "sorted_out: workspace would exceed 128 GiB");
        if (K <= kSortChunk) {                                        // one fused launch, no workspace: merge sort
            if (int rc = ensure_func_attr(kAttrSortMerge, (const void*)sort_rows_merge_kernel, (kSortChunk / 16 * 17 + 1) * 8))
                return rc;
            const int T = (int)((K + 15) / 16), n = 16 * T;
            const int threads = ((T + 63) / 64) * 64;
            hipLaunchKernelGGL(sort_rows_merge_kernel, dim3((unsigned)C), dim3(threads), (size_t)(n / 16 * 17 + 1) * sizeof(double),
                               s, fid, sorted_out, K, n);
            RC_HIP_CHECK(hipGetLastError());
            return RC_OK;
        }
        // workspace of THIS call, allocated and released in stream order (two streams sorting long rows at the same time
        // each get their own; nothing is shared between calls)
        struct SortWs {
            double* work = nullptr;
            int* flags = nullptr;
        } wsv, *ws = &wsv;
        RC_HIP_CHECK(hipMallocAsync((void**)&wsv.work, (size_t)C * P * sizeof(double), s));
        if (hipError_t e = hipMallocAsync((void**)&wsv.flags, (size_t)C * sizeof(int), s); e != hipSuccess) {
            (void)hipFreeAsync(wsv.work, s);
            return fail(RC_EHIP, std::string("hipMallocAsync(sort flags): ") + hipGetErrorString(e));
        }
        struct Release {
            SortWs* w;
            hipStream_t st;
            ~Release() {
                (void)hipFreeAsync(w->work, st);
                (void)hipFreeAsync(w->flags, st);
            }
        } release{ws, s};
        RC_HIP_CHECK(hipMemsetAsync(ws->flags, 0, (size_t)C * sizeof(int), s));
        {
            // long rows (K > 16384): chunk sort -> for each larger size one fused pass over the strides >= 16384 (up to four per
            // launch) and one chunk pass over the rest; the first pass reads `fid`, the last writes `sorted_out`
            if (int rc = ensure_func_attr(kAttrSortChunk, (const void*)sort_chunk16_kernel, kSortChunk / 16 * 17 * 8)) return rc;
            const size_t lds16 = (size_t)(kSortChunk / 16 * 17) * sizeof(double);
            const dim3 cgrid((unsigned)C, (unsigned)(P / kSortChunk));
            hipLaunchKernelGGL(sort_chunk16_kernel, cgrid, dim3(kSortThreads), lds16, s, fid, ws->work, sorted_out, ws->flags,
                               K, P, 2LL, (long long)kSortChunk, 1, 0);
            for (long long size = 2LL * kSortChunk; size <= P; size <<= 1) {
                long long hi = size >> 1;
                while (hi >= kSortChunk) {
                    int nleft = 0;
                    for (long long x = hi; x >= kSortChunk; x >>= 1) ++nleft;
                    const int take = nleft >= 4 ? 4 : nleft;
                    const long long S = hi >> (take - 1);
                    const dim3 ggrid((unsigned)C, 128);
                    switch (take) {
                        case 4: hipLaunchKernelGGL(sort_global_fused_kernel<4>, ggrid, dim3(256), 0, s, ws->work, P, size, S); break;
                        case 3: hipLaunchKernelGGL(sort_global_fused_kernel<3>, ggrid, dim3(256), 0, s, ws->work, P, size, S); break;
                        case 2: hipLaunchKernelGGL(sort_global_fused_kernel<2>, ggrid, dim3(256), 0, s, ws->work, P, size, S); break;
                        default: hipLaunchKernelGGL(sort_global_fused_kernel<1>, ggrid, dim3(256), 0, s, ws->work, P, size, S); break;
                    }
                    hi = S >> 1;
                }
                hipLaunchKernelGGL(sort_chunk16_kernel, cgrid, dim3(kSortThreads), lds16, s, fid, ws->work, sorted_out,
                                   ws->flags, K, P, size, size, 0, size == P ? 1 : 0);
            }
            RC_HIP_CHECK(hipGetLastError());
            return RC_OK;
        }
        RC_HIP_CHECK(hipGetLastError());
    }
    return RC_OK;
}

// ------------------------------------------------------------------------------------------------
// single-process multi-device driver (rc_mc_fidelity_sharded_f64 / rc_mc_metrics_sharded_f64)
// ------------------------------------------------------------------------------------------------
// The (controller x perturbation) sample space is split by CONTROLLER into contiguous balanced blocks, one per device
// (per-controller vectors and reductions stay device-local; the reference's only parallel construct is
// the dead Pool at mcsim.py:451-455).  One host thread per device: its controllers are processed in chunks of at
// most kShardChunkBytes of draws through the device's workspace - H2D of the chunk's draws (or Philox generation on the
// device), fidelity kernel, reduction, D2H of fidelities / metric rows straight into the caller's host arrays.  No
// collective is needed for a host-resident result.
constexpr size_t kShardChunkBytes = (size_t)4 << 30;

// What one device's share of the sample space is computed from, common to the sharded entries and the RCCL entry: the call's
// arguments, filled once per call, and - per share - `device`, its controllers [c0, c1) and the worker's result.
struct ShareSpec {
    int device, kernel, N, in, out, ring;
    const double *h0d, *h0o, *ctrl, *draws;          // host; draws may be null (Philox)
    unsigned long long seed, offset;
    double sigma;
    long long C, K, c0, c1;
    const double* thr;
    int nq;
    double eps;
    int rc = RC_OK;
    std::string err;
};

// Counter-based draws on a chain of <= 16 spins with the eigenvalue-only kernels: generated inside the fidelity kernel
// (k_fidelity_philox.inc.h) - no draw tensor.  ONE predicate for this route and the Python layer's: rc_philox_fused_pays
// (environment switch read per call); who sizes the buffers asks once and hands enqueue_share no draw buffer when it holds.
bool philox_fused_route(const double* draws, int ring, int kernel, int N, int in, int out) {
    return !draws && !ring && rc_philox_fused_pays(N, in, out) == 1 && (kernel == RC_KERNEL_AUTO || kernel == RC_KERNEL_TRIDIAG_ADJ);
}

// Controllers [a, a + cc) of `sp` on its device: their rows into `d_ctrl`, their fidelities into rows [0, cc) of `d_fid` - from
// the host's draws or the Philox stream through `d_draw`, or (`d_draw` NULL: philox_fused_route) by the fused Philox kernel.
// Enqueued on `st`; nothing waits.
int enqueue_share(const ShareSpec& sp, long long a, long long cc, double* d_ctrl, double* d_draw, double* d_fid, hipStream_t st) {
    const long long G = 3LL * sp.N, K = sp.K;
    RC_HIP_CHECK(hipMemcpyAsync(d_ctrl, sp.ctrl + a * (sp.N + 1), (size_t)cc * (sp.N + 1) * sizeof(double), hipMemcpyHostToDevice, st));
    // element ((c K + k) N + i) 3 + slot of the stream: independent of how the controllers are sharded
    const unsigned long long first = sp.offset + (unsigned long long)(a * K * G);
    if (!d_draw)
        return rc_mc_fidelity_philox_f64_async(sp.device, st, sp.kernel, sp.N, sp.in, sp.out, sp.h0d, sp.h0o, d_ctrl, sp.seed, first,
                                               sp.sigma, nullptr, cc, K, d_fid);
    if (sp.draws) {
        RC_HIP_CHECK(hipMemcpyAsync(d_draw, sp.draws + a * K * G, (size_t)cc * K * G * sizeof(double), hipMemcpyHostToDevice, st));
    } else if (int rc = rc_draws_philox_f64_async(sp.device, st, sp.seed, first, cc * K * G, sp.sigma, d_draw)) {
        return rc;
    }
    return enqueue_fidelity(st, sp.kernel, sp.N, sp.in, sp.out, sp.h0d, sp.h0o, sp.ring, d_ctrl, d_draw, -1, cc, K, d_fid);
}

struct ShardJob : ShareSpec {
    double *rim1, *stdv, *minf, *q, *fid_out;        // host, FULL arrays ([3][C], [3][nq][C], [C][K]); may be null
};

int run_shard_locked(ShardJob* j) {
    Staging ws;
    if (int rc = get_ctx(j->device, &ws.ctx)) return rc;
    const long long G = 3LL * j->N, K = j->K, Cl = j->c1 - j->c0;
    if (Cl <= 0 || K == 0) return RC_OK;
    const bool want_red = j->rim1 || j->stdv || j->minf || (j->q && j->nq);
    // a chunk is bounded by its draws; on the fused route by its fidelities only (K x 8 bytes per controller)
    const bool fused = philox_fused_route(j->draws, j->ring, j->kernel, j->N, j->in, j->out);
    long long cc_max = (long long)(kShardChunkBytes / ((size_t)K * (fused ? 1 : G) * sizeof(double)));
    if (cc_max < 1) cc_max = 1;
    if (cc_max > Cl) cc_max = Cl;
    // planned once for cc_max controllers, reused by every chunk
    const size_t nb_c3 = (size_t)3 * cc_max * sizeof(double);
    const int s_ctrl = ws.plan.scratch((size_t)cc_max * (j->N + 1) * sizeof(double)),
              s_draw = ws.plan.scratch(fused ? 0 : (size_t)cc_max * K * G * sizeof(double)),
              s_fid = ws.plan.scratch((size_t)cc_max * K * sizeof(double)), s_rim = ws.plan.scratch(nb_c3),
              s_std = ws.plan.scratch(nb_c3), s_min = ws.plan.scratch(nb_c3),
              s_q = ws.plan.scratch(nb_c3 * (j->nq > 0 ? j->nq : 1));
    if (int rc = ws.stage_in()) return rc;
    double *d_ctrl = ws.ptr(s_ctrl), *d_draw = fused ? nullptr : ws.ptr(s_draw), *d_fid = ws.ptr(s_fid), *d_rim = ws.ptr(s_rim),
           *d_std = ws.ptr(s_std), *d_min = ws.ptr(s_min), *d_q = ws.ptr(s_q);
    hipStream_t st = ws.ctx->stream;
    for (long long a = j->c0; a < j->c1; a += cc_max) {
        const long long cc = (j->c1 - a < cc_max) ? (j->c1 - a) : cc_max;
        if (int rc = enqueue_share(*j, a, cc, d_ctrl, d_draw, d_fid, st)) return rc;
        if (want_red) {
            if (int rc = enqueue_reduce(st, d_fid, cc, K, j->thr, j->nq, j->eps, j->rim1 ? d_rim : nullptr,
                                        j->stdv ? d_std : nullptr, j->minf ? d_min : nullptr,
                                        (j->q && j->nq) ? d_q : nullptr, nullptr, /*standalone=*/true))
                return rc;
            // device rows [3][cc] -> columns [a, a+cc) of the caller's [3][C]
            const size_t wbytes = (size_t)cc * sizeof(double), dpitch = (size_t)j->C * sizeof(double);
            if (j->rim1) RC_HIP_CHECK(hipMemcpy2DAsync(j->rim1 + a, dpitch, d_rim, wbytes, wbytes, 3, hipMemcpyDeviceToHost, st));
            if (j->stdv) RC_HIP_CHECK(hipMemcpy2DAsync(j->stdv + a, dpitch, d_std, wbytes, wbytes, 3, hipMemcpyDeviceToHost, st));
            if (j->minf) RC_HIP_CHECK(hipMemcpy2DAsync(j->minf + a, dpitch, d_min, wbytes, wbytes, 3, hipMemcpyDeviceToHost, st));
            if (j->q && j->nq)
                RC_HIP_CHECK(hipMemcpy2DAsync(j->q + a, dpitch, d_q, wbytes, wbytes, (size_t)3 * j->nq, hipMemcpyDeviceToHost, st));
        }
        if (j->fid_out)
            RC_HIP_CHECK(hipMemcpyAsync(j->fid_out + a * K, d_fid, (size_t)cc * K * sizeof(double), hipMemcpyDeviceToHost, st));
        RC_HIP_CHECK(hipStreamSynchronize(st));       // the workspace is reused by the next chunk
    }
    return RC_OK;
}

void run_shard(ShardJob* j) {
    std::lock_guard<std::mutex> lk(g_ctx[j->device].mu);
    j->rc = run_shard_locked(j);
    if (j->rc) j->err = g_last_error;            // thread-local of THIS worker: hand it to the caller
}

int run_sharded(int ndev, const int* devices, ShardJob proto) {
    if (int rc = check_common(proto.N, proto.in, proto.out, proto.C, proto.K)) return rc;
    if (ndev < 1 || ndev > kMaxDevices) return fail(RC_EINVAL, "ndev must be in [1, 64]");
    if (proto.nq < 0 || proto.nq > kMaxQ) return fail(RC_EINVAL, "nq must be in [0, 8]");
    if (proto.nq > 0 && !proto.thr) return fail(RC_EINVAL, "q_thresholds is NULL");
    if (proto.C == 0 || proto.K == 0) return RC_OK;
    if (!proto.ctrl) return fail(RC_EINVAL, "NULL controllers pointer");
    if (!proto.fid_out && !proto.rim1 && !proto.stdv && !proto.minf && !(proto.q && proto.nq))
        return fail(RC_EINVAL, "no output requested");
    for (int r = 0; r < ndev; ++r) {
        const int dev = devices ? devices[r] : r;
        if (int rc = device_in_range(dev)) return rc;
        // a device listed twice would only serialise on its lock; refused because it is never what a caller wants -
        // except for rehearsing the multi-block assembly on a one-GPU box (RC_ALLOW_DUPLICATE_DEVICES=1, tests only)
        const char* dup = getenv("RC_ALLOW_DUPLICATE_DEVICES");
        for (int r2 = 0; r2 < r && !(dup && dup[0] == '1'); ++r2)
            if ((devices ? devices[r2] : r2) == dev) return fail(RC_EINVAL, "a device is listed twice");
    }
    std::vector<ShardJob> jobs(ndev, proto);
    const long long base = proto.C / ndev, extra = proto.C % ndev;
    long long start = 0;
    for (int r = 0; r < ndev; ++r) {
        jobs[r].device = devices ? devices[r] : r;
        jobs[r].c0 = start;
        start += base + (r < extra ? 1 : 0);
        jobs[r].c1 = start;
    }
    std::vector<std::thread> th;
    for (int r = 1; r < ndev; ++r) th.emplace_back(run_shard, &jobs[r]);
    run_shard(&jobs[0]);
    for (auto& t : th) t.join();
    for (int r = 0; r < ndev; ++r)
        if (jobs[r].rc) return fail(jobs[r].rc, "device " + std::to_string(jobs[r].device) + ": " + jobs[r].err);
    return RC_OK;
}

// ------------------------------------------------------------------------------------------------
// driver of the device-side legacy stream (rc_draws_legacy_f64)
// ------------------------------------------------------------------------------------------------
// The stream is produced in SEGMENTS of at most kLegacySegWords raw words: block-aligned word range [g0, g1) of the
// generator's output sequence, the first block being known (the caller's key / the previous segment's last block).
// After every segment the accepted-attempt count comes back to the host, which decides whether more words are needed.
constexpr long long kLegacySegWords = 1LL << 27;      // 512 MiB of raw words per segment

// `words` (a multiple of 624, >= 1248) raw MT19937 state words into `raw` (device): raw[0 .. 624) = the block `carry`
// (host), the rest is the generator's output sequence behind it - P parallel sub-streams of kMtJumpWords words whose
// start windows come from jump-ahead (k_draws.inc.h).  Enqueued on `st`; `carry` must stay valid until the copy ran.
int mt_fill_raw(hipStream_t st, const unsigned int* carry, long long words, unsigned int* raw) {
    const int P = (int)((words - rcl::kMtN + kMtJumpWords - 1) / kMtJumpWords);
    unsigned int* d_seeds = nullptr;
    RC_HIP_CHECK(hipMallocAsync((void**)&d_seeds, (size_t)P * rcl::kMtN * sizeof(unsigned int), st));
    StreamFree free_seeds{d_seeds, st};
    RC_HIP_CHECK(hipMemcpyAsync(d_seeds, carry, rcl::kMtN * sizeof(unsigned int), hipMemcpyHostToDevice, st));
    if (P > 1) {
        if (int rc = ensure_func_attr(kAttrMtJump, (const void*)mt19937_jump_step_kernel<24>, kJumpLdsWords * (int)sizeof(unsigned int)))
            return rc;
        if (int rc = ensure_func_attr(kAttrMtJumpWide, (const void*)mt19937_jump_step_kernel<12>, kJumpLdsWords * (int)sizeof(unsigned int)))
            return rc;
        // windows 1..3 by jumps of B, then up to 4 at a time by 4 B, up to 16 at a time by 16 B, up to 64 at a time by 64 B
        int have = 1;
        for (int stride = 1; stride <= kJumpMaxStride && have < P; stride *= 4) {
            const int limit = (stride == kJumpMaxStride) ? P : (P < 4 * stride ? P : 4 * stride);
            while (have < limit) {
                const int cnt = (limit - have < stride) ? (limit - have) : stride;
                if (cnt <= 10)                            // few jumps: all workgroups resident at once either way - 24 per jump,
                    hipLaunchKernelGGL((mt19937_jump_step_kernel<24>), dim3(24, cnt), dim3(kJumpThreads),      // 26 words each
                                       kJumpLdsWords * sizeof(unsigned int), st, d_seeds, have, stride);
                else                                      // many: 12 per jump, 52 words each (the regeneration is per workgroup)
                    hipLaunchKernelGGL((mt19937_jump_step_kernel<12>), dim3(12, cnt), dim3(kJumpThreads),
                                       kJumpLdsWords * sizeof(unsigned int), st, d_seeds, have, stride);
                have += cnt;
            }
        }
    }
    hipLaunchKernelGGL(mt19937_raw_kernel, dim3((unsigned)P), dim3(64), 0, st, (const unsigned int*)d_seeds, raw, words);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int legacy_normal_stream(hipStream_t st, rc_mt19937_state* state, long long n_periods, long long period, long long skip,
                         const double* scales_host, double* out_dev) {
    const long long n_total = n_periods * period;
    const long long e_shift = state->has_gauss ? 1 : 0;
    const long long n_need = n_total - e_shift;
    const long long pairs = (n_need + 1) / 2;
    double* d_scales = nullptr;
    RC_HIP_CHECK(hipMallocAsync((void**)&d_scales, (size_t)n_periods * sizeof(double), st));
    StreamFree free_scales{d_scales, st};
    RC_HIP_CHECK(hipMemcpyAsync(d_scales, scales_host, (size_t)n_periods * sizeof(double), hipMemcpyHostToDevice, st));
    if (e_shift) {                                    // element 0 of the stream is the host's cached normal
        long long pi;
        const long long slot = rcl::stream_slot(0, period, skip, &pi);
        if (slot >= 0) {
            const double v = 0.0 + scales_host[pi] * state->gauss;
            RC_HIP_CHECK(hipMemcpyAsync(out_dev + slot, &v, sizeof(double), hipMemcpyHostToDevice, st));
            RC_HIP_CHECK(hipStreamSynchronize(st));   // `v` is a stack temporary
        }
        state->has_gauss = 0;
        state->gauss = 0.0;
    }
    if (pairs == 0) return RC_OK;

    long long* d_last = nullptr;
    RC_HIP_CHECK(hipMallocAsync((void**)&d_last, 5 * sizeof(long long), st));
    StreamFree free_last{d_last, st};
    RC_HIP_CHECK(hipMemsetAsync(d_last, 0xff, 5 * sizeof(long long), st));

    // global word coordinates: word 0 = key[0] of the caller's state; the next unread word is `pos`
    std::vector<unsigned int> carry(state->key, state->key + rcl::kMtN);   // block at g0
    long long g0 = 0;                                 // first global word of the current segment (multiple of 624)
    const long long w0 = state->pos;                  // first word of attempt 0
    long long t_next = 0, rank = 0;                   // attempts processed so far, accepted among them
    long long last[5] = {-1, 0, 0, 0, 0};
    unsigned int* raw = nullptr;
    long long raw_words = 0;
    StreamFree free_raw{nullptr, st};
    while (rank < pairs) {
        // attempts still expected (acceptance pi/4, eight-sigma margin), capped by the segment size
        const long long missing = pairs - rank;
        long long t_want = (long long)((double)missing / 0.78539816339744831 + 12.0 * sqrt((double)missing)) + 64;
        const long long first_word = w0 + 4 * t_next;                // global index; lies in the block at g0 or the one after
        long long words = (first_word - g0) + 4 * t_want;
        if (words > kLegacySegWords) words = kLegacySegWords;
        words = ((words + rcl::kMtN - 1) / rcl::kMtN) * rcl::kMtN;
        if (words < 2 * rcl::kMtN) words = 2 * rcl::kMtN;
        const long long t_count = (g0 + words - first_word) / 4;     // attempts wholly inside [g0, g0 + words)
        const long long cap = words;
        if (raw_words < cap) {
            if (raw) (void)hipFreeAsync(raw, st);
            raw = nullptr;
            free_raw.p = nullptr;
            RC_HIP_CHECK(hipMallocAsync((void**)&raw, (size_t)cap * sizeof(unsigned int), st));
            free_raw.p = raw;
            raw_words = cap;
        }
        if (int rc = mt_fill_raw(st, carry.data(), words, raw)) return rc;
        const long long nwg = (t_count + kLgAttempts - 1) / kLgAttempts;
        unsigned long long* d_counts = nullptr;
        RC_HIP_CHECK(hipMallocAsync((void**)&d_counts, (size_t)(nwg + 1) * sizeof(unsigned long long), st));
        StreamFree free_counts{d_counts, st};
        LegacyParams p{};
        p.raw = raw;
        p.w_first = first_word - g0;
        p.t_first = t_next;
        p.t_count = t_count;
        p.rank_base = rank;
        p.pairs_needed = pairs;
        p.e_shift = e_shift;
        p.n_total = n_total;
        p.period = period;
        p.skip = skip;
        p.scales = d_scales;
        p.out = out_dev;
        p.wg_counts = d_counts;
        p.last = d_last;
        hipLaunchKernelGGL(legacy_count_kernel, dim3((unsigned)nwg), dim3(kLgThreads), 0, st, p);
        hipLaunchKernelGGL(legacy_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, nwg);
        hipLaunchKernelGGL(legacy_emit_kernel, dim3((unsigned)nwg), dim3(kLgThreads), 0, st, p);
        RC_HIP_CHECK(hipGetLastError());
        unsigned long long accepted = 0;
        RC_HIP_CHECK(hipMemcpyAsync(&accepted, d_counts + nwg, sizeof(accepted), hipMemcpyDeviceToHost, st));
        RC_HIP_CHECK(hipMemcpyAsync(last, d_last, sizeof(last), hipMemcpyDeviceToHost, st));
        // the segment's last block is the next segment's first (an attempt may straddle the boundary)
        RC_HIP_CHECK(hipMemcpyAsync(carry.data(), raw + words - rcl::kMtN, rcl::kMtN * sizeof(unsigned int),
                                    hipMemcpyDeviceToHost, st));
        RC_HIP_CHECK(hipStreamSynchronize(st));
        rank += (long long)accepted;
        if (rank >= pairs) {
            // the generator stands right after the last needed attempt: global word wf
            const long long wf = w0 + 4 * (last[0] + 1);
            long long blk = wf / rcl::kMtN, pos = wf % rcl::kMtN;
            if (pos == 0) {                           // NumPy's representation of a block boundary: pos = 624 of the block before
                blk -= 1;
                pos = rcl::kMtN;
            }
            if (blk * rcl::kMtN < g0 || (blk + 1) * rcl::kMtN > g0 + words) return fail(RC_EHIP, "legacy stream: final block outside the segment");
            RC_HIP_CHECK(hipMemcpy(state->key, raw + (blk * rcl::kMtN - g0), rcl::kMtN * sizeof(unsigned int), hipMemcpyDeviceToHost));
            state->pos = (int)pos;
            if (n_need & 1) {
                // odd count: the second normal of the last attempt stays cached - computed HERE with the host's libm,
                // exactly as NumPy computes it (legacy-distributions.c: f = sqrt(-2 log(r2) / r2); gauss = f * x1)
                double x1, x2, r2;
                rcl::polar_attempt((unsigned)last[1], (unsigned)last[2], (unsigned)last[3], (unsigned)last[4], x1, x2, r2);
                const double f = sqrt(-2.0 * log(r2) / r2);
                state->gauss = f * x1;
                state->has_gauss = 1;
            }
            break;
        }
        t_next += t_count;
        g0 += words - rcl::kMtN;
    }
    return RC_OK;
}

// ------------------------------------------------------------------------------------------------
// driver of the device-side directional draws (rc_directional_draws_legacy_dev; kernels + scheme: k_draws.inc.h)
// ------------------------------------------------------------------------------------------------
constexpr long long kDirChunkSamples = 1LL << 23;     // samples per pass (5.7e7 raw words = 228 MB, 57 MB of lengths)

int directional_chunk(hipStream_t st, rc_mt19937_state* state, long long n, unsigned int rng, unsigned int mask, double sigma,
                      int* idx_dev, double* ab_dev) {
    // words per sample: (mask + 1) / (rng + 1) for the index + 4 / (pi / 4) for the accepted attempt; ten-sigma margin
    const double per = (rng ? (double)(mask + 1.0) / (double)(rng + 1.0) : 0.0) + 4.0 / 0.78539816339744831;
    double grow = 1.0;
    const long long ngroups = (n + kDirGroup - 1) / kDirGroup;
    std::vector<long long> starts((size_t)ngroups);
    for (int attempt = 0; attempt < 6; ++attempt, grow *= 1.5) {
        long long words = state->pos + (long long)(grow * ((double)n * per + 40.0 * sqrt((double)n) + 4096.0));
        words = ((words + rcl::kMtN - 1) / rcl::kMtN + 1) * rcl::kMtN;
        if (words < 2 * rcl::kMtN) words = 2 * rcl::kMtN;
        unsigned int* raw = nullptr;
        RC_HIP_CHECK(hipMallocAsync((void**)&raw, (size_t)words * sizeof(unsigned int), st));
        StreamFree free_raw{raw, st};
        if (int rc = mt_fill_raw(st, state->key, words, raw)) return rc;
        const long long first = state->pos;           // the first unread word (raw[0 .. 624) is the caller's block)
        const long long npos = words - first;
        unsigned char* d_len = nullptr;
        RC_HIP_CHECK(hipMallocAsync((void**)&d_len, (size_t)npos, st));
        StreamFree free_len{d_len, st};
        const dim3 pgrid((unsigned)((npos + 255) / 256));
        hipLaunchKernelGGL(dir_len_kernel, pgrid, dim3(256), 0, st, (const unsigned int*)raw, first, words, rng, mask, d_len);
        RC_HIP_CHECK(hipGetLastError());
        const int shift = state->has_gauss ? 1 : 0;
        if (shift) {                                  // a_0 = the cached normal the generator entered with
            const double a0 = 0.0 + sigma * state->gauss;
            RC_HIP_CHECK(hipMemcpyAsync(ab_dev, &a0, sizeof(double), hipMemcpyHostToDevice, st));
            RC_HIP_CHECK(hipStreamSynchronize(st));   // `a0` is a stack temporary
        }
        // ---- the walk over the sample chain ON THE DEVICE (k_draws.inc.h: dir_blk_kernel ...): nothing crosses PCIe but
        // the final state record.  RC_DIR_WALK (environment, read per call; A/B and test knob): "host" = the host walk below
        // only, "fallback" = the device pass runs and is then treated as failed (exercises the hand-over to the host walk).
        const char* walk_env = getenv("RC_DIR_WALK");
        const bool kHostWalk = walk_env && strcmp(walk_env, "host") == 0;
        const bool kForceFallback = walk_env && strcmp(walk_env, "fallback") == 0;
        const long long nblk = (npos + kDwB - 1) / kDwB;
        const int S = (nblk <= 64LL * kDwMaxSup) ? 64 : kDwS;          // blocks per superblock
        const long long nsup = (nblk + S - 1) / S;
        if (!kHostWalk && nsup <= kDwMaxSup) {
            // one allocation: blk_exit [nblk][E] u8 | blk_cnt [nblk][E] u16 | sup_exit [nsup][E] u8 | sup_cnt [nsup][E] u32 |
            // sup_base [nsup] i64 | blk_base [nblk] i64 | sup_entry [nsup] u8 | blk_entry [nblk] u8 | result record
            auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
            const size_t o_bexit = 0, o_bcnt = o_bexit + up((size_t)nblk * kDwE), o_sexit = o_bcnt + up((size_t)nblk * kDwE * 2),
                         o_scnt = o_sexit + up((size_t)nsup * kDwE), o_sbase = o_scnt + up((size_t)nsup * kDwE * 4),
                         o_bbase = o_sbase + up((size_t)nsup * 8), o_sentry = o_bbase + up((size_t)nblk * 8),
                         o_bentry = o_sentry + up((size_t)nsup), o_res = o_bentry + up((size_t)nblk),
                         total = o_res + up(sizeof(DirWalkResult));
            unsigned char* ws = nullptr;
            RC_HIP_CHECK(hipMallocAsync((void**)&ws, total, st));
            StreamFree free_ws{ws, st};
            DirWalkResult* d_res = (DirWalkResult*)(ws + o_res);
            RC_HIP_CHECK(hipMemsetAsync(d_res, 0xff, sizeof(DirWalkResult), st));        // wf = -1: "not reached"
            hipLaunchKernelGGL(dir_blk_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (const unsigned char*)d_len, npos,
                               ws + o_bexit, (unsigned short*)(ws + o_bcnt));
            hipLaunchKernelGGL(dir_sup_kernel, dim3((unsigned)nsup), dim3(64), 0, st, (const unsigned char*)(ws + o_bexit),
                               (const unsigned short*)(ws + o_bcnt), nblk, S, ws + o_sexit, (unsigned int*)(ws + o_scnt));
            hipLaunchKernelGGL(dir_top_kernel, dim3(1), dim3(64), 0, st, (const unsigned char*)(ws + o_sexit),
                               (const unsigned int*)(ws + o_scnt), (int)nsup, n, ws + o_sentry, (long long*)(ws + o_sbase));
            hipLaunchKernelGGL(dir_desc_kernel, dim3((unsigned)nsup), dim3(64), 0, st, (const unsigned char*)(ws + o_bexit),
                               (const unsigned short*)(ws + o_bcnt), nblk, S, n, (const unsigned char*)(ws + o_sentry),
                               (const long long*)(ws + o_sbase), ws + o_bentry, (long long*)(ws + o_bbase));
            DirEmitBlkParams bp{};
            bp.raw = raw;
            bp.len = d_len;
            bp.blk_entry = ws + o_bentry;
            bp.blk_base = (const long long*)(ws + o_bbase);
            bp.first = first;
            bp.npos = npos;
            bp.n = n;
            bp.rng = rng;
            bp.mask = mask;
            bp.shift = shift;
            bp.sigma = sigma;
            bp.idx = idx_dev;
            bp.ab = ab_dev;
            bp.res = d_res;
            hipLaunchKernelGGL(dir_emit_blk_kernel, dim3((unsigned)nblk), dim3(256), 0, st, bp);
            hipLaunchKernelGGL(dir_final_kernel, dim3(1), dim3(256), 0, st, (const unsigned int*)raw, first, words, d_res);
            RC_HIP_CHECK(hipGetLastError());
            static thread_local DirWalkResult* h_res = nullptr;       // pinned, one per host thread (never freed: see `pin` below)
            if (!h_res) RC_HIP_CHECK(hipHostMalloc((void**)&h_res, sizeof(DirWalkResult), hipHostMallocPortable));
            RC_HIP_CHECK(hipMemcpyAsync(h_res, d_res, sizeof(DirWalkResult), hipMemcpyDeviceToHost, st));
            RC_HIP_CHECK(hipStreamSynchronize(st));
            if (h_res->ok == 1 && !kForceFallback) {
                memcpy(state->key, h_res->key, rcl::kMtN * sizeof(unsigned int));
                state->pos = h_res->pos;
                if (shift) {
                    // the second normal of the last sample's attempt stays cached - computed with the host's libm, as NumPy does
                    double x1, x2, r2;
                    rcl::polar_attempt(h_res->last_words[0], h_res->last_words[1], h_res->last_words[2], h_res->last_words[3],
                                       x1, x2, r2);
                    const double f = sqrt(-2.0 * log(r2) / r2);
                    state->gauss = f * x1;
                    state->has_gauss = 1;
                }
                return RC_OK;
            }
            // not reached: the buffer was too short (next attempt: larger), or a sample longer than the walk follows across a
            // block boundary - the host walk below decides which; whatever the device pass wrote is overwritten
        }
        unsigned short* d_lenk = nullptr;
        RC_HIP_CHECK(hipMallocAsync((void**)&d_lenk, (size_t)npos * sizeof(unsigned short), st));
        StreamFree free_lenk{d_lenk, st};
        hipLaunchKernelGGL(dir_lenk_kernel, pgrid, dim3(256), 0, st, (const unsigned char*)d_len, npos, d_lenk);
        RC_HIP_CHECK(hipGetLastError());
        // group lengths to the host through a pinned buffer of this thread (grow-only; portable: the thread may serve several devices)
        // (never freed: a thread-exit destructor would call into the HIP runtime while the process may be tearing it down)
        static thread_local struct Pinned {
            void* p = nullptr;
            size_t bytes = 0;
        } pin;
        const size_t need = (size_t)npos * sizeof(unsigned short);
        if (pin.bytes < need) {
            if (pin.p) (void)hipHostFree(pin.p);
            pin.p = nullptr;
            pin.bytes = 0;
            RC_HIP_CHECK(hipHostMalloc(&pin.p, need + (need >> 2), hipHostMallocPortable));
            pin.bytes = need + (need >> 2);
        }
        const unsigned short* lenk = (const unsigned short*)pin.p;
        RC_HIP_CHECK(hipMemcpyAsync(pin.p, d_lenk, need, hipMemcpyDeviceToHost, st));
        RC_HIP_CHECK(hipStreamSynchronize(st));
        // the sequential part: one dependent load per group of kDirGroup samples ...
        long long p = 0, g = 0;
        const long long nfull = n / kDirGroup;
        for (; g < nfull; ++g) {
            if (p >= npos) break;
            const unsigned short l = lenk[(size_t)p];
            if (l == 0) break;                        // ran off the buffer (or a sample too long): more words needed
            starts[(size_t)g] = first + p;
            p += l;
        }
        if (g < nfull) continue;                      // (ten-sigma margin missed: larger buffer)
        // ... and the last, partial group sample by sample on a small window of the per-sample lengths
        const int rest = (int)(n - nfull * kDirGroup);
        if (rest) {
            if (p >= npos) continue;
            starts[(size_t)nfull] = first + p;
            unsigned char tail[kDirGroup * 256];
            const long long have = (npos - p < (long long)sizeof(tail)) ? (npos - p) : (long long)sizeof(tail);
            RC_HIP_CHECK(hipMemcpyAsync(tail, d_len + p, (size_t)have, hipMemcpyDeviceToHost, st));
            RC_HIP_CHECK(hipStreamSynchronize(st));
            long long o = 0;
            int j = 0;
            for (; j < rest; ++j) {
                if (o >= have || tail[o] == 0 || tail[o] == 255) break;
                o += tail[o];
            }
            if (j < rest) continue;
            p += o;
        }
        const long long wf = first + p;               // the generator stands here afterwards
        long long* d_starts = nullptr;
        RC_HIP_CHECK(hipMallocAsync((void**)&d_starts, (size_t)ngroups * sizeof(long long), st));
        StreamFree free_starts{d_starts, st};
        unsigned int* d_last = nullptr;
        RC_HIP_CHECK(hipMallocAsync((void**)&d_last, 4 * sizeof(unsigned int), st));
        StreamFree free_last{d_last, st};
        RC_HIP_CHECK(hipMemcpyAsync(d_starts, starts.data(), (size_t)ngroups * sizeof(long long), hipMemcpyHostToDevice, st));
        DirEmitParams ep{};
        ep.raw = raw;
        ep.len = d_len;
        ep.starts = d_starts;
        ep.first = first;
        ep.n = n;
        ep.rng = rng;
        ep.mask = mask;
        ep.shift = shift;
        ep.sigma = sigma;
        ep.idx = idx_dev;
        ep.ab = ab_dev;
        ep.last_words = d_last;
        hipLaunchKernelGGL(dir_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ep);
        RC_HIP_CHECK(hipGetLastError());
        long long blk = wf / rcl::kMtN, pos = wf % rcl::kMtN;
        if (pos == 0) {                               // NumPy's representation of a block boundary: pos = 624 of the block before
            blk -= 1;
            pos = rcl::kMtN;
        }
        if ((blk + 1) * rcl::kMtN > words) return fail(RC_EHIP, "directional draws: final block outside the buffer");
        unsigned int lastw[4] = {0, 0, 0, 0};
        RC_HIP_CHECK(hipMemcpyAsync(lastw, d_last, sizeof(lastw), hipMemcpyDeviceToHost, st));
        RC_HIP_CHECK(hipMemcpyAsync(state->key, raw + blk * rcl::kMtN, rcl::kMtN * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        RC_HIP_CHECK(hipStreamSynchronize(st));
        state->pos = (int)pos;
        if (shift) {
            // the second normal of the last sample's attempt stays cached - computed with the host's libm, as NumPy does
            double x1, x2, r2;
            rcl::polar_attempt(lastw[0], lastw[1], lastw[2], lastw[3], x1, x2, r2);
            const double f = sqrt(-2.0 * log(r2) / r2);
            state->gauss = f * x1;
            state->has_gauss = 1;
        }
        return RC_OK;
    }
    return fail(RC_EHIP, "directional draws: word budget exceeded six times");
}

// ------------------------------------------------------------------------------------------------
// driver of the directional model's fidelity pass (rc_mc_fidelity_directional_f64_async; kernels: k_directional.inc.h)
// ------------------------------------------------------------------------------------------------
constexpr long long kDirFidChunk = (long long)kDirPartThreads * 8192;     // samples per partition pass (see dir_class_scatter_kernel)

template <int N>
int launch_directional(hipStream_t s, const DirParams& p, bool ends) {
    const long long nwaves = (p.n + 63) / 64;
    if (nwaves > 0x7fffffffLL) return fail(RC_EINVAL, "too many samples for one launch");
    const dim3 grid((unsigned)nwaves);                        // worst case for either class; waves beyond a class's count end at once
    if (ends) hipLaunchKernelGGL((mc_fid_dir_bond_kernel<N, rc::kWeightsEnds>), grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL((mc_fid_dir_bond_kernel<N, rc::kWeightsAdjugate>), grid, dim3(64), 0, s, p);
    hipLaunchKernelGGL(mc_fid_dir_diag_kernel<N>, grid, dim3(64), 0, s, p);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int enqueue_directional(hipStream_t s, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                        const double* ctrl, const int* idx, const double* ab, long long C, long long K, double* fid) {
    const bool ends = (in == 0 && out == N - 1) || (in == N - 1 && out == 0);
    const long long total = C * K;
    // RC_DIR_FID_CHUNK (environment, read per call; TEST knob): samples per partition pass, rounded down to whole waves - lets
    // a small problem exercise the multi-chunk path (chunk-relative idx / ab / fid pointers, p.first, the expm list's sp_first,
    // one stream-ordered workspace per chunk) that otherwise needs C K > 2^23
    long long chunk = kDirFidChunk;
    if (const char* e = getenv("RC_DIR_FID_CHUNK")) {
        const long long v = atoll(e) / 64 * 64;
        if (v >= 64 && v < chunk) chunk = v;
    }
    for (long long done = 0; done < total; done += chunk) {
        const long long n = (total - done < chunk) ? (total - done) : chunk;
        const long long nblocks = (n + kDirPartThreads - 1) / kDirPartThreads;
        // workspace of THIS chunk, allocated and released in stream order: list + marked (n ints each), block counts, counters
        char* ws = nullptr;
        const size_t nb_list = ((size_t)n * sizeof(int) + 255) & ~(size_t)255;
        const size_t nb_blk = ((size_t)nblocks * sizeof(unsigned int) + 255) & ~(size_t)255;
        RC_HIP_CHECK(hipMallocAsync((void**)&ws, 2 * nb_list + nb_blk + 256, s));
        StreamFree free_ws{ws, s};
        DirParams p{};
        // chunk-relative sample indices: pointers are offset, the controller index needs the chunk's first sample
        p.ctrl = ctrl;
        p.idx = idx + done;
        p.ab = ab + 2 * done;
        p.fid = fid + done;
        p.K = K;
        p.n = n;
        p.in = in;
        p.out = out;
        p.list = (int*)ws;
        p.marked = (int*)(ws + nb_list);
        p.blk_counts = (unsigned int*)(ws + 2 * nb_list);
        p.counts = (unsigned int*)(ws + 2 * nb_list + nb_blk);
        p.first = done;
        fill_h0(p.h0, N, h0_diag, h0_offdiag);
        RC_HIP_CHECK(hipMemsetAsync(p.counts, 0, 256, s));
        hipLaunchKernelGGL(dir_class_count_kernel, dim3((unsigned)nblocks), dim3(kDirPartThreads), 0, s, p, N);
        hipLaunchKernelGGL(dir_class_scatter_kernel, dim3((unsigned)nblocks), dim3(kDirPartThreads), 0, s, p, N);
        int rc = RC_EINVAL;
        switch (N) {
#define RC_DIR_CASE(n) case n: rc = launch_directional<n>(s, p, ends); break;
            RC_DIR_CASE(2) RC_DIR_CASE(3) RC_DIR_CASE(4) RC_DIR_CASE(5) RC_DIR_CASE(6) RC_DIR_CASE(7) RC_DIR_CASE(8) RC_DIR_CASE(9)
            RC_DIR_CASE(10) RC_DIR_CASE(11) RC_DIR_CASE(12)
#undef RC_DIR_CASE
        }
        if (rc) return rc;
        // the expm pass over the samples neither route settled (normally none: its waves read a zero count and end)
        ExpmParams e{};
        e.ctrl = ctrl;
        e.fid = fid + done;
        e.C = C;
        e.K = K;
        e.N = N;
        e.in = in;
        e.out = out;
        e.sp_idx = p.idx;
        e.sp_ab = p.ab;
        e.sp_list = p.marked;
        e.sp_count = p.counts + 1;
        e.sp_first = done;
        e.h0 = p.h0;
        if (int rc2 = ensure_func_attr(kAttrExpm, (const void*)mc_fid_expm_kernel,
                                       kExpmWaves * kExpmBufs * RC_MAX_NSPIN_FAST * RC_MAX_NSPIN_FAST * (int)sizeof(cplx)))
            return rc2;
        hipLaunchKernelGGL(mc_fid_expm_kernel, dim3(64), dim3(64 * kExpmWaves), (size_t)kExpmWaves * kExpmBufs * N * N * sizeof(cplx), s, e);
        RC_HIP_CHECK(hipGetLastError());
    }
    return RC_OK;
}

// ------------------------------------------------------------------------------------------------
// RCCL over xGMI from the C ABI (rc_comm_init / rc_mc_metrics_gathered_f64, ABI 6)
// ------------------------------------------------------------------------------------------------
// north_star's exchange step - "an RCCL all-gather over xGMI to reassemble per-controller fidelity vectors" - without torch: one
// process, one communicator per listed device (ncclCommInitAll), the collective enqueued on every device's stream inside ONE
// group call.  librccl.so is resolved at RUN time (dlsym on what the process already carries - PyTorch ships its own copy - or
// dlopen of librccl.so.1 / librccl.so): the library keeps no link-time dependency on it and every other entry works without it.
typedef int (*rccl_init_all_t)(void**, int, const int*);
typedef int (*rccl_destroy_t)(void*);
typedef int (*rccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*rccl_group_t)(void);
typedef const char* (*rccl_errstr_t)(int);
struct RcclApi {
    rccl_init_all_t init_all = nullptr;
    rccl_destroy_t destroy = nullptr;
    rccl_allgather_t allgather = nullptr;
    rccl_group_t group_start = nullptr, group_end = nullptr;
    rccl_errstr_t errstr = nullptr;
    bool ok = false;
};
constexpr int kNcclFloat64 = 8;                  // rccl.h: ncclFloat64

const RcclApi& rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        void* h = nullptr;                           // RTLD_DEFAULT first: the copy the process already loaded (PyTorch's)
        auto sym = [&h](const char* n) -> void* {
            void* p = dlsym(RTLD_DEFAULT, n);
            if (p) return p;
            if (!h) {
                // RTLD_LOCAL | RTLD_DEEPBIND, never RTLD_GLOBAL: a process that resolves RCCL here (nothing has loaded one yet)
                // and imports PyTorch LATER gets torch's own librccl.so / librocm_smi64.so as well; with the system copies in
                // the global scope the two librocm_smi64 share their global objects by symbol interposition and the process
                // ends in glibc's "double free or corruption" inside rocm_smi's static destructors (seen: pytest running the
                // RCCL test before any test had imported torch).  Kept out of the global scope, each copy binds to itself.
                for (const char* lib : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                    h = dlopen(lib, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
                    if (h) break;
                }
            }
            return h ? dlsym(h, n) : nullptr;
        };
        a.init_all = (rccl_init_all_t)sym("ncclCommInitAll");
        a.destroy = (rccl_destroy_t)sym("ncclCommDestroy");
        a.allgather = (rccl_allgather_t)sym("ncclAllGather");
        a.group_start = (rccl_group_t)sym("ncclGroupStart");
        a.group_end = (rccl_group_t)sym("ncclGroupEnd");
        a.errstr = (rccl_errstr_t)sym("ncclGetErrorString");
        a.ok = a.init_all && a.destroy && a.allgather && a.group_start && a.group_end;
        return a;
    }();
    return api;
}

}  // namespace

struct rc_comm {
    int ndev = 0;
    std::vector<int> devices;
    std::vector<void*> comms;                        // ncclComm_t per device
};

namespace {

int rccl_fail(int code, const char* what) {
    const RcclApi& a = rccl_api();
    return fail(RC_EHIP, std::string(what) + ": " + (a.errstr ? a.errstr(code) : "RCCL error " + std::to_string(code)));
}

// One device's share of rc_mc_metrics_gathered_f64: controllers [c0, c1) -> fidelities into rows [0, c1 - c0) of `d_fid` (Cmax rows,
// the rest zero) and their metric rows into `d_tab` ([NR][Cmax]).  Everything is enqueued on the device's stream; nothing waits.
struct GatherJob : ShareSpec {
    long long Cmax;
    double *d_ctrl, *d_draw, *d_fid, *d_tab;         // device: ctrl [Cmax][N+1], draws (NULL: the fused route), fid [Cmax][K], table [NR][Cmax]
};

int run_gather_share(GatherJob* j) {
    DeviceCtx* ctx = nullptr;
    if (int rc = get_ctx(j->device, &ctx)) return rc;
    hipStream_t st = ctx->stream;
    const long long K = j->K, Cl = j->c1 - j->c0;
    RC_HIP_CHECK(hipMemsetAsync(j->d_fid, 0, (size_t)j->Cmax * K * sizeof(double), st));
    if (Cl > 0)
        if (int rc = enqueue_share(*j, j->c0, Cl, j->d_ctrl, j->d_draw, j->d_fid, st)) return rc;
    // metric rows of all Cmax rows (the padding rows are rows of zeros: harmless, and the table keeps one shape on every device)
    double* t = j->d_tab;
    return enqueue_reduce(st, j->d_fid, j->Cmax, K, j->thr, j->nq, j->eps, t, t + 3 * j->Cmax, t + 6 * j->Cmax,
                          j->nq ? t + 9 * j->Cmax : nullptr, nullptr, /*standalone=*/true);
}

void run_gather_share_locked(GatherJob* j) {
    std::lock_guard<std::mutex> lk(g_ctx[j->device].mu);
    j->rc = run_gather_share(j);
    if (j->rc) j->err = g_last_error;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// Sum of a diagnostic tile counter (synchronises the device; optionally zeroes it): `slots` unsigned 64-bit counters at each of
// the n device addresses addr_of[u]() gives (a hipError_t).  `what`: the text of any failure; NULL: a counter of the chain /
// ring kernels - this unit's copy, then the second unit's (robchar_large.hip: chains of 17 .. 24 spins, rings of 11 .. 16) and
// the Sobol fidelity kernel's (robchar_qmc.hip) and the pick-freeze kernel's (robchar_vidx.hip) -,
// whose texts say what failed and in which unit.
typedef int (*CounterAddr)(void**);
static long long read_tile_counter(int device, int reset, const CounterAddr* addr_of, int n, int slots, const char* what) {
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RC_EHIP, "hipSetDevice failed");
    }
    const size_t nb = sizeof(unsigned long long) * slots;
    unsigned long long sum = 0;
    for (int u = 0; u < n; ++u) {
        const std::string unit = u == 0 ? " the tile counter failed" : u == 1 ? " the tile counter (second unit) failed"
                                 : u == 2 ? " the tile counter (Sobol unit) failed" : " the tile counter (variance-index unit) failed";
        unsigned long long v[64] = {0};
        void* addr = nullptr;
        if ((u == 0 && hipDeviceSynchronize() != hipSuccess) || addr_of[u](&addr) != hipSuccess || !addr ||
            hipMemcpy(v, addr, nb, hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RC_EHIP, what ? what : "reading" + unit);
        }
        if (reset && hipMemset(addr, 0, nb) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RC_EHIP, what ? what : "resetting" + unit);
        }
        for (int i = 0; i < slots; ++i) sum += v[i];
    }
    return (long long)sum;
}

// ------------------------------------------------------------------------------------------------
// the derivative family (robchar_grad.hip): what its entries share on the host
// ------------------------------------------------------------------------------------------------
// Where a sample's draws come from, checked the same way by the derivative and the readout-time entries, in two steps (the
// derivative entries refuse a call without outputs between them).  `stride` set: the entry takes a draw tensor; NULL: it
// generates its draws from `sigma` / `sigma_rows`.
// First the stride: the default is filled in, an overlapping one refused.
static int check_draw_stride(int N, long long* stride, long long K) {
    if (stride && *stride < 0) *stride = K * N * 3;
    if (stride && *stride != 0 && *stride < K * N * 3) return fail(RC_EINVAL, "draws_ctrl_stride overlaps controllers");
    return RC_OK;
}
// Then: a usable sigma where the draws are generated, the empty case (*empty, RC_OK), the NULL pointers and the tile limit.
static int check_draw_source(const void* ctrl, const void* draws, const long long* stride, double sigma, const void* sigma_rows,
                             long long C, long long K, bool* empty) {
    if (!stride && !sigma_rows && !(sigma >= 0.0 && sigma < HUGE_VAL))
        return fail(RC_EINVAL, "sigma must be finite and non-negative (or give sigma_rows)");
    if (C == 0 || K == 0) {
        *empty = true;
        return RC_OK;
    }
    if (!ctrl || (stride && !draws)) return fail(RC_EINVAL, "NULL array pointer");
    if ((C * ((K + 63) / 64)) > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
    return RC_OK;
}

// Argument checks of the entries of the derivative family - all before any HIP call.  `what`: the kernel's name in the
// N > RC_MAX_NSPIN_GRAD refusal; `outs`: the output arguments, of which `any_out` says whether one is set.  `stride` set: the
// entry takes a draw tensor (its default is filled in); NULL: it generates its draws from `sigma` / `sigma_rows`.
// *empty: nothing to do (RC_OK).
static int check_deriv_args(const char* what, const char* outs, int N, int in, int out, const void* ctrl, const void* draws,
                            long long* stride, double sigma, const void* sigma_rows, long long C, long long K, bool any_out,
                            bool* empty) {
    *empty = false;
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (N > RC_MAX_NSPIN_GRAD)
        return fail(RC_ENOSUP, std::string("the ") + what + (stride ? " kernel" : " kernel with draws generated inside it") +
                                   " supports chains of N <= " + std::to_string(RC_MAX_NSPIN_GRAD) + " spins");
    if (int rc = check_draw_stride(N, stride, K)) return rc;
    if (!any_out) return fail(RC_EINVAL, std::string("no output requested (") + outs + " are all NULL)");
    return check_draw_source(ctrl, draws, stride, sigma, sigma_rows, C, K, empty);
}
static const char kGradOuts[] = "fid_out, grad_out and mean_out", kSensOuts[] = "fid_out, sens_out and mean_out";

// what the four parameter blocks of the family have in common: controllers, fidelity output, tile geometry, static Hamiltonian
template <typename P>
static void fill_deriv_params(P& p, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, const double* ctrl,
                              long long C, long long K, double* fid) {
    p.ctrl = ctrl;
    p.fid = fid;
    p.C = C;
    p.K = K;
    p.tiles_per_ctrl = (K + 63) / 64;
    p.ntiles = C * p.tiles_per_ctrl;
    p.in = in;
    p.out = out;
    fill_h0(p.h0, N, h0_diag, h0_offdiag);
}

// With `want_part`: p.part = [ntiles][width] per-tile sums for the second pass, stream-ordered and released behind it.  Then
// `launch()`: the entry `name` of robchar_grad.hip (named in the error text).
template <typename P, typename Launch>
static int launch_with_part(hipStream_t s, P& p, bool want_part, int width, const char* name, Launch launch) {
    StreamFree part{nullptr, s};
    if (want_part) {
        RC_HIP_CHECK(hipMallocAsync(&part.p, (size_t)p.ntiles * width * sizeof(double), s));
        p.part = (double*)part.p;
    }
    const hipError_t e = (hipError_t)launch();
    if (e != hipSuccess) return fail(RC_EHIP, std::string(name) + ": " + hipGetErrorString(e));
    return RC_OK;
}

// device pointers; the arguments have been checked
static int enqueue_grad(hipStream_t s, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, const double* ctrl,
                        const double* draws, long long draw_cstride, long long C, long long K, double* fid, double* grad,
                        double* mean) {
    rckp::GradParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, ctrl, C, K, fid);
    p.draws = draws;
    p.draw_cstride = draw_cstride;
    p.align16 = draws_align16(draws, draw_cstride);
    p.grad = grad;
    return launch_with_part(s, p, mean != nullptr, N + 2, "rc_grad_launch", [&] { return rc_grad_launch(N, (void*)s, &p, mean); });
}
static int enqueue_sens(hipStream_t s, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, const double* ctrl,
                        const double* draws, long long draw_cstride, long long C, long long K, double* fid, double* sens,
                        double* mean) {
    rckp::SensParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, ctrl, C, K, fid);
    p.draws = draws;
    p.draw_cstride = draw_cstride;
    p.align16 = draws_align16(draws, draw_cstride);
    p.sens = sens;
    return launch_with_part(s, p, mean != nullptr, 3 * N + 2, "rc_sens_launch",
                            [&] { return rc_sens_launch(N, (void*)s, &p, mean); });
}

// The blocking form of enqueue_grad / enqueue_sens (`enqueue`) on the device's own stream: either input and any output may be a
// host pointer, which is staged through the device's workspace.  `per_sample`, `per_row`: doubles of the second output per sample
// and of the mean per controller row.  The arguments have been checked.
static int blocking_deriv(decltype(&enqueue_grad) enqueue, int per_sample, int per_row, int device, int N, int in, int out,
                          const double* h0_diag, const double* h0_offdiag, const double* controllers, const double* draws,
                          long long draws_ctrl_stride, long long C, long long K, double* fid_out, double* second_out, double* mean_out) {
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t nb_fid = (size_t)C * K * sizeof(double), nb_draw = draws_bytes(C, K, N, draws_ctrl_stride);
    const int s_ctrl = ws.in(controllers, (size_t)C * (N + 1) * sizeof(double)), s_draw = ws.in(draws, nb_draw),
              s_fid = ws.out(fid_out, nb_fid), s_second = ws.out(second_out, nb_fid * per_sample),
              s_mean = ws.out(mean_out, (size_t)C * per_row * sizeof(double));
    if (int rc = ws.stage_in()) return rc;
    if (int rc = enqueue(ws.ctx->stream, N, in, out, h0_diag, h0_offdiag, ws.ptr(s_ctrl), ws.ptr(s_draw), draws_ctrl_stride, C, K,
                         ws.ptr(s_fid), ws.ptr(s_second), ws.ptr(s_mean)))
        return rc;
    return ws.stage_out();
}

extern "C" {

#ifdef RC_STAMPS
// diagnostic builds only: device buffer of [ntiles][rckp::kStampSlots] int64 receiving per-wave stamps; read when a launch is
// ENQUEUED, so two launches enqueued back to back can write two buffers
int rc_debug_set_stamps(long long* dev_buf) { g_stamps = dev_buf; return 0; }
#endif

// Test and measurement hook, not part of the C ABI (not in robchar_hip.h): moves the tile count below which launch_chain picks
// the non-temporal fidelity store (0: never, a negative value: back to the built-in rule) and returns the value it replaced.
// tests/test_gpu_launch_boundary.py runs both sides of the rule on the same inputs with it.
long long rc_debug_nt_store_tiles(long long tiles) { return g_nt_store_tiles.exchange(tiles < 0 ? kNtStoreTiles : tiles); }

int rc_version(void) { return RC_ABI_VERSION; }

// Which compile-time switches of this build change RESULTS or disable a safety net (0 = the product build).  A library built
// with one of them must never be taken for the product (code-robchar_amd/_lib.py refuses the ones in RC_BUILD_WRONG_RESULTS_MASK
// - timing experiments of earlier trees, which knowingly returned wrong fidelities - unless ROBCHAR_ALLOW_EXPERIMENT_LIB=1;
// bench.py records the value).
int rc_build_flags(void) {
    int f = 0;
#ifdef RC_DEV_FEW_N
    f |= RC_BUILD_DEV_FEW_N;
#endif
#ifdef RC_STAMPS
    f |= RC_BUILD_STAMPS;
#endif
    if (!rc::kSumRuleGuard) f |= RC_BUILD_NO_SUM_RULE_GUARD;
    if (!RC_KEEP_SETTLED) f |= RC_BUILD_NO_KEEP_SETTLED;
    return f;
}

// Where the fused Philox fidelity kernel is the faster of the two bit-identical routes (profiles/r04_philox_fused_sweep.txt:
// 0.70 .. 0.86 of the two-kernel route up to N = 13 and for end-to-end pairs at N = 14; beyond, the fused instantiations run
// one wave per SIMD and the two-kernel route is 7 % faster).  ROBCHAR_PHILOX_FUSED=0 in the environment (read per call)
// switches the route off everywhere - here, in the sharded entries and in the Python layer, which all ask this function.
int rc_philox_fused_pays(int N, int in, int out) {
    if (N < 2 || N > RC_MAX_NSPIN_FAST) return 0;
    const char* e = getenv("ROBCHAR_PHILOX_FUSED");
    if (e && e[0] == '0') return 0;
    const bool ends = (in == 0 && out == N - 1) || (in == N - 1 && out == 0);
    return (N <= 13 || (N == 14 && ends)) ? 1 : 0;
}

int rc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* rc_last_error(void) { return g_last_error.c_str(); }

long long rc_stats_general_tiles(int device, int reset) {
    const CounterAddr units[4] = {[](void** a) { return (int)hipGetSymbolAddress(a, HIP_SYMBOL(g_general_tiles)); },
                                  [](void** a) { return rc_large_counter_addr(0, a); },
                                  [](void** a) { return rc_qmc_counter_addr(0, a); },
                                  [](void** a) { return rc_vidx_counter_addr(0, a); }};
    return read_tile_counter(device, reset, units, 4, 1, nullptr);
}
long long rc_stats_polish_tiles(int device, int reset) {
    const CounterAddr units[4] = {[](void** a) { return (int)hipGetSymbolAddress(a, HIP_SYMBOL(g_polish_tiles)); },
                                  [](void** a) { return rc_large_counter_addr(1, a); },
                                  [](void** a) { return rc_qmc_counter_addr(1, a); },
                                  [](void** a) { return rc_vidx_counter_addr(1, a); }};
    return read_tile_counter(device, reset, units, 4, 64, nullptr);
}

int rc_set_fidelity_kernel(int kernel) {
    if (kernel < RC_KERNEL_AUTO || kernel > RC_KERNEL_RING_HH) return fail(RC_EINVAL, "unknown kernel id");
    std::lock_guard<std::mutex> lk(g_cfg_mu);
    g_default_kernel = kernel;
    return RC_OK;
}

int rc_reserve_ring(int device, void* stream, long long samples) {
    if (samples < 0) return fail(RC_EINVAL, "samples must be non-negative");
    if (int rc = device_in_range(device)) return rc;
    RC_HIP_CHECK(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_ctx[device].ring_mu);
    return ring_buf_reserve(ring_buf_for(g_ctx[device], (hipStream_t)stream), (hipStream_t)stream, samples);
}

int rc_release_stream(int device, void* stream) {
    if (int rc = device_in_range(device)) return rc;
    RC_HIP_CHECK(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_ctx[device].ring_mu);
    auto it = g_ctx[device].ring_bufs.find((hipStream_t)stream);
    if (it == g_ctx[device].ring_bufs.end()) return RC_OK;
    char* mem = it->second.mem;
    g_ctx[device].ring_bufs.erase(it);
    if (mem) RC_HIP_CHECK(hipFreeAsync(mem, (hipStream_t)stream));     // behind the stream's last ring launch
    return RC_OK;
}

int rc_mc_fidelity_f64_async(int device, void* stream, int kernel, int N, int in, int out,
                             const double* h0_diag, const double* h0_offdiag, int ring,
                             const double* controllers_dev, const double* draws_dev, long long C,
                             long long K, double* fid_out_dev) {
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_fidelity((hipStream_t)stream, kernel, N, in, out, h0_diag, h0_offdiag, ring,
                            controllers_dev, draws_dev, -1, C, K, fid_out_dev);
}

int rc_mc_fidelity_ex_f64_async(int device, void* stream, int kernel, int N, int in, int out,
                                const double* h0_diag, const double* h0_offdiag, int ring,
                                const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride,
                                long long C, long long K, double* fid_out_dev) {
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_fidelity((hipStream_t)stream, kernel, N, in, out, h0_diag, h0_offdiag, ring,
                            controllers_dev, draws_dev, draws_ctrl_stride, C, K, fid_out_dev);
}

int rc_mc_fidelity_grad_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                                  const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride, long long C,
                                  long long K, double* fid_out_dev, double* grad_out_dev, double* mean_out_dev) {
    bool empty = false;
    if (int rc = check_deriv_args("fidelity-gradient", kGradOuts, N, in, out, controllers_dev, draws_dev, &draws_ctrl_stride, 0.0,
                                  nullptr, C, K, fid_out_dev || grad_out_dev || mean_out_dev, &empty))
        return rc;
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_grad((hipStream_t)stream, N, in, out, h0_diag, h0_offdiag, controllers_dev, draws_dev, draws_ctrl_stride, C, K,
                        fid_out_dev, grad_out_dev, mean_out_dev);
}

int rc_mc_fidelity_grad_f64(int device, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                            const double* controllers, const double* draws, long long draws_ctrl_stride, long long C, long long K,
                            double* fid_out, double* grad_out, double* mean_out) {
    bool empty = false;
    if (int rc = check_deriv_args("fidelity-gradient", kGradOuts, N, in, out, controllers, draws, &draws_ctrl_stride, 0.0, nullptr, C, K,
                                  fid_out || grad_out || mean_out, &empty))
        return rc;
    if (empty) return RC_OK;
    return blocking_deriv(enqueue_grad, N + 1, N + 2, device, N, in, out, h0_diag, h0_offdiag, controllers, draws, draws_ctrl_stride, C,
                          K, fid_out, grad_out, mean_out);
}

// (one unsigned 64-bit counter of the third or fourth unit; a failed reset reports as a failed read)
static long long read_unit_counter(int device, int reset, CounterAddr addr_of, const char* what) {
    return read_tile_counter(device, reset, &addr_of, 1, 1, what);
}

long long rc_stats_grad_general_tiles(int device, int reset) {
    return read_unit_counter(device, reset, rc_grad_counter_addr, "reading the gradient kernel's tile counter failed");
}

int rc_mc_fidelity_sens_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                                  const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride, long long C,
                                  long long K, double* fid_out_dev, double* sens_out_dev, double* mean_out_dev) {
    bool empty = false;
    if (int rc = check_deriv_args("noise-sensitivity", kSensOuts, N, in, out, controllers_dev, draws_dev, &draws_ctrl_stride, 0.0,
                                  nullptr, C, K, fid_out_dev || sens_out_dev || mean_out_dev, &empty))
        return rc;
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_sens((hipStream_t)stream, N, in, out, h0_diag, h0_offdiag, controllers_dev, draws_dev, draws_ctrl_stride, C, K,
                        fid_out_dev, sens_out_dev, mean_out_dev);
}

int rc_mc_fidelity_sens_f64(int device, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                            const double* controllers, const double* draws, long long draws_ctrl_stride, long long C, long long K,
                            double* fid_out, double* sens_out, double* mean_out) {
    bool empty = false;
    if (int rc = check_deriv_args("noise-sensitivity", kSensOuts, N, in, out, controllers, draws, &draws_ctrl_stride, 0.0, nullptr, C, K,
                                  fid_out || sens_out || mean_out, &empty))
        return rc;
    if (empty) return RC_OK;
    return blocking_deriv(enqueue_sens, 3 * N, 3 * N + 2, device, N, in, out, h0_diag, h0_offdiag, controllers, draws, draws_ctrl_stride,
                          C, K, fid_out, sens_out, mean_out);
}

long long rc_stats_sens_general_tiles(int device, int reset) {
    return read_unit_counter(device, reset, rc_sens_counter_addr, "reading the sensitivity kernel's tile counter failed");
}

// ------------------------------------------------------------------------------------------------
// fidelity on a grid of readout times (robchar_times.hip)
// ------------------------------------------------------------------------------------------------
// Argument checks of the three entries - all before any HIP call.  `stride` set: the entry takes a draw tensor (its default is
// filled in); NULL: it generates its draws from `sigma` / `sigma_rows`.  *empty: nothing to do (RC_OK).
static int check_times_args(int N, int in, int out, int ring, const void* ctrl, const void* draws, long long* stride, double sigma,
                            const void* sigma_rows, long long C, long long K, int M, const void* weights, const void* fid,
                            const void* wsum, const void* fmin, bool* empty) {
    *empty = false;
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (N > RC_MAX_NSPIN_FAST)
        return fail(RC_ENOSUP, "the readout-time kernels support chains of N <= " + std::to_string(RC_MAX_NSPIN_FAST) + " spins");
    if (ring) return fail(RC_ENOSUP, "the readout-time kernels support the chain topology only");
    if (M < 1 || M > RC_MAX_TIMES) return fail(RC_EINVAL, "M must be in [1, " + std::to_string(RC_MAX_TIMES) + "]");
    if (!fid && !wsum && !fmin) return fail(RC_EINVAL, "no output requested (fid_out, wsum_out and fmin_out are all NULL)");
    if (wsum && !weights) return fail(RC_EINVAL, "wsum_out needs weights");
    if (int rc = check_draw_stride(N, stride, K)) return rc;
    return check_draw_source(ctrl, draws, stride, sigma, sigma_rows, C, K, empty);
}

// what the two kernels' parameter blocks have in common; device pointers, checked arguments
static void fill_times_params(rckp::TimesParams& p, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                              const double* ctrl, long long C, long long K, int M, const double* tscale, const double* tshift,
                              const double* weights, double* fid, double* wsum, double* fmin) {
    p.ctrl = ctrl;
    p.fid = fid;
    p.wsum = wsum;
    p.fmin = fmin;
    p.tscale = tscale;
    p.tshift = tshift;
    p.weights = weights;
    p.M = M;
    p.C = C;
    p.K = K;
    p.tiles_per_ctrl = (K + 63) / 64;
    p.ntiles = C * p.tiles_per_ctrl;
    p.in = in;
    p.out = out;
    fill_h0(p.h0, N, h0_diag, h0_offdiag);
}

static int enqueue_times(hipStream_t s, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, const double* ctrl,
                         const double* draws, long long draw_cstride, long long C, long long K, int M, const double* tscale,
                         const double* tshift, const double* weights, double* fid, double* wsum, double* fmin) {
    rckp::TimesParams p{};
    fill_times_params(p, N, in, out, h0_diag, h0_offdiag, ctrl, C, K, M, tscale, tshift, weights, fid, wsum, fmin);
    p.draws = draws;
    p.draw_cstride = draw_cstride;
    p.align16 = draws_align16(draws, draw_cstride);
    const hipError_t e = (hipError_t)rc_times_launch(N, (void*)s, &p);
    if (e != hipSuccess) return fail(RC_EHIP, std::string("rc_times_launch: ") + hipGetErrorString(e));
    return RC_OK;
}

int rc_mc_fidelity_times_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                                   int ring, const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride,
                                   long long C, long long K, int M, const double* tscale_dev, const double* tshift_dev,
                                   const double* weights_dev, double* fid_out_dev, double* wsum_out_dev, double* fmin_out_dev) {
    bool empty = false;
    if (int rc = check_times_args(N, in, out, ring, controllers_dev, draws_dev, &draws_ctrl_stride, 0.0, nullptr, C, K, M, weights_dev,
                                  fid_out_dev, wsum_out_dev, fmin_out_dev, &empty))
        return rc;
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_times((hipStream_t)stream, N, in, out, h0_diag, h0_offdiag, controllers_dev, draws_dev, draws_ctrl_stride, C, K, M,
                         tscale_dev, tshift_dev, weights_dev, fid_out_dev, wsum_out_dev, fmin_out_dev);
}

int rc_mc_fidelity_times_f64(int device, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, int ring,
                             const double* controllers, const double* draws, long long draws_ctrl_stride, long long C, long long K,
                             int M, const double* tscale, const double* tshift, const double* weights, double* fid_out,
                             double* wsum_out, double* fmin_out) {
    bool empty = false;
    if (int rc = check_times_args(N, in, out, ring, controllers, draws, &draws_ctrl_stride, 0.0, nullptr, C, K, M, weights, fid_out,
                                  wsum_out, fmin_out, &empty))
        return rc;
    if (empty) return RC_OK;
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t nb_fid = (size_t)C * K * sizeof(double), nb_grid = (size_t)M * sizeof(double),
                 nb_draw = draws_bytes(C, K, N, draws_ctrl_stride);
    // (an absent grid array stays absent: a slot is declared only for what the caller gave)
    const int s_ctrl = ws.in(controllers, (size_t)C * (N + 1) * sizeof(double)), s_draw = ws.in(draws, nb_draw),
              s_scale = tscale ? ws.in(tscale, nb_grid) : -1, s_shift = tshift ? ws.in(tshift, nb_grid) : -1,
              s_wts = weights ? ws.in(weights, nb_grid) : -1, s_fid = ws.out(fid_out, nb_fid * M), s_wsum = ws.out(wsum_out, nb_fid),
              s_fmin = ws.out(fmin_out, nb_fid);
    if (int rc = ws.stage_in()) return rc;
    if (int rc = enqueue_times(ws.ctx->stream, N, in, out, h0_diag, h0_offdiag, ws.ptr(s_ctrl), ws.ptr(s_draw), draws_ctrl_stride, C, K, M,
                               s_scale >= 0 ? ws.ptr(s_scale) : nullptr, s_shift >= 0 ? ws.ptr(s_shift) : nullptr,
                               s_wts >= 0 ? ws.ptr(s_wts) : nullptr, ws.ptr(s_fid), ws.ptr(s_wsum), ws.ptr(s_fmin)))
        return rc;
    return ws.stage_out();
}

int rc_mc_fidelity_times_philox_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                          const double* h0_offdiag, int ring, const double* controllers_dev, unsigned long long seed,
                                          unsigned long long offset, double sigma, const double* sigma_rows_dev, long long C,
                                          long long K, int M, const double* tscale_dev, const double* tshift_dev,
                                          const double* weights_dev, double* fid_out_dev, double* wsum_out_dev, double* fmin_out_dev) {
    bool empty = false;
    if (int rc = check_times_args(N, in, out, ring, controllers_dev, nullptr, nullptr, sigma, sigma_rows_dev, C, K, M, weights_dev,
                                  fid_out_dev, wsum_out_dev, fmin_out_dev, &empty))
        return rc;
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    rckp::TimesParams p{};
    fill_times_params(p, N, in, out, h0_diag, h0_offdiag, controllers_dev, C, K, M, tscale_dev, tshift_dev, weights_dev, fid_out_dev,
                      wsum_out_dev, fmin_out_dev);
    p.seed = seed;
    p.offset = offset;
    p.sigma_rows = sigma_rows_dev;
    p.sigma = sigma;
    const hipError_t e = (hipError_t)rc_times_philox_launch(N, stream, &p);
    if (e != hipSuccess) return fail(RC_EHIP, std::string("rc_times_philox_launch: ") + hipGetErrorString(e));
    return RC_OK;
}

long long rc_stats_times_general_tiles(int device, int reset) {
    return read_unit_counter(device, reset, rc_times_counter_addr, "reading the readout-time kernels' tile counter failed");
}

int rc_mc_fidelity_sens_philox_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                         const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                         unsigned long long offset, double sigma, const double* sigma_rows_dev, long long C,
                                         long long K, double* fid_out_dev, double* sens_out_dev, double* mean_out_dev) {
    bool empty = false;
    if (int rc = check_deriv_args("noise-sensitivity", kSensOuts, N, in, out, controllers_dev, nullptr, nullptr, sigma, sigma_rows_dev, C,
                                  K, fid_out_dev || sens_out_dev || mean_out_dev, &empty))
        return rc;
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    rckp::SensPhiloxParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, controllers_dev, C, K, fid_out_dev);
    p.sens = sens_out_dev;
    p.seed = seed;
    p.offset = offset;
    p.sigma_rows = sigma_rows_dev;
    p.sigma = sigma;
    return launch_with_part(s, p, mean_out_dev != nullptr, 3 * N + 2, "rc_sens_philox_launch",
                            [&] { return rc_sens_philox_launch(N, (void*)s, &p, mean_out_dev); });
}

int rc_mc_fidelity_grad_philox_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                         const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                         unsigned long long offset, double sigma, const double* sigma_rows_dev, int shared_draws,
                                         long long C, long long K, double* fid_out_dev, double* grad_out_dev, double* mean_out_dev,
                                         double* moment_out_dev) {
    bool empty = false;
    if (int rc = check_deriv_args("fidelity-gradient", "fid_out, grad_out, mean_out and moment_out", N, in, out, controllers_dev, nullptr,
                                  nullptr, sigma, sigma_rows_dev, C, K, fid_out_dev || grad_out_dev || mean_out_dev || moment_out_dev,
                                  &empty))
        return rc;
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    rckp::GradPhiloxParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, controllers_dev, C, K, fid_out_dev);
    p.grad = grad_out_dev;
    p.shared = shared_draws ? 1 : 0;
    p.moments = moment_out_dev ? 1 : 0;
    p.seed = seed;
    p.offset = offset;
    p.sigma_rows = sigma_rows_dev;
    p.sigma = sigma;
    return launch_with_part(s, p, mean_out_dev || moment_out_dev, (N + 2) * (p.moments ? 2 : 1), "rc_grad_philox_launch",
                            [&] { return rc_grad_philox_launch(N, (void*)s, &p, mean_out_dev, moment_out_dev); });
}

int rc_mc_fidelity_grad_times_philox_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                               const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                               unsigned long long offset, double sigma, const double* sigma_rows_dev,
                                               int shared_draws, long long C, long long K, int M, const double* tscale_dev,
                                               const double* tshift_dev, const double* weights_dev, double* wfid_out_dev,
                                               double* wgrad_out_dev, double* mean_out_dev, double* moment_out_dev) {
    bool empty = false;
    if (int rc = check_deriv_args("fidelity-gradient", "wfid_out, wgrad_out, mean_out and moment_out", N, in, out, controllers_dev,
                                  nullptr, nullptr, sigma, sigma_rows_dev, C, K,
                                  wfid_out_dev || wgrad_out_dev || mean_out_dev || moment_out_dev, &empty))
        return rc;
    if (M < 1 || M > RC_MAX_TIMES) return fail(RC_EINVAL, "M must be in [1, " + std::to_string(RC_MAX_TIMES) + "]");
    if (!weights_dev) return fail(RC_EINVAL, "NULL array pointer (weights)");
    if (empty) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    rckp::GradTimesParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, controllers_dev, C, K, wfid_out_dev);
    p.grad = wgrad_out_dev;
    p.shared = shared_draws ? 1 : 0;
    p.moments = moment_out_dev ? 1 : 0;
    p.seed = seed;
    p.offset = offset;
    p.sigma_rows = sigma_rows_dev;
    p.sigma = sigma;
    p.tscale = tscale_dev;
    p.tshift = tshift_dev;
    p.weights = weights_dev;
    p.M = M;
    return launch_with_part(s, p, mean_out_dev || moment_out_dev, (N + 2) * (p.moments ? 2 : 1), "rc_grad_times_philox_launch",
                            [&] { return rc_grad_times_philox_launch(N, (void*)s, &p, mean_out_dev, moment_out_dev); });
}

int rc_mc_fidelity_grad_listed_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                         const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                         unsigned long long offset, double sigma, const double* sigma_rows_dev, int shared_draws,
                                         long long C, long long K, const int* list_dev, const double* weight_dev, long long L,
                                         double* fid_out_dev, double* grad_out_dev, double* sum_out_dev) {
    bool empty = false;
    if (int rc = check_deriv_args("fidelity-gradient", "fid_out, grad_out and sum_out", N, in, out, controllers_dev, nullptr, nullptr,
                                  sigma, sigma_rows_dev, C, K, fid_out_dev || grad_out_dev || sum_out_dev, &empty))
        return rc;
    if (L < 0) return fail(RC_EINVAL, "L must be non-negative");
    if (empty || L == 0) return RC_OK;
    if (!list_dev) return fail(RC_EINVAL, "NULL array pointer (list)");
    if ((C * ((L + 63) / 64)) > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    rckp::GradListedParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, controllers_dev, C, K, fid_out_dev);
    p.tiles_per_ctrl = (L + 63) / 64;              // the tiles cover the L slots of a row, not its K draws
    p.ntiles = C * p.tiles_per_ctrl;
    p.grad = grad_out_dev;
    p.shared = shared_draws ? 1 : 0;
    p.seed = seed;
    p.offset = offset;
    p.sigma_rows = sigma_rows_dev;
    p.sigma = sigma;
    p.list = list_dev;
    p.weight = weight_dev;
    p.L = L;
    return launch_with_part(s, p, sum_out_dev != nullptr, N + 2, "rc_grad_listed_launch",
                            [&] { return rc_grad_listed_launch(N, (void*)s, &p, sum_out_dev); });
}

// m = min(K, ceil(alpha K)) and the two CVaR weights, in double precision and in the order noise.tail_weights computes them
static bool tail_plan(long long K, double alpha, long long* m, double* w_body, double* w_last) {
    if (!(alpha > 0.0 && alpha <= 1.0) || K < 0 || K > 0x7fffffffLL) return false;
    const double ak = alpha * (double)K;
    const long long up = (long long)ceil(ak);
    *m = up < K ? up : K;
    *w_body = 1.0 / ak;
    *w_last = (ak - (double)(*m - 1)) / ak;
    return true;
}

long long rc_tail_select_len(long long K, double alpha) {
    long long m;
    double w_body, w_last;
    if (!tail_plan(K, alpha, &m, &w_body, &w_last)) return -1;
    return m;
}

int rc_tail_select_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K, double alpha,
                             int* list_out_dev, double* weight_out_dev, double* var_out_dev) {
    if (!(alpha > 0.0 && alpha <= 1.0)) return fail(RC_EINVAL, "alpha must be in (0, 1]");
    if (C < 0 || K < 0) return fail(RC_EINVAL, "C and K must be non-negative");
    if (K > 0x7fffffffLL) return fail(RC_EINVAL, "K must be at most 2^31 - 1");
    if (C == 0 || K == 0) return RC_OK;
    if (!fid_dev || !list_out_dev) return fail(RC_EINVAL, "NULL array pointer (fid, list_out)");
    if (C > 0x7fffffffLL) return fail(RC_EINVAL, "too many rows for one launch");
    TailParams p{};
    tail_plan(K, alpha, &p.m, &p.w_body, &p.w_last);
    p.fid = fid_dev;
    p.C = C;
    p.K = K;
    p.list = list_out_dev;
    p.weight = weight_out_dev;
    p.var = var_out_dev;
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)C), wgrid((unsigned)((C + 3) / 4));
    if (K <= 128)                                         // short rows: one wave per row (the route follows K alone)
        hipLaunchKernelGGL(tail_select_rows_wave_kernel<2>, wgrid, dim3(256), 0, s, p);
    else if (K <= 512)
        hipLaunchKernelGGL(tail_select_rows_wave_kernel<8>, wgrid, dim3(256), 0, s, p);
    else if (K <= kWaveRowMaxK)
        hipLaunchKernelGGL(tail_select_rows_wave_kernel<kWaveRowMaxK / 64>, wgrid, dim3(256), 0, s, p);
    else if (K <= (long long)kRedCache * 128)             // the thread count follows K alone, as in enqueue_reduce
        hipLaunchKernelGGL((tail_select_kernel<128, kRedCache, true>), grid, dim3(128), 0, s, p);
    else if (K <= (long long)kRedCache * 256)
        hipLaunchKernelGGL((tail_select_kernel<256, kRedCache, true>), grid, dim3(256), 0, s, p);
    else if (K <= (long long)kRedCache * 512)
        hipLaunchKernelGGL((tail_select_kernel<512, kRedCache, true>), grid, dim3(512), 0, s, p);
    else
        hipLaunchKernelGGL((tail_select_kernel<512, kSelLongU, false>), grid, dim3(512), 0, s, p);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

// ---- bootstrap of the metrics (ABI 15): replicates resampled on the device, summarised through the row sort (k_bootstrap.inc.h) ------
static void launch_bootstrap(hipStream_t s, const BootParams& p, bool lds) {
    const dim3 grid((unsigned)(p.C * p.splits)), block(rcboot::kThreads);
    if (lds && p.nq <= 2)
        hipLaunchKernelGGL((bootstrap_replicates_kernel<2, true>), grid, block, 0, s, p);
    else if (lds)
        hipLaunchKernelGGL((bootstrap_replicates_kernel<rcboot::kMaxQ, true>), grid, block, 0, s, p);
    else if (p.nq <= 2)
        hipLaunchKernelGGL((bootstrap_replicates_kernel<2, false>), grid, block, 0, s, p);
    else
        hipLaunchKernelGGL((bootstrap_replicates_kernel<rcboot::kMaxQ, false>), grid, block, 0, s, p);
}

int rc_bootstrap_metrics_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K, long long B,
                                   unsigned long long seed, unsigned long long offset, const double* q_thresholds, int nq,
                                   long long rank_lo, long long rank_hi, int route, double* rep_out_dev, double* summary_out_dev) {
    if (const char* msg = rcboot::check_args(C, K, B, nq, !q_thresholds, rank_lo, rank_hi, route, offset, !fid_dev))
        return fail(RC_EINVAL, msg);
    if (C == 0 || (!rep_out_dev && !summary_out_dev)) return RC_OK;
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const long long R = (rcboot::kFixedMetrics + nq) * C;          // replicate rows: (metric, c)
    // workspace of THIS call, allocated and released in stream order: the replicates when the caller does not want them, and
    // the sorted rows of the summary
    StreamFree rep_ws{nullptr, s}, sorted_ws{nullptr, s};
    double* rep = rep_out_dev;
    if (!rep) {
        RC_HIP_CHECK(hipMallocAsync(&rep_ws.p, (size_t)R * B * sizeof(double), s));
        rep = (double*)rep_ws.p;
    }
    BootParams p{};
    p.fid = fid_dev;
    p.C = C;
    p.K = K;
    p.B = B;
    p.seed = seed;
    p.offset = offset;
    p.nq = nq;
    p.splits = rcboot::choose_splits(C, B);
    for (int j = 0; j < rcboot::kMaxQ; ++j) p.thr[j] = j < nq ? q_thresholds[j] : __builtin_inf();
    p.rep = rep;
    launch_bootstrap(s, p, route == 1 || (route == 0 && K <= rcboot::kLdsMaxK));
    RC_HIP_CHECK(hipGetLastError());                               // (the LDS route declares 144 KiB of static LDS: a refused launch shows here)
    if (!summary_out_dev) return RC_OK;
    RC_HIP_CHECK(hipMallocAsync(&sorted_ws.p, (size_t)R * B * sizeof(double), s));
    if (int rc = enqueue_reduce(s, rep, R, B, nullptr, 0, 0.0, nullptr, nullptr, nullptr, nullptr, (double*)sorted_ws.p)) return rc;
    hipLaunchKernelGGL(bootstrap_summary_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, rep, (const double*)sorted_ws.p, R, C, B,
                       rank_lo, rank_hi, summary_out_dev);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_bootstrap_metrics_f64(int device, const double* fid, long long C, long long K, long long B, unsigned long long seed,
                             unsigned long long offset, const double* q_thresholds, int nq, long long rank_lo, long long rank_hi,
                             int route, double* rep_out, double* summary_out) {
    if (const char* msg = rcboot::check_args(C, K, B, nq, !q_thresholds, rank_lo, rank_hi, route, offset, !fid))
        return fail(RC_EINVAL, msg);
    if (C == 0 || (!rep_out && !summary_out)) return RC_OK;
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t M = (size_t)(rcboot::kFixedMetrics + nq);
    const int s_fid = ws.in(fid, (size_t)C * K * sizeof(double)), s_rep = ws.out(rep_out, M * C * B * sizeof(double)),
              s_sum = ws.out(summary_out, M * rcboot::kSummaryFields * C * sizeof(double), true);
    if (int rc = ws.stage_in()) return rc;
    if (int rc = rc_bootstrap_metrics_f64_async(device, ws.ctx->stream, ws.ptr(s_fid), C, K, B, seed, offset, q_thresholds, nq, rank_lo,
                                                rank_hi, route, ws.ptr(s_rep), ws.ptr(s_sum)))
        return rc;
    return ws.stage_out();
}

// ---- pairwise Wasserstein matrix (ABI 18): tiles of sorted rows against sorted rows (k_wasserstein.inc.h) ------------------------
static void launch_wasserstein(int P, hipStream_t s, const rcwd::Params& p, bool finish) {
    const dim3 tiles((unsigned)(p.tiles * p.plan.nparts)), elems((unsigned)((p.CA * p.CB + 255) / 256));
    if (!finish && P == 1)
        hipLaunchKernelGGL(wasserstein_tile_kernel<1>, tiles, dim3(rcwd::kThreads), 0, s, p);
    else if (!finish)
        hipLaunchKernelGGL(wasserstein_tile_kernel<2>, tiles, dim3(rcwd::kThreads), 0, s, p);
    else if (P == 1)
        hipLaunchKernelGGL(wasserstein_finish_kernel<1>, elems, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(wasserstein_finish_kernel<2>, elems, dim3(256), 0, s, p);
}

// the checks both entries make before any HIP call; *done: nothing to compute
static int check_wasserstein(int p, const void* a, long long CA, const void* b, long long* CB, long long K, const void* out, bool* done) {
    if (!b) *CB = 0;                                                // symmetric mode: CB is ignored
    if (const char* msg = rcwd::check_args(p, CA, *CB, K)) return fail(RC_EINVAL, msg);
    *done = CA == 0 || K == 0 || (b && *CB == 0);
    if (*done) return RC_OK;
    if (!a || !out) return fail(RC_EINVAL, "NULL array pointer (a, out)");
    if (const char* msg = rcwd::check_sizes(CA, *CB, K)) return fail(RC_EINVAL, msg);
    return RC_OK;
}

int rc_wasserstein_matrix_f64_async(int device, void* stream, int p, const double* a_sorted_dev, long long CA,
                                    const double* b_sorted_dev, long long CB, long long K, double* out_dev) {
    bool done = false;
    if (int rc = check_wasserstein(p, a_sorted_dev, CA, b_sorted_dev, &CB, K, out_dev, &done)) return rc;
    if (done) return RC_OK;
    rcwd::Params q{};
    q.a = a_sorted_dev;
    q.b = b_sorted_dev ? b_sorted_dev : a_sorted_dev;
    q.sym = b_sorted_dev ? 0 : 1;
    q.CA = CA;
    q.CB = q.sym ? CA : CB;
    q.K = K;
    q.nti = (q.CA + rcwd::kTile - 1) / rcwd::kTile;
    q.ntj = (q.CB + rcwd::kTile - 1) / rcwd::kTile;
    q.tiles = q.sym ? q.nti * (q.nti + 1) / 2 : q.nti * q.ntj;
    q.plan = rcwd::choose_plan(q.tiles, K);
    q.out = out_dev;
    if (q.tiles > 0x7fffffffLL / q.plan.nparts) return fail(RC_EINVAL, "too many workgroups for one launch");
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    // partial sums of THIS call, allocated and released in stream order
    StreamFree part_ws{nullptr, s};
    if (q.plan.nparts > 1) {
        RC_HIP_CHECK(hipMallocAsync(&part_ws.p, (size_t)q.plan.nparts * q.CA * q.CB * sizeof(double), s));
        q.part = (double*)part_ws.p;
    }
    launch_wasserstein(p, s, q, false);
    RC_HIP_CHECK(hipGetLastError());
    if (q.plan.nparts > 1) {
        launch_wasserstein(p, s, q, true);
        RC_HIP_CHECK(hipGetLastError());
    }
    return RC_OK;
}

int rc_wasserstein_matrix_f64(int device, int p, const double* a, long long CA, const double* b, long long CB, long long K,
                              int presorted, double* out) {
    bool done = false;
    if (int rc = check_wasserstein(p, a, CA, b, &CB, K, out, &done)) return rc;
    if (done) return RC_OK;
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t nb_a = (size_t)CA * K * sizeof(double), nb_b = (size_t)CB * K * sizeof(double);
    const int s_a = ws.in(a, nb_a), s_b = b ? ws.in(b, nb_b) : -1, s_out = ws.out(out, (size_t)CA * (b ? CB : CA) * sizeof(double)),
              s_as = presorted ? -1 : ws.plan.scratch(nb_a), s_bs = (presorted || !b) ? -1 : ws.plan.scratch(nb_b);
    if (int rc = ws.stage_in()) return rc;
    const double *da = ws.ptr(s_a), *db = b ? ws.ptr(s_b) : nullptr;
    if (!presorted) {                                               // the row sort of the reduce entry
        if (int rc = enqueue_reduce(ws.ctx->stream, da, CA, K, nullptr, 0, 0.0, nullptr, nullptr, nullptr, nullptr, ws.ptr(s_as))) return rc;
        da = ws.ptr(s_as);
        if (b) {
            if (int rc = enqueue_reduce(ws.ctx->stream, db, CB, K, nullptr, 0, 0.0, nullptr, nullptr, nullptr, nullptr, ws.ptr(s_bs)))
                return rc;
            db = ws.ptr(s_bs);
        }
    }
    if (int rc = rc_wasserstein_matrix_f64_async(device, ws.ctx->stream, p, da, CA, db, CB, K, ws.ptr(s_out))) return rc;
    return ws.stage_out();
}

// ---- batched L-BFGS (ABI 13): the state machine of lbfgs.py, one lane per row (k_lbfgs.inc.h) ----------------------------------
static int check_lbfgs(int ndim, int m, long long C) {
    if (ndim < rclb::kMinDim || ndim > rclb::kMaxDim) return fail(RC_EINVAL, "ndim must be 3 .. 13 (N + 1, N = 2 .. RC_MAX_NSPIN_GRAD)");
    if (m < 1 || m > rclb::kMaxM) return fail(RC_EINVAL, "m must be 1 .. 8");
    if (C < 0) return fail(RC_EINVAL, "C must be non-negative");
    if (C > 0x7fffffffLL) return fail(RC_EINVAL, "too many rows for one launch");
    return RC_OK;
}

long long rc_lbfgs_state_len(long long C, int ndim, int m) {
    if (check_lbfgs(ndim, m, C)) return -1;
    return C * (long long)rclb::Layout{ndim, m}.fields();
}

int rc_lbfgs_init_f64_async(int device, void* stream, int ndim, int m, long long C, const double* x0_dev, const double* mask_dev,
                            double* state_dev, double* trial_dev) {
    if (int rc = check_lbfgs(ndim, m, C)) return rc;
    if (C == 0) return RC_OK;
    if (!state_dev) return fail(RC_EINVAL, "NULL array pointer (state)");
    if (!x0_dev || !trial_dev) return fail(RC_EINVAL, "NULL array pointer (x0, trial)");
    RC_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(lbfgs_init_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, state_dev, trial_dev, x0_dev,
                       mask_dev, C, ndim, m);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_lbfgs_advance_f64_async(int device, void* stream, int ndim, int m, long long C, int kind, double lam, const double* row_a_dev,
                               const double* row_b_dev, double c1, double gtol, double ftol, long long maxiter, long long maxback,
                               double* state_dev, double* trial_dev) {
    if (int rc = check_lbfgs(ndim, m, C)) return rc;
    if (kind < rclb::kRaw || kind > rclb::kOneMinusPlusStd) return fail(RC_EINVAL, "kind must be 0 (raw), 1 (one_minus) or 2 (one_minus_plus_std)");
    if (!(c1 > 0.0 && c1 < 1.0)) return fail(RC_EINVAL, "c1 must be in (0, 1)");
    if (!(gtol >= 0.0) || !(ftol >= 0.0)) return fail(RC_EINVAL, "gtol and ftol must be non-negative");
    if (maxiter < 1 || maxback < 0) return fail(RC_EINVAL, "maxiter must be positive and maxback non-negative");
    if (C == 0) return RC_OK;
    if (!state_dev) return fail(RC_EINVAL, "NULL array pointer (state)");
    if (!row_a_dev || !trial_dev) return fail(RC_EINVAL, "NULL array pointer (row_a, trial)");
    if (kind == rclb::kOneMinusPlusStd && !row_b_dev) return fail(RC_EINVAL, "NULL array pointer (row_b: kind 2 reads the moment rows)");
    RC_HIP_CHECK(hipSetDevice(device));
    LbfgsAdvanceParams p{};
    p.state = state_dev;
    p.trial = trial_dev;
    p.a = row_a_dev;
    p.b = row_b_dev;
    p.C = C;
    p.m = m;
    p.kind = kind;
    p.lam = lam;
    p.opt = rclb::Params{c1, gtol, ftol, maxiter, maxback};
    const dim3 grid((unsigned)((C + 63) / 64));
    hipStream_t s = (hipStream_t)stream;
    switch (ndim) {
#define RC_CASE(n) \
    case n: hipLaunchKernelGGL(lbfgs_advance_kernel<n>, grid, dim3(64), 0, s, p); break;
        RC_CASE(3) RC_CASE(4) RC_CASE(5) RC_CASE(6) RC_CASE(7) RC_CASE(8) RC_CASE(9) RC_CASE(10) RC_CASE(11) RC_CASE(12) RC_CASE(13)
#undef RC_CASE
    }
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

// ---- the boxed variant (ABI 14): box bounds lo <= x <= hi, projected steps; same state, same result entry -------------------------
int rc_lbfgs_init_box_f64_async(int device, void* stream, int ndim, int m, long long C, const double* x0_dev, const double* mask_dev,
                                const double* lo_dev, const double* hi_dev, double* state_dev, double* trial_dev) {
    if (int rc = check_lbfgs(ndim, m, C)) return rc;
    if (!lo_dev || !hi_dev) return fail(RC_EINVAL, "NULL array pointer (lo, hi: the boxed entries need both bounds)");
    if (C == 0) return RC_OK;
    if (!state_dev) return fail(RC_EINVAL, "NULL array pointer (state)");
    if (!x0_dev || !trial_dev) return fail(RC_EINVAL, "NULL array pointer (x0, trial)");
    RC_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(lbfgs_init_box_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, state_dev, trial_dev,
                       x0_dev, mask_dev, lo_dev, hi_dev, C, ndim, m);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_lbfgs_advance_box_f64_async(int device, void* stream, int ndim, int m, long long C, int kind, double lam, const double* row_a_dev,
                                   const double* row_b_dev, const double* lo_dev, const double* hi_dev, double c1, double gtol,
                                   double ftol, long long maxiter, long long maxback, double* state_dev, double* trial_dev) {
    if (int rc = check_lbfgs(ndim, m, C)) return rc;
    if (kind < rclb::kRaw || kind > rclb::kOneMinusPlusStd) return fail(RC_EINVAL, "kind must be 0 (raw), 1 (one_minus) or 2 (one_minus_plus_std)");
    if (!(c1 > 0.0 && c1 < 1.0)) return fail(RC_EINVAL, "c1 must be in (0, 1)");
    if (!(gtol >= 0.0) || !(ftol >= 0.0)) return fail(RC_EINVAL, "gtol and ftol must be non-negative");
    if (maxiter < 1 || maxback < 0) return fail(RC_EINVAL, "maxiter must be positive and maxback non-negative");
    if (!lo_dev || !hi_dev) return fail(RC_EINVAL, "NULL array pointer (lo, hi: the boxed entries need both bounds)");
    if (C == 0) return RC_OK;
    if (!state_dev) return fail(RC_EINVAL, "NULL array pointer (state)");
    if (!row_a_dev || !trial_dev) return fail(RC_EINVAL, "NULL array pointer (row_a, trial)");
    if (kind == rclb::kOneMinusPlusStd && !row_b_dev) return fail(RC_EINVAL, "NULL array pointer (row_b: kind 2 reads the moment rows)");
    RC_HIP_CHECK(hipSetDevice(device));
    LbfgsAdvanceBoxParams p{};
    p.adv.state = state_dev;
    p.adv.trial = trial_dev;
    p.adv.a = row_a_dev;
    p.adv.b = row_b_dev;
    p.adv.C = C;
    p.adv.m = m;
    p.adv.kind = kind;
    p.adv.lam = lam;
    p.adv.opt = rclb::Params{c1, gtol, ftol, maxiter, maxback};
    p.lo = lo_dev;
    p.hi = hi_dev;
    const dim3 grid((unsigned)((C + 63) / 64));
    hipStream_t s = (hipStream_t)stream;
    switch (ndim) {
#define RC_CASE(n) \
    case n: hipLaunchKernelGGL(lbfgs_advance_box_kernel<n>, grid, dim3(64), 0, s, p); break;
        RC_CASE(3) RC_CASE(4) RC_CASE(5) RC_CASE(6) RC_CASE(7) RC_CASE(8) RC_CASE(9) RC_CASE(10) RC_CASE(11) RC_CASE(12) RC_CASE(13)
#undef RC_CASE
    }
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_lbfgs_result_f64_async(int device, void* stream, int ndim, int m, long long C, const double* state_dev, double* x_out_dev,
                              double* f_out_dev, double* g_out_dev, int* status_out_dev, long long* iters_out_dev,
                              long long* evals_out_dev) {
    if (int rc = check_lbfgs(ndim, m, C)) return rc;
    if (!x_out_dev && !f_out_dev && !g_out_dev && !status_out_dev && !iters_out_dev && !evals_out_dev)
        return fail(RC_EINVAL, "no output requested (x_out, f_out, g_out, status_out, iters_out and evals_out are all NULL)");
    if (C == 0) return RC_OK;
    if (!state_dev) return fail(RC_EINVAL, "NULL array pointer (state)");
    RC_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(lbfgs_result_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, state_dev, C, ndim, m,
                       x_out_dev, f_out_dev, g_out_dev, status_out_dev, iters_out_dev, evals_out_dev);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_mc_fidelity_philox_f64_async(int device, void* stream, int kernel, int N, int in, int out, const double* h0_diag,
                                    const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                    unsigned long long offset, double sigma, const double* sigma_rows_dev, long long C,
                                    long long K, double* fid_out_dev) {
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers_dev || !fid_out_dev) return fail(RC_EINVAL, "NULL array pointer");
    if (N > RC_MAX_NSPIN_FAST) return fail(RC_ENOSUP, "draws generated in the fidelity kernel: N <= 16 (longer chains: rc_draws_philox_f64_async + rc_mc_fidelity_f64_async)");
    if (kernel != RC_KERNEL_AUTO && kernel != RC_KERNEL_TRIDIAG_ADJ)
        return fail(RC_ENOSUP, "draws generated in the fidelity kernel: the eigenvalue-only chain kernels only (RC_KERNEL_AUTO / RC_KERNEL_TRIDIAG_ADJ)");
    RC_HIP_CHECK(hipSetDevice(device));
    const bool ends = (in == 0 && out == N - 1) || (in == N - 1 && out == 0);
    FidParams p{};
    p.ctrl = controllers_dev;
    p.draws = nullptr;
    p.fid = fid_out_dev;
    p.C = C;
    p.K = K;
    p.draw_cstride = 0;
    p.tiles_per_ctrl = (K + 63) / 64;
    p.ntiles = C * p.tiles_per_ctrl;
    p.in = in;
    p.out = out;
    p.align16 = 0;
    // (no store rule here: the fused kernel has no draw stream for the non-temporal store to protect, and its A/B with the rule
    // on and off read 0.994 .. 1.009 at N = 5, 7, 10 and 25 .. 1 000 controllers - profiles/launch_boundary_ab.txt section 4)
    fill_h0(p.h0, N, h0_diag, h0_offdiag);
    PhiloxDraws q{seed, offset, sigma_rows_dev, sigma};
    hipStream_t s = (hipStream_t)stream;
    switch (N) {
#define RC_CASE(n) \
    case n: return (ends && n <= 14) ? launch_chain_philox<n, rc::kWeightsEnds>(s, p, q)  /* (same choice as enqueue_fidelity: bit-identical) */ \
                                     : launch_chain_philox<n, rc::kWeightsAdjugate>(s, p, q);
#ifdef RC_DEV_FEW_N
        RC_CASE(5) RC_CASE(7) RC_CASE(10)
#else
        RC_CASE(2) RC_CASE(3) RC_CASE(4) RC_CASE(5) RC_CASE(6) RC_CASE(7) RC_CASE(8) RC_CASE(9)
        RC_CASE(10) RC_CASE(11) RC_CASE(12) RC_CASE(13) RC_CASE(14) RC_CASE(15) RC_CASE(16)
#endif
#undef RC_CASE
    }
    return fail(RC_EINVAL, "unsupported N");
}

// ---- randomised quasi-Monte Carlo (ABI 19): scrambled Sobol points, code-robchar_amd/sobol.py is the definition -----------------
int rc_sobol_dirnum_u32(int D, unsigned int* out_host) {
    if (D < 1 || D > RC_SOBOL_MAX_DIM) return fail(RC_EINVAL, "D must be in [1, 96]");
    if (!out_host) return fail(RC_EINVAL, "NULL output pointer");
    memcpy(out_host, kSobolJoeKuo96, (size_t)D * 32 * sizeof(unsigned int));
    return RC_OK;
}

// the contract of sobol.py, in its order; fills `q`
static int check_sobol(int D, const unsigned int* dirnum, const unsigned int* shift, long long shift_cstride, int R, long long P,
                       long long skip, double sigma, const double* sigma_rows, long long C, long long K, rckp::SobolDraws* q) {
    if (D < 1 || D > RC_SOBOL_MAX_DIM) return fail(RC_EINVAL, "D must be in [1, 96]");
    if (C < 0 || K < 0) return fail(RC_EINVAL, "C and K must be non-negative");
    if (R < 1 || P < 1) return fail(RC_EINVAL, "R and P must be positive");
    if (P > (1LL << 32)) return fail(RC_EINVAL, "P must not exceed 2^32");
    if (K > (long long)R * P) return fail(RC_EINVAL, "K must not exceed R P");
    if (skip < 0 || skip % 64 != 0) return fail(RC_EINVAL, "skip must be a non-negative multiple of 64");
    if (R > 1 && P % 64 != 0) return fail(RC_EINVAL, "P must be a multiple of 64 when R > 1");
    if (skip + (P < K ? P : K) > (1LL << 32)) return fail(RC_EINVAL, "skip + min(P, K) must not exceed 2^32");
    if (shift_cstride != 0 && shift_cstride != (long long)R * D) return fail(RC_EINVAL, "shift_cstride must be 0 or R D");
    *q = rckp::SobolDraws{dirnum, shift, shift_cstride, P, (unsigned long long)skip, sigma_rows, sigma, R, D};
    return RC_OK;
}

int rc_draws_sobol_f64_async(int device, void* stream, int D, const unsigned int* dirnum_dev, const unsigned int* shift_dev,
                             long long shift_cstride, int R, long long P, long long skip, double sigma, const double* sigma_rows_dev,
                             long long C, long long K, double* draws_out_dev, unsigned int* bits_out_dev) {
    rckp::SobolDraws q;
    if (int rc = check_sobol(D, dirnum_dev, shift_dev, shift_cstride, R, P, skip, sigma, sigma_rows_dev, C, K, &q)) return rc;
    if (!draws_out_dev && !bits_out_dev) return fail(RC_EINVAL, "no output requested (draws_out and bits_out are both NULL)");
    if (C == 0 || K == 0) return RC_OK;
    if (!dirnum_dev || !shift_dev) return fail(RC_EINVAL, "NULL array pointer");
    if (C * ((K + 63) / 64) > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
    RC_HIP_CHECK(hipSetDevice(device));
    const hipError_t e = (hipError_t)rc_qmc_draws_launch(stream, &q, C, K, draws_out_dev, bits_out_dev);
    if (e != hipSuccess) return fail(RC_EHIP, std::string("rc_qmc_draws_launch: ") + hipGetErrorString(e));
    return RC_OK;
}

int rc_draws_sobol_f64(int device, int D, const unsigned int* dirnum, const unsigned int* shift, long long shift_cstride, int R,
                       long long P, long long skip, double sigma, const double* sigma_rows, long long C, long long K,
                       double* draws_out, unsigned int* bits_out) {
    rckp::SobolDraws q;
    if (int rc = check_sobol(D, dirnum, shift, shift_cstride, R, P, skip, sigma, sigma_rows, C, K, &q)) return rc;
    if (!draws_out && !bits_out) return fail(RC_EINVAL, "no output requested (draws_out and bits_out are both NULL)");
    if (C == 0 || K == 0) return RC_OK;
    if (!dirnum || !shift) return fail(RC_EINVAL, "NULL array pointer");
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t n = (size_t)C * K * D;
    const int s_dir = ws.in(dirnum, (size_t)R * D * 32 * sizeof(unsigned int)),
              s_shift = ws.in(shift, (size_t)(shift_cstride ? C : 1) * R * D * sizeof(unsigned int)),
              s_rows = sigma_rows ? ws.in(sigma_rows, (size_t)C * sizeof(double)) : -1,
              s_draws = ws.out(draws_out, n * sizeof(double)), s_bits = ws.out(bits_out, n * sizeof(unsigned int));
    if (int rc = ws.stage_in()) return rc;
    if (int rc = rc_draws_sobol_f64_async(device, ws.ctx->stream, D, (const unsigned int*)ws.ptr(s_dir), (const unsigned int*)ws.ptr(s_shift),
                                          shift_cstride, R, P, skip, sigma, s_rows >= 0 ? ws.ptr(s_rows) : nullptr, C, K,
                                          ws.ptr(s_draws), (unsigned int*)ws.ptr(s_bits)))
        return rc;
    return ws.stage_out();
}

int rc_mc_fidelity_sobol_f64_async(int device, void* stream, int kernel, int N, int in, int out, const double* h0_diag,
                                   const double* h0_offdiag, const double* controllers_dev, const unsigned int* dirnum_dev,
                                   const unsigned int* shift_dev, long long shift_cstride, int R, long long P, long long skip,
                                   double sigma, const double* sigma_rows_dev, long long C, long long K, double* fid_out_dev) {
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (N > RC_MAX_NSPIN_SOBOL)
        return fail(RC_ENOSUP, "Sobol points generated in the fidelity kernel: N <= 13 (longer chains: the two-kernel route, "
                               "rc_draws_sobol_f64_async + rc_mc_fidelity_f64_async)");
    if (kernel != RC_KERNEL_AUTO && kernel != RC_KERNEL_TRIDIAG_ADJ)
        return fail(RC_ENOSUP, "Sobol points generated in the fidelity kernel: the eigenvalue-only chain kernels only (RC_KERNEL_AUTO / "
                               "RC_KERNEL_TRIDIAG_ADJ; others: the two-kernel route, rc_draws_sobol_f64_async + rc_mc_fidelity_f64_async)");
    rckp::SobolDraws q;
    if (int rc = check_sobol(3 * N, dirnum_dev, shift_dev, shift_cstride, R, P, skip, sigma, sigma_rows_dev, C, K, &q)) return rc;
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers_dev || !dirnum_dev || !shift_dev || !fid_out_dev) return fail(RC_EINVAL, "NULL array pointer");
    FidParams p{};
    p.ctrl = controllers_dev;
    p.draws = nullptr;
    p.fid = fid_out_dev;
    p.C = C;
    p.K = K;
    p.draw_cstride = 0;
    p.tiles_per_ctrl = (K + 63) / 64;
    p.ntiles = C * p.tiles_per_ctrl;
    p.in = in;
    p.out = out;
    p.align16 = 0;
    if (p.ntiles > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
    RC_HIP_CHECK(hipSetDevice(device));
    fill_h0(p.h0, N, h0_diag, h0_offdiag);
    const bool ends = (in == 0 && out == N - 1) || (in == N - 1 && out == 0);     // (same choice as enqueue_fidelity: bit-identical)
    const hipError_t e = (hipError_t)rc_qmc_fidelity_launch(N, ends ? 1 : 0, stream, &p, &q);
    if (e != hipSuccess) return fail(RC_EHIP, std::string("rc_qmc_fidelity_launch: ") + hipGetErrorString(e));
    return RC_OK;
}

// ---- variance indices (ABI 20): the pick-freeze kernel, code-robchar_amd/variance_indices.py is the definition --------------------
int rc_mc_fidelity_pickfreeze_philox_f64_async(int device, void* stream, int kernel, int N, int in, int out, const double* h0_diag,
                                               const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                               unsigned long long offset_a, unsigned long long offset_b, double sigma,
                                               const double* sigma_rows_dev, const unsigned long long* groups, int G, long long C,
                                               long long K, double* fid_out_dev, double* mean_out_dev) {
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (N > RC_MAX_NSPIN_PICKFREEZE)
        return fail(RC_ENOSUP, "pick-freeze kernel: N <= 13 (longer chains: rc_draws_philox_f64_async, the hybrids and "
                               "rc_mc_fidelity_f64_async, with variance_indices.py on their outputs)");
    if (kernel != RC_KERNEL_AUTO && kernel != RC_KERNEL_TRIDIAG_ADJ)
        return fail(RC_ENOSUP, "pick-freeze kernel: the eigenvalue-only chain kernels only (RC_KERNEL_AUTO / RC_KERNEL_TRIDIAG_ADJ)");
    if (G < 0 || G > RC_PICKFREEZE_MAX_GROUPS) return fail(RC_EINVAL, "G must be in [0, 64]");
    if (G > 0 && !groups) return fail(RC_EINVAL, "NULL array pointer (groups)");
    for (int g = 0; g < G; ++g)
        if (groups[g] >> (3 * N))
            return fail(RC_EINVAL, "group " + std::to_string(g) + ": a mask bit at or above 3 N = " + std::to_string(3 * N));
    if (!sigma_rows_dev && !(sigma >= 0.0 && sigma < HUGE_VAL))
        return fail(RC_EINVAL, "sigma must be finite and non-negative (or give sigma_rows)");
    // the two element ranges [offset, offset + C K 3N) as distances modulo 2^64 (a wrapping offset is legal)
    const unsigned long long len = (unsigned long long)C * (unsigned long long)K * (unsigned long long)(3 * N);
    if (len && (offset_b - offset_a < len || offset_a - offset_b < len))
        return fail(RC_EINVAL, "the element ranges of offset_a and offset_b overlap (each covers C K 3N elements)");
    if (!fid_out_dev && !mean_out_dev) return fail(RC_EINVAL, "no output requested (fid_out and mean_out are both NULL)");
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers_dev) return fail(RC_EINVAL, "NULL array pointer (controllers)");
    rckp::PickFreezeParams p{};
    fill_deriv_params(p, N, in, out, h0_diag, h0_offdiag, controllers_dev, C, K, fid_out_dev);
    if (p.ntiles > 0x7fffffffLL) return fail(RC_EINVAL, "too many tiles for one launch");
    p.G = G;
    p.seed = seed;
    p.offset_a = offset_a;
    p.offset_b = offset_b;
    p.sigma_rows = sigma_rows_dev;
    p.sigma = sigma;
    for (int g = 0; g < G; ++g) p.groups[g] = groups[g];
    RC_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const bool ends = (in == 0 && out == N - 1) || (in == N - 1 && out == 0);     // (same choice as enqueue_fidelity: bit-identical)
    return launch_with_part(s, p, mean_out_dev != nullptr, 3 + 2 * G, "rc_vidx_pickfreeze_launch",
                            [&] { return rc_vidx_pickfreeze_launch(N, ends ? 1 : 0, (void*)s, &p, mean_out_dev); });
}

int rc_mc_fidelity_nh_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                const double* h0_offdiag, int ring, const double* controllers_dev,
                                const double* draws_dev, const double* diag_imag_dev, long long C, long long K,
                                double* fid_out_dev) {
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers_dev || !draws_dev || !fid_out_dev) return fail(RC_EINVAL, "NULL array pointer");
    RC_HIP_CHECK(hipSetDevice(device));
    // (RC_NH_EXPM_ONLY=1 in the environment: the dense Pade-expm kernel for every sample - the cross-check of the
    // complex symmetric QL route)
    const char* nh_env = getenv("RC_NH_EXPM_ONLY");
    const bool expm_only = nh_env && nh_env[0] == '1';
    return enqueue_expm((hipStream_t)stream, N, in, out, h0_diag, h0_offdiag, ring, controllers_dev, draws_dev,
                        K * N * 3, diag_imag_dev, K * N, C, K, fid_out_dev, !expm_only);
}

int rc_mc_fidelity_directional_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                         const double* h0_offdiag, int ring, const double* controllers_dev,
                                         const int* idx_dev, const double* ab_dev, long long C, long long K,
                                         double* fid_out_dev) {
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (ring && N > 2) return fail(RC_ENOSUP, "the directional entry handles chain topology (rings: the dense layout + rc_mc_fidelity_nh_f64_async)");
    if (N > kDirMaxN) return fail(RC_ENOSUP, "the directional entry supports N <= 12 (above: the dense layout + rc_mc_fidelity_nh_f64_async)");
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers_dev || !idx_dev || !ab_dev || !fid_out_dev) return fail(RC_EINVAL, "NULL array pointer");
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_directional((hipStream_t)stream, N, in, out, h0_diag, h0_offdiag, controllers_dev, idx_dev, ab_dev, C, K,
                               fid_out_dev);
}

int rc_mc_fidelity_f64(int device, int N, int in, int out, const double* h0_diag,
                       const double* h0_offdiag, int ring, const double* controllers, const double* draws,
                       long long C, long long K, double* fid_out) {
    int kernel;
    {
        std::lock_guard<std::mutex> lk(g_cfg_mu);
        kernel = g_default_kernel;
    }
    return rc_mc_fidelity_kernel_f64(device, kernel, N, in, out, h0_diag, h0_offdiag, ring, controllers, draws, C, K,
                                     fid_out);
}

int rc_mc_fidelity_kernel_f64(int device, int kernel, int N, int in, int out, const double* h0_diag,
                              const double* h0_offdiag, int ring, const double* controllers, const double* draws,
                              long long C, long long K, double* fid_out) {
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers || !draws || !fid_out) return fail(RC_EINVAL, "NULL array pointer");
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t nb_fid = (size_t)C * K * sizeof(double);
    const int s_ctrl = ws.in(controllers, (size_t)C * (N + 1) * sizeof(double)), s_draw = ws.in(draws, nb_fid * N * 3),
              s_fid = ws.out(fid_out, nb_fid);
    if (int rc = ws.stage_in()) return rc;
    if (int rc = enqueue_fidelity(ws.ctx->stream, kernel, N, in, out, h0_diag, h0_offdiag, ring, ws.ptr(s_ctrl), ws.ptr(s_draw), -1, C,
                                  K, ws.ptr(s_fid)))
        return rc;
    return ws.stage_out();
}

int rc_reduce_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K,
                        const double* q_thresholds, int nq, double dkw_eps, double* rim1_dev,
                        double* std_dev, double* minf_dev, double* q_dev, double* sorted_out_dev) {
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_reduce((hipStream_t)stream, fid_dev, C, K, q_thresholds, nq, dkw_eps, rim1_dev, std_dev,
                          minf_dev, q_dev, sorted_out_dev);
}

int rc_reduce_ex_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K,
                           const double* q_thresholds, int nq, double dkw_eps, double* rim1_dev, double* std_dev,
                           double* minf_dev, double* q_dev, double* sorted_out_dev, int flags) {
    if (flags & ~RC_REDUCE_STANDALONE) return fail(RC_EINVAL, "unknown reduction flag");
    RC_HIP_CHECK(hipSetDevice(device));
    return enqueue_reduce((hipStream_t)stream, fid_dev, C, K, q_thresholds, nq, dkw_eps, rim1_dev, std_dev, minf_dev, q_dev,
                          sorted_out_dev, (flags & RC_REDUCE_STANDALONE) != 0);
}

int rc_reduce_f64(int device, const double* fid, long long C, long long K, const double* q_thresholds,
                  int nq, double dkw_eps, double* rim1, double* std_, double* minf, double* q,
                  double* sorted_out) {
    if (C < 0 || K < 0) return fail(RC_EINVAL, "C and K must be non-negative");
    if (nq < 0 || nq > kMaxQ) return fail(RC_EINVAL, "nq must be in [0, 8]");
    if (C == 0) return RC_OK;
    if (!fid) return fail(RC_EINVAL, "NULL fid pointer");
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const size_t nb_fid = (size_t)C * K * sizeof(double), nb_c3 = (size_t)3 * C * sizeof(double);
    // the metric rows are always staged (they are small), the sorted tensor only when it is a host pointer
    const int s_fid = ws.in(fid, nb_fid), s_rim = ws.out(rim1, nb_c3, true), s_std = ws.out(std_, nb_c3, true),
              s_min = ws.out(minf, nb_c3, true), s_q = ws.out(nq ? q : nullptr, nb_c3 * nq, true), s_sorted = ws.out(sorted_out, nb_fid);
    if (int rc = ws.stage_in()) return rc;
    if (int rc = enqueue_reduce(ws.ctx->stream, ws.ptr(s_fid), C, K, q_thresholds, nq, dkw_eps, ws.ptr(s_rim), ws.ptr(s_std),
                                ws.ptr(s_min), ws.ptr(s_q), ws.ptr(s_sorted), /*standalone=*/true))
        return rc;
    return ws.stage_out();
}

int rc_rim_p_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K, double p,
                       double* out_dev) {
    if (C < 0 || K <= 0) return fail(RC_EINVAL, "C must be >= 0 and K > 0");
    if (!(p > 0.0)) return fail(RC_EINVAL, "p must be positive (RIM_0 = 1 is a host constant)");
    if (C == 0) return RC_OK;
    if (!fid_dev || !out_dev) return fail(RC_EINVAL, "NULL array pointer");
    if (C > 0x7fffffffLL) return fail(RC_EINVAL, "too many controllers for one launch");
    RC_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(rim_p_kernel, dim3((unsigned)C), dim3(kRedThreads), 0, (hipStream_t)stream, fid_dev, C, K,
                       p, out_dev);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_rim_p_f64(int device, const double* fid, long long C, long long K, double p, double* out) {
    if (C < 0 || K <= 0) return fail(RC_EINVAL, "C must be >= 0 and K > 0");
    if (!(p > 0.0)) return fail(RC_EINVAL, "p must be positive (RIM_0 = 1 is a host constant)");
    if (C == 0) return RC_OK;
    if (!fid || !out) return fail(RC_EINVAL, "NULL array pointer");
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const int s_fid = ws.in(fid, (size_t)C * K * sizeof(double)), s_out = ws.out(out, (size_t)C * sizeof(double), true);
    if (int rc = ws.stage_in()) return rc;
    if (int rc = rc_rim_p_f64_async(device, ws.ctx->stream, ws.ptr(s_fid), C, K, p, ws.ptr(s_out))) return rc;
    return ws.stage_out();
}

int rc_draws_philox_f64_async(int device, void* stream, unsigned long long seed, unsigned long long offset,
                              long long n, double scale, double* out_dev) {
    if (n < 0) return fail(RC_EINVAL, "n must be non-negative");
    if (n == 0) return RC_OK;
    if (!out_dev) return fail(RC_EINVAL, "NULL output pointer");
    RC_HIP_CHECK(hipSetDevice(device));
    long long blocks = (n / 2 + 1 + 255) / 256;               // one thread per Box-Muller pair
    if (blocks > 256LL * 32) blocks = 256LL * 32;
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, seed, offset,
                       n, scale, out_dev);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_draws_philox_f64(int device, unsigned long long seed, unsigned long long offset, long long n, double scale,
                        double* out) {
    if (n < 0) return fail(RC_EINVAL, "n must be non-negative");
    if (n == 0) return RC_OK;
    if (!out) return fail(RC_EINVAL, "NULL output pointer");
    if (int rc = device_in_range(device)) return rc;
    std::lock_guard<std::mutex> lk(g_ctx[device].mu);
    Staging ws;
    if (int rc = get_ctx(device, &ws.ctx)) return rc;
    const int s_out = ws.out(out, (size_t)n * sizeof(double));
    if (int rc = ws.stage_in()) return rc;
    if (int rc = rc_draws_philox_f64_async(device, ws.ctx->stream, seed, offset, n, scale, ws.ptr(s_out))) return rc;
    return ws.stage_out();
}

int rc_mc_fidelity_sharded_f64(int ndev, const int* devices, int kernel, int N, int in, int out, const double* h0_diag,
                               const double* h0_offdiag, int ring, const double* controllers, const double* draws,
                               long long C, long long K, double* fid_out) {
    if (C > 0 && K > 0 && (!draws || !fid_out)) return fail(RC_EINVAL, "NULL array pointer");
    ShardJob j{};
    j.kernel = kernel; j.N = N; j.in = in; j.out = out; j.ring = ring;
    j.h0d = h0_diag; j.h0o = h0_offdiag; j.ctrl = controllers; j.draws = draws;
    j.C = C; j.K = K; j.fid_out = fid_out;
    return run_sharded(ndev, devices, j);
}

int rc_mc_metrics_sharded_f64(int ndev, const int* devices, int kernel, int N, int in, int out, const double* h0_diag,
                              const double* h0_offdiag, int ring, const double* controllers, const double* draws,
                              unsigned long long philox_seed, unsigned long long philox_offset, double sigma,
                              long long C, long long K, const double* q_thresholds, int nq, double dkw_eps,
                              double* rim1, double* std_, double* minf, double* q, double* fid_out) {
    ShardJob j{};
    j.kernel = kernel; j.N = N; j.in = in; j.out = out; j.ring = ring;
    j.h0d = h0_diag; j.h0o = h0_offdiag; j.ctrl = controllers; j.draws = draws;
    j.seed = philox_seed; j.offset = philox_offset; j.sigma = sigma;
    j.C = C; j.K = K; j.thr = q_thresholds; j.nq = nq; j.eps = dkw_eps;
    j.rim1 = rim1; j.stdv = std_; j.minf = minf; j.q = q; j.fid_out = fid_out;
    return run_sharded(ndev, devices, j);
}

int rc_comm_init(int ndev, const int* devices, rc_comm** comm_out) {
    if (!comm_out) return fail(RC_EINVAL, "NULL communicator pointer");
    *comm_out = nullptr;
    if (ndev < 1 || ndev > kMaxDevices) return fail(RC_EINVAL, "ndev must be in [1, 64]");
    std::vector<int> devs(ndev);
    for (int r = 0; r < ndev; ++r) {
        devs[r] = devices ? devices[r] : r;
        if (int rc = device_in_range(devs[r])) return rc;
        for (int r2 = 0; r2 < r; ++r2)
            if (devs[r2] == devs[r]) return fail(RC_EINVAL, "a device is listed twice (RCCL needs one rank per device)");
    }
    const RcclApi& a = rccl_api();
    if (!a.ok) return fail(RC_ENOSUP, "librccl.so not found (looked in the process, then for librccl.so.1 / librccl.so)");
    auto* c = new rc_comm;
    c->ndev = ndev;
    c->devices = devs;
    c->comms.assign(ndev, nullptr);
    if (int e = a.init_all(c->comms.data(), ndev, devs.data())) {
        delete c;
        return rccl_fail(e, "ncclCommInitAll");
    }
    *comm_out = c;
    return RC_OK;
}

int rc_comm_size(const rc_comm* comm) { return comm ? comm->ndev : 0; }

int rc_comm_destroy(rc_comm* comm) {
    if (!comm) return RC_OK;
    const RcclApi& a = rccl_api();
    int bad = 0;
    for (void* c : comm->comms)
        if (c && a.destroy) bad |= a.destroy(c);
    delete comm;
    return bad ? rccl_fail(bad, "ncclCommDestroy") : RC_OK;
}

int rc_mc_metrics_gathered_f64(rc_comm* comm, int kernel, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                               int ring, const double* controllers, const double* draws, unsigned long long philox_seed,
                               unsigned long long philox_offset, double sigma, long long C, long long K,
                               const double* q_thresholds, int nq, double dkw_eps, double* const* table_dev,
                               double* const* fid_dev, double* table_host, double* fid_host) {
    if (!comm) return fail(RC_EINVAL, "NULL communicator");
    if (int rc = check_common(N, in, out, C, K)) return rc;
    if (nq < 0 || nq > kMaxQ) return fail(RC_EINVAL, "nq must be in [0, 8]");
    if (nq > 0 && !q_thresholds) return fail(RC_EINVAL, "q_thresholds is NULL");
    if (C == 0 || K == 0) return RC_OK;
    if (!controllers) return fail(RC_EINVAL, "NULL controllers pointer");
    const RcclApi& a = rccl_api();
    const int ndev = comm->ndev;
    // (a fidelity gather needs a receive buffer on EVERY rank of the collective: asked for before any work is enqueued)
    if (fid_host && !fid_dev && ndev > 1)
        return fail(RC_EINVAL, "fid_host with more than one device needs fid_dev (a receive buffer on every device)");
    const long long Cmax = (C + ndev - 1) / ndev, G = 3LL * N;
    const int NR = 9 + 3 * nq;
    // per device: send buffers (own share) + - unless the caller provides them - the gathered buffers
    struct Bufs {
        double *ctrl = nullptr, *draw = nullptr, *fid = nullptr, *tab = nullptr, *tab_all = nullptr, *fid_all = nullptr;
        bool own_tab = false, own_fid = false;
    };
    std::vector<Bufs> b(ndev);
    GatherJob proto{};
    proto.kernel = kernel; proto.N = N; proto.in = in; proto.out = out; proto.ring = ring;
    proto.h0d = h0_diag; proto.h0o = h0_offdiag; proto.ctrl = controllers; proto.draws = draws;
    proto.seed = philox_seed; proto.offset = philox_offset; proto.sigma = sigma;
    proto.C = C; proto.K = K; proto.Cmax = Cmax; proto.thr = q_thresholds; proto.nq = nq; proto.eps = dkw_eps;
    std::vector<GatherJob> jobs(ndev, proto);
    const bool fused = philox_fused_route(draws, ring, kernel, N, in, out);     // then no draw buffer: enqueue_share goes by that
    const bool want_fid = fid_dev || fid_host;
    const long long base = C / ndev, extra = C % ndev;
    long long start = 0;
    int rc_all = RC_OK;
    // (plain hipMalloc / hipFree, not the stream-ordered pool: the call is blocking anyway, and a process that had used
    // hipMallocAsync here and then created another stream - torch.cuda.Stream() in a later test - ended in glibc's "double free
    // or corruption" inside the runtime's exit handlers on ROCm 7.2)
    auto cleanup = [&]() {                          // the call is blocking: every stream is drained, then the buffers go
        for (int r = 0; r < ndev; ++r) {
            if (hipSetDevice(comm->devices[r]) != hipSuccess) continue;
            (void)hipStreamSynchronize(g_ctx[comm->devices[r]].stream);
            for (double* p : {b[r].ctrl, b[r].draw, b[r].fid, b[r].tab}) if (p) (void)hipFree(p);
            if (b[r].own_tab && b[r].tab_all) (void)hipFree(b[r].tab_all);
            if (b[r].own_fid && b[r].fid_all) (void)hipFree(b[r].fid_all);
        }
    };
    for (int r = 0; r < ndev && rc_all == RC_OK; ++r) {
        const int dev = comm->devices[r];
        DeviceCtx* ctx = nullptr;
        {
            std::lock_guard<std::mutex> lk(g_ctx[dev].mu);
            if (int rc = get_ctx(dev, &ctx)) { rc_all = rc; break; }
        }
        hipStream_t st = ctx->stream;
        GatherJob& j = jobs[r];
        j.device = dev;
        j.c0 = start;
        start += base + (r < extra ? 1 : 0);
        j.c1 = start;
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) e = hipMalloc((void**)&b[r].ctrl, (size_t)Cmax * (N + 1) * sizeof(double));
        if (e == hipSuccess && !fused) e = hipMalloc((void**)&b[r].draw, (size_t)Cmax * K * G * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&b[r].fid, (size_t)Cmax * K * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&b[r].tab, (size_t)NR * Cmax * sizeof(double));
        b[r].tab_all = table_dev ? table_dev[r] : nullptr;
        if (e == hipSuccess && !b[r].tab_all) {
            e = hipMalloc((void**)&b[r].tab_all, (size_t)ndev * NR * Cmax * sizeof(double));
            b[r].own_tab = true;
        }
        b[r].fid_all = fid_dev ? fid_dev[r] : nullptr;
        if (e == hipSuccess && want_fid && !b[r].fid_all && (fid_dev || r == 0)) {      // a host copy only needs device 0's
            e = hipMalloc((void**)&b[r].fid_all, (size_t)ndev * Cmax * K * sizeof(double));
            b[r].own_fid = true;
        }
        if (e != hipSuccess) rc_all = fail(RC_EHIP, std::string("rc_mc_metrics_gathered_f64 (allocation): ") + hipGetErrorString(e));
        j.d_ctrl = b[r].ctrl; j.d_draw = b[r].draw; j.d_fid = b[r].fid; j.d_tab = b[r].tab;
    }
    if (rc_all) {
        cleanup();
        return rc_all;
    }
    // every device computes and reduces its share (one host thread per device, everything enqueued on the device's stream) ...
    {
        std::vector<std::thread> th;
        for (int r = 1; r < ndev; ++r) th.emplace_back(run_gather_share_locked, &jobs[r]);
        run_gather_share_locked(&jobs[0]);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < ndev; ++r)
        if (jobs[r].rc) {
            rc_all = fail(jobs[r].rc, "device " + std::to_string(jobs[r].device) + ": " + jobs[r].err);
            break;
        }
    // ... and the exchange step: ONE group of all-gathers, each on its device's stream behind that device's kernels.  A fidelity
    // gather needs a receive buffer on EVERY rank of the collective: without fid_dev only device 0 has one, so the slabs are
    // gathered only when every device has (fid_dev given), otherwise device 0's own slab + peers' come through table only.
    const bool gather_fid = want_fid && (fid_dev != nullptr || ndev == 1);
    if (rc_all == RC_OK) {
        int e = a.group_start();
        for (int r = 0; r < ndev && !e; ++r) {
            hipStream_t st = g_ctx[comm->devices[r]].stream;
            e = a.allgather(b[r].tab, b[r].tab_all, (size_t)NR * Cmax, kNcclFloat64, comm->comms[r], st);
            if (!e && gather_fid) e = a.allgather(b[r].fid, b[r].fid_all, (size_t)Cmax * K, kNcclFloat64, comm->comms[r], st);
        }
        const int e2 = a.group_end();
        if (e || e2) rc_all = rccl_fail(e ? e : e2, "ncclAllGather");
    }
    // host copies from device 0's gathered buffers, padding dropped: table_host [NR][C], fid_host [C][K]
    if (rc_all == RC_OK && (table_host || (fid_host && gather_fid))) {
        const int dev0 = comm->devices[0];
        hipStream_t st = g_ctx[dev0].stream;
        hipError_t e = hipSetDevice(dev0);
        long long c_at = 0;
        for (int r = 0; r < ndev && e == hipSuccess; ++r) {
            const long long cl = jobs[r].c1 - jobs[r].c0;
            if (cl > 0 && table_host)
                e = hipMemcpy2DAsync(table_host + c_at, (size_t)C * sizeof(double), b[0].tab_all + (size_t)r * NR * Cmax,
                                     (size_t)Cmax * sizeof(double), (size_t)cl * sizeof(double), NR, hipMemcpyDeviceToHost, st);
            if (cl > 0 && fid_host && gather_fid && e == hipSuccess)
                e = hipMemcpyAsync(fid_host + c_at * K, b[0].fid_all + (size_t)r * Cmax * K, (size_t)cl * K * sizeof(double),
                                   hipMemcpyDeviceToHost, st);
            c_at += cl;
        }
        if (e != hipSuccess) rc_all = fail(RC_EHIP, std::string("rc_mc_metrics_gathered_f64 (copy to the host): ") + hipGetErrorString(e));
    }
    cleanup();                                        // drains every stream first: results (device and host) are complete on return
    return rc_all;
}

int rc_draws_legacy_f64(int device, void* stream, rc_mt19937_state* state, long long n_periods, long long period,
                        long long skip, const double* scales, double* out_dev) {
    if (!state) return fail(RC_EINVAL, "NULL generator state");
    if (state->pos < 0 || state->pos > 624) return fail(RC_EINVAL, "generator state: pos must be in [0, 624]");
    if (n_periods < 0 || period < 0 || skip < 0 || skip > period) return fail(RC_EINVAL, "need n_periods, period >= 0 and 0 <= skip <= period");
    if (n_periods == 0 || period == 0) return RC_OK;
    if (!scales) return fail(RC_EINVAL, "NULL scales pointer");
    if (skip < period && !out_dev) return fail(RC_EINVAL, "NULL output pointer");
    if (int rc = device_in_range(device)) return rc;
    RC_HIP_CHECK(hipSetDevice(device));
    return legacy_normal_stream((hipStream_t)stream, state, n_periods, period, skip, scales, out_dev);
}

int rc_directional_draws_legacy_dev(int device, void* stream, rc_mt19937_state* state, long long n, int ndir, double sigma,
                                    int* idx_dev, double* ab_dev) {
    if (!state) return fail(RC_EINVAL, "NULL generator state");
    if (state->pos < 0 || state->pos > 624) return fail(RC_EINVAL, "generator state: pos must be in [0, 624]");
    if (n < 0 || ndir < 1) return fail(RC_EINVAL, "need n >= 0 and ndir >= 1");
    if (n == 0) return RC_OK;
    if (!idx_dev || !ab_dev) return fail(RC_EINVAL, "NULL output pointer");
    if (int rc = device_in_range(device)) return rc;
    RC_HIP_CHECK(hipSetDevice(device));
    const unsigned int rng = (unsigned int)ndir - 1u;
    unsigned int mask = rng;
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    mask |= mask >> 16;
    for (long long done = 0; done < n; done += kDirChunkSamples) {
        const long long cnt = (n - done < kDirChunkSamples) ? (n - done) : kDirChunkSamples;
        if (int rc = directional_chunk((hipStream_t)stream, state, cnt, rng, mask, sigma, idx_dev + done, ab_dev + 2 * done))
            return rc;
    }
    return RC_OK;
}

}  // extern "C"

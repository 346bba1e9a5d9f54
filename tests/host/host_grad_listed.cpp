// Lock-step host emulation of ONE wave of the fidelity-gradient kernels (code-robchar_amd/csrc/grad_core.h compiled with
// RC_HOST_WAVE, the harness of host_wave.cpp): every active lane is a host thread, every wave-level vote of the QL a barrier that
// returns the ballot mask.  What it is for: grad_eigensystem_fast<N, R, FREEZE> - with FREEZE = true (mc_fid_grad_listed_kernel)
// a lane's bits must not depend on which other samples share its wave; with FREEZE = false (every other kernel) the wave votes
// the sweep counts and they do.
// Two builds: a shared library for tests/test_host_grad_listed.py (rc_host_wave_grad), and with -DRC_HOST_GRAD_LISTED_MAIN a
// stand-alone program that checks the property on inputs of its own and returns 0 / 1 - the build to put under a sanitizer.
// TEST HARNESS ONLY: the product never loads this.
#define RC_HOST_WAVE 1
#include "../../code-robchar_amd/csrc/grad_core.h"
#include <pthread.h>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {
struct WaveCtx {
    pthread_barrier_t bar;
    std::atomic<unsigned long long> acc[3];
};
thread_local WaveCtx* t_ctx = nullptr;
thread_local int t_lane = 0;
thread_local unsigned long long t_k = 0;       // ballots this thread has taken part in
}  // namespace

namespace rc_host_wave {
// (host_wave.cpp: three accumulators in rotation, ballot k collects into acc[k % 3])
unsigned long long ballot(bool v) {
    WaveCtx* c = t_ctx;
    if (!c) return v ? 1ull : 0ull;
    const unsigned long long k = t_k++;
    if (v) c->acc[k % 3].fetch_or(1ull << t_lane, std::memory_order_acq_rel);
    pthread_barrier_wait(&c->bar);
    const unsigned long long m = c->acc[k % 3].load(std::memory_order_acquire);
    c->acc[(k + 2) % 3].store(0ull, std::memory_order_release);
    return m;
}
int lane() { return t_lane; }
}  // namespace rc_host_wave

// the per-sample part of the kernels for one lane: every pass of the QL, then the spectral formulas
template <int N, bool FREEZE>
static bool one_lane(const double* x, const double* h0d, const double* h0o, const double* g, int in, int out, double* fid, double* grad) {
    constexpr int R = rc::grad_batch_rows(N);
    double d0[N], e0[N];
    rc::grad_load_matrix<N>(x, h0d, h0o, [g](int j) { return g[j]; }, d0, e0);
    bool all_ok = true;
    for (int pass = 0; pass < rc::grad_passes(N); ++pass) {
        int site[R];
        rc::grad_pass_rows<N>(in, out, pass, site);
        rc::TriEig<N, R> s;
        all_ok &= rc::grad_eigensystem_fast<N, R, FREEZE>(d0, e0, site, s);
        double f, gr[R + 1];
        rc::gradient_from_eigensystem<N, R>(s, x[N], in == out, f, gr);
        for (int l = 0; l <= R; ++l) {
            const int col = rc::grad_result_column<N>(site, pass, l);
            if (col >= 0) grad[col] = gr[l];
        }
        if (pass == 0) *fid = f;
    }
    return all_ok;
}

template <int N>
static int run_wave(const double* ctrl, const double* h0d, const double* h0o, const double* draws, const int* lanes, int m, int in,
                    int out, int freeze, double* fid, double* grad, long long* ballots, int* okf) {
    WaveCtx ctx;
    pthread_barrier_init(&ctx.bar, nullptr, (unsigned)m);
    for (auto& a : ctx.acc) a.store(0ull);
    std::vector<std::thread> th;
    for (int j = 0; j < m; ++j) {
        const int lane = lanes[j];
        th.emplace_back([&, lane] {
            t_ctx = &ctx;
            t_lane = lane;
            t_k = 0;
            const double* g = draws + (long long)lane * 3 * N;
            const bool ok = freeze ? one_lane<N, true>(ctrl, h0d, h0o, g, in, out, fid + lane, grad + (long long)lane * (N + 1))
                                   : one_lane<N, false>(ctrl, h0d, h0o, g, in, out, fid + lane, grad + (long long)lane * (N + 1));
            okf[lane] = ok ? 1 : 0;
            ballots[lane] = (long long)t_k;
            t_ctx = nullptr;
        });
    }
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&ctx.bar);
    return 0;
}

// One wave of the m samples lanes[0 .. m-1] (distinct values in 0 .. 63; lane l takes draws[l][N][3] and writes fid[l],
// grad[l][N+1], ok[l], ballots[l] = the votes it took part in: in a wave of ONE lane a measure of that sample's own sweeps).
extern "C" int rc_host_wave_grad(int N, const double* ctrl, const double* h0d, const double* h0o, const double* draws,
                                 const int* lanes, int m, int in, int out, int freeze, double* fid, double* grad, long long* ballots,
                                 int* ok) {
    if (m < 1 || m > 64) return -1;
    unsigned long long seen = 0ull;
    for (int j = 0; j < m; ++j) {
        if (lanes[j] < 0 || lanes[j] > 63 || ((seen >> lanes[j]) & 1ull)) return -1;
        seen |= 1ull << lanes[j];
    }
    switch (N) {
#define CASE(n) case n: return run_wave<n>(ctrl, h0d, h0o, draws, lanes, m, in, out, freeze, fid, grad, ballots, ok);
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12)
#undef CASE
    }
    return -1;
}

#ifdef RC_HOST_GRAD_LISTED_MAIN
// Inputs of its own (a 64-bit LCG): delocalised samples (small biases) and localised ones (biases of +-40: the QL deflates at
// once) in one wave; every lane alone, all together, and the odd lanes together - FREEZE = true must give the same bits.
static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uni() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}

static int check(int N) {
    const int n = 64;
    std::vector<double> ctrl(N + 1), h0d(32, 0.0), h0o(32, 1.0), draws((size_t)n * 3 * N);
    for (int i = 0; i < N; ++i) ctrl[i] = uni();
    ctrl[N] = 0.6 * N;
    for (int l = 0; l < n; ++l)
        for (int i = 0; i < N; ++i) {
            double* g = &draws[((size_t)l * N + i) * 3];
            g[0] = (l % 3 == 0 ? 80.0 * uni() : 0.1 * uni());
            g[1] = 0.1 * uni();
            g[2] = 0.1 * uni();
        }
    auto wave = [&](const std::vector<int>& lanes, std::vector<double>& fid, std::vector<double>& grad, std::vector<long long>& b) {
        std::vector<int> ok(n, 1);
        fid.assign(n, 0.0);
        grad.assign((size_t)n * (N + 1), 0.0);
        b.assign(n, 0);
        return rc_host_wave_grad(N, ctrl.data(), h0d.data(), h0o.data(), draws.data(), lanes.data(), (int)lanes.size(), 0, N - 1, 1,
                                 fid.data(), grad.data(), b.data(), ok.data());
    };
    std::vector<int> all(n), odd;
    for (int l = 0; l < n; ++l) {
        all[l] = l;
        if (l & 1) odd.push_back(l);
    }
    std::vector<double> f_all, g_all, f_odd, g_odd, f_one, g_one;
    std::vector<long long> b_all, b_odd, b_one;
    if (wave(all, f_all, g_all, b_all) || wave(odd, f_odd, g_odd, b_odd)) return 1;
    long long bmin = 1 << 30, bmax = 0;
    int bad = 0;
    for (int l = 0; l < n; ++l) {
        if (wave(std::vector<int>{l}, f_one, g_one, b_one)) return 1;
        bmin = b_one[l] < bmin ? b_one[l] : bmin;
        bmax = b_one[l] > bmax ? b_one[l] : bmax;
        bad += std::memcmp(&f_one[l], &f_all[l], sizeof(double)) != 0;
        bad += std::memcmp(&g_one[(size_t)l * (N + 1)], &g_all[(size_t)l * (N + 1)], sizeof(double) * (N + 1)) != 0;
        if (l & 1) {
            bad += std::memcmp(&f_odd[l], &f_all[l], sizeof(double)) != 0;
            bad += std::memcmp(&g_odd[(size_t)l * (N + 1)], &g_all[(size_t)l * (N + 1)], sizeof(double) * (N + 1)) != 0;
        }
    }
    std::printf("N = %d: votes alone %lld .. %lld, lanes whose bits depend on their mates: %d\n", N, bmin, bmax, bad);
    return (bad == 0 && bmax > bmin) ? 0 : 1;
}

int main() {
    int rc = 0;
    for (int N : {3, 7, 10}) rc |= check(N);
    std::printf(rc ? "FAILED\n" : "OK\n");
    return rc;
}
#endif

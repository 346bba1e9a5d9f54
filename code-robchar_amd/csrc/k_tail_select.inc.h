// tail_select_kernel: the lower tail of every row of a fidelity table - list, CVaR weights and value at risk in one launch
// (rc_tail_select_f64_async; the definition is noise.tail_weights).
//
// Part of ONE translation unit: this file is #included by robchar_hip.hip INSIDE its anonymous namespace, behind
// k_reduce_sort.inc.h (kRedCache); it is not a stand-alone header.  The per-element arithmetic is select_core.h.
//
// One workgroup per row, no workspace.  (1) Threshold: radix select over the order-preserving key, eight 8-bit digits, most
// significant first: a 256-bin histogram in LDS (32-bit integer LDS atomics: integer addition commutes, the counts do not depend
// on arrival order), the first wave walks it to the digit that holds the element of the wanted rank.  After eight passes the key
// T of the m-th smallest element and the tie quota (how many elements equal to T are selected) are known.  (2) Compaction in
// index order: an exclusive scan over the two flags key < T and key == T - ballot / popcount within a wave, the wave totals
// through LDS in index order - gives every taken element its slot.
// Rows of up to 16384 values are read from HBM once and kept in registers (CACHED; the thread count follows K as in reduce_kernel:
// 128 / 256 / 512 threads for rows of up to 4096 / 8192 / 16384 values); longer rows are re-read, from L2, tile by tile in every
// pass.  A thread's values are k = tile * TILE + i * THREADS + threadIdx.x: coalesced, and (tile, i, wave, lane) is index order.
// Short rows (K <= 2048), many of them - the paper's 11 000 rows of 100 draws: tail_select_rows_wave_kernel below, one WAVE per row in
// the manner of reduce_rows_wave_kernel.  Every output is an integer or a copied double: the routes cannot differ in their results.
// CONTROL FLOW: every trip count and every branch around a barrier depends on K, on the pass number or on a value all threads
// read from LDS behind a barrier (the NaN flag among them) - never on a thread's own data.
constexpr int kSelLongU = 8;           // values per thread and tile of the long-row route

struct TailParams {
    const double* fid;     // [C][K]
    long long C, K, m;
    double w_body, w_last;
    int* list;             // [C][m]
    double* weight;        // [C][m] or null
    double* var;           // [C] or null
};

template <int THREADS, int U, bool CACHED>
__global__ __launch_bounds__(THREADS) void tail_select_kernel(const TailParams p) {
    constexpr int kWaves = THREADS / 64;
    constexpr int TILE = THREADS * U;
    constexpr int E = U * kWaves;                         // (value slot, wave) segments of a tile, in index order
    constexpr int PER = E / 64;                           // segments a lane of the first wave scans
    static_assert(E % 64 == 0, "the first wave scans the segment table");
    __shared__ unsigned int hist[rcsel::kBins];
    __shared__ unsigned long long seg[E + 1];             // packed counts: key < T low word, key == T high word; [E] = tile total
    __shared__ unsigned int ctl[3];                       // threshold digit, elements below it, NaN flag
    const long long c = blockIdx.x;
    const long long K = p.K;
    const double* row = p.fid + c * K;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long ntiles = CACHED ? 1 : (K + TILE - 1) / TILE;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;

    double val[U];
    auto load = [&](long long tile) {
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const long long k = tile * TILE + (long long)i * THREADS + threadIdx.x;
            val[i] = (k < K) ? row[k] : 0.0;
        }
    };
    if (CACHED) load(0);

    // (1) threshold
    unsigned long long prefix = 0;
    unsigned int rank = (unsigned int)(p.m - 1);          // 0-based rank of the m-th smallest among the elements still in the prefix
    int bad = 0;
    if (threadIdx.x == 0) ctl[2] = 0u;                    // (ordered before its use by the barrier behind the histogram's zeroing)
    for (int pass = 0; pass < rcsel::kPasses; ++pass) {
        for (int b = threadIdx.x; b < rcsel::kBins; b += THREADS) hist[b] = 0u;
        __syncthreads();
        for (long long tile = 0; tile < ntiles; ++tile) {
            if (!CACHED) load(tile);
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const long long base = tile * TILE + (long long)i * THREADS;
                if (base >= K) continue;                                         // workgroup-uniform
                const bool in = base + threadIdx.x < K;
                const double x = val[i];
                if (pass == 0) bad |= (in && x != x);
                const unsigned long long key = rcsel::key_of(x);
                const bool act = in && rcsel::in_prefix(key, prefix, pass);
                const unsigned int d = rcsel::digit_of(key, pass);
                // fidelities share their leading digits: the lanes that agree with the first active lane go in as ONE add
                const unsigned long long am = __ballot(act);
                if (am != 0ull) {                                                // wave-uniform
                    const int first = __ffsll((long long)am) - 1;
                    const unsigned int d0 = __shfl(d, first, 64);
                    const unsigned long long same = __ballot(act && d == d0);
                    if (lane == first) atomicAdd(&hist[d0], (unsigned int)__popcll(same));
                    else if (act && d != d0) atomicAdd(&hist[d], 1u);
                }
            }
        }
        if (pass == 0 && __ballot(bad != 0) != 0ull && lane == 0) atomicOr(&ctl[2], 1u);
        __syncthreads();
        if (pass == 0) {
            if (ctl[2] != 0u) {                           // a row with a NaN (every thread reads the flag): empty slots, weight 0, NaN
                for (long long s = threadIdx.x; s < p.m; s += THREADS) {
                    p.list[c * p.m + s] = -1;
                    if (p.weight) p.weight[c * p.m + s] = 0.0;
                }
                if (threadIdx.x == 0 && p.var) p.var[c] = __builtin_nan("");
                return;
            }
        }
        if (wave == 0) {
            unsigned int mine = 0;
#pragma unroll
            for (int j = 0; j < rcsel::kBins / 64; ++j) mine += hist[(rcsel::kBins / 64) * lane + j];
            unsigned int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            const unsigned int excl = incl - mine;
            if (excl <= rank && rank < incl) {            // exactly one lane: rank < the sum of the histogram
                unsigned int below;
                const int d = rcsel::walk(hist, (rcsel::kBins / 64) * lane, rcsel::kBins / 64, rank - excl, &below);
                ctl[0] = (unsigned int)d;
                ctl[1] = excl + below;
            }
        }
        __syncthreads();
        prefix = (prefix << rcsel::kDigitBits) | ctl[0];
        rank -= ctl[1];
    }
    const unsigned long long T = prefix;
    const unsigned int quota = rank + 1u;                 // elements equal to T that are selected: the first `quota` in index order

    // (2) compaction in index order
    unsigned long long run = 0;                           // packed counts of the tiles in front of this one
    for (long long tile = 0; tile < ntiles; ++tile) {
        if (!CACHED) load(tile);
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const bool in = tile * TILE + (long long)i * THREADS + threadIdx.x < K;
            const unsigned long long key = rcsel::key_of(val[i]);
            const unsigned long long lt = __ballot(in && key < T), eq = __ballot(in && key == T);
            if (lane == 0) seg[i * kWaves + wave] = (unsigned long long)__popcll(lt) | ((unsigned long long)__popcll(eq) << 32);
        }
        __syncthreads();
        if (wave == 0) {                                  // exclusive scan of the E segments, written back in place
            unsigned long long own[PER], mine = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                own[j] = seg[PER * lane + j];
                mine += own[j];
            }
            unsigned long long incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            unsigned long long acc = incl - mine;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                seg[PER * lane + j] = acc;
                acc += own[j];
            }
            if (lane == 63) seg[E] = incl;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const long long base = tile * TILE + (long long)i * THREADS;
            if (base >= K) continue;                                             // workgroup-uniform
            const long long k = base + threadIdx.x;
            const bool in = k < K;
            const double x = val[i];
            const unsigned long long key = rcsel::key_of(x);
            const unsigned long long lt = __ballot(in && key < T), eq = __ballot(in && key == T);
            const unsigned long long before = run + seg[i * kWaves + wave];
            const unsigned int lt_before = (unsigned int)before + (unsigned int)__popcll(lt & lanes_below);
            const unsigned int eq_before = (unsigned int)(before >> 32) + (unsigned int)__popcll(eq & lanes_below);
            if (in && rcsel::take(key, T, eq_before, quota)) {
                const long long slot = rcsel::slot_of(lt_before, eq_before, quota);
                if (slot < p.m) {                         // (always: m - quota keys are below T; the guard keeps a store in its row)
                    const bool last = rcsel::is_last(key, T, eq_before, quota);
                    p.list[c * p.m + slot] = (int)k;
                    if (p.weight) p.weight[c * p.m + slot] = last ? p.w_last : p.w_body;
                    if (last && p.var) p.var[c] = x;
                }
            }
        }
        run += seg[E];
        if (!CACHED) __syncthreads();                     // the next tile writes the segment table again
    }
}

// Short rows (K <= kWaveRowMaxK = 2048): one WAVE per row, 4 rows per workgroup, the row in registers (SLOTS = 2 / 8 / 32 values per
// lane for rows of up to 128 / 512 / 2048 values), no LDS and no barrier.  The threshold comes from a search over the 64 key bits,
// most significant first: T is the largest key with fewer than m keys below it - the key of the m-th smallest element; a count is
// one ballot + popcount per value slot, so the counts are scalars and every branch is wave-uniform.  The compaction carries its two
// running counts as scalars from slot to slot (slot-major, then lane, is index order).  Same take rule, same outputs.
template <int SLOTS>
__global__ __launch_bounds__(256) void tail_select_rows_wave_kernel(const TailParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 4 + wave;
    if (c >= p.C) return;                                   // wave-uniform (the kernel has no barrier)
    const double* row = p.fid + c * p.K;
    const int K = (int)p.K;
    const unsigned int m = (unsigned int)p.m;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    double val[SLOTS];
    unsigned long long key[SLOTS];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int k = i * 64 + lane;
        const bool in = i * 64 < K && k < K;
        val[i] = in ? row[k] : 0.0;
        bad |= in && val[i] != val[i];
        key[i] = in ? rcsel::key_of(val[i]) : ~0ull;        // (above every key of a row without a NaN: never below or equal to T)
    }
    if (__ballot(bad) != 0ull) {                            // a row with a NaN: empty slots, weight 0, NaN
        for (unsigned int s = lane; s < m; s += 64) {
            p.list[c * p.m + s] = -1;
            if (p.weight) p.weight[c * p.m + s] = 0.0;
        }
        if (lane == 0 && p.var) p.var[c] = __builtin_nan("");
        return;
    }
    unsigned long long T = 0;
    for (int b = 63; b >= 0; --b) {
        const unsigned long long cand = T | (1ull << b);
        unsigned int below = 0;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            if (i * 64 < K) below += (unsigned int)__popcll(__ballot(key[i] < cand));
        if (below < m) T = cand;                            // wave-uniform
    }
    unsigned int n_lt = 0;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
        if (i * 64 < K) n_lt += (unsigned int)__popcll(__ballot(key[i] < T));
    const unsigned int quota = m - n_lt;
    unsigned int lt_run = 0, eq_run = 0;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        if (i * 64 >= K) continue;                          // wave-uniform
        const int k = i * 64 + lane;
        const bool in = k < K;
        const unsigned long long lt = __ballot(in && key[i] < T), eq = __ballot(in && key[i] == T);
        const unsigned int lt_before = lt_run + (unsigned int)__popcll(lt & lanes_below);
        const unsigned int eq_before = eq_run + (unsigned int)__popcll(eq & lanes_below);
        if (in && rcsel::take(key[i], T, eq_before, quota)) {
            const unsigned int slot = rcsel::slot_of(lt_before, eq_before, quota);
            if (slot < m) {                                 // (always; the guard keeps a store in its row)
                const bool last = rcsel::is_last(key[i], T, eq_before, quota);
                p.list[c * p.m + slot] = k;
                if (p.weight) p.weight[c * p.m + slot] = last ? p.w_last : p.w_body;
                if (last && p.var) p.var[c] = val[i];
            }
        }
        lt_run += (unsigned int)__popcll(lt);
        eq_run += (unsigned int)__popcll(eq);
    }
}

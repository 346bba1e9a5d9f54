// The tail selection of tail_select_kernel on the CPU: a SERIAL select built from the functions of select_core.h (key, digit,
// prefix test, histogram walk, take rule, slot) against std::stable_sort - the order (value, index) by construction.  A
// stand-alone program with its own main, so that a sanitizer can be put on it (tests/test_host_tail_select.py builds it plain and
// with -fsanitize=address,undefined).
//   argv: the file of cases.  File: int64 ncases, then per case int64 C, int64 K, double alpha, C*K doubles.
//   stdout: one line per case, then OK; exit status 1 on the first difference.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../code-robchar_amd/csrc/select_core.h"

struct Plan {
    long long m;
    double w_body, w_last;
};

static Plan plan(long long K, double alpha) {
    const double ak = alpha * (double)K;
    const long long up = (long long)std::ceil(ak);
    Plan p;
    p.m = up < K ? up : K;
    p.w_body = 1.0 / ak;
    p.w_last = (ak - (double)(p.m - 1)) / ak;
    return p;
}

static bool has_nan(const double* row, long long K) {
    for (long long k = 0; k < K; ++k)
        if (row[k] != row[k]) return true;
    return false;
}

// what the kernel does, one element at a time
static void select_serial(const double* row, long long K, const Plan& p, int* list, double* weight, double* var) {
    if (has_nan(row, K)) {
        for (long long s = 0; s < p.m; ++s) list[s] = -1, weight[s] = 0.0;
        *var = std::nan("");
        return;
    }
    unsigned long long prefix = 0;
    unsigned int rank = (unsigned int)(p.m - 1);
    for (int pass = 0; pass < rcsel::kPasses; ++pass) {
        unsigned int hist[rcsel::kBins] = {0};
        for (long long k = 0; k < K; ++k) {
            const unsigned long long key = rcsel::key_of(row[k]);
            if (rcsel::in_prefix(key, prefix, pass)) ++hist[rcsel::digit_of(key, pass)];
        }
        unsigned int below;
        const int d = rcsel::walk(hist, 0, rcsel::kBins, rank, &below);
        prefix = (prefix << rcsel::kDigitBits) | (unsigned long long)d;
        rank -= below;
    }
    const unsigned long long T = prefix;
    const unsigned int quota = rank + 1u;
    unsigned int lt_before = 0, eq_before = 0;
    for (long long k = 0; k < K; ++k) {
        const unsigned long long key = rcsel::key_of(row[k]);
        if (rcsel::take(key, T, eq_before, quota)) {
            const unsigned int slot = rcsel::slot_of(lt_before, eq_before, quota);
            const bool last = rcsel::is_last(key, T, eq_before, quota);
            list[slot] = (int)k;
            weight[slot] = last ? p.w_last : p.w_body;
            if (last) *var = row[k];
        }
        lt_before += key < T;
        eq_before += key == T;
    }
}

static void select_sorted(const double* row, long long K, const Plan& p, int* list, double* weight, double* var) {
    if (has_nan(row, K)) {
        for (long long s = 0; s < p.m; ++s) list[s] = -1, weight[s] = 0.0;
        *var = std::nan("");
        return;
    }
    std::vector<int> order((size_t)K);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [row](int a, int b) { return row[a] < row[b]; });
    const int last = order[(size_t)p.m - 1];
    std::vector<int> tail(order.begin(), order.begin() + p.m);
    std::sort(tail.begin(), tail.end());
    for (long long s = 0; s < p.m; ++s) {
        list[s] = tail[(size_t)s];
        weight[s] = tail[(size_t)s] == last ? p.w_last : p.w_body;
    }
    *var = row[last];
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ncases = 0;
    if (fread(&ncases, sizeof ncases, 1, f) != 1) return 2;
    for (int64_t t = 0; t < ncases; ++t) {
        int64_t C, K;
        double alpha;
        if (fread(&C, sizeof C, 1, f) != 1 || fread(&K, sizeof K, 1, f) != 1 || fread(&alpha, sizeof alpha, 1, f) != 1) return 2;
        std::vector<double> fid((size_t)(C * K));
        if (fread(fid.data(), sizeof(double), fid.size(), f) != fid.size()) return 2;
        const Plan p = plan(K, alpha);
        std::vector<int> la((size_t)p.m, -7), lb((size_t)p.m, -7);
        std::vector<double> wa((size_t)p.m, -7.0), wb((size_t)p.m, -7.0);
        for (int64_t c = 0; c < C; ++c) {
            double va = -7.0, vb = -7.0;
            select_serial(fid.data() + c * K, K, p, la.data(), wa.data(), &va);
            select_sorted(fid.data() + c * K, K, p, lb.data(), wb.data(), &vb);
            const bool var_ok = (va != va && vb != vb) || std::memcmp(&va, &vb, sizeof va) == 0;
            if (la != lb || std::memcmp(wa.data(), wb.data(), wa.size() * sizeof(double)) != 0 || !var_ok) {
                printf("case %lld (C = %lld, K = %lld, alpha = %.17g): row %lld differs\n", (long long)t, (long long)C, (long long)K, alpha,
                       (long long)c);
                return 1;
            }
        }
        printf("case %lld: C = %lld, K = %lld, alpha = %.17g, m = %lld\n", (long long)t, (long long)C, (long long)K, alpha, p.m);
    }
    fclose(f);
    printf("OK\n");
    return 0;
}

// Per-element pieces of the tail selection (tail_select_kernel, k_tail_select.inc.h) - plain C++ so that the CPU unit test runs
// the exact key, digit, walk and take logic (tests/host/host_tail_select.cpp); the product only ever runs it inside the kernel.
//
// The m smallest values of a row under the order (value, index) are found without a sort: every value maps to an unsigned
// 64-bit key with the same order, a radix select over the key (most significant digit first, one 256-bin histogram per digit)
// gives the key T of the m-th smallest element and how many elements equal to T are selected (the tie quota), and an element is
// taken when its key is below T, or equals T with fewer than `quota` equal elements in front of it.
#pragma once

#ifndef RC_HD
#if defined(__HIPCC__)
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif
#endif

namespace rcsel {

constexpr int kDigitBits = 8;
constexpr int kBins = 1 << kDigitBits;
constexpr int kPasses = 64 / kDigitBits;

// Order-preserving key of a double that is not a NaN: the sign bit flipped, and every bit of a negative value.  -0.0 is made
// +0.0 first: NumPy's sort compares them equal, so the index breaks that tie.
RC_HD unsigned long long key_of(double x) {
    unsigned long long u;
    __builtin_memcpy(&u, &x, sizeof u);
    if (x == 0.0) u = 0ull;
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

// digit of pass 0 .. kPasses - 1, most significant first
RC_HD unsigned int digit_of(unsigned long long key, int pass) {
    return (unsigned int)(key >> (64 - kDigitBits * (pass + 1))) & (unsigned int)(kBins - 1);
}

// does `key` still carry the threshold's digits of the passes before `pass` (`prefix`: those digits, first one highest)?
RC_HD bool in_prefix(unsigned long long key, unsigned long long prefix, int pass) {
    return pass == 0 || (key >> (64 - kDigitBits * pass)) == prefix;
}

// Walk over the bins first .. first + n - 1 of a histogram to the one that holds the element of 0-based `rank` among them
// (rank < their sum): returns the bin, *below = the elements in the bins in front of it.
RC_HD int walk(const unsigned int* hist, int first, int n, unsigned int rank, unsigned int* below) {
    unsigned int acc = 0;
    int d = first;
    for (; d < first + n - 1; ++d) {
        const unsigned int h = hist[d];
        if (rank < acc + h) break;
        acc += h;
    }
    *below = acc;
    return d;
}

// take rule: `eq_before` = elements with key == T and a lower index
RC_HD bool take(unsigned long long key, unsigned long long T, unsigned int eq_before, unsigned int quota) {
    return key < T || (key == T && eq_before < quota);
}

// slot of a taken element in the ascending-index list: `lt_before` = elements with key < T and a lower index
RC_HD unsigned int slot_of(unsigned int lt_before, unsigned int eq_before, unsigned int quota) {
    return lt_before + (eq_before < quota ? eq_before : quota);
}

// the taken element that is the m-th smallest in (value, index) order: it carries w_last and is the value at risk
RC_HD bool is_last(unsigned long long key, unsigned long long T, unsigned int eq_before, unsigned int quota) {
    return key == T && eq_before + 1 == quota;
}

}  // namespace rcsel

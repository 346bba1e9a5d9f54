// Host build of the workspace plan of the blocking entries (code-robchar_amd/csrc/ws_plan.h) for tests/test_host_ws_plan.py:
//   g++ -O2 -std=c++17 -shared -fPIC -o librc_wsplan.so tests/host/host_ws_plan.cpp
// Nothing is allocated or dereferenced: the workspace base and the callers' arrays are plain numbers.
#include <stdint.h>

#include "../../code-robchar_amd/csrc/ws_plan.h"

namespace {

// how a slot is declared (the test's numbering)
enum { kInHost, kInDev, kOutAbsent, kOutHost, kOutDev, kOutAlwaysHost, kOutAlwaysDev, kOutAlwaysAbsent, kScratch };

int declare(rcws::Plan& pl, int kind, void* user, size_t bytes) {
    switch (kind) {
        case kInHost: return pl.in(user, bytes, false);
        case kInDev: return pl.in(user, bytes, true);
        case kOutAbsent: return pl.out(nullptr, bytes, false);
        case kOutHost: return pl.out(user, bytes, false);
        case kOutDev: return pl.out(user, bytes, true);
        case kOutAlwaysHost: return pl.out(user, bytes, false, true);
        case kOutAlwaysDev: return pl.out(user, bytes, true, true);
        case kOutAlwaysAbsent: return pl.out(nullptr, bytes, false, true);
        default: return pl.scratch(bytes);
    }
}

// The carving as the entries wrote it by hand before ws_plan.h: a sum of the staged sizes and, separately, a pointer walk that
// has to repeat the sum's terms and conditions.  Deliberately WRONG, for the checks' own test - `slip` 1: the walk does not round
// the first staged slot; 2: the walk gives an absent output space, the sum does not.
void hand_carved(int slip, int n, const int* kind, const uint64_t* bytes, const uint64_t* user, uint64_t ws, uint64_t* ptr,
                 uint64_t* total) {
    auto absent = [](int k) { return k == kOutAbsent || k == kOutAlwaysAbsent; };
    auto staged = [](int k) { return k == kInHost || k == kOutHost || k == kOutAlwaysHost || k == kOutAlwaysDev || k == kScratch; };
    uint64_t need = 0, w = ws;
    for (int i = 0; i < n; ++i)
        if (staged(kind[i])) need += rcws::up(bytes[i]);
    bool first = true;
    for (int i = 0; i < n; ++i) {
        if (staged(kind[i]) || (slip == 2 && absent(kind[i]))) {
            ptr[i] = w;
            w += (slip == 1 && first) ? bytes[i] : rcws::up(bytes[i]);
            first = false;
        } else {
            ptr[i] = absent(kind[i]) ? 0 : user[i];
        }
    }
    *total = need;
}

}  // namespace

// `nplans` plans of `n` slots each ([nplans][n] arrays): the pointer every slot's kernel argument gets with the workspace at `ws`,
// and every plan's total.  slip 0: ws_plan.h; otherwise the hand-carved stand-in above.
extern "C" int rc_host_ws_plans(int slip, long long nplans, int n, const int* kind, const uint64_t* bytes, const uint64_t* user,
                                uint64_t ws, uint64_t* ptr, uint64_t* total) {
    if (n < 0 || n > rcws::kMaxSlots) return 1;
    for (long long m = 0; m < nplans; ++m) {
        const long long o = m * n;
        if (slip) {
            hand_carved(slip, n, kind + o, bytes + o, user + o, ws, ptr + o, total + m);
            continue;
        }
        rcws::Plan pl;
        for (int i = 0; i < n; ++i)
            if (declare(pl, kind[o + i], (void*)(uintptr_t)user[o + i], (size_t)bytes[o + i]) != i) return 2;
        for (int i = 0; i < n; ++i) ptr[o + i] = (uint64_t)(uintptr_t)pl.ptr(i, (void*)(uintptr_t)ws);
        total[m] = pl.total;
    }
    return 0;
}

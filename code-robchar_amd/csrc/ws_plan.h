// The carving of a device workspace for one blocking call: which of its arrays take space, where, and how much in all.  Plain
// arithmetic, no HIP (tests/host/host_ws_plan.cpp compiles it with g++); robchar_hip.hip adds the pointer queries and the copies.
// A call declares its arrays once, in order; the total, every device pointer and the copies to enqueue follow from that record.
#pragma once
#include <assert.h>
#include <stddef.h>

namespace rcws {

constexpr int kMaxSlots = 10;
constexpr size_t up(size_t b) { return (b + 255) & ~(size_t)255; }

struct Slot {
    const void* user;     // the caller's array (NULL: scratch, or an output that is not wanted)
    size_t bytes, offset; // offset: of a staged slot in the workspace
    bool input, staged, always;
};

struct Plan {
    Slot s[kMaxSlots];
    int n = 0;
    size_t total = 0;     // bytes of workspace: the staged slots, each rounded up to 256, in declaration order

    int add(const void* user, size_t bytes, bool input, bool staged, bool always) {
        assert(n < kMaxSlots);
        s[n] = Slot{user, bytes, total, input, staged, always};
        if (staged) total += up(bytes);
        return n++;
    }
    // input: a host array is staged (copied in before the launch), a device array is used where it is
    int in(const void* p, size_t bytes, bool on_device) { return add(p, bytes, true, !on_device, false); }
    // output: NULL = not wanted (no space, NULL to the kernel); a device array is written in place, a host array is staged
    // (copied out behind the launch); `always`: staged wherever it lives (small rows: one copy of any kind brings them back)
    int out(void* p, size_t bytes, bool on_device, bool always = false) {
        return add(p, bytes, false, p && (always || !on_device), always);
    }
    int scratch(size_t bytes) { return add(nullptr, bytes, false, true, false); }
    // what the kernel is given for slot i when the workspace starts at `ws`
    void* ptr(int i, void* ws) const { return s[i].staged ? (char*)ws + s[i].offset : const_cast<void*>(s[i].user); }
};

}  // namespace rcws

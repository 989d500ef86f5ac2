// covt_arena.h -- the layout of one device allocation holding several arrays (the device plan's arenas,
// covt_plan_device.hip).  An arena is declared once, as a run of take() calls in member order, allocated with
// bytes(), and its members bound with at(base).  Every member starts on a 256-byte boundary of the arena.
// Plain C++17, no HIP: tests/arena_layout/arena_layout_check.cc runs it on the CPU under sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

constexpr size_t kArenaAlign = 256;

template <class T>
struct ArenaSlot {
    size_t off = 0;
    bool on = false;  // false: a member this arena does not hold (no bytes, no pointer)
    T* at(void* base) const {
        if (!on) std::abort();  // binding an absent member: a mistake in the code that declared the arena
        return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off);
    }
};

class ArenaLayout {
public:
    // the next member: n elements of T at the running end (on == false: absent, the end stays)
    template <class T>
    ArenaSlot<T> take(size_t n, bool on = true) {
        const ArenaSlot<T> slot{end_, on};
        if (on) end_ += (n * sizeof(T) + kArenaAlign - 1) & ~(kArenaAlign - 1);
        return slot;
    }
    size_t bytes() const { return end_; }

private:
    size_t end_ = 0;
};

// arena_layout_check.cc -- TEST INFRASTRUCTURE: the arena layout helper of cov-tiles_amd/csrc/covt_arena.h
// (members in declaration order, each on a 256-byte boundary, absent members taking no bytes) run on the CPU
// in a stand-alone program, built by tests/test_arena_layout.py with -fsanitize=address,undefined.
// Prints "ok <declarations checked>".
#include <sys/wait.h>
#include <unistd.h>

#include <csignal>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "covt_arena.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

struct Rec24 {  // (a size that is no power of two, like the plan's records)
    uint8_t b[24];
};
struct Member {
    size_t off, bytes;  // bytes: what the member holds, before rounding
    bool on;
};

template <class T>
Member take(ArenaLayout& a, size_t n, bool on) {
    const ArenaSlot<T> s = a.take<T>(n, on);
    return Member{s.off, n * sizeof(T), on};
}

// binding an absent member ends the program: in a child process, so this one goes on
static bool absent_member_aborts() {
    std::fflush(nullptr);
    const pid_t pid = fork();
    if (pid < 0) return false;
    if (pid == 0) {
        std::fclose(stderr);
        ArenaLayout a;
        uint8_t base[256];
        const auto s = a.take<int64_t>(4, false);
        _exit(s.at(base) ? 0 : 1);
    }
    int status = 0;
    return waitpid(pid, &status, 0) == pid && WIFSIGNALED(status) && WTERMSIG(status) == SIGABRT;
}

int main() {
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const size_t edge[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097};
    const size_t n_edge = sizeof edge / sizeof edge[0];
    long checked = 0;
    for (int it = 0; it < 200000; ++it) {
        ArenaLayout a;
        std::vector<Member> ms;
        const int members = 1 + (int)(next() % 16);
        for (int k = 0; k < members; ++k) {
            const uint64_t r = next();
            const size_t n = (r & 3) == 0 ? edge[(r >> 8) % n_edge] : (size_t)((r >> 8) % 400);
            const bool on = ((r >> 2) & 7) != 0;
            const size_t before = a.bytes();
            Member m{};
            switch ((r >> 5) % 5) {
                case 0: m = take<uint8_t>(a, n, on); break;
                case 1: m = take<uint16_t>(a, n, on); break;
                case 2: m = take<int32_t>(a, n, on); break;
                case 3: m = take<int64_t>(a, n, on); break;
                default: m = take<Rec24>(a, n, on); break;
            }
            REQUIRE(m.off == before);  // at the running end: declaration order
            if (!on) REQUIRE(a.bytes() == before);  // an absent member adds no bytes
            else REQUIRE(a.bytes() >= before + m.bytes && a.bytes() - (before + m.bytes) < kArenaAlign);
            REQUIRE(a.bytes() % kArenaAlign == 0);
            ms.push_back(m);
        }
        // the whole declaration: aligned, in order, disjoint, inside bytes(), and bytes() the last end
        size_t end = 0;
        for (const Member& m : ms) {
            REQUIRE(m.off % kArenaAlign == 0 && m.off >= end);
            if (m.on) end = m.off + ((m.bytes + kArenaAlign - 1) & ~(kArenaAlign - 1));
        }
        REQUIRE(end == a.bytes());
        // bound to an allocation of bytes(): every member's first and last byte written (a heap array, under ASan)
        std::vector<uint8_t> arena(a.bytes());
        for (size_t k = 0; k < ms.size(); ++k) {
            if (!ms[k].on || !ms[k].bytes) continue;
            const ArenaSlot<uint8_t> s{ms[k].off, true};
            uint8_t* q = s.at(arena.data());
            REQUIRE(q[0] == 0 && q[ms[k].bytes - 1] == 0);  // nobody else's bytes
            q[0] = q[ms[k].bytes - 1] = (uint8_t)(k + 1);
        }
        ++checked;
    }
    // typed binding, and the default-constructed slot is absent
    ArenaLayout a;
    const auto s0 = a.take<int32_t>(3), s1 = a.take<int32_t>(0), s2 = a.take<int32_t>(65);
    const auto s3 = a.take<double>(1, false);
    alignas(256) static uint8_t base[1024];
    REQUIRE((uint8_t*)s0.at(base) == base && (uint8_t*)s1.at(base) == base + 256 && (uint8_t*)s2.at(base) == base + 256);
    REQUIRE(s3.off == 768 && a.bytes() == 768 && !ArenaSlot<int>().on);
    REQUIRE(absent_member_aborts());
    std::printf("ok %ld\n", checked);
    return 0;
}

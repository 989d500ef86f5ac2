// wkb_layout_check.cc -- TEST INFRASTRUCTURE: the WKB layout rule of cov-tiles_amd/csrc/covt_wkb_plan.h
// (capacity, 16-byte aligned slices, the INT32_MAX check) run on the CPU in a stand-alone program, built
// by tests/test_wkb_writer.py with -fsanitize=address,undefined.  Prints "ok <columns checked>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "covt_wkb_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    // capacity: the table of include/covt.h bounded by 9 (n + parts) + 4 rings + 16 coordinates
    REQUIRE(wkb_capacity(0, 0, 0, 0) == 0);
    REQUIRE(wkb_capacity(1, 1, 1, 1) == 38);  // a POINT takes 21 of them
    REQUIRE(wkb_capacity(INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX) == 38ll * INT32_MAX);  // no int32 arithmetic
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 15, 16, 17, 1 << 25, (1 << 25) + 1, INT32_MAX - 1, INT32_MAX, -1, INT32_MIN};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    std::vector<covt_wkb_desc> descs;
    int64_t off = 0;
    long checked = 0;
    for (int it = 0; it < 200000; ++it) {
        auto pick = [&]() -> int32_t {
            const uint64_t r = next();
            return (r & 3) == 0 ? edge[(r >> 8) % (uint64_t)n_edge] : (int32_t)((r >> 8) % 5000);
        };
        const int32_t n = pick(), pc = pick(), rc = pick(), cc = pick();
        const uint32_t gflags = (next() & 15) == 0 ? COVT_GEOM_TOO_LARGE : (uint32_t)(next() & 1);
        covt_wkb_desc d{};
        const int64_t end = wkb_column_layout(n, pc, rc, cc, gflags, off, d);
        const bool neg = n < 0 || pc < 0 || rc < 0 || cc < 0;
        const bool fits = !(gflags & COVT_GEOM_TOO_LARGE) && !neg && wkb_capacity(n, pc, rc, cc) <= INT32_MAX;
        REQUIRE((d.flags == 0) == fits);
        REQUIRE(d.n_features == (fits ? n : 0));
        REQUIRE(d.byte_cap == (fits ? wkb_capacity(n, pc, rc, cc) : 0));
        REQUIRE(d.byte_cap >= 0 && d.byte_cap <= INT32_MAX);
        REQUIRE(d.offsets_off == off && (d.offsets_off & 15) == 0 && (d.bytes_off & 15) == 0 && (end & 15) == 0);
        REQUIRE(d.bytes_off >= d.offsets_off + 4 * ((int64_t)d.n_features + 1));
        REQUIRE(d.bytes_off - (d.offsets_off + 4 * ((int64_t)d.n_features + 1)) < 16);
        REQUIRE(end >= d.bytes_off + d.byte_cap && end - (d.bytes_off + d.byte_cap) < 16);
        if (fits && n >= 1) {
            // one MULTIPOLYGON holding every part, ring and coordinate, the other features empty ones
            REQUIRE(9 + 9 * (int64_t)pc + 4 * (int64_t)rc + 16 * (int64_t)cc + 9 * ((int64_t)n - 1) <= d.byte_cap);
            // a column of POINTs (a part and a coordinate each)
            if (pc >= n && cc >= n) REQUIRE(21 * (int64_t)n <= d.byte_cap);
        }
        if (descs.size() < 4096) descs.push_back(d);  // (what a plan keeps: a heap array, under ASan)
        off = end;
        ++checked;
    }
    // a plan's records in order: disjoint, increasing
    for (size_t i = 1; i < descs.size(); ++i)
        REQUIRE(descs[i].offsets_off >= descs[i - 1].bytes_off + descs[i - 1].byte_cap);
    std::printf("ok %ld\n", checked);
    return 0;
}

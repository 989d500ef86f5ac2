// measures_layout_check.cc -- TEST INFRASTRUCTURE: the measures layout rule of
// cov-tiles_amd/csrc/covt_measures_plan.h (area | length | num_coords padded to 16 bytes | per-ring scratch,
// 16-byte aligned slices, the too-large flag) run on the CPU in a stand-alone program, built by
// tests/test_measures_ref.py with -fsanitize=address,undefined.  Prints "ok <columns checked>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "covt_measures_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    static_assert(sizeof(covt_measures_desc) == 24, "covt_measures_desc");
    static_assert(sizeof(covt_measures_result) == 8, "covt_measures_result");
    static_assert(sizeof(covt_measures_info) == 32, "covt_measures_info");
    REQUIRE(measures_slice_bytes(0, 0) == 0 && measures_slice_bytes(1, 0) == 32 && measures_slice_bytes(1, 1) == 48);
    REQUIRE(measures_slice_bytes(4, 0) == 80 && measures_slice_bytes(5, 2) == 80 + 32 + 32);
    // no int32 arithmetic
    REQUIRE(measures_slice_bytes(INT32_MAX, INT32_MAX) == 16ll * INT32_MAX + ((4ll * INT32_MAX + 15) & ~15ll) + 16ll * INT32_MAX);
    REQUIRE(measures_ring_len_off(INT32_MAX, INT32_MAX) == measures_rows_bytes(INT32_MAX) + 8ll * INT32_MAX);
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 1 << 25, (1 << 25) + 1, INT32_MAX - 1, INT32_MAX, -1, INT32_MIN};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    std::vector<covt_measures_desc> descs;
    int64_t off = 0;
    long checked = 0;
    for (int it = 0; it < 200000; ++it) {
        const uint64_t r = next(), q = next();
        const int32_t n = (r & 3) == 0 ? edge[(r >> 8) % (uint64_t)n_edge] : (int32_t)((r >> 8) % 5000);
        const int32_t rc = (q & 3) == 0 ? edge[(q >> 8) % (uint64_t)n_edge] : (int32_t)((q >> 8) % 9000);
        const uint32_t gflags = (next() & 15) == 0 ? COVT_GEOM_TOO_LARGE : (uint32_t)(next() & 1);
        covt_measures_desc d;
        std::memset(&d, 0xee, sizeof d);  // every field is set by the rule
        const int64_t end = measures_column_layout(n, rc, gflags, off, d);
        const bool fits = !(gflags & COVT_GEOM_TOO_LARGE) && n >= 0 && rc >= 0;
        REQUIRE((d.flags == 0) == fits && (d.flags == 0 || d.flags == COVT_MEASURES_TOO_LARGE));
        // a refused column: zero rows and no scratch
        REQUIRE(d.n_features == (fits ? n : 0) && d.ring_cap == (fits ? rc : 0) && d.reserved == 0);
        REQUIRE(d.off == off && (d.off & 15) == 0 && (end & 15) == 0);
        const int64_t nf = d.n_features, cap = d.ring_cap;
        const int64_t bytes = measures_slice_bytes(nf, cap);
        REQUIRE(end >= d.off + bytes && end - (d.off + bytes) < 16);
        if (!fits) REQUIRE(bytes == 0 && end == off);
        // the three arrays back to back, aligned to their element; the count array padded to 16 bytes
        REQUIRE(measures_area_off(nf) == 0 && measures_length_off(nf) == 8 * nf && measures_count_off(nf) == 16 * nf);
        const int64_t rows = measures_rows_bytes(nf);
        REQUIRE((rows & 15) == 0 && rows >= 20 * nf && rows - 20 * nf < 16);
        // the scratch: two arrays of ring_cap 8-byte values after the rows, inside the slice, ending with it
        const int64_t s0 = measures_ring_s_off(nf, cap), s1 = measures_ring_len_off(nf, cap);
        REQUIRE(s0 == rows && s1 == s0 + 8 * cap && (s0 & 15) == 0 && (s1 & 7) == 0);
        REQUIRE(s1 + 8 * cap == bytes && measures_scratch_bytes(cap) == bytes - rows);
        if (descs.size() < 4096) descs.push_back(d);  // (what a plan keeps: a heap array, under ASan)
        off = end;
        ++checked;
    }
    // a plan's records in order: slices back to back (alignment gaps only), inside the total
    for (size_t i = 1; i < descs.size(); ++i) {
        const int64_t prev_end = descs[i - 1].off + measures_slice_bytes(descs[i - 1].n_features, descs[i - 1].ring_cap);
        REQUIRE(descs[i].off >= prev_end && descs[i].off - prev_end < 16);
    }
    REQUIRE(descs.back().off + measures_slice_bytes(descs.back().n_features, descs.back().ring_cap) <= off);
    std::printf("ok %ld\n", checked);
    return 0;
}

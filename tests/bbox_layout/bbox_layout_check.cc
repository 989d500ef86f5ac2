// bbox_layout_check.cc -- TEST INFRASTRUCTURE: the bounding-box layout rule of
// cov-tiles_amd/csrc/covt_bbox_plan.h (32 bytes per feature in four arrays, 16-byte aligned slices, the
// too-large flag) run on the CPU in a stand-alone program, built by tests/test_bbox_ref.py with
// -fsanitize=address,undefined.  Prints "ok <columns checked>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "covt_bbox_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    static_assert(sizeof(covt_bbox_desc) == 16, "covt_bbox_desc");
    static_assert(sizeof(covt_bbox_result) == 40, "covt_bbox_result");
    static_assert(sizeof(covt_bbox_info) == 32, "covt_bbox_info");
    REQUIRE(bbox_slice_bytes(0) == 0 && bbox_slice_bytes(1) == 32);
    REQUIRE(bbox_slice_bytes(INT32_MAX) == 32ll * INT32_MAX);  // no int32 arithmetic
    REQUIRE(bbox_array_off(INT32_MAX, 3) == 24ll * INT32_MAX);
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 15, 16, 17, 1 << 25, (1 << 25) + 1, INT32_MAX - 1, INT32_MAX, -1, INT32_MIN};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    std::vector<covt_bbox_desc> descs;
    int64_t off = 0;
    long checked = 0;
    for (int it = 0; it < 200000; ++it) {
        const uint64_t r = next();
        const int32_t n = (r & 3) == 0 ? edge[(r >> 8) % (uint64_t)n_edge] : (int32_t)((r >> 8) % 5000);
        const uint32_t gflags = (next() & 15) == 0 ? COVT_GEOM_TOO_LARGE : (uint32_t)(next() & 1);
        covt_bbox_desc d;
        std::memset(&d, 0xee, sizeof d);  // every field is set by the rule
        const int64_t end = bbox_column_layout(n, gflags, off, d);
        const bool fits = !(gflags & COVT_GEOM_TOO_LARGE) && n >= 0;
        REQUIRE((d.flags == 0) == fits && (d.flags == 0 || d.flags == COVT_BBOX_TOO_LARGE));
        REQUIRE(d.n_features == (fits ? n : 0));
        REQUIRE(d.off == off && (d.off & 15) == 0 && (end & 15) == 0);
        const int64_t bytes = bbox_slice_bytes(d.n_features);
        REQUIRE(end >= d.off + bytes && end - (d.off + bytes) < 16);
        // the four arrays: back to back, 8-byte aligned, inside the slice
        for (int k = 0; k < 4; ++k) {
            const int64_t a = d.off + bbox_array_off(d.n_features, k);
            REQUIRE((a & 7) == 0 && a >= d.off && a + 8 * (int64_t)d.n_features <= d.off + bytes);
            if (k) REQUIRE(a == d.off + bbox_array_off(d.n_features, k - 1) + 8 * (int64_t)d.n_features);
        }
        if (descs.size() < 4096) descs.push_back(d);  // (what a plan keeps: a heap array, under ASan)
        off = end;
        ++checked;
    }
    // a plan's records in order: disjoint, increasing, inside the total
    for (size_t i = 1; i < descs.size(); ++i)
        REQUIRE(descs[i].off >= descs[i - 1].off + bbox_slice_bytes(descs[i - 1].n_features));
    REQUIRE(descs.back().off + bbox_slice_bytes(descs.back().n_features) <= off);
    std::printf("ok %ld\n", checked);
    return 0;
}

// select_layout_check.cc -- TEST INFRASTRUCTURE: the select layout rule and the predicate's argument rule of
// cov-tiles_amd/csrc/covt_select_plan.h (mask | sel | offsets | bytes, every member and slice 16-byte aligned,
// the too-large flag set where the WKB layout sets its own) run on the CPU in a stand-alone program, built by
// tests/test_select_ref.py with -fsanitize=address,undefined.  Prints "ok <columns checked>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "covt_select_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int check_pred() {
    covt_select_pred p;
    std::memset(&p, 0xee, sizeof p);
    p.size = sizeof p;
    p.flags = 0;
    for (double& v : p.window) v = 0.0;
    p.min_area = p.min_length = 0.0;
    REQUIRE(select_pred_valid(&p) && !select_pred_valid(nullptr));
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int k = 0; k < 6; ++k) {  // a NaN anywhere; an infinity is a value
        covt_select_pred q = p;
        double* slot = k < 4 ? &q.window[k] : k == 4 ? &q.min_area : &q.min_length;
        *slot = nan;
        REQUIRE(!select_pred_valid(&q));
        *slot = k & 1 ? inf : -inf;
        REQUIRE(select_pred_valid(&q));
    }
    covt_select_pred q = p;
    q.size = sizeof p - 8;
    REQUIRE(!select_pred_valid(&q));
    q = p;
    q.flags = COVT_SELECT_WINDOW | COVT_SELECT_MIN_SIZE | COVT_SELECT_KEEP_EMPTY;
    REQUIRE(select_pred_valid(&q));
    q.flags |= 0x8u;
    REQUIRE(!select_pred_valid(&q));
    q.flags = 0x80000000u;
    REQUIRE(!select_pred_valid(&q));
    // the definition on single rows: closed window edges, an inverted window, empties, features without extent
    q = p;
    q.flags = COVT_SELECT_WINDOW;
    q.window[0] = 10, q.window[1] = 20, q.window[2] = 30, q.window[3] = 40;
    REQUIRE(select_keep(q, 30, 40, 50, 60, 0, 0) == 1 && select_keep(q, 0, 0, 10, 20, 0, 0) == 1);
    REQUIRE(select_keep(q, 30.000001, 40, 50, 60, 0, 0) == 0 && select_keep(q, 0, 0, 10, 19.9, 0, 0) == 0);
    REQUIRE(select_keep(q, nan, nan, nan, nan, 0, 0) == 0);
    q.flags |= COVT_SELECT_KEEP_EMPTY;
    REQUIRE(select_keep(q, nan, nan, nan, nan, 0, 0) == 1);
    q.window[0] = 30, q.window[2] = 10;  // inverted in x
    REQUIRE(select_keep(q, 0, 0, 100, 100, 0, 0) == 0 && select_keep(q, 20, 30, 20, 30, 0, 0) == 0);
    q = p;
    q.flags = COVT_SELECT_MIN_SIZE;
    q.min_area = 4, q.min_length = 8;
    REQUIRE(select_keep(q, 0, 0, 1, 1, 4, 0) == 1 && select_keep(q, 0, 0, 1, 1, 3.9, 8) == 1);
    REQUIRE(select_keep(q, 0, 0, 1, 1, 3.9, 7.9) == 0 && select_keep(q, 0, 0, 1, 1, 0.0, -0.0) == 1);
    REQUIRE(select_keep(q, 0, 0, 1, 1, -96.0, 1) == 0);
    return 0;
}

int main() {
    static_assert(sizeof(covt_select_desc) == 24, "covt_select_desc");
    static_assert(sizeof(covt_select_result) == 16, "covt_select_result");
    static_assert(sizeof(covt_select_info) == 40, "covt_select_info");
    static_assert(sizeof(covt_select_pred) == 56, "covt_select_pred");
    if (check_pred()) return 1;
    REQUIRE(select_slice_bytes(0, 0) == 16 && select_slice_bytes(1, 21) == 16 + 16 + 16 + 21);
    REQUIRE(select_sel_off(16) == 16 && select_sel_off(17) == 32 && select_offsets_off(4) == 32 && select_bytes_off(3) == 48);
    REQUIRE(select_bytes_off(4) == 16 + 16 + 32);
    // no int32 arithmetic
    REQUIRE(select_bytes_off(INT32_MAX) == ((int64_t)INT32_MAX + 1) + 4ll * ((int64_t)INT32_MAX + 1) + 4ll * ((int64_t)INT32_MAX + 1));
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 1 << 25, (1 << 25) + 1, INT32_MAX - 1, INT32_MAX, -1, INT32_MIN};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    std::vector<covt_select_desc> descs;
    int64_t off = 0;
    long checked = 0, too_large = 0;
    for (int it = 0; it < 200000; ++it) {
        int32_t v[4];
        for (int k = 0; k < 4; ++k) {
            const uint64_t r = next();
            v[k] = (r & 3) == 0 ? edge[(r >> 8) % (uint64_t)n_edge] : (int32_t)((r >> 8) % 9000);
        }
        const uint32_t gflags = (next() & 15) == 0 ? COVT_GEOM_TOO_LARGE : (uint32_t)(next() & 1);
        covt_select_desc d;
        covt_wkb_desc w;
        std::memset(&d, 0xee, sizeof d);  // every field is set by the rule
        std::memset(&w, 0xee, sizeof w);
        const int64_t end = select_column_layout(v[0], v[1], v[2], v[3], gflags, off, d);
        (void)wkb_column_layout(v[0], v[1], v[2], v[3], gflags, 0, w);
        // the WKB column's rows, capacity and refusal, exactly
        REQUIRE(d.n_features == w.n_features && d.byte_cap == w.byte_cap);
        REQUIRE((d.flags == COVT_SELECT_TOO_LARGE) == (w.flags == COVT_WKB_TOO_LARGE) && (d.flags & ~COVT_SELECT_TOO_LARGE) == 0);
        if (d.flags) REQUIRE(d.n_features == 0 && d.byte_cap == 0 && ++too_large);
        REQUIRE(d.byte_cap >= 0 && d.byte_cap <= INT32_MAX && d.n_features >= 0);
        REQUIRE(d.off == off && (d.off & 15) == 0 && (end & 15) == 0);
        const int64_t n = d.n_features;
        const int64_t bytes = select_slice_bytes(n, d.byte_cap);
        REQUIRE(end >= d.off + bytes && end - (d.off + bytes) < 16);
        // the members in order, each 16-byte aligned and long enough, the bytes member ending the slice
        const int64_t m0 = select_mask_off(n), m1 = select_sel_off(n), m2 = select_offsets_off(n), m3 = select_bytes_off(n);
        REQUIRE(m0 == 0 && ((m1 | m2 | m3) & 15) == 0);
        REQUIRE(m1 >= n && m1 - n < 16 && m2 >= m1 + 4 * n && m2 - (m1 + 4 * n) < 16);
        REQUIRE(m3 >= m2 + 4 * (n + 1) && m3 - (m2 + 4 * (n + 1)) < 16 && m3 + d.byte_cap == bytes);
        if (descs.size() < 4096) descs.push_back(d);  // (what a plan keeps: a heap array, under ASan)
        off = end;
        ++checked;
    }
    REQUIRE(too_large > 1000);
    // a plan's records in order: slices back to back (alignment gaps only), inside the total
    for (size_t i = 1; i < descs.size(); ++i) {
        const int64_t prev_end = descs[i - 1].off + select_slice_bytes(descs[i - 1].n_features, descs[i - 1].byte_cap);
        REQUIRE(descs[i].off >= prev_end && descs[i].off - prev_end < 16);
    }
    REQUIRE(descs.back().off + select_slice_bytes(descs.back().n_features, descs.back().byte_cap) <= off);
    std::printf("ok %ld\n", checked);
    return 0;
}

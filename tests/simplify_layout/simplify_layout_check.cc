// simplify_layout_check.cc -- TEST INFRASTRUCTURE: the simplify layout rule of
// cov-tiles_amd/csrc/covt_simplify_plan.h (geometry_offsets | part_offsets | ring_offsets | coords | scratch,
// every member padded to 16 bytes, 16-byte aligned slices, the too-large flag) held against the geometry
// capacities, the retargeted geometry descriptor, the shift's argument rule and snap() run on the CPU in a
// stand-alone program, built by tests/test_simplify_ref.py with -fsanitize=address,undefined.  Prints
// "ok <columns checked>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "covt_simplify_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int64_t a16(int64_t x) { return (x + 15) & ~(int64_t)15; }

int main() {
    static_assert(sizeof(covt_simplify_desc) == 32, "covt_simplify_desc");
    static_assert(sizeof(covt_simplify_info) == 40, "covt_simplify_info");
    static_assert(sizeof(covt_geom_result) == 16, "covt_geom_result");
    // the argument rule
    REQUIRE(simplify_shift_valid(0) && simplify_shift_valid(30) && COVT_SIMPLIFY_MAX_SHIFT == 30);
    REQUIRE(!simplify_shift_valid(-1) && !simplify_shift_valid(31) && !simplify_shift_valid(INT32_MIN) &&
            !simplify_shift_valid(INT32_MAX));
    // snap: round half up, clamped to the largest grid value that fits
    for (int s = 0; s <= 30; ++s) {
        const int32_t m = (int32_t)((INT32_MAX >> s) << s);
        REQUIRE(simplify_snap(INT32_MAX, s) == m && simplify_snap(INT32_MIN, s) == INT32_MIN && simplify_snap(0, s) == 0);
        REQUIRE(simplify_snap(-1, s) == (s ? 0 : -1) && simplify_snap(m, s) == m);
        if (s) {
            const int32_t h = (int32_t)1 << (s - 1);
            REQUIRE(simplify_snap(INT32_MAX - h, s) == m && simplify_snap(h - 1, s) == 0);
            REQUIRE(simplify_snap(h, s) == (s == 30 ? m : (int32_t)1 << s) && simplify_snap(-h, s) == 0);
            REQUIRE((int64_t)simplify_snap(-h - 1, s) == -((int64_t)1 << s));
        }
    }
    REQUIRE(simplify_snap(20, 4) == 16 && simplify_snap(5, 4) == 0 && simplify_snap(-9, 2) == -8 && simplify_snap(7, 2) == 8);
    // a few slices by hand: n = 0 and no capacity is five padded members of one or no entry
    REQUIRE(simplify_slice_bytes(0, 0, 0, 0) == 16 + 16 + 16 + 0 + 0 + 16);
    REQUIRE(simplify_slice_bytes(3, 3, 4, 9) == 16 + 16 + 32 + 80 + 16 + 16);
    REQUIRE(simplify_chunks(0) == 0 && simplify_chunks(1) == 1 && simplify_chunks(COVT_SIMPLIFY_CHUNK) == 1 &&
            simplify_chunks(COVT_SIMPLIFY_CHUNK + 1) == 2);
    // no int32 arithmetic
    REQUIRE(simplify_coords_off(INT32_MAX, INT32_MAX, INT32_MAX) == 3 * a16(4ll * INT32_MAX + 4));
    REQUIRE(simplify_ring_k_off(0, 0, 0, INT32_MAX) == 48 + a16(8ll * INT32_MAX));
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 1 << 25, (1 << 25) + 1, INT32_MAX - 1, INT32_MAX, -1,
                            INT32_MIN};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    auto pick = [&](uint64_t r, int32_t mod) {
        return (r & 3) == 0 ? edge[(r >> 8) % (uint64_t)n_edge] : (int32_t)((r >> 8) % (uint64_t)mod);
    };
    std::vector<covt_simplify_desc> descs;
    int64_t off = 0;
    long checked = 0;
    for (int it = 0; it < 200000; ++it) {
        const int32_t n = pick(next(), 5000), pc = pick(next(), 6000), rc = pick(next(), 9000), cc = pick(next(), 70000);
        const uint32_t gflags = (next() & 15) == 0 ? COVT_GEOM_TOO_LARGE : (uint32_t)(next() & 1);
        covt_simplify_desc d;
        std::memset(&d, 0xee, sizeof d);  // every field is set by the rule
        const int64_t end = simplify_column_layout(n, pc, rc, cc, gflags, off, d);
        const bool fits = !(gflags & COVT_GEOM_TOO_LARGE) && n >= 0 && pc >= 0 && rc >= 0 && cc >= 0;
        REQUIRE((d.flags == 0) == fits && (d.flags == 0 || d.flags == COVT_SIMPLIFY_TOO_LARGE));
        // the capacities are the geometry column's; a refused column: zero rows and no capacity
        REQUIRE(d.n_features == (fits ? n : 0) && d.part_cap == (fits ? pc : 0) && d.ring_cap == (fits ? rc : 0) &&
                d.coord_cap == (fits ? cc : 0) && d.reserved == 0);
        REQUIRE(d.off == off && (d.off & 15) == 0 && (end & 15) == 0);
        const int64_t nf = d.n_features, P = d.part_cap, R = d.ring_cap, V = d.coord_cap;
        const int64_t bytes = simplify_slice_bytes(nf, P, R, V);
        REQUIRE(end == d.off + bytes && (bytes & 15) == 0);
        // the members back to back, each 16-byte aligned and large enough for the capacity it holds
        const int64_t o_geo = simplify_geo_off(nf), o_part = simplify_part_off(nf), o_ring = simplify_ring_off(nf, P),
                      o_xy = simplify_coords_off(nf, P, R), o_rk = simplify_ring_k_off(nf, P, R, V),
                      o_ck = simplify_chunk_k_off(nf, P, R, V);
        REQUIRE(o_geo == 0 && o_part == a16(4 * (nf + 1)) && o_ring == o_part + a16(4 * (P + 1)));
        REQUIRE(o_xy == o_ring + a16(4 * (R + 1)) && o_rk == o_xy + a16(8 * V) && o_ck == o_rk + a16(4 * R));
        REQUIRE(bytes == o_ck + a16(4 * (simplify_chunks(V) + 1)));
        REQUIRE(!((o_part | o_ring | o_xy | o_rk | o_ck) & 15));
        // a chunk count for every chunk of a full column
        REQUIRE(simplify_chunks(V) * COVT_SIMPLIFY_CHUNK >= V && (simplify_chunks(V) - 1) * COVT_SIMPLIFY_CHUNK < V + (V == 0));
        // the retargeted geometry descriptor: the four column members in the slice, everything else kept
        covt_geom_desc g;
        std::memset(&g, 0x5a, sizeof g);
        const covt_geom_desc t = simplify_retarget(g, d);
        REQUIRE(t.out_off[0] == d.off + o_geo && t.out_off[1] == d.off + o_part && t.out_off[2] == d.off + o_ring &&
                t.out_off[3] == d.off + o_xy && t.out_off[4] == g.out_off[4] && t.out_off[5] == g.out_off[5]);
        REQUIRE(!std::memcmp(t.in_off, g.in_off, sizeof g.in_off) && !std::memcmp(t.in_len, g.in_len, sizeof g.in_len) &&
                !std::memcmp(t.in_res, g.in_res, sizeof g.in_res) && t.part_cap == g.part_cap && t.ring_cap == g.ring_cap &&
                t.coord_cap == g.coord_cap && t.flags == g.flags);
        if (descs.size() < 4096) descs.push_back(d);  // (what a plan keeps: a heap array, under ASan)
        off = end;
        ++checked;
    }
    // a plan's records in order: slices back to back, inside the total
    for (size_t i = 1; i < descs.size(); ++i) {
        const covt_simplify_desc& p = descs[i - 1];
        REQUIRE(descs[i].off == p.off + simplify_slice_bytes(p.n_features, p.part_cap, p.ring_cap, p.coord_cap));
    }
    std::printf("ok %ld\n", checked);
    return 0;
}

// mvt_layout_check.cc -- TEST INFRASTRUCTURE: the MVT layout rule of cov-tiles_amd/csrc/covt_mvt_plan.h (type |
// offsets | bytes | scratch, every member padded to 16 bytes, 16-byte aligned disjoint slices, the too-large
// flag), the option rule, zigzag and the varint length, and the capacity formula held against the bytes the
// definition emits for worst-case columns (every delta a 5-byte varint), run on the CPU in a stand-alone program,
// built by tests/test_mvt_ref.py with -fsanitize=address,undefined.  Prints "ok <columns checked>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "covt_mvt_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int64_t a16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// bytes of a varint, the slow way
static int slow_len(uint32_t v) {
    int n = 1;
    while (v >= 0x80) v >>= 7, ++n;
    return n;
}

// The bytes the definition emits for a feature of `kind` (0 points, 1 lines, 2 polygons) whose rings have the
// lengths m[], every coordinate alternating between the int32 extremes (so every parameter takes 5 bytes; a
// polygon ring of odd length is closed, one of even length is not).
static int64_t worst_bytes(int kind, const std::vector<int32_t>& m) {
    int64_t total = 0, coords = 0;
    for (int32_t k : m) coords += k;
    if (kind == 0) return coords ? slow_len((uint32_t)(coords << 3) | 1u) + 10 * coords : 0;
    for (int32_t mm : m) {
        if (mm == 0) continue;
        const bool closed = kind == 2 && mm >= 2 && (mm & 1);
        const int32_t k = mm - (closed ? 1 : 0);
        total += 1 + 10 * (int64_t)k;
        if (k > 1) total += slow_len(((uint32_t)(k - 1) << 3) | 2u);
        if (kind == 2) total += 1;
    }
    return total;
}

int main() {
    static_assert(sizeof(covt_mvt_desc) == 32, "covt_mvt_desc");
    static_assert(sizeof(covt_mvt_info) == 48, "covt_mvt_info");
    static_assert(sizeof(covt_mvt_result) == 16, "covt_mvt_result");
    static_assert(sizeof(covt_mvt_options) == 16, "covt_mvt_options");
    // the option rule
    covt_mvt_options o{(uint32_t)sizeof(covt_mvt_options), 0, 0, 0};
    REQUIRE(mvt_options_valid(&o) && !mvt_options_valid(nullptr));
    o.flags = COVT_MVT_ORIENT, o.shift = COVT_MVT_MAX_SHIFT;
    REQUIRE(mvt_options_valid(&o) && COVT_MVT_MAX_SHIFT == 30);
    for (int32_t s : {-1, 31, INT32_MIN, INT32_MAX}) {
        o.shift = s;
        REQUIRE(!mvt_options_valid(&o));
    }
    o.shift = 0;
    for (uint32_t f : {2u, 3u, 0x80000000u, 0xffffffffu}) {
        o.flags = f;
        REQUIRE(!mvt_options_valid(&o));
    }
    o.flags = 0;
    for (uint32_t sz : {0u, 12u, 15u, 17u, 32u}) {
        o.size = sz;
        REQUIRE(!mvt_options_valid(&o));
    }
    // zigzag and the varint length
    REQUIRE(mvt_zigzag(0) == 0 && mvt_zigzag((uint32_t)-1) == 1 && mvt_zigzag(1) == 2 && mvt_zigzag((uint32_t)-2) == 3);
    REQUIRE(mvt_zigzag((uint32_t)INT32_MAX) == 0xfffffffeu && mvt_zigzag((uint32_t)INT32_MIN) == 0xffffffffu);
    for (int b = 0; b < 32; ++b)
        for (int64_t d = -2; d <= 2; ++d) {
            const int64_t v = ((int64_t)1 << b) + d;
            if (v < 0 || v > (int64_t)UINT32_MAX) continue;
            REQUIRE(mvt_varint_len((uint32_t)v) == slow_len((uint32_t)v));
        }
    REQUIRE(mvt_varint_len(0) == 1 && mvt_varint_len(UINT32_MAX) == 5);
    // a few slices by hand
    REQUIRE(mvt_capacity(0, 0, 0) == 0 && mvt_capacity(1, 1, 1) == 22 && mvt_capacity(3, 4, 9) == 133);
    REQUIRE(mvt_slice_bytes(0, 0, 0, 0) == 0 + 16 + 0 + 0 + 0 + 16);
    REQUIRE(mvt_slice_bytes(3, 133, 4, 9) == 16 + 16 + 144 + 64 + 16 + 16);
    REQUIRE(mvt_chunks(0) == 0 && mvt_chunks(1) == 1 && mvt_chunks(COVT_MVT_CHUNK) == 1 && mvt_chunks(COVT_MVT_CHUNK + 1) == 2);
    // no int32 arithmetic
    REQUIRE(mvt_capacity(INT32_MAX, INT32_MAX, INT32_MAX) == 22ll * INT32_MAX);
    REQUIRE(mvt_ring_base_off(0, 0, INT32_MAX) == 16 + a16(16ll * INT32_MAX));
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 1 << 25, (1 << 25) + 1, 97612892, 97612893,
                            214748364, 214748365, INT32_MAX - 1, INT32_MAX, -1, INT32_MIN};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    auto pick = [&](uint64_t r, int32_t mod) {
        return (r & 3) == 0 ? edge[(r >> 8) % (uint64_t)n_edge] : (int32_t)((r >> 8) % (uint64_t)mod);
    };
    std::vector<covt_mvt_desc> descs;
    int64_t off = 0;
    long checked = 0;
    for (int it = 0; it < 200000; ++it) {
        const int32_t n = pick(next(), 5000), rc = pick(next(), 9000), cc = pick(next(), 70000);
        const uint32_t gflags = (next() & 15) == 0 ? COVT_GEOM_TOO_LARGE : (uint32_t)(next() & 1);
        covt_mvt_desc d;
        std::memset(&d, 0xee, sizeof d);  // every field is set by the rule
        const int64_t end = mvt_column_layout(n, rc, cc, gflags, off, d);
        const int64_t cap = 10ll * cc + 7ll * rc + 5ll * n;
        const bool fits = !(gflags & COVT_GEOM_TOO_LARGE) && n >= 0 && rc >= 0 && cc >= 0 && cap <= INT32_MAX;
        REQUIRE((d.flags == 0) == fits && (d.flags == 0 || d.flags == COVT_MVT_TOO_LARGE));
        // a refused column: zero rows and no capacity
        REQUIRE(d.n_features == (fits ? n : 0) && d.ring_cap == (fits ? rc : 0) && d.coord_cap == (fits ? cc : 0) &&
                d.byte_cap == (fits ? cap : 0));
        REQUIRE(d.off == off && (d.off & 15) == 0 && (end & 15) == 0);
        const int64_t nf = d.n_features, R = d.ring_cap, V = d.coord_cap, B = d.byte_cap;
        const int64_t bytes = mvt_slice_bytes(nf, B, R, V);
        REQUIRE(end == d.off + bytes && (bytes & 15) == 0);
        // the members back to back, each 16-byte aligned and large enough for what it holds
        const int64_t o_t = mvt_type_off(nf), o_o = mvt_offsets_off(nf), o_b = mvt_bytes_off(nf), o_r = mvt_ring_rec_off(nf, B),
                      o_rb = mvt_ring_base_off(nf, B, R), o_ck = mvt_chunk_k_off(nf, B, R);
        REQUIRE(o_t == 0 && o_o == a16(nf) && o_b == o_o + a16(4 * (nf + 1)) && o_r == o_b + a16(B));
        REQUIRE(o_rb == o_r + a16(COVT_MVT_RING_REC * R) && o_ck == o_rb + a16(4 * R));
        REQUIRE(bytes == o_ck + a16(4 * (mvt_chunks(V) + 1)));
        REQUIRE(!((o_o | o_b | o_r | o_rb | o_ck) & 15));
        REQUIRE(mvt_chunks(V) * COVT_MVT_CHUNK >= V && (mvt_chunks(V) - 1) * COVT_MVT_CHUNK < V + (V == 0));
        if (descs.size() < 4096) descs.push_back(d);  // (what a plan keeps: a heap array, under ASan)
        off = end;
        ++checked;
    }
    // a plan's records in order: slices disjoint, back to back, inside the total
    for (size_t i = 1; i < descs.size(); ++i) {
        const covt_mvt_desc& p = descs[i - 1];
        REQUIRE(descs[i].off == p.off + mvt_slice_bytes(p.n_features, p.byte_cap, p.ring_cap, p.coord_cap));
    }
    // the capacity against worst-case columns with exactly the capacities they need: features of every kind, rings
    // of 0 .. 40 coordinates and a few long ones (LineTo counts of 2, 3 and 4 bytes)
    for (int it = 0; it < 20000; ++it) {
        const int nf = (int)(next() % 6);
        int64_t total = 0, rings = 0, coords = 0;
        for (int f = 0; f < nf; ++f) {
            const int kind = (int)(next() % 3);
            std::vector<int32_t> m((size_t)(next() % 5));
            for (int32_t& x : m) {
                const uint64_t r = next();
                x = (r & 31) == 0 ? (int32_t)(1 + (r >> 8) % 3000000) : (int32_t)((r >> 8) % 41);
            }
            total += worst_bytes(kind, m);
            rings += (int64_t)m.size();
            for (int32_t x : m) coords += x;
        }
        REQUIRE(total <= mvt_capacity(nf, rings, coords));
    }
    // the formula is tight per term: one coordinate, one ring, one point feature
    REQUIRE(worst_bytes(1, {1}) == 11 && worst_bytes(2, {2}) == 1 + 20 + 1 + 1);
    REQUIRE(worst_bytes(0, std::vector<int32_t>{1 << 28}) == 5 + 10ll * (1 << 28));
    std::printf("ok %ld\n", checked);
    return 0;
}

// product_records_check.cc -- TEST INFRASTRUCTURE: the per-column products of cov-tiles_amd/csrc/covt_products.h
// (the list, each product's trait and product_record, the one writer of a column's record and descriptor) run on
// the CPU in a stand-alone program, built by tests/test_product_records.py with -fsanitize=address,undefined.
// Over random runs of geometry columns, for every listed product: the host plan's loop (a running offset) and the
// device plan's formulation (a column's bytes from layout at 0, their exclusive sum) give the same slices, and
// every record agrees with its column and its descriptor.  Prints "ok <(run, product) pairs checked>".
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "covt_products.h"

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::fprintf(stderr, "line %d (%s): %s\n", __LINE__, __PRETTY_FUNCTION__, #c); \
            return false;                                                           \
        }                                                                           \
    } while (0)

// has_f<T>: T has a member f; same_f(a, b, n): a.f == b.f if both have one (n counts the fields compared)
#define FIELD(f)                                                                              \
    template <class T, class = void>                                                          \
    struct has_##f : std::false_type {};                                                      \
    template <class T>                                                                        \
    struct has_##f<T, std::void_t<decltype(std::declval<T>().f)>> : std::true_type {};        \
    template <class A, class B>                                                               \
    bool same_##f(const A& a, const B& b, int& n) {                                           \
        if constexpr (has_##f<A>::value && has_##f<B>::value) {                               \
            ++n;                                                                              \
            return a.f == b.f;                                                                \
        } else {                                                                              \
            return true;                                                                      \
        }                                                                                     \
    }                                                                                         \
    template <class A>                                                                        \
    int64_t get_##f(const A& a) {                                                             \
        if constexpr (has_##f<A>::value) return (int64_t)a.f;                                 \
        else return 0;                                                                        \
    }
// every member name of a product's descriptor
FIELD(off)
FIELD(offsets_off)
FIELD(bytes_off)
FIELD(byte_cap)
FIELD(n_features)
FIELD(flags)
FIELD(part_cap)
FIELD(ring_cap)
FIELD(coord_cap)
FIELD(reserved)

// the geometry column's capacities a product's layout rule reads (include/covt.h, the product's section): a
// negative one refuses the column
enum { PART = 1, RING = 2, COORD = 4 };
template <class P> constexpr int kReads = -1;
template <> constexpr int kReads<WkbProduct> = PART | RING | COORD;
template <> constexpr int kReads<BboxProduct> = 0;
template <> constexpr int kReads<MeasuresProduct> = RING;
template <> constexpr int kReads<SelectProduct> = PART | RING | COORD;  // (its byte_cap is the WKB column's)
template <> constexpr int kReads<SimplifyProduct> = PART | RING | COORD;
template <> constexpr int kReads<MvtProduct> = RING | COORD;

template <class P>
bool check_product(const std::vector<covt_geom_info>& g) {
    using Info = typename P::Info;
    using Desc = typename P::Desc;
    static_assert(kReads<P> >= 0, "a listed product this check does not know");
    const size_t nc = g.size();
    // the host plan's loop
    std::vector<Info> info(nc);
    std::vector<Desc> desc(nc);
    std::vector<int64_t> next(nc);
    int64_t off = 0;
    for (size_t c = 0; c < nc; ++c) next[c] = off = product_record<P>(g[c], off, info[c], desc.data());
    // the device plan's: column bytes from the rule at offset 0, the slices at their exclusive sum
    int64_t sum = 0, prev_end = 0;
    for (size_t c = 0; c < nc; ++c) {
        const Info& r = info[c];
        const Desc& d = desc[(size_t)g[c].desc_index];
        REQUIRE(r.tile == g[c].tile && r.layer == g[c].layer && r.desc_index == g[c].desc_index);
        int shared = 0;
        REQUIRE(same_off(r, d, shared) && same_offsets_off(r, d, shared) && same_bytes_off(r, d, shared) &&
                same_byte_cap(r, d, shared) && same_n_features(r, d, shared) && same_flags(r, d, shared) &&
                same_part_cap(r, d, shared) && same_ring_cap(r, d, shared) && same_coord_cap(r, d, shared) &&
                same_reserved(r, d, shared));
        REQUIRE(shared >= 3);  // rows, flags and where the slice is, at the least
        const int64_t start = has_off<Desc>::value ? get_off(d) : get_offsets_off(d);
        REQUIRE(start % 16 == 0 && start >= prev_end && start == sum);
        Desc d0{};
        const int64_t bytes = P::layout(g[c], 0, d0);
        REQUIRE(bytes >= 0 && bytes % 16 == 0);
        sum += bytes;
        prev_end = next[c];
        REQUIRE(prev_end == sum && prev_end % 16 == 0);
        // refused columns
        const bool must_refuse = ((uint32_t)g[c].flags & COVT_GEOM_TOO_LARGE) || ((kReads<P> & PART) && g[c].part_cap < 0) ||
                                 ((kReads<P> & RING) && g[c].ring_cap < 0) || ((kReads<P> & COORD) && g[c].coord_cap < 0);
        const bool refused = ((uint32_t)d.flags & P::kTooLarge) != 0;
        REQUIRE(refused || !must_refuse);
        if (refused) {
            REQUIRE((uint32_t)d.flags == P::kTooLarge && d.n_features == 0);
            REQUIRE(get_byte_cap(d) == 0 && get_part_cap(d) == 0 && get_ring_cap(d) == 0 && get_coord_cap(d) == 0);
        } else {
            REQUIRE(d.flags == 0 && d.n_features == g[c].n_features);
            REQUIRE(get_byte_cap(d) >= 0 && get_byte_cap(d) <= INT32_MAX);
            REQUIRE(!has_part_cap<Desc>::value || get_part_cap(d) == g[c].part_cap);
            REQUIRE(!has_ring_cap<Desc>::value || get_ring_cap(d) == g[c].ring_cap);
            REQUIRE(!has_coord_cap<Desc>::value || get_coord_cap(d) == g[c].coord_cap);
        }
    }
    REQUIRE(off == sum);  // the final offset is the total
    return true;
}

int main() {
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int32_t edge[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, COVT_GEOM_MAX_CAP - 1, COVT_GEOM_MAX_CAP};
    const size_t n_edge = sizeof edge / sizeof edge[0];
    // a count or capacity in [0, COVT_GEOM_MAX_CAP]: an edge value, a small one or any
    auto value = [&]() {
        const uint64_t r = next();
        if ((r & 3) == 0) return edge[(r >> 8) % n_edge];
        if ((r & 3) == 1) return (int32_t)((r >> 8) % ((uint64_t)COVT_GEOM_MAX_CAP + 1));
        return (int32_t)((r >> 8) % 3000);
    };
    long checked = 0;
    for (int it = 0; it < 20000; ++it) {
        const size_t nc = it < 64 ? (size_t)(it % 4) : (size_t)(next() % 48);
        std::vector<covt_geom_info> g(nc);
        for (size_t c = 0; c < nc; ++c) {  // (desc_index: a random permutation)
            g[c].desc_index = (int32_t)c;
            std::swap(g[c].desc_index, g[(size_t)(next() % (c + 1))].desc_index);
        }
        int32_t tile = 0;
        for (size_t c = 0; c < nc; ++c) {
            covt_geom_info& q = g[c];
            tile += (int32_t)(next() % 3);
            q.tile = tile;
            q.layer = (int32_t)(next() % 5);
            q.n_features = value();
            q.part_cap = value();
            q.ring_cap = value();
            q.coord_cap = value();
            const uint64_t r = next();
            q.flags = (r & 1) ? (int32_t)COVT_GEOM_CLOSED_IN_STREAM : 0;
            if (((r >> 1) & 15) == 0) {  // a column assembly refuses: no capacity
                q.flags = (int32_t)((uint32_t)q.flags | COVT_GEOM_TOO_LARGE);
                q.part_cap = q.ring_cap = q.coord_cap = 0;
            }
            if (((r >> 5) & 15) == 0) {  // a capacity no plan writes
                int32_t* cap[3] = {&q.part_cap, &q.ring_cap, &q.coord_cap};
                *cap[(r >> 9) % 3] = ((r >> 12) & 1) ? -1 : -(int32_t)((r >> 13) % COVT_GEOM_MAX_CAP) - 1;
            }
        }
        bool ok = true;
        Products::for_each([&](auto product) {
            ok = ok && check_product<decltype(product)>(g);
            ++checked;
        });
        if (!ok) return 1;
    }
    std::printf("ok %ld\n", checked);
    return 0;
}

// query_check -- covt_query_plan.h on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, against a
// table the Python reference (tests/covt_query.py, query_ref's parts) writes to stdin:
//
//   S ax ay bx by wx0 wy0 wx1 wy1 in_a meets cross edge    one segment against one window
//   P x y wx0 wy0 wx1 wy1 value                            a ring of one coordinate
//   V size flags relation reserved valid                   query_valid
//   F value type has_coord relation keep                   the per-feature rule
//
// and, with no table, the join: associative, commutative, 0 its identity, over all 8 x 8 x 8 triples.
// Prints "ok <checks>"; the first disagreement is printed and the exit status is 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "covt_query_plan.h"

static long checks = 0;

static int fail(const char* what, const char* line) {
    std::printf("FAIL %s: %s\n", what, line);
    return 1;
}

int main() {
    for (uint32_t a = 0; a < 8; ++a)
        for (uint32_t b = 0; b < 8; ++b) {
            if (query_join(a, b) != query_join(b, a) || query_join(a, b) > 7u) return fail("join commutes", "");
            for (uint32_t c = 0; c < 8; ++c, ++checks)
                if (query_join(query_join(a, b), c) != query_join(a, query_join(b, c))) return fail("join associates", "");
        }
    for (uint32_t a = 0; a < 8; ++a)
        if (query_join(a, 0u) != a || query_join(0u, a) != a) return fail("join identity", "");
    if (query_valid(nullptr)) return fail("query_valid(null)", "");

    char line[512];
    while (std::fgets(line, sizeof line, stdin)) {
        long long v[12];
        if (line[0] == 'S') {
            if (std::sscanf(line + 1, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3,
                            v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11) != 12)
                return fail("parse", line);
            const QueryWindow w{(int32_t)v[4], (int32_t)v[5], (int32_t)v[6], (int32_t)v[7]};
            const int32_t ax = (int32_t)v[0], ay = (int32_t)v[1], bx = (int32_t)v[2], by = (int32_t)v[3];
            if (query_in(w, ax, ay) != (v[8] != 0)) return fail("in", line);
            if (query_meets(w, ax, ay, bx, by) != (v[9] != 0)) return fail("meets", line);
            if (query_meets(w, bx, by, ax, ay) != (v[9] != 0)) return fail("meets, reversed", line);
            if (query_cross(w, ax, ay, bx, by) != (v[10] != 0)) return fail("cross", line);
            if (query_edge(w, ax, ay, bx, by) != (uint32_t)v[11]) return fail("edge", line);
            // the routes: the corner test alone agrees wherever the early answers did not already say no
            if (v[9] != 0 && !query_corners_split(w, ax, ay, bx, by)) return fail("corners", line);
            checks += 6;
        } else if (line[0] == 'P') {
            if (std::sscanf(line + 1, "%lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) != 7)
                return fail("parse", line);
            const QueryWindow w{(int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)v[5]};
            if (query_point(w, (int32_t)v[0], (int32_t)v[1]) != (uint32_t)v[6]) return fail("point", line);
            ++checks;
        } else if (line[0] == 'V') {
            if (std::sscanf(line + 1, "%lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4) != 5) return fail("parse", line);
            covt_select_query q;
            std::memset(&q, 0, sizeof q);
            q.size = (uint32_t)v[0], q.flags = (uint32_t)v[1], q.relation = (int32_t)v[2], q.reserved = (int32_t)v[3];
            if (query_valid(&q) != (v[4] != 0)) return fail("valid", line);
            ++checks;
        } else if (line[0] == 'F') {
            if (std::sscanf(line + 1, "%lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4) != 5) return fail("parse", line);
            if (query_feature((uint32_t)v[0], (uint32_t)v[1], v[2] != 0, (int32_t)v[3]) != (v[4] != 0)) return fail("feature", line);
            ++checks;
        }
    }
    std::printf("ok %ld\n", checks);
    return 0;
}

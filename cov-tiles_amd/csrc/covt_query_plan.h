// covt_query_plan.h -- the rules of the query pass (include/covt.h "Geometry queries"), shared by the kernels
// (covt_query.hip), the host entry points and a host-only check program: the argument rule, the point, segment
// and crossing tests against a closed int32 window, an edge's term, the join of two ring values and the
// per-feature rule.  Plain integer arithmetic, no HIP calls, so a host-only program can include it.
//
// A ring's value is three bits: touch | out << 1 | par << 2 (kQueryTouch, kQueryOut, kQueryPar).  touch and
// out are ORed and par is XORed over edges, rings and parts alike, so one join serves every level.
//
// The signs of the two wide expressions (33-bit differences, 66-bit products) are taken in __int128, exact.
// Both stand behind compares on the coordinates themselves: query_meets first rejects on the segment's box and
// accepts on an end point inside, query_cross first asks whether the segment straddles the ray's line, so the
// common edge costs a handful of 32-bit compares and the answers do not depend on which route was taken.
#ifndef COVT_QUERY_PLAN_H
#define COVT_QUERY_PLAN_H

#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_QUERY_HD __host__ __device__
#else
#define COVT_QUERY_HD
#endif

constexpr uint32_t kQueryTouch = 1u, kQueryOut = 2u, kQueryPar = 4u;

// the closed window [x0, x1] x [y0, y1]; Q = (x0, y0)
struct QueryWindow {
    int32_t x0, y0, x1, y1;
};

// the query a call accepts: its size, no flag, nothing reserved, a known relation
COVT_QUERY_HD inline bool query_valid(const covt_select_query* q) {
    if (!q || q->size != (uint32_t)sizeof(covt_select_query)) return false;
    if (q->flags != 0 || q->reserved != 0) return false;
    return q->relation == COVT_QUERY_INTERSECTS || q->relation == COVT_QUERY_WITHIN;
}
COVT_QUERY_HD inline QueryWindow query_window(const covt_select_query& q) {
    return QueryWindow{q.window[0], q.window[1], q.window[2], q.window[3]};
}
// an inverted window holds no point: every feature gets 0 for both relations
COVT_QUERY_HD inline bool query_inverted(const QueryWindow& w) { return w.x0 > w.x1 || w.y0 > w.y1; }

// in(p)
COVT_QUERY_HD inline bool query_in(const QueryWindow& w, int32_t x, int32_t y) {
    return w.x0 <= x && x <= w.x1 && w.y0 <= y && y <= w.y1;
}

// the sign (-1, 0, 1) of dx * ey - dy * ex, every factor a difference of two int32
COVT_QUERY_HD inline int query_wide_sign(int64_t dx, int64_t ey, int64_t dy, int64_t ex) {
    const __int128 s = (__int128)dx * ey - (__int128)dy * ex;
    return s > 0 ? 1 : s < 0 ? -1 : 0;
}

// step 3 of meets(a, b): the corners of W are not all strictly on one side of the line ab
COVT_QUERY_HD inline bool query_corners_split(const QueryWindow& w, int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay;
    const int64_t ex0 = (int64_t)w.x0 - ax, ex1 = (int64_t)w.x1 - ax, ey0 = (int64_t)w.y0 - ay, ey1 = (int64_t)w.y1 - ay;
    const int s0 = query_wide_sign(dx, ey0, dy, ex0), s1 = query_wide_sign(dx, ey0, dy, ex1);
    const int s2 = query_wide_sign(dx, ey1, dy, ex0), s3 = query_wide_sign(dx, ey1, dy, ex1);
    const bool all_pos = s0 > 0 && s1 > 0 && s2 > 0 && s3 > 0, all_neg = s0 < 0 && s1 < 0 && s2 < 0 && s3 < 0;
    return !all_pos && !all_neg;
}

// meets(a, b): the closed segment ab and W share a point
COVT_QUERY_HD inline bool query_meets(const QueryWindow& w, int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    const int32_t lox = ax < bx ? ax : bx, hix = ax < bx ? bx : ax, loy = ay < by ? ay : by, hiy = ay < by ? by : ay;
    if (hix < w.x0 || lox > w.x1 || hiy < w.y0 || loy > w.y1) return false;
    if (query_in(w, ax, ay) || query_in(w, bx, by)) return true;
    return query_corners_split(w, ax, ay, bx, by);
}

// cross(a, b): the edge ab crosses the ray from Q in +x, half-open in y
COVT_QUERY_HD inline bool query_cross(const QueryWindow& w, int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    if ((ay > w.y0) == (by > w.y0)) return false;
    const int d = query_wide_sign((int64_t)w.y0 - ay, (int64_t)bx - ax, (int64_t)w.x0 - ax, (int64_t)by - ay);
    return (d > 0) == (by > ay);
}

// the term of the edge from (x0, y0) to (x1, y1)
COVT_QUERY_HD inline uint32_t query_edge(const QueryWindow& w, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    uint32_t v = query_meets(w, x0, y0, x1, y1) ? kQueryTouch : 0u;
    if (!query_in(w, x0, y0) || !query_in(w, x1, y1)) v |= kQueryOut;
    if (query_cross(w, x0, y0, x1, y1)) v |= kQueryPar;
    return v;
}
// the value of a ring of the one coordinate (x, y): no edge, so touch is in(p)
COVT_QUERY_HD inline uint32_t query_point(const QueryWindow& w, int32_t x, int32_t y) {
    return query_in(w, x, y) ? kQueryTouch : kQueryOut;
}

// two values joined: touch and out ORed, par XORed (associative and commutative, 0 its identity)
COVT_QUERY_HD inline uint32_t query_join(uint32_t a, uint32_t b) { return ((a | b) & 3u) | ((a ^ b) & 4u); }

// P_f from the join of the feature's ring values, its GeometryTypes ordinal and whether it has a coordinate
// (the window not inverted)
COVT_QUERY_HD inline bool query_feature(uint32_t v, uint32_t type, bool has_coord, int32_t relation) {
    if (!has_coord) return false;
    if (relation == COVT_QUERY_WITHIN) return !(v & kQueryOut);
    return (v & kQueryTouch) || ((type == 2u || type == 5u) && (v & kQueryPar));
}

#endif

// covt_simplify_plan.h -- the simplify output layout of a plan and the shift's argument rule (include/covt.h
// "Geometry simplification"), shared by the host plan (covt_host.cpp), the device plan (covt_plan_device.hip)
// and the kernels (covt_simplify.hip): plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_SIMPLIFY_PLAN_H
#define COVT_SIMPLIFY_PLAN_H

#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_SIMPLIFY_HD __host__ __device__
#else
#define COVT_SIMPLIFY_HD
#endif

COVT_SIMPLIFY_HD inline int64_t simplify_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// coordinates per chunk of the count and write passes: the scratch holds one kept count per chunk
#define COVT_SIMPLIFY_CHUNK 1024

// A column's slice: geometry_offsets[n + 1] int32 | part_offsets[part_cap + 1] int32 | ring_offsets[ring_cap + 1]
// int32 | coords[2 * coord_cap] int32 | scratch: ring_k[ring_cap] uint32 (a ring's kept count, bit 31: a ring of
// points) | chunk_k[chunks(coord_cap) + 1] uint32 (a chunk's kept count, then its first destination); every
// member padded to 16 bytes.  Byte offsets inside the slice:
COVT_SIMPLIFY_HD inline int64_t simplify_geo_off(int64_t) { return 0; }
COVT_SIMPLIFY_HD inline int64_t simplify_part_off(int64_t n) { return simplify_align16(4 * (n + 1)); }
COVT_SIMPLIFY_HD inline int64_t simplify_ring_off(int64_t n, int64_t part_cap) {
    return simplify_part_off(n) + simplify_align16(4 * (part_cap + 1));
}
COVT_SIMPLIFY_HD inline int64_t simplify_coords_off(int64_t n, int64_t part_cap, int64_t ring_cap) {
    return simplify_ring_off(n, part_cap) + simplify_align16(4 * (ring_cap + 1));
}
COVT_SIMPLIFY_HD inline int64_t simplify_ring_k_off(int64_t n, int64_t part_cap, int64_t ring_cap, int64_t coord_cap) {
    return simplify_coords_off(n, part_cap, ring_cap) + simplify_align16(8 * coord_cap);
}
COVT_SIMPLIFY_HD inline int64_t simplify_chunks(int64_t coord_cap) {
    return (coord_cap + COVT_SIMPLIFY_CHUNK - 1) / COVT_SIMPLIFY_CHUNK;
}
COVT_SIMPLIFY_HD inline int64_t simplify_chunk_k_off(int64_t n, int64_t part_cap, int64_t ring_cap, int64_t coord_cap) {
    return simplify_ring_k_off(n, part_cap, ring_cap, coord_cap) + simplify_align16(4 * ring_cap);
}
COVT_SIMPLIFY_HD inline int64_t simplify_slice_bytes(int64_t n, int64_t part_cap, int64_t ring_cap, int64_t coord_cap) {
    return simplify_chunk_k_off(n, part_cap, ring_cap, coord_cap) + simplify_align16(4 * (simplify_chunks(coord_cap) + 1));
}

// The simplify record of one geometry column whose slice starts at `off` (16-byte aligned); returns the offset
// after it.  The capacities are the geometry column's: the output never exceeds the input.  A column assembly
// refuses (COVT_GEOM_TOO_LARGE) gets COVT_SIMPLIFY_TOO_LARGE, no rows and no capacity.
COVT_SIMPLIFY_HD inline int64_t simplify_column_layout(int32_t n_features, int32_t part_cap, int32_t ring_cap,
                                                       int32_t coord_cap, uint32_t geom_flags, int64_t off,
                                                       covt_simplify_desc& s) {
    const bool fits = !(geom_flags & COVT_GEOM_TOO_LARGE) && n_features >= 0 && part_cap >= 0 && ring_cap >= 0 &&
                      coord_cap >= 0;
    s.off = off;
    s.n_features = fits ? n_features : 0;
    s.flags = fits ? 0 : COVT_SIMPLIFY_TOO_LARGE;
    s.part_cap = fits ? part_cap : 0;
    s.ring_cap = fits ? ring_cap : 0;
    s.coord_cap = fits ? coord_cap : 0;
    s.reserved = 0;
    return simplify_align16(off + simplify_slice_bytes(s.n_features, s.part_cap, s.ring_cap, s.coord_cap));
}

// The simplify product of a plan (covt_products.h).  Its result is a geometry result: the simplified column's
// counts.
struct SimplifyProduct {
    using Info = covt_simplify_info;
    using Desc = covt_simplify_desc;
    using Res = covt_geom_result;
    static constexpr uint32_t kTooLarge = COVT_SIMPLIFY_TOO_LARGE;
    static constexpr bool kReadsSimplified = false;  // the pass that writes the simplified column reads the assembled one
    COVT_SIMPLIFY_HD static int64_t layout(const covt_geom_info& g, int64_t off, Desc& d) {
        return simplify_column_layout(g.n_features, g.part_cap, g.ring_cap, g.coord_cap, (uint32_t)g.flags, off, d);
    }
    COVT_SIMPLIFY_HD static void fill(Info& r, const Desc& d) {
        r.off = d.off;
        r.part_cap = d.part_cap;
        r.ring_cap = d.ring_cap;
        r.coord_cap = d.coord_cap;
    }
};

// the geometry descriptor whose out_off[0 .. 3] name the simplified column in the simplify buffer (the inputs,
// the capacities and the two scratch offsets stay): what every pass that reads an assembled column takes
COVT_SIMPLIFY_HD inline covt_geom_desc simplify_retarget(covt_geom_desc g, const covt_simplify_desc& s) {
    g.out_off[0] = s.off + simplify_geo_off(s.n_features);
    g.out_off[1] = s.off + simplify_part_off(s.n_features);
    g.out_off[2] = s.off + simplify_ring_off(s.n_features, s.part_cap);
    g.out_off[3] = s.off + simplify_coords_off(s.n_features, s.part_cap, s.ring_cap);
    return g;
}

// the shifts a call accepts
COVT_SIMPLIFY_HD inline bool simplify_shift_valid(int32_t s) { return s >= 0 && s <= COVT_SIMPLIFY_MAX_SHIFT; }

// snap(v) of the definition: round half up to the grid of 2^s, clamped to the largest grid value in int32
COVT_SIMPLIFY_HD inline int32_t simplify_snap(int32_t v, int32_t s) {
    const int64_t h = s ? (int64_t)1 << (s - 1) : 0;
    const int64_t t = (int64_t)((uint64_t)(((int64_t)v + h) >> s) << s);
    const int64_t m = (int64_t)((INT32_MAX >> s) << s);
    return (int32_t)(t < m ? t : m);
}

#endif

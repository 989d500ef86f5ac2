// covt_wkb_plan.h -- the WKB output layout of a plan (include/covt.h "Geometry as WKB"), shared by the
// host plan (covt_host.cpp), the device plan (covt_plan_device.hip) and the kernels (covt_wkb.hip):
// plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_WKB_PLAN_H
#define COVT_WKB_PLAN_H

#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_WKB_HD __host__ __device__
#else
#define COVT_WKB_HD
#endif

COVT_WKB_HD inline int64_t wkb_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// bytes a column's WKB values can take at most: every feature and part a 9-byte header (a POINT's 5 and a
// MULTIPOINT point's 5 + its 16 coordinate bytes are within 9 + 16), every ring a count, every coordinate 16
COVT_WKB_HD inline int64_t wkb_capacity(int64_t n_features, int64_t part_cap, int64_t ring_cap, int64_t coord_cap) {
    return 9 * (n_features + part_cap) + 4 * ring_cap + 16 * coord_cap;
}

// The WKB record of one geometry column whose slices start at `off` (16-byte aligned); returns the offset
// after them.  A column assembly refuses (COVT_GEOM_TOO_LARGE) or whose capacity passes INT32_MAX (the
// offsets are int32) gets COVT_WKB_TOO_LARGE, a one-entry offsets slice and no bytes.
COVT_WKB_HD inline int64_t wkb_column_layout(int32_t n_features, int32_t part_cap, int32_t ring_cap, int32_t coord_cap,
                                             uint32_t geom_flags, int64_t off, covt_wkb_desc& w) {
    const int64_t cap = wkb_capacity(n_features, part_cap, ring_cap, coord_cap);
    const bool fits = !(geom_flags & COVT_GEOM_TOO_LARGE) && n_features >= 0 && part_cap >= 0 && ring_cap >= 0 &&
                      coord_cap >= 0 && cap <= INT32_MAX;
    w.n_features = fits ? n_features : 0;
    w.flags = fits ? 0 : COVT_WKB_TOO_LARGE;
    w.byte_cap = fits ? cap : 0;
    w.offsets_off = off;
    off = wkb_align16(off + 4 * ((int64_t)w.n_features + 1));
    w.bytes_off = off;
    return wkb_align16(off + w.byte_cap);
}

// The WKB product of a plan (covt_products.h): its record, descriptor and result types, the layout rule over a
// geometry column and the offsets the record repeats from the descriptor.
struct WkbProduct {
    using Info = covt_wkb_info;
    using Desc = covt_wkb_desc;
    using Res = covt_wkb_result;
    static constexpr uint32_t kTooLarge = COVT_WKB_TOO_LARGE;
    static constexpr bool kReadsSimplified = true;  // covt_plan_set_simplify: the pass takes the simplified column
    COVT_WKB_HD static int64_t layout(const covt_geom_info& g, int64_t off, Desc& d) {
        return wkb_column_layout(g.n_features, g.part_cap, g.ring_cap, g.coord_cap, (uint32_t)g.flags, off, d);
    }
    COVT_WKB_HD static void fill(Info& w, const Desc& d) {
        w.offsets_off = d.offsets_off;
        w.bytes_off = d.bytes_off;
        w.byte_cap = d.byte_cap;
    }
};

#endif

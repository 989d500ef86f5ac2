// covt_bbox_plan.h -- the bounding-box output layout of a plan (include/covt.h "Geometry bounding boxes"),
// shared by the host plan (covt_host.cpp), the device plan (covt_plan_device.hip) and the kernels
// (covt_bbox.hip): plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_BBOX_PLAN_H
#define COVT_BBOX_PLAN_H

#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_BBOX_HD __host__ __device__
#else
#define COVT_BBOX_HD
#endif

COVT_BBOX_HD inline int64_t bbox_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// bytes of a column's slice: xmin | ymin | xmax | ymax, n_features float64 each
COVT_BBOX_HD inline int64_t bbox_slice_bytes(int64_t n_features) { return 32 * n_features; }
// byte offset of array k (0 xmin, 1 ymin, 2 xmax, 3 ymax) inside a column's slice
COVT_BBOX_HD inline int64_t bbox_array_off(int64_t n_features, int k) { return 8 * n_features * k; }

// The bounding-box record of one geometry column whose slice starts at `off` (16-byte aligned); returns the
// offset after it.  A column assembly refuses (COVT_GEOM_TOO_LARGE) gets COVT_BBOX_TOO_LARGE and no rows.
COVT_BBOX_HD inline int64_t bbox_column_layout(int32_t n_features, uint32_t geom_flags, int64_t off, covt_bbox_desc& b) {
    const bool fits = !(geom_flags & COVT_GEOM_TOO_LARGE) && n_features >= 0;
    b.off = off;
    b.n_features = fits ? n_features : 0;
    b.flags = fits ? 0 : COVT_BBOX_TOO_LARGE;
    return bbox_align16(off + bbox_slice_bytes(b.n_features));
}

// The bounding-box product of a plan (covt_products.h).
struct BboxProduct {
    using Info = covt_bbox_info;
    using Desc = covt_bbox_desc;
    using Res = covt_bbox_result;
    static constexpr uint32_t kTooLarge = COVT_BBOX_TOO_LARGE;
    static constexpr bool kReadsSimplified = true;
    COVT_BBOX_HD static int64_t layout(const covt_geom_info& g, int64_t off, Desc& d) {
        return bbox_column_layout(g.n_features, (uint32_t)g.flags, off, d);
    }
    COVT_BBOX_HD static void fill(Info& b, const Desc& d) { b.off = d.off; }
};

#endif

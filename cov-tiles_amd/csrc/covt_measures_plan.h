// covt_measures_plan.h -- the measures output layout of a plan (include/covt.h "Geometry measures"), shared by
// the host plan (covt_host.cpp), the device plan (covt_plan_device.hip) and the kernels (covt_measures.hip):
// plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_MEASURES_PLAN_H
#define COVT_MEASURES_PLAN_H

#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_MEASURES_HD __host__ __device__
#else
#define COVT_MEASURES_HD
#endif

COVT_MEASURES_HD inline int64_t measures_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// A column's slice: area[n] float64 | length[n] float64 | num_coords[n] int32 (padded to 16 bytes) | the
// per-ring scratch: ring_s[ring_cap] int64 (a ring's doubled signed area) | ring_len[ring_cap] float64.
// Byte offsets inside the slice:
COVT_MEASURES_HD inline int64_t measures_area_off(int64_t) { return 0; }
COVT_MEASURES_HD inline int64_t measures_length_off(int64_t n_features) { return 8 * n_features; }
COVT_MEASURES_HD inline int64_t measures_count_off(int64_t n_features) { return 16 * n_features; }
// bytes of the three arrays with their padding = where the scratch starts
COVT_MEASURES_HD inline int64_t measures_rows_bytes(int64_t n_features) {
    return 16 * n_features + measures_align16(4 * n_features);
}
COVT_MEASURES_HD inline int64_t measures_scratch_bytes(int64_t ring_cap) { return 16 * ring_cap; }
COVT_MEASURES_HD inline int64_t measures_ring_s_off(int64_t n_features, int64_t) { return measures_rows_bytes(n_features); }
COVT_MEASURES_HD inline int64_t measures_ring_len_off(int64_t n_features, int64_t ring_cap) {
    return measures_rows_bytes(n_features) + 8 * ring_cap;
}
COVT_MEASURES_HD inline int64_t measures_slice_bytes(int64_t n_features, int64_t ring_cap) {
    return measures_rows_bytes(n_features) + measures_scratch_bytes(ring_cap);
}

// The measures record of one geometry column whose slice starts at `off` (16-byte aligned); returns the offset
// after it.  A column assembly refuses (COVT_GEOM_TOO_LARGE) gets COVT_MEASURES_TOO_LARGE, no rows and no scratch.
COVT_MEASURES_HD inline int64_t measures_column_layout(int32_t n_features, int32_t ring_cap, uint32_t geom_flags,
                                                       int64_t off, covt_measures_desc& m) {
    const bool fits = !(geom_flags & COVT_GEOM_TOO_LARGE) && n_features >= 0 && ring_cap >= 0;
    m.off = off;
    m.n_features = fits ? n_features : 0;
    m.flags = fits ? 0 : COVT_MEASURES_TOO_LARGE;
    m.ring_cap = fits ? ring_cap : 0;
    m.reserved = 0;
    return measures_align16(off + measures_slice_bytes(m.n_features, m.ring_cap));
}

// The measures product of a plan (covt_products.h).
struct MeasuresProduct {
    using Info = covt_measures_info;
    using Desc = covt_measures_desc;
    using Res = covt_measures_result;
    static constexpr uint32_t kTooLarge = COVT_MEASURES_TOO_LARGE;
    static constexpr bool kReadsSimplified = true;
    COVT_MEASURES_HD static int64_t layout(const covt_geom_info& g, int64_t off, Desc& d) {
        return measures_column_layout(g.n_features, g.ring_cap, (uint32_t)g.flags, off, d);
    }
    COVT_MEASURES_HD static void fill(Info& m, const Desc& d) {
        m.off = d.off;
        m.ring_cap = d.ring_cap;
    }
};

#endif

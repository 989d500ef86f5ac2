// covt_select_plan.h -- the select output layout of a plan and the predicate's argument rule (include/covt.h
// "Feature selection"), shared by the host plan (covt_host.cpp), the device plan (covt_plan_device.hip) and the
// kernels (covt_select.hip): plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_SELECT_PLAN_H
#define COVT_SELECT_PLAN_H

#include <stdint.h>

#include "covt.h"
#include "covt_wkb_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_SELECT_HD __host__ __device__
#else
#define COVT_SELECT_HD
#endif

COVT_SELECT_HD inline int64_t select_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// A column's slice: mask[n] uint8 | sel[n] int32 | offsets[n + 1] int32 | bytes[byte_cap], every member padded
// to 16 bytes.  Byte offsets inside the slice:
COVT_SELECT_HD inline int64_t select_mask_off(int64_t) { return 0; }
COVT_SELECT_HD inline int64_t select_sel_off(int64_t n_features) { return select_align16(n_features); }
COVT_SELECT_HD inline int64_t select_offsets_off(int64_t n_features) {
    return select_sel_off(n_features) + select_align16(4 * n_features);
}
COVT_SELECT_HD inline int64_t select_bytes_off(int64_t n_features) {
    return select_offsets_off(n_features) + select_align16(4 * (n_features + 1));
}
COVT_SELECT_HD inline int64_t select_slice_bytes(int64_t n_features, int64_t byte_cap) {
    return select_bytes_off(n_features) + byte_cap;
}

// The select record of one geometry column whose slice starts at `off` (16-byte aligned); returns the offset
// after it.  byte_cap is the column's WKB capacity (wkb_column_layout); a column that gets COVT_WKB_TOO_LARGE
// there gets COVT_SELECT_TOO_LARGE here, no rows and no bytes (a one-entry offsets member, as its WKB column).
COVT_SELECT_HD inline int64_t select_column_layout(int32_t n_features, int32_t part_cap, int32_t ring_cap,
                                                   int32_t coord_cap, uint32_t geom_flags, int64_t off,
                                                   covt_select_desc& s) {
    covt_wkb_desc w;
    (void)wkb_column_layout(n_features, part_cap, ring_cap, coord_cap, geom_flags, 0, w);
    s.off = off;
    s.byte_cap = w.byte_cap;
    s.n_features = w.n_features;
    s.flags = (w.flags & COVT_WKB_TOO_LARGE) ? COVT_SELECT_TOO_LARGE : 0;
    return select_align16(off + select_slice_bytes(s.n_features, s.byte_cap));
}

// The select product of a plan (covt_products.h).
struct SelectProduct {
    using Info = covt_select_info;
    using Desc = covt_select_desc;
    using Res = covt_select_result;
    static constexpr uint32_t kTooLarge = COVT_SELECT_TOO_LARGE;
    static constexpr bool kReadsSimplified = true;
    COVT_SELECT_HD static int64_t layout(const covt_geom_info& g, int64_t off, Desc& d) {
        return select_column_layout(g.n_features, g.part_cap, g.ring_cap, g.coord_cap, (uint32_t)g.flags, off, d);
    }
    COVT_SELECT_HD static void fill(Info& r, const Desc& d) {
        r.off = d.off;
        r.byte_cap = d.byte_cap;
    }
};

// the predicate a call accepts: its size, known flags only, no NaN in the window or the minima
COVT_SELECT_HD inline bool select_pred_valid(const covt_select_pred* p) {
    if (!p || p->size != (uint32_t)sizeof(covt_select_pred)) return false;
    if (p->flags & ~(uint32_t)(COVT_SELECT_WINDOW | COVT_SELECT_MIN_SIZE | COVT_SELECT_KEEP_EMPTY)) return false;
    for (int k = 0; k < 4; ++k)
        if (p->window[k] != p->window[k]) return false;
    return p->min_area == p->min_area && p->min_length == p->min_length;
}

// mask[f] of the definition: plain IEEE comparisons (a NaN xmin: the feature has no coordinate)
COVT_SELECT_HD inline uint8_t select_keep(const covt_select_pred& p, double xmin, double ymin, double xmax, double ymax,
                                          double area, double length) {
    if (xmin != xmin) return (p.flags & COVT_SELECT_KEEP_EMPTY) ? 1 : 0;
    // (the first two terms: an inverted window selects nothing, a box that spans both its ends included)
    const bool w = !(p.flags & COVT_SELECT_WINDOW) ||
                   (p.window[0] <= p.window[2] && p.window[1] <= p.window[3] && xmin <= p.window[2] &&
                    xmax >= p.window[0] && ymin <= p.window[3] && ymax >= p.window[1]);
    const bool s = !(p.flags & COVT_SELECT_MIN_SIZE) || area >= p.min_area || length >= p.min_length ||
                   (area == 0.0 && length == 0.0);
    return (w && s) ? 1 : 0;
}

#endif

// covt_mvt_plan.h -- the MVT output layout of a plan and the option rules (include/covt.h "Geometry as MVT"),
// shared by the host plan (covt_host.cpp), the device plan (covt_plan_device.hip) and the kernels
// (covt_mvt.hip): plain arithmetic, no HIP calls, so a host-only program can include it.
#ifndef COVT_MVT_PLAN_H
#define COVT_MVT_PLAN_H

#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_MVT_HD __host__ __device__
#else
#define COVT_MVT_HD
#endif

COVT_MVT_HD inline int64_t mvt_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// coordinates per chunk of the count and write passes: the scratch holds one byte total per chunk
#define COVT_MVT_CHUNK 1024
// bytes of a ring's record in the scratch: k | cursor predecessor | flags | a point feature's coordinate count
#define COVT_MVT_RING_REC 16

// bytes a column's values can take at most: a coordinate two 5-byte varints, a ring MoveTo 1 + LineTo 5 +
// ClosePath 1, a point feature's MoveTo 5
COVT_MVT_HD inline int64_t mvt_capacity(int64_t n_features, int64_t ring_cap, int64_t coord_cap) {
    return 10 * coord_cap + 7 * ring_cap + 5 * n_features;
}
COVT_MVT_HD inline int64_t mvt_chunks(int64_t coord_cap) { return (coord_cap + COVT_MVT_CHUNK - 1) / COVT_MVT_CHUNK; }

// A column's slice: type[n] uint8 | offsets[n + 1] int32 | bytes[byte_cap] | scratch: ring_rec[ring_cap] 16 bytes
// | ring_base[ring_cap] uint32 (the byte offset of a non-empty ring's first item) | chunk_k[chunks(coord_cap) + 1]
// uint32 (a chunk's byte total, then its first byte offset); every member padded to 16 bytes.  Byte offsets inside
// the slice:
COVT_MVT_HD inline int64_t mvt_type_off(int64_t) { return 0; }
COVT_MVT_HD inline int64_t mvt_offsets_off(int64_t n) { return mvt_align16(n); }
COVT_MVT_HD inline int64_t mvt_bytes_off(int64_t n) { return mvt_offsets_off(n) + mvt_align16(4 * (n + 1)); }
COVT_MVT_HD inline int64_t mvt_ring_rec_off(int64_t n, int64_t byte_cap) { return mvt_bytes_off(n) + mvt_align16(byte_cap); }
COVT_MVT_HD inline int64_t mvt_ring_base_off(int64_t n, int64_t byte_cap, int64_t ring_cap) {
    return mvt_ring_rec_off(n, byte_cap) + mvt_align16(COVT_MVT_RING_REC * ring_cap);
}
COVT_MVT_HD inline int64_t mvt_chunk_k_off(int64_t n, int64_t byte_cap, int64_t ring_cap) {
    return mvt_ring_base_off(n, byte_cap, ring_cap) + mvt_align16(4 * ring_cap);
}
COVT_MVT_HD inline int64_t mvt_slice_bytes(int64_t n, int64_t byte_cap, int64_t ring_cap, int64_t coord_cap) {
    return mvt_chunk_k_off(n, byte_cap, ring_cap) + mvt_align16(4 * (mvt_chunks(coord_cap) + 1));
}

// The MVT record of one geometry column whose slice starts at `off` (16-byte aligned); returns the offset after
// it.  A column assembly refuses (COVT_GEOM_TOO_LARGE) or whose capacity passes INT32_MAX (the offsets are int32)
// gets COVT_MVT_TOO_LARGE, no rows and no capacity.
COVT_MVT_HD inline int64_t mvt_column_layout(int32_t n_features, int32_t ring_cap, int32_t coord_cap, uint32_t geom_flags,
                                             int64_t off, covt_mvt_desc& m) {
    const int64_t cap = mvt_capacity(n_features, ring_cap, coord_cap);
    const bool fits = !(geom_flags & COVT_GEOM_TOO_LARGE) && n_features >= 0 && ring_cap >= 0 && coord_cap >= 0 &&
                      cap <= INT32_MAX;
    m.off = off;
    m.byte_cap = fits ? cap : 0;
    m.n_features = fits ? n_features : 0;
    m.flags = fits ? 0 : COVT_MVT_TOO_LARGE;
    m.ring_cap = fits ? ring_cap : 0;
    m.coord_cap = fits ? coord_cap : 0;
    return mvt_align16(off + mvt_slice_bytes(m.n_features, m.byte_cap, m.ring_cap, m.coord_cap));
}

// The MVT product of a plan (covt_products.h).
struct MvtProduct {
    using Info = covt_mvt_info;
    using Desc = covt_mvt_desc;
    using Res = covt_mvt_result;
    static constexpr uint32_t kTooLarge = COVT_MVT_TOO_LARGE;
    static constexpr bool kReadsSimplified = true;
    COVT_MVT_HD static int64_t layout(const covt_geom_info& g, int64_t off, Desc& d) {
        return mvt_column_layout(g.n_features, g.ring_cap, g.coord_cap, (uint32_t)g.flags, off, d);
    }
    COVT_MVT_HD static void fill(Info& r, const Desc& d) {
        r.off = d.off;
        r.byte_cap = d.byte_cap;
        r.ring_cap = d.ring_cap;
        r.coord_cap = d.coord_cap;
    }
};

// the options a call accepts
COVT_MVT_HD inline bool mvt_options_valid(const covt_mvt_options* o) {
    return o && o->size == (uint32_t)sizeof(covt_mvt_options) && !(o->flags & ~(uint32_t)COVT_MVT_ORIENT) && o->shift >= 0 &&
           o->shift <= COVT_MVT_MAX_SHIFT;
}

// a uint32 as a LEB128 varint: its length in bytes
COVT_MVT_HD inline int32_t mvt_varint_len(uint32_t v) {
    return v < 0x80u ? 1 : v < 0x4000u ? 2 : v < 0x200000u ? 3 : v < 0x10000000u ? 4 : 5;
}
// zz(d) of the definition
COVT_MVT_HD inline uint32_t mvt_zigzag(uint32_t d) { return (d << 1) ^ (uint32_t)((int32_t)d >> 31); }

#endif

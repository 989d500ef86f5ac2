// covt_wkb.hip -- gfx950 WKB serialization of assembled geometry columns (include/covt.h "Geometry as
// WKB"): GeoArrow-style nested offsets + int32 coordinates -> one little-endian ISO WKB value per feature.
//
// Two kernels per launch, no scratch, no look-back (so a captured graph replays as it is):
//
//   1. size scan: a feature's byte count is a closed form of its type and six offset gathers
//      (geo[f], geo[f + 1], part[..], ring[..]); the exclusive scan over the column's features is
//      wkb_offsets, the total the column's byte count.  One wave per column in a large batch, a workgroup
//      of kWkbCoopWaves waves per column in a small one (Coop / StepScan of covt_coop.h, the assembly's
//      scans; sums saturate and the total is checked against the slice capacity).
//   2. write: with wkb_offsets known every output byte has a closed-form address, so the column's
//      coordinates, rings, parts and features are four flat item ranges cut into chunks of kWkbChunk
//      items; every wave of the column's gridDim.y workgroups (sized from the batch: many for a small
//      batch's long columns, one for a large batch) takes a run of consecutive chunks.  An item's owners
//      (a coordinate's ring, part and feature) are the last segment starting at or before it in
//      ring_offsets / part_offsets / geometry_offsets: the wave finds its first item's owners with a
//      64-ary search over the column, then stages, per chunk and level, the offsets that follow the
//      previous chunk's last owner in LDS and searches there (WkbLevel).  Chunks carry nothing but those
//      three segment indices, and waves nothing between each other.
//
// Destinations are byte-aligned only (headers are 5, 9 and 4 bytes), so the 16-byte coordinate stores
// and the 4-byte counts go through vector types of alignment 1: gfx950 runs with unaligned access
// mode on, and the compiler keeps them as single global_store_dwordx4 / _dword instructions (DESIGN.md
// section 8e has the ISA check and why the LDS-staged alternative was not built).
//
// The projected pass (include/covt.h "Georeferenced geometry") is the same launch instantiated on the
// transform: a coordinate is converted at one place (wkb_write_coords), and there the column's map is applied
// to the two doubles; byte counts and addresses do not change.  GEO 0 is the plain pass and compiles to what
// it was; GEO 1 carries no latitude code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "covt.h"
#include "covt_coop.h"
#include "covt_geo_plan.h"
#include "covt_segscan.h"
#include "covt_wave.h"
#include "covt_wkb_plan.h"

namespace covt {

constexpr int kWkbCoopWaves = 16;          // size scan, small batches: waves per column
constexpr int kWkbCoopMaxColumns = 4096;   // batches of at most this many columns are "small"
constexpr int kWkbIpl = 4;                 // items per thread and step
constexpr int kWkbWriteWaves = 4;          // write: waves per workgroup
constexpr int kWkbChunk = 64 * kWkbIpl;    // write: items per wave chunk (lane-major, kWkbIpl per lane)
constexpr int kWkbWin = 384;               // write: offsets of a level staged in LDS per chunk (a multiple of 64)

// G parts, R rings, C coordinates of feature f (assembled offsets; types <= 5 checked by the assembly)
__device__ __forceinline__ uint32_t wkb_feature_size(uint32_t t, const int32_t* geo, const int32_t* part,
                                                     const int32_t* ring, int32_t f) {
    if (t == 0u) return 21u;
    const int32_t g0 = ((const g_i32*)geo)[f], g1 = ((const g_i32*)geo)[f + 1];
    const uint32_t G = (uint32_t)(g1 - g0);
    if (t == 3u) return 9u + 21u * G;
    const int32_t r0 = ((const g_i32*)part)[g0], r1 = ((const g_i32*)part)[g1];
    const int32_t c0 = ((const g_i32*)ring)[r0], c1 = ((const g_i32*)ring)[r1];
    const uint32_t R = (uint32_t)(r1 - r0), C = (uint32_t)(c1 - c0);
    // (G, R, C <= 2^25 capacities: no term reaches 2^30)
    return 9u + 16u * C + ((t == 2u || t == 5u) ? 4u * R : 0u) + (t >= 4u ? 9u * G : 0u);
}

struct WkbCol {
    const uint8_t* types;
    const int32_t *geo, *part, *ring;
    const uint64_t* xy;
    int32_t* woff;
    uint8_t* bytes;
    int32_t n;
};
__device__ __forceinline__ WkbCol wkb_col(const uint8_t* dec, const covt_geom_desc& gd, const uint8_t* asmb,
                                          const covt_wkb_desc& wd, uint8_t* wkb) {
    WkbCol c;
    c.types = dec + gd.in_off[0];
    c.geo = (const int32_t*)(asmb + gd.out_off[0]);
    c.part = (const int32_t*)(asmb + gd.out_off[1]);
    c.ring = (const int32_t*)(asmb + gd.out_off[2]);
    c.xy = (const uint64_t*)(asmb + gd.out_off[3]);
    c.woff = (int32_t*)(wkb + wd.offsets_off);
    c.bytes = wkb + wd.bytes_off;
    c.n = wd.n_features;
    return c;
}

// the column's status before any work: the assembly's, then the layout's (the byte capacity an int32 offset)
__device__ __forceinline__ int32_t wkb_precheck(const covt_geom_desc& gd, const covt_geom_result& gr,
                                                const covt_wkb_desc& wd) {
    return geom_product_precheck(gd, gr, (wd.flags & COVT_WKB_TOO_LARGE) != 0,
                                 wd.byte_cap >= 0 && wd.byte_cap <= INT32_MAX, wd.n_features);
}

// ---- 1. size scan ------------------------------------------------------------------------------------
template <int NW, int IPL>
__device__ void wkb_scan_column(const uint8_t* __restrict__ dec, const covt_geom_desc& gd,
                                const uint8_t* __restrict__ asmb, const covt_geom_result& gr, const covt_wkb_desc& wd,
                                uint8_t* __restrict__ wkb, covt_wkb_result& res, AsmSmemT<NW, IPL>& sm,
                                int32_t geo_status = COVT_OK) {
    const int l = Coop<NW, IPL>::tid();
    res.reserved = 0;
    res.n_bytes = 0;
    res.status = wkb_precheck(gd, gr, wd);
    if (res.status == COVT_OK) res.status = geo_status;  // (a projected launch: the column's transform kind)
    if (res.status != COVT_OK) return;
    const WkbCol c = wkb_col(dec, gd, asmb, wd, wkb);
    StepScan<NW, IPL> scan{sm};
    const uint32_t B = scan.run(
        c.n, [&](int32_t f) { return wkb_feature_size((uint32_t)((const g_u8*)c.types)[f], c.geo, c.part, c.ring, f); },
        [&](int32_t f, uint32_t before) { c.woff[f] = (int32_t)before; });  // (saturated only in a column that fails below)
    if ((int64_t)B > wd.byte_cap) {
        res.status = COVT_ERR_COUNT_MISMATCH;
        return;
    }
    if (l == 0) c.woff[c.n] = (int32_t)B;
    res.n_bytes = (int64_t)B;
}

// the status of column c's transform in a projected launch (GEO; xf, kinds: its table and promise)
template <bool GEO>
__device__ __forceinline__ int32_t wkb_geo_status(const covt_geo_xform* __restrict__ xf, uint32_t kinds, int64_t c) {
    if constexpr (GEO) return geo_kind_status(xf[c].kind, kinds);
    return COVT_OK;
}

// one wave per column
template <bool GEO>
__global__ __launch_bounds__(64 * kWkbWriteWaves) void wkb_scan_kernel(
    const uint8_t* __restrict__ dec, const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb,
    const covt_geom_result* __restrict__ gres, const covt_wkb_desc* __restrict__ wdescs, int64_t n_cols,
    uint8_t* __restrict__ wkb, covt_wkb_result* __restrict__ wres, const covt_geo_xform* __restrict__ xf,
    uint32_t kinds) {
    __shared__ AsmSmemT<1, kWkbIpl> smem[kWkbWriteWaves];
    const int w = threadIdx.x >> 6;
    const int64_t c = uni64((int64_t)blockIdx.x * kWkbWriteWaves + w);
    if (c >= n_cols) return;
    const covt_geom_desc gd = gdescs[c];
    const covt_geom_result gr = gres[c];
    const covt_wkb_desc wd = wdescs[c];
    covt_wkb_result r;
    wkb_scan_column<1, kWkbIpl>(dec, gd, asmb, gr, wd, wkb, r, smem[w], wkb_geo_status<GEO>(xf, kinds, c));
    if (lane_id() == 0) wres[c] = r;
}

// a workgroup per column (small batches: a long column's scan in steps of 4096 features)
template <bool GEO>
__global__ __launch_bounds__(64 * kWkbCoopWaves) void wkb_scan_coop_kernel(
    const uint8_t* __restrict__ dec, const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb,
    const covt_geom_result* __restrict__ gres, const covt_wkb_desc* __restrict__ wdescs, int64_t n_cols,
    uint8_t* __restrict__ wkb, covt_wkb_result* __restrict__ wres, const covt_geo_xform* __restrict__ xf,
    uint32_t kinds) {
    __shared__ AsmSmemT<kWkbCoopWaves, kWkbIpl> smem;
    const int64_t c = blockIdx.x;
    if (c >= n_cols) return;
    const covt_geom_desc gd = gdescs[c];
    const covt_geom_result gr = gres[c];
    const covt_wkb_desc wd = wdescs[c];
    covt_wkb_result r;
    wkb_scan_column<kWkbCoopWaves, kWkbIpl>(dec, gd, asmb, gr, wd, wkb, r, smem, wkb_geo_status<GEO>(xf, kinds, c));
    if (threadIdx.x == 0) wres[c] = r;
}

// ---- 2. write ----------------------------------------------------------------------------------------
// One level of ownership: items (coordinates / rings / parts) over the segments of O (ring_offsets /
// part_offsets / geometry_offsets; n_seg + 1 entries).  A wave walks consecutive chunks of items, so the
// segments of a chunk start where the previous chunk's ended: the kWkbWin entries from there are staged in
// LDS with one load per lane and row, and the chunk's bracket and every item's owner are searched in LDS.
// A chunk whose segments pass the window (a run of more than ~128 empty segments) searches global memory.
struct WkbLevel {
    const int32_t* O;
    int32_t* lds;
    int32_t n_seg;
    int32_t ws;      // first staged segment: the previous chunk's last owner (uniform)
    int32_t lo, hi;  // owners of the chunk's first and last item (uniform)
    bool staged;     // lo .. hi + 1 lie inside the window

    // the last segment s in [a, b] with O[s] <= x (O nondecreasing, O[a] <= x): the wave probes 64 evenly
    // spaced entries per step (a, b, x uniform)
    __device__ __forceinline__ int32_t wave_owner(int32_t a, int32_t b, int32_t x) const {
        while (b > a) {
            const int32_t step = (b - a + 63) >> 6;
            const int32_t probe = min(a + (lane_id() + 1) * step, b);
            const int cnt = __popcll(__ballot(((const g_i32*)O)[probe] <= x));  // (a prefix of the lanes)
            if (cnt == 64) {
                a = b;
            } else {
                b = min(a + (cnt + 1) * step, b) - 1;
                a += cnt * step;
            }
        }
        return a;
    }
    __device__ __forceinline__ int32_t lane_owner_global(int32_t a, int32_t b, int32_t x) const {
        while (a < b) {
            const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b + 1u) >> 1);
            if (((const g_i32*)O)[mid] <= x) a = mid;
            else b = mid - 1;
        }
        return a;
    }
    __device__ __forceinline__ int32_t lane_owner_lds(int32_t a, int32_t b, int32_t x) const {
        while (a < b) {
            const int32_t mid = (a + b + 1) >> 1;
            if (lds[mid - ws] <= x) a = mid;
            else b = mid - 1;
        }
        return a;
    }
    // the wave's first chunk: the owner of its first item, over the whole column
    __device__ __forceinline__ void seek(int32_t first) { ws = uni(wave_owner(0, n_seg - 1, first)); }
    // stage O[ws .. ws + kWkbWin) (entries past the terminal one read as INT32_MAX); sync before use
    __device__ __forceinline__ void load() const {
#pragma unroll
        for (int k = 0; k < kWkbWin / 64; ++k) {
            const int32_t i = ws + 64 * k + lane_id();
            lds[64 * k + lane_id()] = i <= n_seg ? ((const g_i32*)O)[i] : 0x7fffffff;
        }
    }
    // owners of the chunk's first and last item (first <= last, both owned at or after ws)
    __device__ __forceinline__ void bracket(int32_t first, int32_t last) {
        staged = lds[kWkbWin - 1] > last;  // the window holds the end of last's segment
        if (staged) {
            const int32_t top = min(ws + kWkbWin - 2, n_seg - 1);
            lo = uni(lane_owner_lds(ws, top, first));
            hi = uni(lane_owner_lds(lo, top, last));
        } else {
            lo = uni(wave_owner(ws, n_seg - 1, first));
            hi = uni(wave_owner(lo, n_seg - 1, last));
        }
    }
    __device__ __forceinline__ int32_t owner(int32_t x) const {
        return staged ? lane_owner_lds(lo, hi, x) : lane_owner_global(lo, hi, x);
    }
    // O[i] (any entry: the window's copy when it has one)
    __device__ __forceinline__ int32_t at(int32_t i) const {
        return (uint32_t)(i - ws) < (uint32_t)kWkbWin ? lds[i - ws] : ((const g_i32*)O)[i];
    }
    __device__ __forceinline__ void next() { ws = hi; }  // the next chunk starts in this chunk's last segment
};

struct __attribute__((aligned(16))) WkbSmem {
    int32_t win[3][kWkbWin];  // ring, part, feature windows of one wave
};

__device__ __forceinline__ void wkb_put_u32(uint8_t* p, uint32_t v) { *(gw_u32u*)p = v; }
// byte order + geometry code + a count: the 9-byte header of a feature or part
__device__ __forceinline__ void wkb_put_header(uint8_t* p, uint32_t code, uint32_t count) {
    *(gw_u8*)p = 1;
    wkb_put_u32(p + 1, code);
    wkb_put_u32(p + 5, count);
}

// The latitude as a call, not inlined: inlined into the unrolled item loop the four items' sinh / atan
// temporaries are live at once (140 VGPRs, 3 waves a SIMD against the plain pass's 68 and 7).
__device__ __attribute__((noinline)) double wkb_lat(double t) { return geo_lat(t); }

// one wave, one chunk of coordinates [v0, v0 + L), 1 <= L <= kWkbChunk; the levels' windows start at or
// before the chunk's first owners
template <int GEO>
__device__ __forceinline__ void wkb_write_coords(const WkbCol& c, WkbLevel& lr, WkbLevel& lp, WkbLevel& lf,
                                                 int32_t v0, int32_t L, int64_t nb, const GeoHold<GEO>& geo) {
    const int l = lane_id();
    uint64_t xy[kWkbIpl];
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k)
        xy[k] = 64 * k + l < L ? __builtin_nontemporal_load(c.xy + v0 + 64 * k + l) : 0ull;  // (read once)
    lr.load();
    lp.load();
    lf.load();
    wave_sync();
    lr.bracket(v0, v0 + L - 1);
    lp.bracket(lr.lo, lr.hi);
    lf.bracket(lp.lo, lp.hi);
    int32_t r[kWkbIpl], p[kWkbIpl], f[kWkbIpl];
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) r[k] = 64 * k + l < L ? lr.owner(v0 + 64 * k + l) : lr.lo;
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) p[k] = lp.owner(r[k]);
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) f[k] = lf.owner(p[k]);
    uint32_t t[kWkbIpl];
    int32_t g0[kWkbIpl], r0[kWkbIpl], c0[kWkbIpl], wo[kWkbIpl];
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) {
        t[k] = (uint32_t)((const g_u8*)c.types)[f[k]];
        wo[k] = ((const g_i32*)c.woff)[f[k]];
        g0[k] = lf.at(f[k]);
    }
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) r0[k] = lp.at(g0[k]);
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) c0[k] = lr.at(r0[k]);
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) {
        const uint32_t dp = (uint32_t)(p[k] - g0[k]), dr = (uint32_t)(r[k] - r0[k]);
        const uint32_t dc = (uint32_t)(v0 + 64 * k + l - c0[k]);
        uint32_t o;
        switch (t[k]) {
            case 0u: o = 5u; break;
            case 1u: o = 9u + 16u * dc; break;
            case 2u: o = 9u + 4u * (dr + 1u) + 16u * dc; break;
            case 3u: o = 9u + 21u * dp + 5u; break;
            case 4u: o = 9u + 9u * (dp + 1u) + 16u * dc; break;
            default: o = 9u + 9u * (dp + 1u) + 4u * (dr + 1u) + 16u * dc; break;
        }
        const int64_t pos = (int64_t)wo[k] + o;
        if (64 * k + l < L && pos + 16 <= nb) {  // (inside the counted bytes: never past the slice)
            f64x2u d;
            d.x = (double)(int32_t)(uint32_t)xy[k];
            d.y = (double)(int32_t)(uint32_t)(xy[k] >> 32);
            if constexpr (GEO != 0) {
                d.x = geo_x(geo.t, d.x);
                d.y = geo_y<false>(geo.t, d.y);
                if constexpr (GEO == 2)
                    if (geo.lat) d.y = wkb_lat(d.y);  // (uniform over the column)
            }
            __builtin_nontemporal_store(d, (gw_f64x2u*)(c.bytes + pos));
        }
    }
    wave_sync();  // (the windows are rewritten by the next chunk)
    lr.next();
    lp.next();
    lf.next();
}

// polygon rings [q0, q0 + L): the ring's coordinate count, 4 bytes before its first coordinate
__device__ __forceinline__ void wkb_write_rings(const WkbCol& c, WkbLevel& lp, WkbLevel& lf, int32_t q0, int32_t L,
                                                int64_t nb) {
    const int l = lane_id();
    lp.load();
    lf.load();
    wave_sync();
    lp.bracket(q0, q0 + L - 1);
    lf.bracket(lp.lo, lp.hi);
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) {
        if (64 * k + l >= L) continue;
        const int32_t r = q0 + 64 * k + l;
        const int32_t p = lp.owner(r);
        const int32_t f = lf.owner(p);
        const uint32_t t = (uint32_t)((const g_u8*)c.types)[f];
        if (t != 2u && t != 5u) continue;
        const int32_t g0 = lf.at(f), r0 = lp.at(g0), c0 = ((const g_i32*)c.ring)[r0];
        const int32_t cs = ((const g_i32*)c.ring)[r], ce = ((const g_i32*)c.ring)[r + 1];
        const uint32_t dp = (uint32_t)(p - g0), dr = (uint32_t)(r - r0), dc = (uint32_t)(cs - c0);
        const uint32_t o = 9u + (t == 5u ? 9u * (dp + 1u) : 0u) + 4u * dr + 16u * dc;
        const int64_t pos = (int64_t)((const g_i32*)c.woff)[f] + o;
        if (pos + 4 <= nb) wkb_put_u32(c.bytes + pos, (uint32_t)(ce - cs));
    }
    wave_sync();
    lp.next();
    lf.next();
}

// parts [q0, q0 + L) of MULTI* features: byte order, single-geometry code and (lines, polygons) the count
// that follows
__device__ __forceinline__ void wkb_write_parts(const WkbCol& c, WkbLevel& lf, int32_t q0, int32_t L, int64_t nb) {
    const int l = lane_id();
    lf.load();
    wave_sync();
    lf.bracket(q0, q0 + L - 1);
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) {
        if (64 * k + l >= L) continue;
        const int32_t p = q0 + 64 * k + l;
        const int32_t f = lf.owner(p);
        const uint32_t t = (uint32_t)((const g_u8*)c.types)[f];
        if (t < 3u) continue;
        const int32_t g0 = lf.at(f);
        const uint32_t dp = (uint32_t)(p - g0);
        const int64_t w = ((const g_i32*)c.woff)[f];
        uint8_t* base = c.bytes + w;
        if (t == 3u) {
            const uint32_t o = 9u + 21u * dp;
            if (w + o + 5 <= nb) {
                *(gw_u8*)(base + o) = 1;
                wkb_put_u32(base + o + 1, 1u);
            }
        } else {
            const int32_t r0 = ((const g_i32*)c.part)[g0], c0 = ((const g_i32*)c.ring)[r0];
            const int32_t rs = ((const g_i32*)c.part)[p], re = ((const g_i32*)c.part)[p + 1];
            const int32_t cs = ((const g_i32*)c.ring)[rs];
            const uint32_t o = 9u + 9u * dp + (t == 5u ? 4u * (uint32_t)(rs - r0) : 0u) + 16u * (uint32_t)(cs - c0);
            // a line part is one ring: its coordinate count; a polygon part: its ring count
            const uint32_t cnt = t == 4u ? (uint32_t)(((const g_i32*)c.ring)[re] - cs) : (uint32_t)(re - rs);
            if (w + o + 9 <= nb) wkb_put_header(base + o, t - 2u, cnt);
        }
    }
    wave_sync();
    lf.next();
}

// features [q0, q0 + L): byte order, geometry code, and (all but POINT) the count of what follows
__device__ __forceinline__ void wkb_write_features(const WkbCol& c, int32_t q0, int32_t L, int64_t nb) {
    const int l = lane_id();
#pragma unroll
    for (int k = 0; k < kWkbIpl; ++k) {
        if (64 * k + l >= L) continue;
        const int32_t f = q0 + 64 * k + l;
        const uint32_t t = (uint32_t)((const g_u8*)c.types)[f];
        const int64_t w = ((const g_i32*)c.woff)[f];
        uint8_t* base = c.bytes + w;
        if (t == 0u) {
            if (w + 5 <= nb) {
                *(gw_u8*)base = 1;
                wkb_put_u32(base + 1, 1u);
            }
            continue;
        }
        const int32_t g0 = ((const g_i32*)c.geo)[f], g1 = ((const g_i32*)c.geo)[f + 1];
        uint32_t cnt = (uint32_t)(g1 - g0);  // MULTI*: parts
        if (t <= 2u) {
            const int32_t r0 = ((const g_i32*)c.part)[g0], r1 = ((const g_i32*)c.part)[g1];
            cnt = t == 2u ? (uint32_t)(r1 - r0)  // POLYGON: rings; LINESTRING: coordinates
                          : (uint32_t)(((const g_i32*)c.ring)[r1] - ((const g_i32*)c.ring)[r0]);
        }
        if (w + 9 <= nb) wkb_put_header(base, t + 1u, cnt);
    }
}

// the chunks [begin, end) of `items` items this wave takes: an equal share of consecutive chunks
__device__ __forceinline__ void wkb_share(int32_t items, int32_t wave, int32_t waves, int32_t& begin, int32_t& end) {
    const int64_t chunks = ((int64_t)items + kWkbChunk - 1) / kWkbChunk;
    begin = (int32_t)(chunks * wave / waves);
    end = (int32_t)(chunks * (wave + 1) / waves);
}

// blockIdx.x: the column; each of its gridDim.y * kWkbWriteWaves waves takes a run of consecutive chunks of
// every item kind
template <int GEO>
__global__ __launch_bounds__(64 * kWkbWriteWaves) void wkb_write_kernel(
    const uint8_t* __restrict__ dec, const covt_geom_desc* __restrict__ gdescs, const uint8_t* __restrict__ asmb,
    const covt_geom_result* __restrict__ gres, const covt_wkb_desc* __restrict__ wdescs,
    uint8_t* __restrict__ wkb, const covt_wkb_result* __restrict__ wres, const covt_geo_xform* __restrict__ xf) {
    __shared__ WkbSmem smem[kWkbWriteWaves];
    const int64_t col = blockIdx.x;
    const covt_wkb_result wr = wres[col];  // (the size scan's, earlier on this stream)
    if (wr.status != COVT_OK || wr.n_bytes <= 0) return;
    const covt_geom_desc gd = gdescs[col];
    const covt_wkb_desc wd = wdescs[col];
    const covt_geom_result gr = gres[col];
    const WkbCol c = wkb_col(dec, gd, asmb, wd, wkb);
    const int32_t P = gr.num_parts, R = gr.num_rings, V = gr.num_coords;
    const int64_t nb = wr.n_bytes;
    const GeoHold<GEO> geo = geo_hold<GEO>(xf, col);
    const int w = threadIdx.x >> 6;
    const int32_t wave = uni((int32_t)(blockIdx.y * kWkbWriteWaves + w));
    const int32_t waves = (int32_t)(gridDim.y * kWkbWriteWaves);
    WkbLevel lr{c.ring, smem[w].win[0], R, 0, 0, 0, false};
    WkbLevel lp{c.part, smem[w].win[1], P, 0, 0, 0, false};
    WkbLevel lf{c.geo, smem[w].win[2], c.n, 0, 0, 0, false};
    int32_t cb, ce;
    wkb_share(V, wave, waves, cb, ce);
    if (cb < ce) {
        lr.seek(cb * kWkbChunk);
        lp.seek(lr.ws);
        lf.seek(lp.ws);
        for (int32_t j = cb; j < ce; ++j)
            wkb_write_coords<GEO>(c, lr, lp, lf, j * kWkbChunk, min(kWkbChunk, V - j * kWkbChunk), nb, geo);
    }
    wkb_share(R, wave, waves, cb, ce);
    if (cb < ce) {
        lp.seek(cb * kWkbChunk);
        lf.seek(lp.ws);
        for (int32_t j = cb; j < ce; ++j)
            wkb_write_rings(c, lp, lf, j * kWkbChunk, min(kWkbChunk, R - j * kWkbChunk), nb);
    }
    wkb_share(P, wave, waves, cb, ce);
    if (cb < ce) {
        lf.seek(cb * kWkbChunk);
        for (int32_t j = cb; j < ce; ++j)
            wkb_write_parts(c, lf, j * kWkbChunk, min(kWkbChunk, P - j * kWkbChunk), nb);
    }
    wkb_share(c.n, wave, waves, cb, ce);
    for (int32_t j = cb; j < ce; ++j)
        wkb_write_features(c, j * kWkbChunk, min(kWkbChunk, c.n - j * kWkbChunk), nb);
}

// GEO 0: the plain pass; 1: transforms without a latitude; 2: with
template <int GEO>
int wkb_launch(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
               const covt_geom_result* d_gres, const covt_wkb_desc* d_wdesc, int64_t n_columns, uint8_t* d_wkb,
               covt_wkb_result* d_wres, const covt_geo_xform* d_xf, uint32_t kinds, hipStream_t s) {
    constexpr bool G = GEO != 0;
    const bool small = n_columns <= kWkbCoopMaxColumns;
    if (small) {
        hipLaunchKernelGGL(wkb_scan_coop_kernel<G>, dim3((unsigned)n_columns), dim3(64 * kWkbCoopWaves), 0, s, d_decoded,
                           d_gdesc, d_asm, d_gres, d_wdesc, n_columns, d_wkb, d_wres, d_xf, kinds);
    } else {
        const int64_t blocks = (n_columns + kWkbWriteWaves - 1) / kWkbWriteWaves;
        hipLaunchKernelGGL(wkb_scan_kernel<G>, dim3((unsigned)blocks), dim3(64 * kWkbWriteWaves), 0, s, d_decoded,
                           d_gdesc, d_asm, d_gres, d_wdesc, n_columns, d_wkb, d_wres, d_xf, kinds);
    }
    const unsigned gy = small ? product_blocks_y(n_columns) : 1u;
    hipLaunchKernelGGL(wkb_write_kernel<GEO>, dim3((unsigned)n_columns, gy), dim3(64 * kWkbWriteWaves), 0, s,
                       d_decoded, d_gdesc, d_asm, d_gres, d_wdesc, d_wkb, d_wres, d_xf);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

}  // namespace covt

extern "C" int covt_geometry_wkb_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                        const covt_geom_result* d_gres, const covt_wkb_desc* d_wdesc, int64_t n_columns,
                                        uint8_t* d_wkb, covt_wkb_result* d_wres, void* hip_stream) {
    if (n_columns < 0 || (n_columns && (!d_decoded || !d_gdesc || !d_asm || !d_gres || !d_wdesc || !d_wkb || !d_wres)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff) return COVT_ERR_INVALID_ARG;
    return covt::wkb_launch<0>(d_decoded, d_gdesc, d_asm, d_gres, d_wdesc, n_columns, d_wkb, d_wres, nullptr, 0u,
                               (hipStream_t)hip_stream);
}

extern "C" int covt_geometry_wkb_projected_device(const uint8_t* d_decoded, const covt_geom_desc* d_gdesc,
                                                  const uint8_t* d_asm, const covt_geom_result* d_gres,
                                                  const covt_wkb_desc* d_wdesc, int64_t n_columns, uint8_t* d_wkb,
                                                  covt_wkb_result* d_wres, const covt_geo_xform* d_xf, uint32_t kinds,
                                                  void* hip_stream) {
    if (n_columns < 0 || (kinds & ~7u) ||
        (n_columns && (!d_decoded || !d_gdesc || !d_asm || !d_gres || !d_wdesc || !d_wkb || !d_wres || !d_xf)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff) return COVT_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)hip_stream;
    // the latitude code (device sinh, atan and their registers) only where the caller's table may need it
    return (kinds & (1u << COVT_GEO_AFFINE_LAT))
               ? covt::wkb_launch<2>(d_decoded, d_gdesc, d_asm, d_gres, d_wdesc, n_columns, d_wkb, d_wres, d_xf, kinds, s)
               : covt::wkb_launch<1>(d_decoded, d_gdesc, d_asm, d_gres, d_wdesc, n_columns, d_wkb, d_wres, d_xf, kinds, s);
}

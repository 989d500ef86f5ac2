// covt_bbox.hip -- gfx950 per-feature bounding boxes of assembled geometry columns (include/covt.h
// "Geometry bounding boxes"): GeoArrow-style nested offsets + int32 coordinates -> xmin | ymin | xmax | ymax
// float64 arrays per column, the column's extent and its count of empty features.
//
// Offsets are nested and absolute, so feature f's coordinates are the one range [start(f), start(f + 1)) of
// coords, start(f) = ring[part[geo[f]]]: the pass is a segmented min / max.  Three launches, no scratch, no
// float atomics, every output double written exactly once by one thread (so a captured graph replays the
// pass as it is and the result does not depend on scheduling):
//
//   1. init: the column's status (the assembly's, then the layout's), n_empty = 0 and the extent as four
//      int32 identities in the first 16 bytes of covt_bbox_result.extent.
//   2. boxes: the column's coordinates are cut into chunks of kBboxChunk; every wave of the column's
//      gridDim.y workgroups (sized from the batch as the WKB pass sizes them) takes a run of consecutive
//      chunks and owns the features that start inside its run (an empty feature: where start(f) falls;
//      those at the column's end: the last run).  Per chunk the wave loads the coordinates once (16 bytes a
//      lane), marks the chunk's feature heads in LDS from a window of kBboxWin staged start() values (three
//      dependent gathers per feature, never per coordinate), runs a segmented inclusive min / max scan over
//      the chunk (DPP, carried from chunk to chunk) into LDS, and a lane per feature that ends in the chunk
//      picks the scan value of its last coordinate up and stores its four doubles.  The one feature still
//      open at the end of the run is finished by its owner: by the wave if fewer than kBboxWide coordinates
//      remain, else by the whole workgroup through LDS once all its waves are through their runs.  Chunks
//      that hold neither a head nor a coordinate of one of the wave's features are not loaded.
//      Lanes keep the int32 min / max of the boxes they stored and their count of empty features; one
//      int32 atomic min / max / add per wave and value folds them into the result that launch 1 initialised
//      (order-independent, so still deterministic).
//   3. finish: the int32 extent -> float64, NaN where the column has no coordinate or failed.
//
// The projected pass (include/covt.h "Georeferenced geometry") is the same three launches instantiated on
// the transform: boxes stay int32 up to the stores, and each of the four store sites (a chunk's features, the
// feature the wave finishes, the one the workgroup finishes, the extent) maps the box's two ends per axis and
// takes their fmin / fmax (bb_map).  GEO 0 is the plain pass and compiles to what it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "covt.h"
#include "covt_bbox_plan.h"
#include "covt_coop.h"
#include "covt_geo_plan.h"
#include "covt_wave.h"

namespace covt {

constexpr int kBboxWaves = 4;                // waves per workgroup
constexpr int kBboxRows = 2;                 // rows of 64 lanes x 2 coordinates (one 16-byte load) per chunk
constexpr int kBboxChunk = 128 * kBboxRows;  // coordinates per wave chunk
constexpr int kBboxWin = 512;                // start() values of consecutive features staged in LDS per wave
constexpr int kBboxAhead = 320;              // window entries wanted past the first open feature at a chunk's start
constexpr int kBboxWide = 2048;              // coordinates left past a run from which the workgroup finishes a feature
constexpr int kBboxSmallBlocks = 8192;       // workgroups over all columns of a small batch (at most 64 each)
constexpr int kBboxMaxBlocksY = 64;

typedef __attribute__((address_space(1))) double gw_f64;

// a box: (xmin, ymin, xmax, ymax) in the int32 domain
__device__ __forceinline__ i32x4 bb_id() { return i32x4{INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN}; }
__device__ __forceinline__ i32x4 bb_pt(int32_t x, int32_t y) { return i32x4{x, y, x, y}; }
__device__ __forceinline__ i32x4 bb_join(i32x4 a, i32x4 b) {
    return i32x4{min(a.x, b.x), min(a.y, b.y), max(a.z, b.z), max(a.w, b.w)};
}
__device__ __forceinline__ i32x4 bb_sel(bool p, i32x4 a, i32x4 b) {
    return i32x4{p ? a.x : b.x, p ? a.y : b.y, p ? a.z : b.z, p ? a.w : b.w};
}
// the DPP-moved box of another lane; lanes without a source read `old`
template <int CTRL, int RMASK>
__device__ __forceinline__ i32x4 bb_dpp(i32x4 old, i32x4 v) {
    i32x4 r;
    r.x = __builtin_amdgcn_update_dpp(old.x, v.x, CTRL, RMASK, 0xf, false);
    r.y = __builtin_amdgcn_update_dpp(old.y, v.y, CTRL, RMASK, 0xf, false);
    r.z = __builtin_amdgcn_update_dpp(old.z, v.z, CTRL, RMASK, 0xf, false);
    r.w = __builtin_amdgcn_update_dpp(old.w, v.w, CTRL, RMASK, 0xf, false);
    return r;
}
// one step of the segmented inclusive scan: (v, f) := (pv, pf) (+) (v, f); a lane with f set starts a segment
// (selects, not branches: the DPP moves run with every lane enabled)
template <int CTRL, int RMASK>
__device__ __forceinline__ void bb_seg_step(i32x4& v, int32_t& f) {
    const i32x4 pv = bb_dpp<CTRL, RMASK>(bb_id(), v);
    const int32_t pf = __builtin_amdgcn_update_dpp(0, f, CTRL, RMASK, 0xf, false);
    v = bb_sel(f != 0, v, bb_join(pv, v));
    f |= pf;
}
template <int CTRL, int RMASK>
__device__ __forceinline__ void bb_red_step(i32x4& v) {
    v = bb_join(v, bb_dpp<CTRL, RMASK>(bb_id(), v));
}
// the join of the 64 lanes' boxes, uniform (the wave64 DPP sequence of covt_wave.h)
__device__ __forceinline__ i32x4 bb_wave_join(i32x4 v) {
    bb_red_step<0x111, 0xf>(v);  // row_shr:1
    bb_red_step<0x112, 0xf>(v);  // row_shr:2
    bb_red_step<0x114, 0xf>(v);  // row_shr:4
    bb_red_step<0x118, 0xf>(v);  // row_shr:8
    bb_red_step<0x142, 0xa>(v);  // row_bcast:15
    bb_red_step<0x143, 0xc>(v);  // row_bcast:31
    return i32x4{(int32_t)lane_bcast((uint32_t)v.x, 63), (int32_t)lane_bcast((uint32_t)v.y, 63),
                 (int32_t)lane_bcast((uint32_t)v.z, 63), (int32_t)lane_bcast((uint32_t)v.w, 63)};
}

// One row of a chunk: the lane holds two consecutive coordinates c0, c1 (identity boxes past the column's
// end) and their head flags; `carry` is the running box of the segment open before lane 0 (uniform).
// r0, r1: the inclusive segmented min / max at the two coordinates; carry: that of the row's last one.
__device__ __forceinline__ void bb_row_scan(i32x4 c0, i32x4 c1, int32_t h0, int32_t h1, i32x4& carry, i32x4& r0,
                                            i32x4& r1) {
    i32x4 v = bb_sel(h1 != 0, c1, bb_join(c0, c1));
    int32_t f = h0 | h1;
    v = bb_sel(lane_id() == 0 && f == 0, bb_join(carry, v), v);
    bb_seg_step<0x111, 0xf>(v, f);  // row_shr:1
    bb_seg_step<0x112, 0xf>(v, f);  // row_shr:2
    bb_seg_step<0x114, 0xf>(v, f);  // row_shr:4
    bb_seg_step<0x118, 0xf>(v, f);  // row_shr:8
    bb_seg_step<0x142, 0xa>(v, f);  // row_bcast:15
    bb_seg_step<0x143, 0xc>(v, f);  // row_bcast:31
    const i32x4 ex = bb_dpp<0x138, 0xf>(carry, v);  // wave_shr:1: the lane before (lane 0: the carry)
    r0 = bb_sel(h0 != 0, c0, bb_join(ex, c0));
    r1 = bb_sel(h1 != 0, c1, bb_join(r0, c1));
    carry = i32x4{(int32_t)lane_bcast((uint32_t)v.x, 63), (int32_t)lane_bcast((uint32_t)v.y, 63),
                  (int32_t)lane_bcast((uint32_t)v.z, 63), (int32_t)lane_bcast((uint32_t)v.w, 63)};
}

struct BboxCol {
    const int32_t *geo, *part, *ring, *xy;
    gw_f64* out;  // xmin | ymin | xmax | ymax, n doubles each
    int32_t n, P, R, V;
};

__device__ __forceinline__ int32_t bb_clamp(int32_t x, int32_t hi) { return min(max(x, 0), hi); }
// first coordinate of feature f in [0, n] (start(n): the column's coordinate count); indices clamped, so a
// column whose offsets are not what assembly promises is still read inside its slices
__device__ __forceinline__ int32_t bb_start(const BboxCol& c, int32_t f) {
    const int32_t g = bb_clamp(((const g_i32*)c.geo)[f], c.P);
    const int32_t r = bb_clamp(((const g_i32*)c.part)[g], c.R);
    return bb_clamp(((const g_i32*)c.ring)[r], c.V);
}
// coordinates i, i + 1 (i even: 16-byte aligned) as (x0, y0, x1, y1); those at or past `end` are not read
__device__ __forceinline__ i32x4 bb_load2(const BboxCol& c, int32_t i, int32_t end) {
    i32x4 q = i32x4{0, 0, 0, 0};
    if (i + 1 < end) {
        q = *(g_i32x4*)(c.xy + 2 * (int64_t)i);
    } else if (i < end) {
        const uint64_t v = *(g_u64*)(c.xy + 2 * (int64_t)i);
        q.x = (int32_t)(uint32_t)v;
        q.y = (int32_t)(uint32_t)(v >> 32);
    }
    return q;
}
// the join of coordinates i, i + 1 below `end` into box
__device__ __forceinline__ i32x4 bb_take2(const BboxCol& c, i32x4 box, int32_t i, int32_t end) {
    const i32x4 q = bb_load2(c, i, end);
    box = bb_sel(i < end, bb_join(box, bb_pt(q.x, q.y)), box);
    return bb_sel(i + 1 < end, bb_join(box, bb_pt(q.z, q.w)), box);
}

// the first feature f in [0, n] with start(f) >= x (start nondecreasing): the wave probes 64 evenly spaced
// features per step (x uniform)
__device__ __forceinline__ int32_t bb_first_at(const BboxCol& c, int32_t x) {
    int32_t lo = 0, hi = c.n;
    while (lo < hi) {
        const int32_t step = (hi - lo + 63) >> 6;
        const int32_t p = min(lo + lane_id() * step, hi);
        const bool below = p < hi && bb_start(c, p) < x;  // (a prefix of the lanes)
        const int cnt = __popcll(__ballot(below));
        if (cnt == 0) {
            hi = lo;
        } else {
            const int32_t nlo = min(lo + (cnt - 1) * step, hi) + 1;
            hi = cnt < 64 ? min(lo + cnt * step, hi) : hi;
            lo = nlo;
        }
    }
    return uni(lo);
}

// stage start(wbase .. wbase + kBboxWin) (features past n read as INT32_MAX), level by level so the gathers
// of a level are in flight together; sync before use
__device__ __forceinline__ void bb_stage(const BboxCol& c, int32_t* win, int32_t wbase) {
    constexpr int K = kBboxWin / 64;
    int32_t v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((const g_i32*)c.geo)[min(wbase + 64 * k + lane_id(), c.n)];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((const g_i32*)c.part)[bb_clamp(v[k], c.P)];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((const g_i32*)c.ring)[bb_clamp(v[k], c.R)];
#pragma unroll
    for (int k = 0; k < K; ++k)
        win[64 * k + lane_id()] = wbase + 64 * k + lane_id() <= c.n ? bb_clamp(v[k], c.V) : 0x7fffffff;
}

struct __attribute__((aligned(16))) BboxSmem {
    i32x4 res[kBboxWaves][kBboxChunk];     // the chunk's inclusive segmented min / max per coordinate
    int32_t win[kBboxWaves][kBboxWin];     // start() of the features from the wave's window base on
    uint8_t head[kBboxWaves][kBboxChunk];  // 1: a feature starts at this coordinate of the chunk
    i32x4 wide_box[kBboxWaves];            // a wave's feature left to the workgroup: its box so far,
    int32_t wide_f[kBboxWaves];            //   its index (-1: none),
    int32_t wide_from[kBboxWaves];         //   and the coordinates [from, to) still to take
    int32_t wide_to[kBboxWaves];
    i32x4 red[kBboxWaves];
};

// The column's transform as the kernels hold it (uniform): nothing for the plain pass (GEO 0), the affine
// coefficients for a launch without latitudes (GEO 1: a tile-local column maps by 0 + 1 * p), and with them
// whether y goes on through the Gudermannian (GEO 2).
template <int GEO>
struct BboxGeo {
    covt_geo_xform t;
    bool lat;
};
template <>
struct BboxGeo<0> {};
template <int GEO>
__device__ __forceinline__ BboxGeo<GEO> bb_geo(const covt_geo_xform* __restrict__ xf, int64_t col) {
    BboxGeo<GEO> g;
    if constexpr (GEO != 0) {
        g.t = xf[col];
        g.lat = GEO == 2 && g.t.kind == COVT_GEO_AFFINE_LAT;
        if (g.t.kind == COVT_GEO_IDENTITY) g.t = geo_identity_affine();
    }
    return g;
}
// an int32 box as its four float64 (xmin, ymin, xmax, ymax): per axis the fmin / fmax of the two transformed
// ends, so a map that flips an axis (sy < 0) needs no sign test
template <int GEO>
__device__ __forceinline__ void bb_map(const BboxGeo<GEO>& geo, i32x4 box, double (&o)[4]) {
    o[0] = (double)box.x, o[1] = (double)box.y, o[2] = (double)box.z, o[3] = (double)box.w;
    if constexpr (GEO != 0) {
        const double x0 = geo_x(geo.t, o[0]), x1 = geo_x(geo.t, o[2]);
        double y0 = geo_y<false>(geo.t, o[1]), y1 = geo_y<false>(geo.t, o[3]);
        if constexpr (GEO == 2)
            if (geo.lat) y0 = geo_lat(y0), y1 = geo_lat(y1);  // (uniform over the column)
        o[0] = fmin(x0, x1), o[1] = fmin(y0, y1), o[2] = fmax(x0, x1), o[3] = fmax(y0, y1);
    }
}

template <int GEO>
__device__ __forceinline__ void bb_put(const BboxCol& c, const BboxGeo<GEO>& geo, int32_t f, i32x4 box, bool any) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double o[4];
    bb_map<GEO>(geo, box, o);
    // (the four arrays of covt_bbox_plan.h; byte offsets are multiples of 8)
    c.out[bbox_array_off(c.n, 0) / 8 + f] = any ? o[0] : nan;
    c.out[bbox_array_off(c.n, 1) / 8 + f] = any ? o[1] : nan;
    c.out[bbox_array_off(c.n, 2) / 8 + f] = any ? o[2] : nan;
    c.out[bbox_array_off(c.n, 3) / 8 + f] = any ? o[3] : nan;
}

// the column's status before any work: the assembly's, then the layout's
__device__ __forceinline__ int32_t bbox_precheck(const covt_geom_desc& gd, const covt_geom_result& gr,
                                                 const covt_bbox_desc& bd) {
    if (gr.status != COVT_OK) return gr.status;
    if (((uint32_t)gd.flags & COVT_GEOM_TOO_LARGE) || (bd.flags & COVT_BBOX_TOO_LARGE) || bd.off < 0 || (bd.off & 15))
        return COVT_ERR_INVALID_ARG;
    const int32_t n = gd.in_off[0] >= 0 ? gd.in_len[0] : 0;  // the features the assembly walked
    return bd.n_features == n ? COVT_OK : COVT_ERR_INVALID_ARG;
}

// ---- 1. init ------------------------------------------------------------------------------------------
// (GEO: a projected launch; then the kind of the column's transform under the caller's promise `kinds`)
template <bool GEO>
__global__ __launch_bounds__(256) void bbox_init_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                        const covt_geom_result* __restrict__ gres,
                                                        const covt_bbox_desc* __restrict__ bdescs, int64_t n_cols,
                                                        covt_bbox_result* __restrict__ bres,
                                                        const covt_geo_xform* __restrict__ xf, uint32_t kinds) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    int32_t* r = (int32_t*)(bres + c);
    int32_t st = bbox_precheck(gdescs[c], gres[c], bdescs[c]);
    if constexpr (GEO)
        if (st == COVT_OK) st = geo_kind_status(xf[c].kind, kinds);
    r[0] = st;
    r[1] = 0;
    r[2] = INT32_MAX;  // the int32 extent, folded by the boxes kernel's atomics
    r[3] = INT32_MAX;
    r[4] = INT32_MIN;
    r[5] = INT32_MIN;
    r[6] = r[7] = r[8] = r[9] = 0;
}

// ---- 2. boxes -----------------------------------------------------------------------------------------
// blockIdx.x: the column; each of its gridDim.y * kBboxWaves waves takes a run of consecutive chunks
template <int GEO>
__global__ __launch_bounds__(64 * kBboxWaves) void bbox_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                               const uint8_t* __restrict__ asmb,
                                                               const covt_geom_result* __restrict__ gres,
                                                               const covt_bbox_desc* __restrict__ bdescs,
                                                               uint8_t* __restrict__ bbox,
                                                               covt_bbox_result* __restrict__ bres,
                                                               const covt_geo_xform* __restrict__ xf) {
    __shared__ BboxSmem sm;
    const int64_t col = blockIdx.x;
    int32_t* const rcol = (int32_t*)(bres + col);
    if (rcol[0] != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const covt_geom_desc gd = gdescs[col];
    const covt_bbox_desc bd = bdescs[col];
    const covt_geom_result gr = gres[col];
    const BboxGeo<GEO> geo = bb_geo<GEO>(xf, col);
    BboxCol c;
    c.geo = (const int32_t*)(asmb + gd.out_off[0]);
    c.part = (const int32_t*)(asmb + gd.out_off[1]);
    c.ring = (const int32_t*)(asmb + gd.out_off[2]);
    c.xy = (const int32_t*)(asmb + gd.out_off[3]);
    c.out = (gw_f64*)(bbox + bd.off);
    c.n = bd.n_features;
    c.P = bb_clamp(gr.num_parts, gd.part_cap);
    c.R = bb_clamp(gr.num_rings, gd.ring_cap);
    c.V = bb_clamp(gr.num_coords, gd.coord_cap);
    const int l = lane_id();
    const int w = threadIdx.x >> 6;
    const int32_t wave = uni((int32_t)(blockIdx.y * kBboxWaves + w));
    const int32_t waves = (int32_t)(gridDim.y * kBboxWaves);
    // (a column without coordinates is one chunk of none: its features are all empty)
    const int64_t chunks = std::max<int64_t>(1, ((int64_t)c.V + kBboxChunk - 1) / kBboxChunk);
    const int32_t cb = (int32_t)(chunks * wave / waves), ce = (int32_t)(chunks * (wave + 1) / waves);
    int32_t* const win = sm.win[w];
    i32x4* const res = sm.res[w];
    uint8_t* const head = sm.head[w];

    i32x4 ext = bb_id();  // per lane: the join of the boxes it stored
    int32_t n_empty = 0;  // per lane: the empty features it stored
    int32_t wide_f = -1, wide_to = 0, run_end = 0;
    i32x4 carry = bb_id();
    if (cb < ce && c.n > 0) {
        const bool last = ce == chunks;  // the column's last run: owns the empty features at its end
        const int32_t A = cb * kBboxChunk, B = last ? c.V : ce * kBboxChunk;
        run_end = B;
        int32_t fc = A == 0 ? 0 : bb_first_at(c, A);  // the first feature not yet stored
        int32_t wbase = fc;
        ((uint32_t*)head)[l] = 0;
        bb_stage(c, win, wbase);
        wave_sync();
        // the window holds start(f .. f + need - 1)
        auto ensure = [&](int32_t f, int32_t need) {
            if (f < wbase || f + need > wbase + kBboxWin) {
                wave_sync();
                wbase = f;
                bb_stage(c, win, wbase);
                wave_sync();
            }
        };
        for (int32_t j = cb; j < ce && fc < c.n; ++j) {
            const int32_t a = j * kBboxChunk, L = min(kBboxChunk, c.V - a), b = a + L;
            ensure(fc, kBboxAhead);
            const int32_t s_fc = uni(win[fc - wbase]);
            if (!last && s_fc >= B) break;  // the next feature starts in a later run
            const bool process = s_fc < b;  // a feature of this wave's has a coordinate here
            if (!process && j != chunks - 1) continue;
            if (process) {
                i32x4 q[kBboxRows];
#pragma unroll
                for (int k = 0; k < kBboxRows; ++k) q[k] = bb_load2(c, a + 128 * k + 2 * l, b);
                // heads: the features from fc on that start below b
                for (int32_t fh = fc;; fh += 64) {
                    ensure(fh, 64);
                    const int32_t f = fh + l;
                    const int32_t s = win[f - wbase];
                    const bool in = f < c.n && s < b;
                    if (in && (uint32_t)(s - a) < (uint32_t)L) head[s - a] = 1;
                    if (__ballot(in) != ~0ull) break;
                }
                wave_sync();
#pragma unroll
                for (int k = 0; k < kBboxRows; ++k) {
                    const int32_t p0 = 128 * k + 2 * l;
                    const uint32_t hh = *(const uint16_t*)(head + p0);
                    const i32x4 c0 = p0 < L ? bb_pt(q[k].x, q[k].y) : bb_id();
                    const i32x4 c1 = p0 + 1 < L ? bb_pt(q[k].z, q[k].w) : bb_id();
                    i32x4 r0, r1;
                    bb_row_scan(c0, c1, (int32_t)(hh & 0xffu), (int32_t)(hh >> 8), carry, r0, r1);
                    res[p0] = r0;
                    res[p0 + 1] = r1;
                }
                wave_sync();
                ((uint32_t*)head)[l] = 0;  // (read above; written again after the next chunk's syncs)
            }
            // the features that end in this chunk: a lane each, in steps of 64
            for (;;) {
                ensure(fc, 65);
                const int32_t f = fc + l;
                const int32_t s = win[f - wbase], e = win[f + 1 - wbase];
                const bool done = f < c.n && (last || s < B) && e <= b;  // (a prefix of the lanes)
                if (done) {
                    const uint32_t at = (uint32_t)(e - 1 - a);
                    const bool any = e > s && process && at < (uint32_t)kBboxChunk;
                    const i32x4 box = any ? res[at] : bb_id();
                    bb_put<GEO>(c, geo, f, box, any);
                    ext = bb_join(ext, box);
                    n_empty += any ? 0 : 1;
                }
                const int cnt = __popcll(__ballot(done));
                fc += cnt;
                if (cnt < 64) break;
            }
            wave_sync();  // (res is rewritten by the next chunk)
        }
        // the feature still open at the end of the run: the coordinates [B, e) are left
        if (!last && fc < c.n) {
            ensure(fc, 2);
            const int32_t s = uni(win[fc - wbase]), e = uni(win[fc + 1 - wbase]);
            if (s < B && e > B) {
                if (e - B >= kBboxWide) {
                    wide_f = fc;
                    wide_to = e;
                } else {
                    i32x4 box = bb_id();
                    for (int32_t i = B + 2 * l; i < e; i += 128) box = bb_take2(c, box, i, e);
                    box = bb_join(carry, bb_wave_join(box));
                    if (l == 0) {
                        bb_put<GEO>(c, geo, fc, box, true);
                        ext = bb_join(ext, box);
                    }
                }
            }
        }
    }
    if (l == 0) {
        sm.wide_f[w] = wide_f;
        sm.wide_from[w] = run_end;
        sm.wide_to[w] = wide_to;
        sm.wide_box[w] = carry;
    }
    __syncthreads();
    // features left to the workgroup: all its threads take the remaining coordinates, 16 bytes each a step
    for (int k = 0; k < kBboxWaves; ++k) {
        const int32_t f = sm.wide_f[k];
        if (f < 0) continue;  // (uniform)
        const int32_t from = sm.wide_from[k], to = sm.wide_to[k];
        i32x4 box = bb_id();
        for (int32_t i = from + 2 * (int32_t)threadIdx.x; i < to; i += 2 * 64 * kBboxWaves) box = bb_take2(c, box, i, to);
        box = bb_wave_join(box);
        if (l == 0) sm.red[w] = box;
        __syncthreads();
        if (threadIdx.x == 0) {
            box = sm.wide_box[k];
#pragma unroll
            for (int i = 0; i < kBboxWaves; ++i) box = bb_join(box, sm.red[i]);
            bb_put<GEO>(c, geo, f, box, true);
            ext = bb_join(ext, box);
        }
        __syncthreads();
    }
    // the column's extent and empty count: one atomic per wave and value, on launch 1's identities
    ext = bb_wave_join(ext);
    const int32_t ne = (int32_t)lane_bcast(incl_scan((uint32_t)n_empty), 63);
    if (l == 0) {
        if (ext.x <= ext.z) {
            atomicMin(rcol + 2, ext.x);
            atomicMin(rcol + 3, ext.y);
            atomicMax(rcol + 4, ext.z);
            atomicMax(rcol + 5, ext.w);
        }
        if (ne) atomicAdd(rcol + 1, ne);
    }
}

// ---- 3. finish ----------------------------------------------------------------------------------------
template <int GEO>
__global__ __launch_bounds__(256) void bbox_finish_kernel(int64_t n_cols, covt_bbox_result* __restrict__ bres,
                                                          const covt_geo_xform* __restrict__ xf) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    const int32_t* r = (const int32_t*)(bres + c);
    const int32_t x0 = r[2], y0 = r[3], x1 = r[4], y1 = r[5];
    const bool any = r[0] == COVT_OK && x0 <= x1;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double o[4];
    bb_map<GEO>(bb_geo<GEO>(xf, c), i32x4{x0, y0, x1, y1}, o);  // (a column that failed: not stored)
    double* e = bres[c].extent;
    e[0] = any ? o[0] : nan;
    e[1] = any ? o[1] : nan;
    e[2] = any ? o[2] : nan;
    e[3] = any ? o[3] : nan;
}

// GEO 0: the plain pass; 1: transforms without a latitude; 2: with
template <int GEO>
int bbox_launch(const covt_geom_desc* d_gdesc, const uint8_t* d_asm, const covt_geom_result* d_gres,
                const covt_bbox_desc* d_bdesc, int64_t n_columns, uint8_t* d_bbox, covt_bbox_result* d_bres,
                const covt_geo_xform* d_xf, uint32_t kinds, hipStream_t s) {
    const unsigned cols256 = (unsigned)((n_columns + 255) / 256);
    hipLaunchKernelGGL(bbox_init_kernel<GEO != 0>, dim3(cols256), dim3(256), 0, s, d_gdesc, d_gres, d_bdesc, n_columns,
                       d_bres, d_xf, kinds);
    // small batches: up to 64 workgroups per column (a 72k-coordinate column: a chunk or two per wave)
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(kBboxMaxBlocksY, kBboxSmallBlocks / n_columns));
    hipLaunchKernelGGL(bbox_kernel<GEO>, dim3((unsigned)n_columns, (unsigned)gy), dim3(64 * kBboxWaves), 0, s, d_gdesc,
                       d_asm, d_gres, d_bdesc, d_bbox, d_bres, d_xf);
    hipLaunchKernelGGL(bbox_finish_kernel<GEO>, dim3(cols256), dim3(256), 0, s, n_columns, d_bres, d_xf);
    return hipGetLastError() == hipSuccess ? COVT_OK : COVT_ERR_DEVICE;
}

}  // namespace covt

extern "C" int covt_geometry_bbox_device(const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                         const covt_geom_result* d_gres, const covt_bbox_desc* d_bdesc,
                                         int64_t n_columns, uint8_t* d_bbox, covt_bbox_result* d_bres, void* hip_stream) {
    if (n_columns < 0 || (n_columns && (!d_gdesc || !d_asm || !d_gres || !d_bdesc || !d_bbox || !d_bres)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff) return COVT_ERR_INVALID_ARG;
    return covt::bbox_launch<0>(d_gdesc, d_asm, d_gres, d_bdesc, n_columns, d_bbox, d_bres, nullptr, 0u,
                                (hipStream_t)hip_stream);
}

extern "C" int covt_geometry_bbox_projected_device(const covt_geom_desc* d_gdesc, const uint8_t* d_asm,
                                                   const covt_geom_result* d_gres, const covt_bbox_desc* d_bdesc,
                                                   int64_t n_columns, uint8_t* d_bbox, covt_bbox_result* d_bres,
                                                   const covt_geo_xform* d_xf, uint32_t kinds, void* hip_stream) {
    if (n_columns < 0 || (kinds & ~7u) ||
        (n_columns && (!d_gdesc || !d_asm || !d_gres || !d_bdesc || !d_bbox || !d_bres || !d_xf)))
        return COVT_ERR_INVALID_ARG;
    if (n_columns == 0) return COVT_OK;
    if (n_columns > 0x7fffffff) return COVT_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)hip_stream;
    // the latitude code (device sinh, atan and their registers) only where the caller's table may need it
    return (kinds & (1u << COVT_GEO_AFFINE_LAT))
               ? covt::bbox_launch<2>(d_gdesc, d_asm, d_gres, d_bdesc, n_columns, d_bbox, d_bres, d_xf, kinds, s)
               : covt::bbox_launch<1>(d_gdesc, d_asm, d_gres, d_bdesc, n_columns, d_bbox, d_bres, d_xf, kinds, s);
}

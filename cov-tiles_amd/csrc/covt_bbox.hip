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
//   2. boxes: the segmented reduction of covt_segscan.h (the chunks, the runs and their owners, the hand-over
//      to the workgroup: described there) under BboxPolicy: the segments are the features, the value is the
//      int32 box under min / max, a coordinate's term is its point, a chunk is two rows of 128 coordinates
//      (16 bytes a lane and row), and start() is read from a window of kBboxWin values staged in LDS per wave
//      (three dependent gathers per feature, never per coordinate).  A feature's result goes out as its four
//      doubles.  Lanes keep the int32 min / max of the boxes they stored and their count of empty features;
//      one int32 atomic min / max / add per wave and value folds them into the result that launch 1
//      initialised (order-independent, so still deterministic).
//   3. finish: the int32 extent -> float64, NaN where the column has no coordinate or failed.
//
// The projected pass (include/covt.h "Georeferenced geometry") is the same three launches instantiated on
// the transform: boxes stay int32 up to the stores, and the two store sites (a feature's box, the extent) map
// the box's two ends per axis and take their fmin / fmax (bb_map).  GEO 0 is the plain pass and compiles to
// what it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covt.h"
#include "covt_bbox_plan.h"
#include "covt_geo_plan.h"
#include "covt_segscan.h"

namespace covt {

constexpr int kBboxWin = 512;    // start() values of consecutive features staged in LDS per wave
constexpr int kBboxAhead = 320;  // window entries wanted past the first open feature at a chunk's start

// a box: (xmin, ymin, xmax, ymax) in the int32 domain, joined by min / max
struct BoxV {
    typedef i32x4 T;
    static __device__ __forceinline__ T id() { return T{INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN}; }
    static __device__ __forceinline__ T pt(int32_t x, int32_t y) { return T{x, y, x, y}; }
    static __device__ __forceinline__ T join(T a, T b) {
        return T{min(a.x, b.x), min(a.y, b.y), max(a.z, b.z), max(a.w, b.w)};
    }
    static __device__ __forceinline__ T sel(bool p, T a, T b) {
        return T{p ? a.x : b.x, p ? a.y : b.y, p ? a.z : b.z, p ? a.w : b.w};
    }
    template <int CTRL, int RMASK>
    static __device__ __forceinline__ T dpp(T old, T v) {
        return T{(int32_t)dpp_move<CTRL, RMASK>((uint32_t)old.x, (uint32_t)v.x),
                 (int32_t)dpp_move<CTRL, RMASK>((uint32_t)old.y, (uint32_t)v.y),
                 (int32_t)dpp_move<CTRL, RMASK>((uint32_t)old.z, (uint32_t)v.z),
                 (int32_t)dpp_move<CTRL, RMASK>((uint32_t)old.w, (uint32_t)v.w)};
    }
    static __device__ __forceinline__ T bcast(T v, int src) {
        return T{(int32_t)lane_bcast((uint32_t)v.x, src), (int32_t)lane_bcast((uint32_t)v.y, src),
                 (int32_t)lane_bcast((uint32_t)v.z, src), (int32_t)lane_bcast((uint32_t)v.w, src)};
    }
    template <int N>
    struct Lds {
        T a[N];
        __device__ __forceinline__ T get(int i) const { return a[i]; }
        __device__ __forceinline__ void put(int i, T v) { a[i] = v; }
    };
};

// an int32 box as its four float64 (xmin, ymin, xmax, ymax): per axis the fmin / fmax of the two transformed
// ends, so a map that flips an axis (sy < 0) needs no sign test
template <int GEO>
__device__ __forceinline__ void bb_map(const GeoHold<GEO>& geo, i32x4 box, double (&o)[4]) {
    o[0] = (double)box.x, o[1] = (double)box.y, o[2] = (double)box.z, o[3] = (double)box.w;
    if constexpr (GEO != 0) {
        const double x0 = geo_x(geo.t, o[0]), x1 = geo_x(geo.t, o[2]);
        double y0 = geo_y<false>(geo.t, o[1]), y1 = geo_y<false>(geo.t, o[3]);
        if constexpr (GEO == 2)
            if (geo.lat) y0 = geo_lat(y0), y1 = geo_lat(y1);  // (uniform over the column)
        o[0] = fmin(x0, x1), o[1] = fmin(y0, y1), o[2] = fmax(x0, x1), o[3] = fmax(y0, y1);
    }
}

// the four arrays of covt_bbox_plan.h (out: the column's slice; byte offsets are multiples of 8)
template <int GEO>
__device__ __forceinline__ void bb_put(gw_f64* out, int32_t n, const GeoHold<GEO>& geo, int32_t f, i32x4 box, bool any) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double o[4];
    bb_map<GEO>(geo, box, o);
    out[bbox_array_off(n, 0) / 8 + f] = any ? o[0] : nan;
    out[bbox_array_off(n, 1) / 8 + f] = any ? o[1] : nan;
    out[bbox_array_off(n, 2) / 8 + f] = any ? o[2] : nan;
    out[bbox_array_off(n, 3) / 8 + f] = any ? o[3] : nan;
}

// The features of a column as the segments of covt_segscan.h, one per wave.  start(f .. ) is read from the
// wave's window win[kBboxWin] of staged values from feature wbase on; ext and n_empty: per lane, the join of
// the boxes it put and the empty features among them.
template <int GEO>
struct BboxPolicy {
    typedef BoxV V;
    static constexpr int kWaves = 4;    // waves per workgroup
    static constexpr int kRows = 2;     // rows of 64 lanes x 2 coordinates per chunk: 256 coordinates
    static constexpr int kWide = 2048;  // coordinates left past a run from which the workgroup finishes a feature
    static constexpr int kIncl = 0;
    static constexpr int kAhead = kBboxAhead;
    struct Raw {
        i32x4 q[kRows];
    };

    const GeomCol& c;
    const GeoHold<GEO>& geo;
    gw_f64* out;  // xmin | ymin | xmax | ymax, n doubles each
    int32_t* win;
    int32_t wbase;
    i32x4 ext;
    int32_t n_empty;

    __device__ __forceinline__ int32_t count() const { return c.n; }
    __device__ __forceinline__ int32_t items() const { return c.V; }
    __device__ __forceinline__ int32_t first_at(int32_t x) const {
        return seg_first_at(c.n, x, [&](int32_t f) { return c.start(f); });
    }
    // stage start(wbase .. wbase + kBboxWin) (features past n read as INT32_MAX), level by level so the
    // gathers of a level are in flight together; sync before use
    __device__ __forceinline__ void open(int32_t f) {
        constexpr int K = kBboxWin / 64;
        const int l = lane_id();
        wbase = f;
        int32_t v[K], ix[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ix[k] = wbase + 64 * k + l;
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = ((const g_i32*)c.geo)[min(ix[k], c.n)];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = ((const g_i32*)c.part)[clamp0(v[k], c.P)];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = ((const g_i32*)c.ring)[clamp0(v[k], c.R)];
        // (an or, not a select: every lane's three gathers stay with the others instead of moving under a branch)
#pragma unroll
        for (int k = 0; k < K; ++k) win[64 * k + l] = clamp0(v[k], c.V) | (ix[k] <= c.n ? 0 : 0x7fffffff);
    }
    // the window holds start(f .. f + need - 1)
    __device__ __forceinline__ void ensure(int32_t f, int32_t need) {
        if (f < wbase || f + need > wbase + kBboxWin) {
            wave_sync();
            open(f);
            wave_sync();
        }
    }
    __device__ __forceinline__ int32_t start(int32_t f) const { return win[f - wbase]; }
    __device__ __forceinline__ void load(Raw& r, int32_t a, int32_t b) const {
#pragma unroll
        for (int k = 0; k < kRows; ++k) r.q[k] = c.load2(a + 128 * k + 2 * lane_id(), b);
    }
    __device__ __forceinline__ void terms(const Raw& r, int k, int32_t, int32_t p0, int32_t L, int32_t, int32_t, i32x4& c0,
                                          i32x4& c1) const {
        c0 = p0 < L ? V::pt(r.q[k].x, r.q[k].y) : V::id();
        c1 = p0 + 1 < L ? V::pt(r.q[k].z, r.q[k].w) : V::id();
    }
    // 16 bytes a thread and step
    __device__ __forceinline__ i32x4 tail(int32_t from, int32_t to, int32_t tid, int32_t threads) const {
        i32x4 box = V::id();
        for (int32_t i = from + 2 * tid; i < to; i += 2 * threads) {
            const i32x4 q = c.load2(i, to);
            box = V::sel(i < to, V::join(box, V::pt(q.x, q.y)), box);
            box = V::sel(i + 1 < to, V::join(box, V::pt(q.z, q.w)), box);
        }
        return box;
    }
    __device__ __forceinline__ void put(int32_t f, i32x4 box, bool any) {
        bb_put<GEO>(out, c.n, geo, f, box, any);
        ext = V::join(ext, box);
        n_empty += any ? 0 : 1;
    }
};

template <int GEO>
struct __attribute__((aligned(16))) BboxSmem {
    int32_t win[BboxPolicy<GEO>::kWaves][kBboxWin];  // start() of the features from the wave's window base on
    SegSmem<BboxPolicy<GEO>> seg;
};

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
    const covt_bbox_desc bd = bdescs[c];
    int32_t st = geom_product_precheck(gdescs[c], gres[c], (bd.flags & COVT_BBOX_TOO_LARGE) != 0,
                                       bd.off >= 0 && !(bd.off & 15), bd.n_features);
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
template <int GEO>
__global__ __launch_bounds__(64 * BboxPolicy<GEO>::kWaves) void bbox_kernel(const covt_geom_desc* __restrict__ gdescs,
                                                                            const uint8_t* __restrict__ asmb,
                                                                            const covt_geom_result* __restrict__ gres,
                                                                            const covt_bbox_desc* __restrict__ bdescs,
                                                                            uint8_t* __restrict__ bbox,
                                                                            covt_bbox_result* __restrict__ bres,
                                                                            const covt_geo_xform* __restrict__ xf) {
    __shared__ BboxSmem<GEO> sm;
    const int64_t col = blockIdx.x;
    int32_t* const rcol = (int32_t*)(bres + col);
    if (rcol[0] != COVT_OK) return;  // (launch 1's, earlier on this stream; uniform over the workgroup)
    const covt_bbox_desc bd = bdescs[col];
    const GeoHold<GEO> geo = geo_hold<GEO>(xf, col);
    const GeomCol c = geom_col(gdescs[col], gres[col], asmb, bd.n_features);
    BboxPolicy<GEO> p{c, geo, (gw_f64*)(bbox + bd.off), sm.win[threadIdx.x >> 6], 0, BoxV::id(), 0};
    seg_run(p, sm.seg);
    // the column's extent and empty count: one atomic per wave and value, on launch 1's identities
    const i32x4 ext = seg_wave_join<BoxV>(p.ext);
    const int32_t ne = (int32_t)lane_bcast(incl_scan((uint32_t)p.n_empty), 63);
    if (lane_id() == 0) {
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
    bb_map<GEO>(geo_hold<GEO>(xf, c), i32x4{x0, y0, x1, y1}, o);  // (a column that failed: not stored)
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
    hipLaunchKernelGGL(bbox_kernel<GEO>, dim3((unsigned)n_columns, product_blocks_y(n_columns)),
                       dim3(64 * BboxPolicy<GEO>::kWaves), 0, s, d_gdesc, d_asm, d_gres, d_bdesc, d_bbox, d_bres, d_xf);
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

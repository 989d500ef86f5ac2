// covt_geo_plan.h -- the georeferencing transform of a geometry column (include/covt.h "Georeferenced
// geometry"), shared by the host plan (covt_host.cpp) and the kernels (covt_wkb.hip, covt_bbox.hip): plain
// arithmetic, no HIP calls, so a host-only program can include it.
//
// Everything here is evaluated in float64 in the order written, one rounding per operation: the multiply of
// an affine map is never contracted into its add (hipcc compiles with -ffp-contract=fast-honor-pragmas, so
// every function that rounds carries the pragma), which is what makes the host table, the device output and
// a two-line numpy reference agree bit for bit.
#ifndef COVT_GEO_PLAN_H
#define COVT_GEO_PLAN_H

#include <math.h>
#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_GEO_HD __host__ __device__
#else
#define COVT_GEO_HD
#endif
#if defined(__clang__)
#define COVT_GEO_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define COVT_GEO_NO_CONTRACT
#endif

#define COVT_GEO_W 20037508.342789244     /* pi * 6378137 in float64: half the side of the Web Mercator square */
#define COVT_GEO_PI 3.141592653589793     /* the float64 nearest pi */
#define COVT_GEO_DEG (180.0 / COVT_GEO_PI) /* degrees per radian, one division */

// o + s * p: two roundings
COVT_GEO_HD inline double geo_affine(double o, double s, double p) {
    COVT_GEO_NO_CONTRACT
    const double m = s * p;
    return o + m;
}
// the latitude in degrees of the Mercator ordinate t (radians on the unit sphere): the Gudermannian
COVT_GEO_HD inline double geo_lat(double t) { return atan(sinh(t)) * COVT_GEO_DEG; }

// the transformed x of pixel px; every kind maps x affinely
COVT_GEO_HD inline double geo_x(const covt_geo_xform& t, double px) { return geo_affine(t.ox, t.sx, px); }
// the transformed y of pixel py under AFFINE (LAT = false) or AFFINE_LAT
template <bool LAT>
COVT_GEO_HD inline double geo_y(const covt_geo_xform& t, double py) {
    const double v = geo_affine(t.oy, t.sy, py);
    return LAT ? geo_lat(v) : v;
}

// IDENTITY as an affine map: 0 + 1 * p is p bit for bit for every int32 p (+0.0 for 0), so a launch that
// maps affinely needs no branch for its tile-local columns
COVT_GEO_HD inline covt_geo_xform geo_identity_affine() {
    covt_geo_xform t;
    t.sx = 1.0, t.ox = 0.0, t.sy = 1.0, t.oy = 0.0;
    t.kind = COVT_GEO_AFFINE, t.reserved = 0;
    return t;
}

// The column's transform as a kernel holds it (uniform): nothing for a plain pass (GEO 0), the affine
// coefficients for a launch without latitudes (GEO 1: a tile-local column maps by 0 + 1 * p), and with them
// whether y goes on through the Gudermannian (GEO 2).
template <int GEO>
struct GeoHold {
    covt_geo_xform t;
    bool lat;
};
template <>
struct GeoHold<0> {};
template <int GEO>
COVT_GEO_HD inline GeoHold<GEO> geo_hold(const covt_geo_xform* xf, int64_t col) {
    GeoHold<GEO> g;
    if constexpr (GEO != 0) {
        g.t = xf[col];
        g.lat = GEO == 2 && g.t.kind == COVT_GEO_AFFINE_LAT;
        if (g.t.kind == COVT_GEO_IDENTITY) g.t = geo_identity_affine();
    }
    return g;
}

// The coefficient table of include/covt.h for tile z/x/y of a layer with `extent` pixels a side.
COVT_GEO_HD inline int geo_transform(int32_t crs, int32_t z, int32_t x, int32_t y, int32_t extent, covt_geo_xform& out) {
    COVT_GEO_NO_CONTRACT
    out.sx = out.ox = out.sy = out.oy = 0.0;
    out.kind = COVT_GEO_IDENTITY;
    out.reserved = 0;
    if (crs != COVT_CRS_TILE && crs != COVT_CRS_WEB_MERCATOR && crs != COVT_CRS_CRS84) return COVT_ERR_INVALID_ARG;
    if (z < 0 || z > 30 || x < 0 || y < 0 || extent < 1) return COVT_ERR_INVALID_ARG;
    const int64_t tiles = (int64_t)1 << z;
    if (x >= tiles || y >= tiles) return COVT_ERR_INVALID_ARG;
    if (crs == COVT_CRS_TILE) return COVT_OK;
    const double n = (double)tiles, E = (double)extent, W = COVT_GEO_W, PI = COVT_GEO_PI;
    const double nE = n * E, xn = (double)x / n, yn = (double)y / n;
    if (crs == COVT_CRS_WEB_MERCATOR) {
        const double W2 = 2 * W;
        out.sx = W2 / nE;
        out.ox = W2 * xn - W;
        out.sy = -out.sx;
        out.oy = W - W2 * yn;
        out.kind = COVT_GEO_AFFINE;
    } else {
        const double P2 = 2 * PI;
        out.sx = 360.0 / nE;
        out.ox = 360.0 * xn - 180.0;
        out.sy = -P2 / nE;
        out.oy = PI - P2 * yn;
        out.kind = COVT_GEO_AFFINE_LAT;
    }
    return COVT_OK;
}

// the status a projected pass gives column-transform `t` under the caller's promise `kinds`
COVT_GEO_HD inline int32_t geo_kind_status(int32_t kind, uint32_t kinds) {
    return ((uint32_t)kind <= (uint32_t)COVT_GEO_AFFINE_LAT && ((kinds >> kind) & 1u)) ? COVT_OK : COVT_ERR_INVALID_ARG;
}

#endif

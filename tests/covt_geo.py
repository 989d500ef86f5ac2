"""Reference for the georeferencing transform (include/covt.h "Georeferenced geometry"): the coefficient
table in plain Python floats, evaluated in the order the header writes it (one rounding per operation,
which is what Python's float arithmetic does), and ``apply`` in numpy float64 (numpy does not fuse a
multiply into an add).  The latitude is ``np.arctan(np.sinh(t)) * (180 / np.pi)``.
"""
from __future__ import annotations

import math

import numpy as np

CRS_TILE, CRS_WEB_MERCATOR, CRS_CRS84 = 0, 1, 2
IDENTITY, AFFINE, AFFINE_LAT = 0, 1, 2
W = 20037508.342789244
PI = math.pi
assert PI == 3.141592653589793 and W == math.pi * 6378137
XFORM_DTYPE = np.dtype([("sx", np.float64), ("ox", np.float64), ("sy", np.float64), ("oy", np.float64),
                        ("kind", np.int32), ("reserved", np.int32)])
NAN_BITS = 0x7FF8000000000000


def valid(crs, z, x, y, extent):
    return crs in (0, 1, 2) and 0 <= z <= 30 and 0 <= x < (1 << z) and 0 <= y < (1 << z) and extent >= 1


def transform(crs, z, x, y, extent):
    """(sx, ox, sy, oy, kind) of tile z/x/y for a layer of `extent` pixels a side."""
    assert valid(crs, z, x, y, extent)
    if crs == CRS_TILE:
        return 0.0, 0.0, 0.0, 0.0, IDENTITY
    n = float(1 << z)
    E = float(extent)
    if crs == CRS_WEB_MERCATOR:
        sx = (2 * W) / (n * E)
        ox = (2 * W) * (x / n) - W
        sy = -sx
        oy = W - (2 * W) * (y / n)
        return sx, ox, sy, oy, AFFINE
    sx = 360.0 / (n * E)
    ox = 360.0 * (x / n) - 180.0
    sy = -(2 * PI) / (n * E)
    oy = PI - (2 * PI) * (y / n)
    return sx, ox, sy, oy, AFFINE_LAT


def record(crs, z, x, y, extent):
    """transform() as one XFORM_DTYPE record (the bytes of covt_geo_xform)."""
    r = np.zeros(1, dtype=XFORM_DTYPE)
    r[0] = transform(crs, z, x, y, extent) + (0,)
    return r[0]


def apply(xf, xy):
    """xf: an XFORM_DTYPE record or (sx, ox, sy, oy, kind); xy: int32 [..., 2] -> float64 [..., 2]."""
    sx, ox, sy, oy, kind = (xf[k] for k in ("sx", "ox", "sy", "oy", "kind")) if isinstance(xf, np.void) else xf
    p = np.asarray(xy, dtype=np.int32).astype(np.float64)
    out = np.empty_like(p)
    if int(kind) == IDENTITY:
        out[...] = p
        return out
    sx, ox, sy, oy = (np.float64(v) for v in (sx, ox, sy, oy))
    out[..., 0] = ox + sx * p[..., 0]
    t = oy + sy * p[..., 1]
    with np.errstate(over="ignore"):  # (a coordinate far outside its tile: sinh overflows to inf, atan gives pi/2)
        out[..., 1] = np.arctan(np.sinh(t)) * (180 / np.pi) if int(kind) == AFFINE_LAT else t
    return out


def apply_boxes(xf, ref):
    """The transform of a covt_bbox result (xmin, ymin, xmax, ymax, extent, n_empty) whose values are
    integral float64: per axis min / max of the two transformed ends; NaN rows stay the quiet NaN."""
    xmin, ymin, xmax, ymax, extent, n_empty = ref

    def both(lo_x, lo_y, hi_x, hi_y):
        lo_x, lo_y, hi_x, hi_y = (np.asarray(a, dtype=np.float64) for a in (lo_x, lo_y, hi_x, hi_y))
        nan = np.isnan(lo_x)
        ints = lambda a: np.where(nan, 0.0, a).astype(np.int64).astype(np.int32)  # noqa: E731
        a = apply(xf, np.stack([ints(lo_x), ints(lo_y)], axis=-1))
        b = apply(xf, np.stack([ints(hi_x), ints(hi_y)], axis=-1))
        q = np.full(lo_x.shape, np.nan)
        res = [np.where(nan, q, f(a[..., k], b[..., k])) for f in (np.minimum, np.maximum) for k in (0, 1)]
        return res  # xmin, ymin, xmax, ymax

    bx = both(xmin, ymin, xmax, ymax)
    ex = both(extent[0], extent[1], extent[2], extent[3])
    return bx[0], bx[1], bx[2], bx[3], np.array([float(v) for v in ex], dtype=np.float64), n_empty


def zxy_of_key(key: str):
    """'omt/5_16_20' or 'bing/4-8-5' -> (z, x, y)."""
    name = key.split("/")[-1]
    z, x, y = (int(v) for v in name.replace("-", "_").split("_"))
    return z, x, y

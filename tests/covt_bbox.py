"""Reference bounding boxes of an assembled geometry column (include/covt.h "Geometry bounding boxes"):
per feature the min / max of every coordinate the nested offsets attribute to it, as float64; the quiet
NaN for a feature without a coordinate.

* ``bbox_plain``: the definition, nested loops over features, parts and rings;
* ``bbox_numpy``: the same, vectorised (a feature's coordinates are one contiguous range; empty ranges are
  masked out, never reduced);
* ``wkb_bounds``: the bounds of parsed WKB features (``covt_wkb.parse``), so a box can be held against the
  WKB value beside it.

All return ``(xmin, ymin, xmax, ymax, extent, n_empty)``: four float64 arrays of n values, the column's
extent as float64[4] and the number of NaN rows.
"""
from __future__ import annotations

import numpy as np

NAN_BITS = 0x7FF8000000000000


def _nan(n):
    a = np.full(n, np.nan, dtype=np.float64)
    assert n == 0 or int(a.view(np.uint64)[0]) == NAN_BITS  # numpy's nan is the quiet NaN of the definition
    return a


def _finish(xmin, ymin, xmax, ymax):
    empty = np.isnan(xmin)
    if empty.all():
        extent = _nan(4)
    else:
        k = ~empty
        extent = np.array([xmin[k].min(), ymin[k].min(), xmax[k].max(), ymax[k].max()], dtype=np.float64)
    return xmin, ymin, xmax, ymax, extent, int(empty.sum())


def bbox_plain(geo, part, ring, coords):
    n = len(geo) - 1
    xmin, ymin, xmax, ymax = _nan(n), _nan(n), _nan(n), _nan(n)
    geo, part, ring = (np.asarray(a).tolist() for a in (geo, part, ring))  # (Python ints: the loops run faster)
    xy = np.asarray(coords).reshape(-1, 2)
    X, Y = xy[:, 0].tolist(), xy[:, 1].tolist()
    for f in range(n):
        xs, ys = [], []
        for p in range(geo[f], geo[f + 1]):
            for r in range(part[p], part[p + 1]):
                for v in range(ring[r], ring[r + 1]):
                    xs.append(X[v])
                    ys.append(Y[v])
        if xs:
            xmin[f], ymin[f], xmax[f], ymax[f] = float(min(xs)), float(min(ys)), float(max(xs)), float(max(ys))
    return _finish(xmin, ymin, xmax, ymax)


def bbox_numpy(geo, part, ring, coords):
    geo, part, ring = (np.asarray(a, dtype=np.int64) for a in (geo, part, ring))
    n = geo.size - 1
    xmin, ymin, xmax, ymax = _nan(n), _nan(n), _nan(n), _nan(n)
    start = ring[part[geo]]  # feature f: coords[start[f]:start[f + 1]]
    s, e = start[:-1], start[1:]
    full = np.nonzero(e > s)[0]
    if full.size:
        xy = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
        # the nonempty features' ranges: consecutive ones may leave gaps (none in an assembled column), so
        # every range is reduced between its own start and the next range's start, then its tail cut off by
        # reducing [s, e) only: reduceat over [s0, e0, s1, e1, ...] and every second result
        idx = np.stack([s[full], e[full]], axis=1).reshape(-1)
        last = idx[-1] == xy.shape[0]
        if last:  # reduceat takes no index == len: pad one row
            xy = np.concatenate([xy, xy[-1:]], axis=0)
        for k, (lo, hi) in enumerate(((xmin, xmax), (ymin, ymax))):
            lo[full] = np.minimum.reduceat(xy[:, k], idx)[0::2]
            hi[full] = np.maximum.reduceat(xy[:, k], idx)[0::2]
    return _finish(xmin, ymin, xmax, ymax)


def wkb_bounds(features):
    """Bounds of [(geom_class, parts)] as covt_wkb.parse gives them (parse with unclose=False, so the
    rings hold every vertex the value holds)."""
    n = len(features)
    xmin, ymin, xmax, ymax = _nan(n), _nan(n), _nan(n), _nan(n)
    for f, (_, parts) in enumerate(features):
        pts = [pt for p in parts for pt in p]
        if pts:
            xs, ys = [p[0] for p in pts], [p[1] for p in pts]
            xmin[f], ymin[f], xmax[f], ymax[f] = float(min(xs)), float(min(ys)), float(max(xs)), float(max(ys))
    return _finish(xmin, ymin, xmax, ymax)


def wkb_column_bounds(offsets, data):
    """Bounds of the WKB values of a column (int32 offsets [n + 1] into data), read with struct straight
    from the bytes: wkb_bounds(covt_wkb.parse_column(...)) without a tuple per point, for whole tile sets.
    Little-endian 2-D ISO WKB, codes 1 .. 6."""
    import struct

    buf = bytes(data)
    n = len(offsets) - 1
    xmin, ymin, xmax, ymax = _nan(n), _nan(n), _nan(n), _nan(n)
    u32 = struct.Struct("<I").unpack_from

    def value(pos, xs, ys):  # one geometry at pos -> the position after it
        if buf[pos] != 1:
            raise ValueError("byte order")
        code = u32(buf, pos + 1)[0]
        pos += 5
        if code == 1:
            x, y = struct.unpack_from("<dd", buf, pos)
            xs.append(x)
            ys.append(y)
            return pos + 16
        if code in (2, 3):
            rings = 1
            if code == 3:
                rings = u32(buf, pos)[0]
                pos += 4
            for _ in range(rings):
                k = u32(buf, pos)[0]
                pos += 4
                if k:
                    v = struct.unpack_from("<%dd" % (2 * k), buf, pos)
                    xs.extend(v[0::2])
                    ys.extend(v[1::2])
                    pos += 16 * k
            return pos
        if code in (4, 5, 6):
            parts = u32(buf, pos)[0]
            pos += 4
            for _ in range(parts):
                if u32(buf, pos + 1)[0] != code - 3:
                    raise ValueError("part code")
                pos = value(pos, xs, ys)
            return pos
        raise ValueError("geometry code %d" % code)

    offs = np.asarray(offsets).tolist()
    for f in range(n):
        xs, ys = [], []
        if value(offs[f], xs, ys) != offs[f + 1]:
            raise ValueError("feature %d: length" % f)
        if xs:
            xmin[f], ymin[f], xmax[f], ymax[f] = min(xs), min(ys), max(xs), max(ys)
    return _finish(xmin, ymin, xmax, ymax)


def same(a, b):
    """Two results equal as bytes (NaN rows included)."""
    return all(np.asarray(x, np.float64).tobytes() == np.asarray(y, np.float64).tobytes()
               for x, y in zip(a[:5], b[:5])) and int(a[5]) == int(b[5])

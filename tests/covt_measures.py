"""Reference measures of an assembled geometry column (include/covt.h "Geometry measures"): per feature its
area (exact 64-bit integer shoelace, shell minus holes by absolute value, mod 2^64 as the header defines it),
its length (float64 segment lengths) and its number of coordinates.

* ``measures_plain``: the definition, nested loops over features, parts and rings with Python ints reduced
  mod 2^64; the length is ``math.fsum`` of the per-segment ``math.sqrt``, i.e. the exactly rounded sum;
* ``measures_numpy``: the same, vectorised with int64 wraparound (prefix-sum differences are exact mod 2^64);
  the length is summed by ``np.add.reduceat``, so it agrees with ``measures_plain`` within ``length_bound``, or
  with ``fsum=True`` by ``math.fsum`` over each feature's terms: ``measures_plain``'s bytes, fast enough for
  whole tile sets and long rings;
* ``wkb_measures``: the same three values from the WKB values of a column (``covt_wkb.parse`` for the points,
  a walk of the headers for which rings are shells), so they can be held against the WKB beside them; with
  ``parse=False`` through ``wkb_nested``, the values' nested offsets, and ``measures_numpy``.

All return ``(area float64[n], length float64[n], num_coords int32[n])``.  ``length_bound`` is the header's
promise: a length within ``(m_f + 4) * 2^-52`` relative of the exactly rounded sum, m_f the segment count.
"""
from __future__ import annotations

import math
import struct

import numpy as np

import covt_wkb as W

M64 = (1 << 64) - 1
POLYGONAL = (2, 5)  # GeometryTypes ordinals with an area
LINEAR = (1, 2, 4, 5)  # ... with a length


def _mag(s):  # |S| of S mod 2^64 read as int64, as uint64
    s &= M64
    return s if s < 1 << 63 else (1 << 64) - s


def _as_i64(t):
    t &= M64
    return t - (1 << 64) if t >= 1 << 63 else t


def ring_terms(pts):
    """(S mod 2^64, [segment lengths]) of one ring given as [(x, y)] Python ints."""
    s, seg = 0, []
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        s += x0 * y1 - x1 * y0
        dx, dy = float(x1 - x0), float(y1 - y0)
        seg.append(math.sqrt(dx * dx + dy * dy))
    return s & M64, seg


def feature_measures(t, polygons):
    """One feature of GeometryTypes ordinal t whose parts are `polygons`: a list of parts, each a list of
    rings, each a list of (x, y) -> (area, length, num_coords)."""
    total, seg, n = 0, [], 0
    for rings in polygons:
        for k, pts in enumerate(rings):
            s, sg = ring_terms(pts)
            total += _mag(s) if k == 0 else -_mag(s)
            seg += sg
            n += len(pts)
    area = float(_as_i64(total)) * 0.5 if t in POLYGONAL else 0.0
    return area, (math.fsum(seg) if t in LINEAR else 0.0), n


def measures_plain(types, geo, part, ring, coords):
    n = len(geo) - 1
    area, length, count = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    geo, part, ring = (np.asarray(a).tolist() for a in (geo, part, ring))
    xy = np.asarray(coords).reshape(-1, 2)
    pts = list(zip(xy[:, 0].tolist(), xy[:, 1].tolist()))
    for f in range(n):
        polygons = [[pts[ring[r]:ring[r + 1]] for r in range(part[p], part[p + 1])] for p in range(geo[f], geo[f + 1])]
        area[f], length[f], count[f] = feature_measures(int(types[f]), polygons)
    return area, length, count


def measures_numpy(types, geo, part, ring, coords, fsum=False):
    t = np.asarray(types, dtype=np.int64)
    geo, part, ring = (np.asarray(a, dtype=np.int64) for a in (geo, part, ring))
    n = geo.size - 1
    xy = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
    g0, g1 = geo[:-1], geo[1:]
    r0, r1 = part[g0], part[g1]
    c0, c1 = ring[r0], ring[r1]
    P, R = (int(geo[-1]), int(part[int(geo[-1])])) if n else (0, 0)
    V = int(ring[R]) if n else 0
    # edge i -> i + 1, zero where i + 1 starts another ring or the column ends (index V: padding)
    term = np.zeros(V + 1, dtype=np.int64)
    seg = np.zeros(V + 1, dtype=np.float64)
    if V > 1:
        x, y = xy[:V, 0], xy[:V, 1]
        inside = np.ones(V - 1, dtype=bool)
        heads = ring[:R + 1]
        inside[heads[(heads > 0) & (heads < V)] - 1] = False
        with np.errstate(over="ignore"):
            term[:V - 1] = np.where(inside, x[:-1] * y[1:] - x[1:] * y[:-1], 0)
        dx, dy = (x[1:] - x[:-1]).astype(np.float64), (y[1:] - y[:-1]).astype(np.float64)
        seg[:V - 1] = np.where(inside, np.sqrt(dx * dx + dy * dy), 0.0)
    with np.errstate(over="ignore"):
        pre = np.concatenate([np.zeros(1, np.int64), np.cumsum(term)])  # pre[k]: the sum of the edges below k
        rs, re = ring[:R], ring[1:R + 1]
        s_ring = pre[np.maximum(re - 1, rs)] - pre[rs]
        mag = np.where(s_ring < 0, -s_ring, s_ring).view(np.uint64)
        all_pre = np.concatenate([np.zeros(1, np.uint64), np.cumsum(mag, dtype=np.uint64)])
        ps, pe = part[:P], part[1:P + 1]
        shell = np.where(pe > ps, mag[np.minimum(ps, max(R - 1, 0))] if R else 0, 0).astype(np.uint64)
        shell_pre = np.concatenate([np.zeros(1, np.uint64), np.cumsum(shell, dtype=np.uint64)])
        total = (np.uint64(2) * (shell_pre[g1] - shell_pre[g0]) - (all_pre[r1] - all_pre[r0])).view(np.int64)
    polygonal, linear = np.isin(t, POLYGONAL), np.isin(t, LINEAR)
    area = np.where(polygonal, total.astype(np.float64) * 0.5, 0.0)
    length = np.zeros(n, dtype=np.float64)
    full = np.nonzero(linear & (c1 - c0 > 1))[0]  # (the features with an edge: reduceat takes no empty range)
    if full.size and fsum:
        length[full] = [math.fsum(seg[a:b].tolist()) for a, b in zip(c0[full].tolist(), (c1[full] - 1).tolist())]
    elif full.size:
        idx = np.stack([c0[full], c1[full] - 1], axis=1).reshape(-1)
        length[full] = np.add.reduceat(seg, idx)[0::2]
    return area, length, (c1 - c0).astype(np.int32)


_U32 = struct.Struct("<I").unpack_from


def _wkb_single(buf, pos, code):
    """The rings of a POINT / LINESTRING / POLYGON body (after its header) at pos -> (rings, end)."""
    if code == 1:
        counts = (1,)
    elif code == 2:
        counts = (_U32(buf, pos)[0],)
        pos += 4
    else:
        counts = None
        k = _U32(buf, pos)[0]
        pos += 4
    rings = []
    for _ in range(k if counts is None else 1):
        if counts is None:
            c = _U32(buf, pos)[0]
            pos += 4
        else:
            c = counts[0]
        v = struct.unpack_from("<%dd" % (2 * c), buf, pos)
        pos += 16 * c
        rings.append([(int(x), int(y)) for x, y in zip(v[0::2], v[1::2])])
    return rings, pos


def _wkb_polygons(buf, pos):
    """The WKB value at pos -> (GeometryTypes ordinal, parts as lists of rings as lists of (x, y) ints, end):
    covt_wkb.parse keeps the points, this walk of the headers keeps which ring opens a polygon."""
    code = _U32(buf, pos + 1)[0]
    pos += 5
    if code <= 3:
        rings, pos = _wkb_single(buf, pos, code)
        return code - 1, [rings], pos
    parts = []
    k = _U32(buf, pos)[0]
    pos += 4
    for _ in range(k):
        rings, pos = _wkb_single(buf, pos + 5, code - 3)
        parts.append(rings)
    return code - 1, parts, pos


def wkb_nested(offsets, data):
    """The WKB values of a column back as nested offsets -> (types, geo, part, ring, coords int64 (n, 2)): a
    walk of the headers only, the coordinates taken a ring at a time, for whole tile sets."""
    b = bytes(data)
    offs = np.asarray(offsets).tolist()
    types, geo, part, ring, xy = [], [0], [0], [0], []
    u32, f8 = _U32, np.frombuffer

    def single(code, pos):  # one part: its rings appended -> the position after it
        if code == 3:
            k = u32(b, pos)[0]
            pos += 4
        else:
            k = 1
        for _ in range(k):
            if code == 1:
                c = 1
            else:
                c = u32(b, pos)[0]
                pos += 4
            if c:
                xy.append(f8(b, "<f8", 2 * c, pos))
                pos += 16 * c
            ring.append(ring[-1] + c)
        part.append(len(ring) - 1)
        return pos

    for f in range(len(offs) - 1):
        pos = offs[f]
        code = u32(b, pos + 1)[0]
        types.append(code - 1)
        if code <= 3:
            pos = single(code, pos + 5)
        else:
            k = u32(b, pos + 5)[0]
            pos += 9
            for _ in range(k):
                pos = single(code - 3, pos + 5)
        assert pos == offs[f + 1]
        geo.append(len(part) - 1)
    coords = np.concatenate(xy).reshape(-1, 2) if xy else np.zeros((0, 2))
    assert (coords == np.rint(coords)).all()
    return np.asarray(types, np.uint8), np.asarray(geo), np.asarray(part), np.asarray(ring), coords.astype(np.int64)


def wkb_measures(offsets, data, with_segments=False, parse=True):
    """The measures of the WKB values of a column (int32 offsets [n + 1] into data); with_segments: and m_f,
    the number of segments of every value, as a fourth array.  parse=True reads every value with
    covt_wkb.parse (and with the header walk that tells which ring opens a polygon) and measures it by
    feature_measures; parse=False takes the nested offsets of wkb_nested through measures_numpy(fsum=True):
    the same bytes (test_measures_ref.py), several times faster over whole tile sets."""
    if not parse:
        col = wkb_nested(offsets, data)
        return measures_numpy(*col, fsum=True) + ((segments(*col[1:4]),) if with_segments else ())
    b = bytes(data)
    offs = np.asarray(offsets).tolist()
    n = len(offs) - 1
    area, length, count = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    m = np.zeros(n, dtype=np.int64)
    for f in range(n):
        t, parts, end = _wkb_polygons(b, offs[f])
        assert end == offs[f + 1]
        # (the two readers see the same points)
        assert [tuple(r) for p in parts for r in p] == [tuple(r) for r in W.parse(b[offs[f]:end])[1]]
        area[f], length[f], count[f] = feature_measures(t, parts)
        m[f] = sum(max(len(r) - 1, 0) for p in parts for r in p)
    return (area, length, count, m) if with_segments else (area, length, count)


def segments(geo, part, ring):
    """m_f of every feature: the number of edge terms (a ring of m coordinates has max(m - 1, 0))."""
    geo, part, ring = (np.asarray(a, dtype=np.int64) for a in (geo, part, ring))
    R = int(part[int(geo[-1])]) if geo.size > 1 else 0
    per_ring = np.concatenate([[0], np.cumsum(np.maximum(np.diff(ring[:R + 1]) - 1, 0))])
    return per_ring[part[geo[1:]]] - per_ring[part[geo[:-1]]]


def length_bound(exact, m):
    """The header's promise around the exactly rounded lengths `exact`: (m_f + 4) * 2^-52 relative."""
    return (np.asarray(m, dtype=np.float64) + 4.0) * 2.0 ** -52 * np.abs(exact)


def same(got, ref, m):
    """got equals ref (measures_plain's): area and num_coords as bytes, length within length_bound."""
    return (np.asarray(got[0], np.float64).tobytes() == np.asarray(ref[0], np.float64).tobytes()
            and np.asarray(got[2], np.int32).tobytes() == np.asarray(ref[2], np.int32).tobytes()
            and not np.signbit(np.asarray(got[1])).any()
            and bool((np.abs(np.asarray(got[1], np.float64) - ref[1]) <= length_bound(ref[1], m)).all()))

"""Test helpers for the WKB serialization (include/covt.h "Geometry as WKB").

* ``write_plain``: a nested-loop writer over one assembled column ``(types, geo, part, ring, coords)``
  -- the definition the kernel is held to: little-endian ISO WKB, geometry code = GeometryTypes ordinal
  + 1, uint32 counts, float64 coordinates, the assembled structure as it is (closed rings, empty parts and
  rings with count 0);
* ``write_numpy``: the same bytes from vectorised closed forms (per-feature sizes, a cumulative sum,
  every header and coordinate scattered to its address), fast enough for whole fixture sets and the
  10k-tile batch; pinned against ``write_plain`` in test_wkb_writer.py;
* ``parse``: a small WKB reader, ``[(geom_class, parts)]`` in the representation of
  ``covt_asm.to_features`` (``unclose`` drops the closing vertex of polygon rings as that function does).
"""
from __future__ import annotations

import struct

import numpy as np

POINT, LINESTRING, POLYGON, MULTIPOINT, MULTILINESTRING, MULTIPOLYGON = range(6)
_CLASS = {1: 1, 4: 1, 2: 2, 5: 2, 3: 3, 6: 3}  # WKB code -> point / line / polygon class


def _pts(coords, a, b):  # points a .. b - 1 as x, y float64 pairs
    return np.asarray(coords[a:b], dtype="<f8").tobytes()


def write_plain(types, geo, part, ring, coords):
    """-> (int32 offsets [n + 1], bytes) of one column, feature by feature."""
    out, offs = bytearray(), [0]
    for f, t in enumerate(types):
        t = int(t)
        g0, g1 = int(geo[f]), int(geo[f + 1])
        hdr = struct.pack("<BI", 1, t + 1)

        def rings_of(p):
            return range(int(part[p]), int(part[p + 1]))

        def line(r):  # count + points of ring r
            a, b = int(ring[r]), int(ring[r + 1])
            return struct.pack("<I", b - a) + _pts(coords, a, b)

        def polygon(p):  # ring count + rings of part p
            return struct.pack("<I", len(rings_of(p))) + b"".join(line(r) for r in rings_of(p))

        if t == POINT:
            r = int(part[g0])
            out += hdr + _pts(coords, int(ring[r]), int(ring[r]) + 1)
        elif t == LINESTRING:
            out += hdr + line(int(part[g0]))
        elif t == POLYGON:
            out += hdr + polygon(g0)
        elif t == MULTIPOINT:
            out += hdr + struct.pack("<I", g1 - g0)
            for p in range(g0, g1):
                r = int(part[p])
                out += struct.pack("<BI", 1, 1) + _pts(coords, int(ring[r]), int(ring[r]) + 1)
        elif t == MULTILINESTRING:
            out += hdr + struct.pack("<I", g1 - g0)
            for p in range(g0, g1):
                out += struct.pack("<BI", 1, 2) + line(int(part[p]))
        elif t == MULTIPOLYGON:
            out += hdr + struct.pack("<I", g1 - g0)
            for p in range(g0, g1):
                out += struct.pack("<BI", 1, 3) + polygon(p)
        else:
            raise ValueError("geometry type %d" % t)
        offs.append(len(out))
    return np.asarray(offs, dtype=np.int32), bytes(out)


def _put(buf, pos, vals, dt):
    v = np.ascontiguousarray(vals, dtype=dt)
    w = v.size * v.itemsize // max(len(pos), 1)  # bytes per position (a coordinate pair: 16)
    buf[np.asarray(pos, dtype=np.int64)[:, None] + np.arange(w)] = v.view(np.uint8).reshape(len(pos), w)


def write_numpy(types, geo, part, ring, coords):
    """-> (int32 offsets [n + 1], uint8 array): write_plain's bytes, vectorised."""
    t = np.asarray(types, dtype=np.int64)
    geo, part, ring = (np.asarray(a, dtype=np.int64) for a in (geo, part, ring))
    xy = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
    n = t.size
    g0, g1 = geo[:-1], geo[1:]
    r0, r1 = part[g0], part[g1]
    c0, c1 = ring[r0], ring[r1]
    G, R, C = g1 - g0, r1 - r0, c1 - c0
    poly, multi = (t == POLYGON) | (t == MULTIPOLYGON), t >= MULTIPOINT
    size = np.where(t == POINT, 21, np.where(t == MULTIPOINT, 9 + 21 * G, 9 + 16 * C + 4 * R * poly
                                             + 9 * G * (t >= MULTILINESTRING)))
    off = np.concatenate([[0], np.cumsum(size)])
    assert off[-1] < 1 << 31
    buf = np.zeros(int(off[-1]), dtype=np.uint8)
    fo = off[:-1]
    # feature headers
    buf[fo] = 1
    _put(buf, fo + 1, t + 1, "<u4")
    has = t != POINT
    cnt = np.where(t == LINESTRING, C, np.where(t == POLYGON, R, G))
    _put(buf, fo[has] + 5, cnt[has], "<u4")
    # owners by repetition (empty segments repeat zero times)
    P, NR, V = int(geo[-1]) if n else 0, int(part[int(geo[-1])]) if n else 0, 0
    V = int(ring[NR]) if n else 0
    f_of_p = np.repeat(np.arange(n), G)
    p_of_r = np.repeat(np.arange(P), np.diff(part[:P + 1]))
    r_of_c = np.repeat(np.arange(NR), np.diff(ring[:NR + 1]))
    # part headers (MULTI* only)
    p = np.arange(P)
    f = f_of_p
    tp, dp = t[f], p - g0[f]
    rs, re = part[:P], part[1:P + 1]
    cs = ring[rs]
    m = tp == MULTIPOINT
    pos = fo[f] + 9 + 21 * dp
    buf[pos[m]] = 1
    _put(buf, pos[m] + 1, np.ones(int(m.sum())), "<u4")
    m = tp >= MULTILINESTRING
    pos = fo[f] + 9 + 9 * dp + 4 * (rs - r0[f]) * (tp == MULTIPOLYGON) + 16 * (cs - c0[f])
    buf[pos[m]] = 1
    _put(buf, pos[m] + 1, tp[m] - 2, "<u4")
    _put(buf, pos[m] + 5, np.where(tp == MULTILINESTRING, ring[re] - cs, re - rs)[m], "<u4")
    # ring counts (polygons only)
    r = np.arange(NR)
    pr = p_of_r
    f = f_of_p[pr]
    tr = t[f]
    m = poly[f]
    pos = fo[f] + 9 + 9 * (pr - g0[f] + 1) * (tr == MULTIPOLYGON) + 4 * (r - r0[f]) + 16 * (ring[:NR] - c0[f])
    _put(buf, pos[m], (ring[1:NR + 1] - ring[:NR])[m], "<u4")
    # coordinates
    c = np.arange(V)
    rc = r_of_c
    pc = p_of_r[rc]
    f = f_of_p[pc]
    tc = t[f]
    dp, dr, dc = pc - g0[f], rc - r0[f], c - c0[f]
    pos = fo[f] + np.select([tc == POINT, tc == LINESTRING, tc == POLYGON, tc == MULTIPOINT, tc == MULTILINESTRING],
                            [5, 9 + 16 * dc, 9 + 4 * (dr + 1) + 16 * dc, 9 + 21 * dp + 5, 9 + 9 * (dp + 1) + 16 * dc],
                            9 + 9 * (dp + 1) + 4 * (dr + 1) + 16 * dc)
    _put(buf, pos, xy[:V].astype("<f8"), "<f8")
    return off.astype(np.int32), buf


def parse(value: bytes, unclose: bool = False):
    """One WKB value -> (geom_class, parts): parts are tuples of (x, y) int tuples, one per point / line /
    ring in order.  Little-endian 2-D ISO WKB only; coordinates must be integral."""
    pos = 0

    def u32():
        nonlocal pos
        v = struct.unpack_from("<I", value, pos)[0]
        pos += 4
        return v

    def head():
        nonlocal pos
        if value[pos] != 1:
            raise ValueError("byte order %d" % value[pos])
        pos += 1
        return u32()

    def points(k):
        nonlocal pos
        out = []
        for _ in range(k):
            x, y = struct.unpack_from("<dd", value, pos)
            pos += 16
            if x != int(x) or y != int(y):
                raise ValueError("non-integral coordinate")
            out.append((int(x), int(y)))
        return tuple(out)

    def ring():
        pts = points(u32())
        return pts[:-1] if unclose and pts else pts

    def single(code, parts):
        if code == 1:
            parts.append(points(1))
        elif code == 2:
            parts.append(points(u32()))
        elif code == 3:
            for _ in range(u32()):
                parts.append(ring())
        else:
            raise ValueError("geometry code %d" % code)

    code = head()
    parts = []
    if code in (1, 2, 3):
        single(code, parts)
    elif code in (4, 5, 6):
        for _ in range(u32()):
            sub = head()
            if sub != code - 3:
                raise ValueError("part code %d in a geometry of code %d" % (sub, code))
            single(sub, parts)
    else:
        raise ValueError("geometry code %d" % code)
    if pos != len(value):
        raise ValueError("%d trailing bytes" % (len(value) - pos))
    return _CLASS[code], parts


def parse_column(offsets, data, unclose: bool = False):
    b = bytes(data)
    return [parse(b[int(offsets[i]):int(offsets[i + 1])], unclose) for i in range(len(offsets) - 1)]

"""Reference MVT geometry encoding of an assembled geometry column (include/covt.h "Geometry as MVT"): shifted
coordinates, closedness, the winding rule, cursor deltas, zigzag, varints and the command integers; numpy, and
nothing the kernel uses.

``mvt_ref(types, geo, part, ring, coords, orient, shift)`` -> ``(type uint8[n], offsets int32[n + 1], bytes uint8[])``.
``ring_plan`` gives what the definition fixes per ring (k, closed, reversed, S_r), for tests that assert on it.
``bare_layer`` wraps values into a minimal MVT layer (no ids, no tags) that tests/covt_geom.mvt_layers reads.
"""
from __future__ import annotations

import numpy as np

from covt_simplify import LINES, POINTS, POLYGONS, _owner

U32 = 0xFFFFFFFF
GEOM_TYPE = np.array([1, 2, 3, 1, 2, 3], dtype=np.uint8)


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def ring_plan(types, geo, part, ring, coords, orient: bool, shift: int):
    """Per ring: its feature, its type, m, k, closed, reversed and S_r (int64); and q, the shifted coordinates."""
    assert 0 <= shift <= 30
    geo, part, ring = _i64(geo), _i64(part), _i64(ring)
    n = geo.size - 1
    n_parts, n_rings = int(geo[n]), int(part[int(geo[n])])
    R = ring.size - 1
    assert n_rings == R, "every ring belongs to a part of a feature"
    V = int(ring[R])
    q = (np.asarray(coords, dtype=np.int32).reshape(-1, 2)[:V] >> np.int32(shift)).astype(np.int64)
    ring_part = _owner(part[:n_parts + 1], R)
    ring_feature = _owner(geo, n_parts)[ring_part]
    t = _i64(types)[ring_feature]
    first = part[ring_part] == np.arange(R)  # the first ring of its part
    a, b = ring[:-1], ring[1:]
    m = b - a
    poly = np.isin(t, POLYGONS)
    closed = np.zeros(R, dtype=bool)
    two = poly & (m >= 2)
    closed[two] = (q[a[two]] == q[b[two] - 1]).all(axis=1)
    k = m - closed
    # S_r: the sum over i in a .. b - 2 of x_i y_{i+1} - x_{i+1} y_i, mod 2^64, read as int64
    S = np.zeros(R, dtype=np.int64)
    if V > 1:
        e = (q[:-1, 0] * q[1:, 1]).astype(np.uint64) - (q[1:, 0] * q[:-1, 1]).astype(np.uint64)
        c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(e, dtype=np.uint64)])  # c[i]: the edges before i
        has = m >= 1
        S[has] = (c[b[has] - 1] - c[a[has]]).view(np.int64)
    rev = closed & np.where(first, S < 0, S > 0) if orient else np.zeros(R, dtype=bool)
    return {"feature": ring_feature, "t": t, "a": a, "b": b, "m": m, "k": k, "closed": closed, "rev": rev, "S": S,
            "q": q, "n": n, "R": R, "V": V}


def _varints(vals: np.ndarray):
    """uint32 values -> (their LEB128 bytes back to back, the length of each)."""
    v = vals.astype(np.uint64)
    ln = 1 + (v >= 1 << 7) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(ln)])
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    for j in range(5):
        sel = ln > j
        out[off[:-1][sel] + j] = ((v[sel] >> np.uint64(7 * j)) & np.uint64(0x7F)).astype(np.uint8) | \
            np.where(ln[sel] > j + 1, 0x80, 0).astype(np.uint8)
    return out, ln


def _zigzag(d: np.ndarray) -> np.ndarray:
    """zz(d) of the int32 difference (two's-complement wrap-around) of int64 values."""
    d32 = ((d + (1 << 31)) & U32) - (1 << 31)
    return ((d32 << 1) ^ (d32 >> 31)) & U32


def mvt_ref(types, geo, part, ring, coords, orient: bool = False, shift: int = 0):
    p = ring_plan(types, geo, part, ring, coords, orient, shift)
    n, R, V, q = p["n"], p["R"], p["V"], p["q"]
    gtype = GEOM_TYPE[_i64(types)] if n else np.zeros(0, np.uint8)
    ring_of = _owner(np.concatenate([p["a"], p["b"][-1:]]) if R else np.zeros(1, np.int64), V)
    j = np.arange(V, dtype=np.int64) - p["a"][ring_of]
    item = j < p["k"][ring_of]  # (a closed polygon ring's last position is no item)
    ring_of, j = ring_of[item], j[item]
    N = j.size
    a, b, k, t = p["a"][ring_of], p["b"][ring_of], p["k"][ring_of], p["t"][ring_of]
    src = np.where(p["rev"][ring_of], b - 1 - j, a + j)
    v = q[src]
    f = p["feature"][ring_of]
    head = np.ones(N, dtype=bool)  # the first item of its feature: the cursor is the origin
    head[1:] = f[1:] != f[:-1]
    prev = np.zeros((N, 2), dtype=np.int64)
    prev[1:] = v[:-1]
    prev[head] = 0
    zx, zy = _zigzag(v[:, 0] - prev[:, 0]), _zigzag(v[:, 1] - prev[:, 1])
    pts, poly = np.isin(t, POINTS), np.isin(t, POLYGONS)
    per_feature = np.bincount(f, minlength=n).astype(np.int64) if N else np.zeros(n, np.int64)
    cmd = np.zeros(N, dtype=np.int64)  # the command in front of the item (0: none)
    cmd[pts & head] = (per_feature[f[pts & head]] << 3) | 1
    cmd[~pts & (j == 0)] = 9
    lt = ~pts & (j == 1)
    cmd[lt] = ((k[lt] - 1) << 3) | 2
    close = poly & (j == k - 1)
    vals = np.stack([cmd & U32, zx, zy, np.full(N, 15, np.int64)], axis=1)
    present = np.stack([cmd != 0, np.ones(N, bool), np.ones(N, bool), close], axis=1)
    data, ln = _varints(vals[present])
    size = np.zeros((N, 4), dtype=np.int64)
    size[present] = ln
    per = np.bincount(f, weights=size.sum(axis=1), minlength=n).astype(np.int64) if N else np.zeros(n, np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(per)
    assert int(offsets[-1]) == data.size <= 0x7FFFFFFF
    return gtype, offsets.astype(np.int32), data


def feature_value(offsets, data, i: int) -> bytes:
    return bytes(data[int(offsets[i]):int(offsets[i + 1])])


def _pb_varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def bare_layer(name: str, gtype, offsets, data, extent: int = 4096) -> bytes:
    """A Tile with one layer whose features carry only type and geometry (every feature, empty values too)."""
    body = bytearray(b"\x78\x02" + b"\x0a" + _pb_varint(len(name)) + name.encode())
    for i in range(len(gtype)):
        g = feature_value(offsets, data, i)
        f = b"\x18" + _pb_varint(int(gtype[i])) + b"\x22" + _pb_varint(len(g)) + g
        body += b"\x12" + _pb_varint(len(f)) + f
    body += b"\x28" + _pb_varint(extent)
    return b"\x1a" + _pb_varint(len(body)) + bytes(body)

"""Reference simplification of an assembled geometry column (include/covt.h "Geometry simplification"): snap to
the grid of 2^s, keep, collapse, shell rule, new ring offsets and coordinates; numpy, and nothing else.

``simplify_ref(types, geo, part, ring, coords, s)`` -> ``(ring_offsets' int32[R + 1], coords' int32[V', 2])``;
geometry_offsets and part_offsets are the input's.  ``ring_types`` gives every ring its feature's type.
"""
from __future__ import annotations

import numpy as np

I32_MAX = 2 ** 31 - 1
POINTS = (0, 3)
LINES = (1, 4)
POLYGONS = (2, 5)


def snap(v, s: int) -> np.ndarray:
    """snap(v) = min((((int64)v + h) >> s) << s, M), h = s ? 2^(s-1) : 0, M = (INT32_MAX >> s) << s."""
    v = np.asarray(v, dtype=np.int64)
    h = (1 << (s - 1)) if s else 0
    m = (I32_MAX >> s) << s
    return np.minimum(((v + h) >> s) << s, m).astype(np.int32)


def _owner(offsets, count: int) -> np.ndarray:
    """For items 0 .. count - 1 in segments given by nested offsets: the segment of every item."""
    offsets = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))[:count]


def ring_types(types, geo, part) -> np.ndarray:
    """The GeometryTypes ordinal of every ring's feature, and the first ring of every ring's part."""
    geo, part = np.asarray(geo, dtype=np.int64), np.asarray(part, dtype=np.int64)
    n_parts, n_rings = int(geo[-1]), int(part[int(geo[-1])])
    part_feature = _owner(geo, n_parts)
    ring_part = _owner(part[:n_parts + 1], n_rings)
    t = np.asarray(types, dtype=np.int64)[part_feature][ring_part]
    return t, part[ring_part]


def simplify_ref(types, geo, part, ring, coords, s: int):
    assert 0 <= s <= 30
    ring = np.asarray(ring, dtype=np.int64)
    R = ring.size - 1
    V = int(ring[R])
    q = snap(np.asarray(coords, dtype=np.int32).reshape(-1, 2)[:V], s)
    t, shell = ring_types(types, geo, part)
    assert t.size == R, "every ring belongs to a part of a feature"
    ring_of = _owner(ring, V)
    # keep
    head = np.zeros(V, dtype=bool)
    head[ring[:-1][np.diff(ring) > 0]] = True
    differs = np.ones(V, dtype=bool)
    differs[1:] = (q[1:] != q[:-1]).any(axis=1)
    keep = head | differs | np.isin(t, POINTS)[ring_of]
    k = np.bincount(ring_of[keep], minlength=R).astype(np.int64)
    # collapse
    gone = (np.isin(t, LINES) & (k < 2)) | (np.isin(t, POLYGONS) & (k < 4))
    gone |= np.isin(t, POLYGONS) & gone[shell]  # the shell rule
    k[gone] = 0
    out_ring = np.zeros(R + 1, dtype=np.int32)
    out_ring[1:] = np.cumsum(k)
    return out_ring, q[keep & ~gone[ring_of]]

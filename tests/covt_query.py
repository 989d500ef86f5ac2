"""Test helpers for the query pass (include/covt.h "Geometry queries"): two references over an assembled
column ``(types, geo, part, ring, coords)`` -- nested absolute offsets and int32 coordinates, as the assembly
writes them --, builders of hand-made columns, a generator of *valid* random features and the table of known
answers the CPU and the GPU tests share.

* ``query_ref``: the header's definition word for word, in Python ints (exact).
* ``query_clip_ref``: the same two relations another way -- Liang-Barsky clipping and ray casting in
  ``fractions.Fraction``, polygons part by part, WITHIN from the feature's extent.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

POINT, LINESTRING, POLYGON, MULTIPOINT, MULTILINESTRING, MULTIPOLYGON = range(6)
INTERSECTS, WITHIN = 0, 1
LO, HI = -(1 << 31), (1 << 31) - 1
EXTREMES = (LO, LO + 1, -1, 0, 1, HI - 1, HI)


# ---- the definition ---------------------------------------------------------------------------------------
def q_in(w, p):
    return w[0] <= p[0] <= w[2] and w[1] <= p[1] <= w[3]


def q_meets(w, a, b):
    if max(a[0], b[0]) < w[0] or min(a[0], b[0]) > w[2] or max(a[1], b[1]) < w[1] or min(a[1], b[1]) > w[3]:
        return False
    if q_in(w, a) or q_in(w, b):
        return True
    s = [(b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0]) for cx in (w[0], w[2]) for cy in (w[1], w[3])]
    return not all(v > 0 for v in s) and not all(v < 0 for v in s)


def q_cross(w, a, b):
    qx, qy = w[0], w[1]
    if (a[1] > qy) == (b[1] > qy):
        return False
    d = (qy - a[1]) * (b[0] - a[0]) - (qx - a[0]) * (b[1] - a[1])
    return (d > 0) == (b[1] > a[1])


def ring_bits(w, pts):
    """touch | out << 1 | par << 2 of one ring (a list of (x, y))."""
    m = len(pts)
    if m == 0:
        return 0
    touch = q_in(w, pts[0]) if m == 1 else any(q_meets(w, pts[i], pts[i + 1]) for i in range(m - 1))
    out = any(not q_in(w, p) for p in pts)
    par = sum(q_cross(w, pts[i], pts[i + 1]) for i in range(m - 1)) & 1
    return int(touch) | int(out) << 1 | par << 2


def _pts(coords, a, b):
    return [(int(x), int(y)) for x, y in np.asarray(coords[a:b]).reshape(-1, 2)]


def query_ref(types, geo, part, ring, coords, window):
    """(intersects, within) uint8 arrays of the definition, one entry per feature."""
    w = tuple(int(v) for v in window)
    n = len(types)
    inter, within = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if w[0] > w[2] or w[1] > w[3]:
        return inter, within
    for f in range(n):
        r0, r1 = int(part[int(geo[f])]), int(part[int(geo[f + 1])])
        if int(ring[r1]) == int(ring[r0]):
            continue  # no coordinate
        touch = out = par = 0
        for r in range(r0, r1):
            v = ring_bits(w, _pts(coords, int(ring[r]), int(ring[r + 1])))
            touch |= v & 1
            out |= (v >> 1) & 1
            par ^= (v >> 2) & 1
        inter[f] = 1 if touch or (int(types[f]) in (POLYGON, MULTIPOLYGON) and par) else 0
        within[f] = 0 if out else 1
    return inter, within


def query_ref_numpy(types, geo, part, ring, coords, window):
    """query_ref for large columns, in int64 arrays: exact, and so the same answers, while every coordinate and
    window corner lies within +-2^30 (differences below 2^31, products below 2^62; asserted)."""
    w = tuple(int(v) for v in window)
    types = np.asarray(types)
    geo, part, ring = (np.asarray(a, np.int64) for a in (geo, part, ring))
    xy = np.asarray(coords, np.int64).reshape(-1, 2)
    n, R, V = types.size, ring.size - 1, xy.shape[0]
    assert max(abs(v) for v in w) <= 1 << 30 and (V == 0 or int(np.abs(xy).max()) <= 1 << 30)
    inter, within = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if w[0] > w[2] or w[1] > w[3] or n == 0:
        return inter, within
    ring_len = np.diff(ring)
    ring_of = np.repeat(np.arange(R), ring_len)  # the ring of every coordinate
    x, y = xy[:, 0], xy[:, 1]
    inside = (w[0] <= x) & (x <= w[2]) & (w[1] <= y) & (y <= w[3])
    e = np.nonzero(ring_of[:-1] == ring_of[1:])[0] if V > 1 else np.zeros(0, np.int64)  # edges i -> i + 1
    ax, ay, bx, by = x[e], y[e], x[e + 1], y[e + 1]
    reject = (np.maximum(ax, bx) < w[0]) | (np.minimum(ax, bx) > w[2]) | (np.maximum(ay, by) < w[1]) | (np.minimum(ay, by) > w[3])
    s = [(bx - ax) * (cy - ay) - (by - ay) * (cx - ax) for cx in (w[0], w[2]) for cy in (w[1], w[3])]
    split = ~((s[0] > 0) & (s[1] > 0) & (s[2] > 0) & (s[3] > 0)) & ~((s[0] < 0) & (s[1] < 0) & (s[2] < 0) & (s[3] < 0))
    meets = ~reject & (inside[e] | inside[e + 1] | split)
    d = (w[1] - ay) * (bx - ax) - (w[0] - ax) * (by - ay)
    cross = ((ay > w[1]) != (by > w[1])) & ((d > 0) == (by > ay))
    touch_r = np.bincount(ring_of[e], weights=meets, minlength=R) > 0
    one = np.nonzero(ring_len == 1)[0]
    touch_r[one] = inside[ring[one]]
    out_r = np.bincount(ring_of, weights=~inside, minlength=R) > 0
    par_r = np.bincount(ring_of[e], weights=cross, minlength=R).astype(np.int64) & 1
    r0, r1 = part[geo[:-1]], part[geo[1:]]
    feat_of = np.repeat(np.arange(n), r1 - r0)  # the feature of every ring (rings lie in feature order)
    touch = np.bincount(feat_of, weights=touch_r[:feat_of.size], minlength=n) > 0
    out = np.bincount(feat_of, weights=out_r[:feat_of.size], minlength=n) > 0
    par = np.bincount(feat_of, weights=par_r[:feat_of.size], minlength=n).astype(np.int64) & 1
    has = ring[r1] > ring[r0]
    poly = (types == POLYGON) | (types == MULTIPOLYGON)
    inter[:] = has & (touch | (poly & (par == 1)))
    within[:] = has & ~out
    return inter, within


# ---- the same another way ---------------------------------------------------------------------------------
def _clip_nonempty(w, a, b):
    """Liang-Barsky: the closed segment ab has a point in the closed window."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    t0, t1 = Fraction(0), Fraction(1)
    for p, q in ((-dx, a[0] - w[0]), (dx, w[2] - a[0]), (-dy, a[1] - w[1]), (dy, w[3] - a[1])):
        if p == 0:
            if q < 0:
                return False
            continue
        r = Fraction(q, p)
        if p < 0:
            t0 = max(t0, r)
        else:
            t1 = min(t1, r)
    return t0 <= t1


def _ray_odd(q, pts):
    """The ray from q in +x crosses the ring an odd number of times (edges half-open in y, the crossing's x a
    Fraction)."""
    k = 0
    for a, b in zip(pts, pts[1:]):
        if (a[1] > q[1]) != (b[1] > q[1]):
            x = a[0] + Fraction((q[1] - a[1]) * (b[0] - a[0]), b[1] - a[1])
            k += x > q[0]
    return k & 1


def query_clip_ref(types, geo, part, ring, coords, window):
    """(intersects, within) by clipping: a feature intersects if an edge (or a ring's only coordinate) has a
    point in the window, or, a polygon, if Q lies in a part -- inside its shell (first ring) and inside none of
    its holes; it is within if it has a coordinate and its extent lies in the window.

    The part rule and the definition's even-odd rule over all rings differ on invalid polygons (overlapping
    parts, holes outside their shell or overlapping each other): use this only on inputs built valid --
    disjoint parts, holes inside their shells and disjoint from each other."""
    w = tuple(int(v) for v in window)
    n = len(types)
    inter, within = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if w[0] > w[2] or w[1] > w[3]:
        return inter, within
    for f in range(n):
        t = int(types[f])
        allp, hit = [], False
        for p in range(int(geo[f]), int(geo[f + 1])):
            rings = [_pts(coords, int(ring[r]), int(ring[r + 1])) for r in range(int(part[p]), int(part[p + 1]))]
            for pts in rings:
                allp += pts
                if len(pts) == 1:
                    hit = hit or q_in(w, pts[0])
                hit = hit or any(_clip_nonempty(w, a, b) for a, b in zip(pts, pts[1:]))
            if t in (POLYGON, MULTIPOLYGON) and rings and _ray_odd(w[:2], rings[0]) and \
                    not any(_ray_odd(w[:2], h) for h in rings[1:]):
                hit = True
        if not allp:
            continue
        inter[f] = 1 if hit else 0
        xs, ys = [p[0] for p in allp], [p[1] for p in allp]
        within[f] = 1 if w[0] <= min(xs) and max(xs) <= w[2] and w[1] <= min(ys) and max(ys) <= w[3] else 0
    return inter, within


# ---- hand-made columns ------------------------------------------------------------------------------------
# A feature is (type, parts): parts a list of parts, a part a list of rings, a ring a list of (x, y).  POINT: one
# part of one ring of one coordinate; MULTIPOINT: a part per point; LINESTRING: one part of one ring;
# MULTILINESTRING: a part per line; POLYGON: one part; MULTIPOLYGON: its parts.  Polygon rings are written closed.
def point(x, y):
    return (POINT, [[[(x, y)]]])


def multipoint(pts):
    return (MULTIPOINT, [[[tuple(p)]] for p in pts])


def line(pts):
    return (LINESTRING, [[list(pts)]])


def multiline(lines):
    return (MULTILINESTRING, [[list(l)] for l in lines])


def polygon(rings):
    return (POLYGON, [[list(r) for r in rings]])


def multipolygon(parts):
    return (MULTIPOLYGON, [[list(r) for r in p] for p in parts])


def box(x0, y0, w, h, cw=False):
    r = [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h), (x0, y0)]
    return r[::-1] if cw else r


def assemble(features):
    """(types, geo, part, ring, coords) of a list of features: what the assembly writes for source_column()."""
    types, geo, part, ring, coords = [], [0], [0], [0], []
    for t, parts in features:
        types.append(t)
        for p in parts:
            for r in p:
                coords += r
                ring.append(len(coords))
            part.append(len(ring) - 1)
        geo.append(len(part) - 1)
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return np.asarray(types, np.uint8), i32(geo), i32(part), i32(ring), i32(coords).reshape(-1, 2)


def source_column(features):
    """The source streams of the features' GeometryColumn (covt_asm.synth_column's dict; rings as given, so
    closed=True)."""
    go, po, ro, vb = [], [], [], []
    for t, parts in features:
        rings = [r for p in parts for r in p]
        if t == POINT:
            assert len(rings) == 1 and len(rings[0]) == 1
        elif t == MULTIPOINT:
            assert all(len(r) == 1 for r in rings)
            go.append(len(rings))
        elif t == LINESTRING:
            assert len(rings) == 1
            po.append(len(rings[0]))
        elif t == MULTILINESTRING:
            go.append(len(rings))
            po += [len(r) for r in rings]
        else:
            if t == MULTIPOLYGON:
                go.append(len(parts))
            else:
                assert len(parts) == 1
            po += [len(p) for p in parts]
            ro += [len(r) for r in rings]
        vb += [v for r in rings for pt in r for v in pt]
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return {"types": np.asarray([t for t, _ in features], np.uint8), "go": i32(go), "po": i32(po), "ro": i32(ro),
            "vo": None, "vb": i32(vb), "closed": True}


# ---- valid random features --------------------------------------------------------------------------------
def _shape(rng, x0, y0, x1, y1):
    """A simple closed ring with its vertices in the box [x0, x1] x [y0, y1] (x0 < x1, y0 < y1): the box, one of
    its four right triangles, or a quadrilateral with one vertex on each side."""
    k = int(rng.integers(0, 6))
    if k == 0:
        r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    elif k < 5:
        c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        r = c[:k - 1] + c[k:]
    else:
        r = [(int(rng.integers(x0, x1 + 1)), y0), (x1, int(rng.integers(y0, y1 + 1))),
             (int(rng.integers(x0, x1 + 1)), y1), (x0, int(rng.integers(y0, y1 + 1)))]
        if len(set(r)) < 4 or r[0][0] == r[2][0] == x0 or r[0][0] == r[2][0] == x1:
            r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    if rng.integers(0, 2):
        r = r[::-1]
    return r + r[:1]


def _valid_part(rng, x0, y0, x1, y1):
    """A shell inside [x0, x1] x [y0, y1] and, for a box shell wide enough, holes strictly inside it, apart."""
    ax, bx = sorted(int(v) for v in rng.choice(np.arange(x0, x1 + 1), 2, replace=False))
    ay, by = sorted(int(v) for v in rng.choice(np.arange(y0, y1 + 1), 2, replace=False))
    rings = [_shape(rng, ax, ay, bx, by)]
    if bx - ax >= 4 and by - ay >= 4 and rng.integers(0, 2):
        rings = [box(ax, ay, bx - ax, by - ay, cw=bool(rng.integers(0, 2)))]
        # holes in disjoint vertical strips of the shell's open interior, a column of slack between them
        xs = ax + 1
        while xs + 1 <= bx - 1 and len(rings) < 4:
            hx1 = int(rng.integers(xs + 1, bx))
            hy0 = int(rng.integers(ay + 1, by - 1))
            hy1 = int(rng.integers(hy0 + 1, by))
            if rng.integers(0, 3):
                rings.append(_shape(rng, xs, hy0, hx1, hy1))
            xs = hx1 + 2
    return rings


def valid_feature(rng, lim=12):
    """A feature of a random type whose polygons are valid: disjoint parts (in separate vertical bands), holes
    inside their shells and apart from each other."""
    t = int(rng.integers(0, 6))
    pt = lambda: (int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1)))  # noqa: E731
    if t == POINT:
        return point(*pt())
    if t == MULTIPOINT:
        return multipoint([pt() for _ in range(int(rng.integers(0, 4)))])
    if t == LINESTRING:
        return line([pt() for _ in range(int(rng.integers(0, 6)))])
    if t == MULTILINESTRING:
        return multiline([[pt() for _ in range(int(rng.integers(0, 5)))] for _ in range(int(rng.integers(0, 4)))])
    if t == POLYGON:
        return polygon(_valid_part(rng, -lim, -lim, lim, lim))
    bands = [(-lim, -lim // 3 - 1), (-lim // 3 + 1, lim // 3 - 1), (lim // 3 + 1, lim)]
    keep = [b for b in bands if rng.integers(0, 3)]
    return multipolygon([_valid_part(rng, b[0], -lim, b[1], lim) for b in keep])


def random_window(rng, lim=12):
    """A window with small corners: a point, a sliver or a box, now and then inverted."""
    x0, y0 = int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1))
    k = int(rng.integers(0, 8))
    if k == 0:
        return (x0, y0, x0, y0)
    if k == 1:
        return (x0, y0, x0 - 1 - int(rng.integers(0, 3)), y0 + 2)
    return (x0, y0, x0 + int(rng.integers(0, lim)), y0 + int(rng.integers(0, lim)))


# ---- known answers ----------------------------------------------------------------------------------------
W10 = (0, 0, 10, 10)
_BIG = box(-5, -5, 20, 20)
_SHELL = box(-10, -10, 30, 30)
# (name, window, feature, INTERSECTS, WITHIN)
KNOWN = [
    ("diagonal passing a corner at distance one", W10, line([(-6, 5), (5, -6)]), 0, 0),
    ("diagonal touching a corner exactly", W10, line([(-5, 5), (5, -5)]), 1, 0),
    ("diagonal touching the far corner exactly", W10, line([(5, 15), (15, 5)]), 1, 0),
    ("diagonal passing the far corner at distance one", W10, line([(5, 16), (16, 5)]), 0, 0),
    ("collinear along an edge, overhanging", W10, line([(-3, 0), (4, 0)]), 1, 0),
    ("collinear along an edge, inside it", W10, line([(2, 0), (7, 0)]), 1, 1),
    ("collinear with an edge, beside the window", W10, line([(-5, 0), (-1, 0)]), 0, 0),
    ("collinear with an edge, ending at the corner", W10, line([(-5, 0), (0, 0)]), 1, 0),
    ("through the window, both ends outside", W10, line([(-2, 5), (12, 6)]), 1, 0),
    ("a line inside the window", W10, line([(1, 1), (9, 2), (3, 8)]), 1, 1),
    ("a polygon containing the window", W10, polygon([_BIG]), 1, 0),
    ("the same, clockwise", W10, polygon([_BIG[::-1]]), 1, 0),
    ("a closed line around the window is no polygon", W10, line(_BIG), 0, 0),
    ("a polygon whose hole contains the window", W10, polygon([_SHELL, box(-2, -2, 14, 14, cw=True)]), 0, 0),
    ("a polygon whose hole boundary touches the window", W10, polygon([_SHELL, box(10, 2, 5, 5, cw=True)]), 1, 0),
    ("a polygon whose hole boundary runs along an edge", W10, polygon([_SHELL, box(-2, -2, 14, 12, cw=True)]), 1, 0),
    ("a polygon whose hole lies in the window", W10, polygon([_SHELL, box(4, 4, 2, 2)]), 1, 0),
    ("a polygon inside the window", W10, polygon([box(1, 1, 3, 3)]), 1, 1),
    ("a polygon filling the window", W10, polygon([box(0, 0, 10, 10)]), 1, 1),
    ("a polygon beside the window", W10, polygon([box(12, 0, 3, 3)]), 0, 0),
    ("a multipolygon with the window in its second part", W10, multipolygon([[box(100, 100, 5, 5)], [_BIG]]), 1, 0),
    ("a multipolygon with the window in its second part's hole", W10,
     multipolygon([[box(100, 100, 5, 5)], [_SHELL, box(-2, -2, 14, 14)]]), 0, 0),
    ("the window between two parts", W10, multipolygon([[box(-20, 0, 10, 10)], [box(20, 0, 10, 10)]]), 0, 0),
    ("a multipolygon inside the window", W10, multipolygon([[box(1, 1, 2, 2)], [box(5, 5, 5, 5), box(6, 6, 1, 1)]]), 1, 1),
    ("a multiline with one line through the window", W10, multiline([[(20, 20), (30, 30)], [(-2, 5), (12, 6)]]), 1, 0),
    ("a multipoint with one point inside", W10, multipoint([(-1, -1), (5, 5), (11, 11)]), 1, 0),
    ("a multipoint inside", W10, multipoint([(0, 0), (5, 5), (10, 10)]), 1, 1),
    ("a zero-length line inside", W10, line([(3, 3), (3, 3)]), 1, 1),
    ("a zero-length line outside", W10, line([(30, 3), (30, 3)]), 0, 0),
    ("a line of one coordinate inside", W10, line([(3, 3)]), 1, 1),
    ("a line of one coordinate outside", W10, line([(3, 11)]), 0, 0),
    ("an empty line", W10, line([]), 0, 0),
    ("an empty multipoint", W10, multipoint([]), 0, 0),
    ("an empty multipolygon", W10, multipolygon([]), 0, 0),
    ("a polygon of no ring", W10, polygon([]), 0, 0),
    ("a multiline of empty lines", W10, multiline([[], []]), 0, 0),
    ("an inverted window, a polygon around it", (10, 10, 0, 0), polygon([_BIG]), 0, 0),
    ("an inverted window, a point in its span", (10, 10, 0, 0), point(5, 5), 0, 0),
    ("a window inverted in y only, a line through its span", (0, 10, 10, 0), line([(-2, 5), (12, 5)]), 0, 0),
    ("a point query on a vertex", (4, 4, 4, 4), line([(0, 0), (4, 4), (9, 0)]), 1, 0),
    ("a point query on an edge's interior", (2, 2, 2, 2), line([(0, 0), (4, 4)]), 1, 0),
    ("a point query beside an edge", (2, 3, 2, 3), line([(0, 0), (4, 4)]), 0, 0),
    ("a point query in a polygon", (2, 3, 2, 3), polygon([box(0, 0, 5, 5)]), 1, 0),
    ("a point query in a hole", (2, 3, 2, 3), polygon([box(0, 0, 5, 5), box(1, 1, 3, 3)]), 0, 0),
    ("a point query on a point", (7, -7, 7, -7), point(7, -7), 1, 1),
    ("a point with radius reaching an edge", (4, 0, 8, 4), line([(0, 0), (6, 6)]), 1, 0),
    ("a point with radius one short of an edge", (5, 0, 9, 4), line([(0, 0), (6, 6)]), 0, 0),
] + [("a point on the window's boundary (%d, %d)" % p, W10, point(*p), 1, 1)
     for p in ((0, 0), (10, 0), (0, 10), (10, 10), (5, 0), (0, 5), (10, 5), (5, 10))] \
  + [("a point one off the window's boundary (%d, %d)" % p, W10, point(*p), 0, 0)
     for p in ((-1, 0), (11, 10), (5, -1), (5, 11), (-1, -1), (11, 11))]
# (every polygon above is valid, so query_clip_ref applies to all of them)

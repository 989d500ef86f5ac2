"""CPU: the reference MVT encoding of tests/covt_mvt.py (the definition the GPU pass of covt_mvt.hip is held to,
include/covt.h "Geometry as MVT"), and the layout rule of covt_mvt_plan.h.

1. known answers: the worked examples of the MVT 2.1 specification (section 4.3.5), the winding rule, the
   two's-complement wrap-around;
2. the emptiness rules, the cursor across empty rings, the shift;
3. the pin: over the 780 layers of tests/golden/mvt_digests.json the oracle's assembly, encoded by the reference,
   wrapped in a bare layer and read back by tests/covt_geom.mvt_layers, reproduces the digest of the MVT original,
   with orientation off and on;
4. the layout rule, the option rule and the capacity formula in a stand-alone program under AddressSanitizer +
   UBSan.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import covt_asm as A
import covt_geom as G
import covt_mvt as MV
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX, MIN = 2 ** 31 - 1, -2 ** 31


def _column(features):
    """features: [(type, parts)], parts: [rings], ring: [(x, y)] -> (types, geo, part, ring, xy)."""
    types, geo, part, ring, xy = [], [0], [0], [0], []
    for t, parts in features:
        types.append(t)
        for rings in parts:
            for r in rings:
                xy += [v for pt in r for v in pt]
                ring.append(ring[-1] + len(r))
            part.append(part[-1] + len(rings))
        geo.append(geo[-1] + len(parts))
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return np.asarray(types, np.uint8), i32(geo), i32(part), i32(ring), i32(xy).reshape(-1, 2)


def _values(features, orient=False, shift=0):
    gt, offs, data = MV.mvt_ref(*_column(features), orient, shift)
    assert gt.dtype == np.uint8 and offs.dtype == np.int32 and data.dtype == np.uint8 and offs[0] == 0
    return gt.tolist(), [list(MV.feature_value(offs, data, i)) for i in range(len(features))]


SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]
SHELL = [(11, 11), (20, 11), (20, 20), (11, 20), (11, 11)]
HOLE = [(13, 13), (13, 17), (17, 17), (17, 13), (13, 13)]
LINE = [(2, 2), (2, 10), (10, 10)]
SPEC_MULTIPOLYGON = [9, 0, 0, 26, 20, 0, 0, 20, 19, 0, 15, 9, 22, 2, 26, 18, 0, 0, 18, 17, 0, 15, 9, 4, 13, 26, 0, 8, 8, 0, 0,
                     7, 15]
# (name, type, parts, GeomType, the value as the spec prints it)
KATS = [
    ("POINT", 0, [[[(25, 17)]]], 1, [9, 50, 34]),
    ("MULTIPOINT", 3, [[[(5, 7)]], [[(3, 2)]]], 1, [17, 10, 14, 3, 9]),
    ("MULTIPOINT in one ring", 3, [[[(5, 7), (3, 2)]]], 1, [17, 10, 14, 3, 9]),
    ("LINESTRING", 1, [[LINE]], 2, [9, 4, 4, 18, 0, 16, 16, 0]),
    ("MULTILINESTRING", 4, [[LINE], [[(1, 1), (3, 5)]]], 2, [9, 4, 4, 18, 0, 16, 16, 0, 9, 17, 17, 10, 4, 8]),
    ("POLYGON", 2, [[[(3, 6), (8, 12), (20, 34), (3, 6)]]], 3, [9, 6, 12, 18, 10, 12, 24, 44, 15]),
    ("MULTIPOLYGON", 5, [[SQUARE], [SHELL, HOLE]], 3, SPEC_MULTIPOLYGON),
]


@pytest.mark.parametrize("name,t,parts,gtype,want", KATS, ids=[k[0] for k in KATS])
@pytest.mark.parametrize("orient", [False, True])
def test_spec_examples(name, t, parts, gtype, want, orient):
    """The spec's examples are wound as the spec asks, so orientation changes nothing."""
    gt, vals = _values([(t, parts)], orient)
    assert gt == [gtype] and vals == [want]


def test_orientation():
    cw = [(0, 0), (0, 10), (10, 10), (10, 0), (0, 0)]  # S < 0
    stored, oriented = [9, 0, 0, 26, 0, 20, 20, 0, 0, 19, 15], [9, 0, 0, 26, 20, 0, 0, 20, 19, 0, 15]
    assert _values([(2, [[cw]])])[1] == [stored]
    assert _values([(2, [[cw]])], orient=True)[1] == [oriented]
    # a hole wound as a shell is reversed, a hole wound as a hole is not; the second part's first ring is a shell
    # again; a degenerate ring (S = 0) and an unclosed one stay as stored
    p = MV.ring_plan(*_column([(5, [[SQUARE, SHELL, HOLE], [cw, HOLE[::-1]]]),
                               (2, [[[(0, 0), (5, 5), (9, 9), (0, 0)], cw[:-1]]])]), True, 0)
    assert p["S"].tolist()[:5] == [200, 162, -32, -200, 32] and p["S"][5] == 0
    assert p["rev"].tolist() == [False, True, False, True, True, False, False]
    assert p["closed"].tolist() == [True] * 6 + [False] and p["k"].tolist() == [4, 4, 4, 4, 4, 3, 4]
    # the reversed ring still starts at its stored first vertex, and the cursor goes on from its last emitted one
    # (the hole has S = +1: reversed to (1,1), (2,2), (2,1); from the cursor (0,10): +1 -9, then +1 +1, then 0 -1)
    both = _values([(2, [[cw, [(1, 1), (2, 1), (2, 2), (1, 1)]]])], orient=True)[1][0]
    assert both == oriented + [9, 2, 17, 18, 2, 2, 0, 1, 15]
    # shift before the shoelace: the ring is judged on the shifted coordinates
    big = [(x << 4, y << 4) for x, y in cw]
    assert _values([(2, [[big]])], orient=True, shift=4)[1] == [oriented]


def test_wrap_around():
    want = [0x09, 0xFF, 0xFF, 0xFF, 0xFF, 0x0F, 0xFE, 0xFF, 0xFF, 0xFF, 0x0F, 0x0A, 0x01, 0x02]
    gt, vals = _values([(1, [[[(MIN, MAX), (MAX, MIN)]]])])
    assert gt == [2] and vals == [want]
    # a reader that sums mod 2^32 recovers the coordinates
    feats = G.mvt_layers(MV.bare_layer("w", *MV.mvt_ref(*_column([(1, [[[(MIN, MAX), (MAX, MIN)]]])]))))["w"]["features"]
    (x0, y0), (x1, y1) = feats[0][2][0]
    wrap = lambda v: ((v + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31  # noqa: E731
    assert (wrap(x0), wrap(y0), wrap(x1), wrap(y1)) == (MIN, MAX, MAX, MIN)


def test_emptiness_and_the_cursor():
    # an empty ring between two non-empty ones: the cursor carries across
    assert _values([(4, [[[(1, 1), (2, 2)]], [[]], [[(3, 3), (4, 4)]]])])[1] == [[9, 2, 2, 10, 2, 2, 9, 2, 2, 10, 2, 2]]
    # a polygon ring of 1 point, of 2 equal points (closed: k = 1), unclosed
    assert _values([(2, [[[(3, 4)]]])])[1] == [[9, 6, 8, 15]]
    assert _values([(2, [[[(3, 4), (3, 4)]]])])[1] == [[9, 6, 8, 15]]
    assert _values([(2, [[[(0, 0), (4, 0), (4, 4)]]])])[1] == [[9, 0, 0, 18, 8, 0, 0, 8, 15]]
    # features without a coordinate: empty values, their GeomType all the same; the cursor restarts per feature
    gt, vals = _values([(3, []), (1, [[[]]]), (2, [[[], []]]), (0, [[[(1, 1)]]]), (5, []), (0, [[[(1, 1)]]])])
    assert gt == [1, 2, 3, 1, 3, 1] and vals == [[], [], [], [9, 2, 2], [], [9, 2, 2]]
    # a line of one point: MoveTo alone
    assert _values([(1, [[[(5, 5)]]])])[1] == [[9, 10, 10]]
    # a LineTo count of two bytes: 17 coordinates, (16 << 3) | 2 = 130
    v = _values([(1, [[[(i, 0) for i in range(17)]]])])[1][0]
    assert v[:5] == [9, 0, 0, 0x82, 0x01] and len(v) == 5 + 32


def test_shift():
    pts = [(-1, 17), (16, -17), (31, 32)]
    assert _values([(1, [[pts]])], shift=4)[1] == _values([(1, [[[(-1, 1), (1, -2), (1, 2)]]])])[1]  # floor, not round
    assert _values([(1, [[[(MIN, MAX), (MAX, MIN)]]])], shift=30)[1] == [[9, 3, 2, 10, 6, 5]]  # (-2, 1) -> (1, -2)
    # closedness is judged after the shift
    assert _values([(2, [[[(0, 0), (64, 0), (64, 64), (3, 5)]]])], shift=4)[1] == [[9, 0, 0, 18, 8, 0, 0, 8, 15]]
    with pytest.raises(AssertionError):
        MV.mvt_ref(*_column([(0, [[[(1, 1)]]])]), False, 31)


def test_pin_against_the_mvt_originals(oracle):
    """Every pinned layer: the reference's value of every feature, read back by the independent MVT reader, is the
    geometry of the MVT original.  The fixtures hold no ring wound against its role and no empty feature, so
    orientation on gives the same bytes; if that stops being true this fails rather than skips."""
    dig = json.load(open(os.path.join(GOLDEN, "mvt_digests.json")))
    pinned = rings = 0
    for name, layers in dig.items():
        tile = open(os.path.join(GOLDEN, "tiles", "omt", name + ".covt"), "rb").read()
        cols = A.oracle_tile_columns(oracle, tile)
        for L, rec in layers.items():
            if not rec["oracle_geom_match"]:
                continue
            c = cols[int(L)]
            col = (c["types"],) + tuple(c["asm"][1:])
            gt, offs, data = MV.mvt_ref(*col, False, 0)
            got = G.mvt_layers(MV.bare_layer(rec["name"], gt, offs, data))[rec["name"]]["features"]
            assert G.layer_digest([(cls, parts) for _, cls, parts in got]) == rec["geom"], (name, L, rec["name"])
            p = MV.ring_plan(*col, True, 0)
            poly = np.isin(p["t"], (2, 5))
            assert not p["rev"].any() and (p["S"][poly] != 0).all(), (name, L)
            assert (np.diff(offs) > 0).all(), (name, L)
            gt1, offs1, data1 = MV.mvt_ref(*col, True, 0)
            assert gt1.tobytes() == gt.tobytes() and offs1.tobytes() == offs.tobytes() and data1.tobytes() == data.tobytes()
            pinned += 1
            rings += int(poly.sum())
    assert pinned == 780 and rings == 111825


def test_layout_rule_under_sanitizers(tmp_path):
    """The host-side layout code (covt_mvt_plan.h) in a stand-alone program built with AddressSanitizer and
    UndefinedBehaviorSanitizer, on the CPU."""
    exe = str(tmp_path / "mvt_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "mvt_layout", "mvt_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])

"""CPU: the reference simplification of tests/covt_simplify.py (the definition the GPU pass of covt_simplify.hip
is held to, include/covt.h "Geometry simplification"), and the layout rule of covt_simplify_plan.h.

1. known answers worked by hand: merged vertices, the collapse minima, the shell rule, points, s = 0, the int32
   extremes;
2. properties on synthetic columns and on the oracle's assembly of every fixture tile: idempotence, closed rings
   stay closed, polygon rings of 0 or >= 4 and lines of 0 or >= 2 coordinates;
3. the fixtures are not vacuous at FIXTURE_SHIFT, the shift tests/test_gpu_simplify.py uses on them;
4. the layout rule and the argument rule in a stand-alone program under AddressSanitizer + UBSan.
"""
import os
import subprocess

import numpy as np
import pytest

import covt_asm as A
import covt_simplify as S
from conftest import ROOT, tile_paths

FIXTURE_SHIFT = 4
MAX, MIN = 2 ** 31 - 1, -2 ** 31


def _col(geo, part, ring, coords):
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return i32(geo), i32(part), i32(ring), i32(coords).reshape(-1, 2)


SHELL64 = [0, 0, 64, 0, 64, 64, 0, 64, 0, 0]
# (name, types, (geo, part, ring, coords), shift, ring_offsets', coords')
KATS = [
    # snap(20) = 16, snap(5) = 0 at s = 4: the left pair and the right pair merge, 5 coordinates become 3
    ("square whose left vertices merge", [2], _col([0, 1], [0, 1], [0, 5], [0, 0, 20, 0, 20, 5, 0, 5, 0, 0]), 4,
     [0, 0], []),
    ("shell collapses, its hole would not", [2],
     _col([0, 1], [0, 2], [0, 5, 10], [0, 0, 20, 0, 20, 5, 0, 5, 0, 0] + SHELL64), 4, [0, 0, 0], []),
    ("hole collapses inside a standing shell", [2],
     _col([0, 1], [0, 2], [0, 5, 10], SHELL64 + [30, 30, 31, 30, 31, 31, 30, 31, 30, 30]), 4, [0, 5, 5], SHELL64),
    ("second part's shell collapses, first part stands", [5],
     _col([0, 2], [0, 1, 3], [0, 5, 10, 15], SHELL64 + [1, 1, 2, 1, 2, 2, 1, 2, 1, 1] + SHELL64), 4, [0, 5, 5, 5], SHELL64),
    ("an empty shell takes its holes at s = 0", [2], _col([0, 1], [0, 2], [0, 0, 5], SHELL64), 0, [0, 0, 0], []),
    ("line A A' B", [1], _col([0, 1], [0, 1], [0, 3], [0, 0, 1, 1, 40, 40]), 3, [0, 2], [0, 0, 40, 40]),
    ("line that snaps to one point", [1], _col([0, 1], [0, 1], [0, 3], [0, 0, 1, 1, 2, 2]), 3, [0, 0], []),
    ("multilinestring: one line goes, one stays", [4],
     _col([0, 2], [0, 1, 2], [0, 2, 4], [0, 0, 1, 1, 0, 0, 9, 0]), 3, [0, 0, 2], [0, 0, 8, 0]),
    ("MULTIPOINT with equal neighbours", [3], _col([0, 3], [0, 1, 2, 3], [0, 1, 2, 3], [1, 1, 1, 1, 2, 2]), 3,
     [0, 1, 2, 3], [0, 0, 0, 0, 0, 0]),
    ("points sharing a ring", [3], _col([0, 1], [0, 1], [0, 3], [1, 1, 1, 1, 12, 2]), 3, [0, 3], [0, 0, 0, 0, 16, 0]),
    ("POINT", [0], _col([0, 1], [0, 1], [0, 1], [7, -9]), 2, [0, 1], [8, -8]),
    ("s = 0 with exact repeats", [1], _col([0, 1], [0, 1], [0, 5], [5, 5, 5, 5, 7, 7, 7, 7, 5, 5]), 0, [0, 3],
     [5, 5, 7, 7, 5, 5]),
    ("s = 0, triangle ring stands, 3-point ring goes", [2],
     _col([0, 1], [0, 2], [0, 4, 7], [0, 0, 9, 0, 0, 9, 0, 0, 1, 1, 2, 1, 1, 1]), 0, [0, 4, 4], [0, 0, 9, 0, 0, 9, 0, 0]),
    ("equal neighbours across a ring boundary stay", [4], _col([0, 2], [0, 1, 2], [0, 2, 4], [0, 0, 8, 8, 8, 8, 0, 0]), 0,
     [0, 2, 4], [0, 0, 8, 8, 8, 8, 0, 0]),
    ("empty features", [3, 1, 2, 5], _col([0, 0, 1, 2, 3], [0, 1, 3, 3], [0, 0, 0, 0], []), 4, [0, 0, 0, 0], []),
]


@pytest.mark.parametrize("name,types,col,s,ring,coords", KATS, ids=[k[0] for k in KATS])
def test_known_answers(name, types, col, s, ring, coords):
    got_ring, got_xy = S.simplify_ref(np.asarray(types, np.uint8), *col, s)
    assert got_ring.dtype == np.int32 and got_xy.dtype == np.int32 and got_xy.shape[1:] == (2,)
    assert got_ring.tolist() == ring and got_xy.reshape(-1).tolist() == coords


@pytest.mark.parametrize("s", [1, 4, 30])
def test_snap_at_the_int32_extremes(s):
    """INT32_MAX and INT32_MAX - 2^(s-1) round to (or past) the largest grid value that fits, M; INT32_MIN is on
    every grid; -1 + 2^(s-1) is below 2^s, so -1 rounds up to 0."""
    m = (MAX >> s) << s
    assert S.snap([MAX, MAX - (1 << (s - 1)), MIN, -1], s).tolist() == [m, m, MIN, 0]
    assert {1: 2 ** 31 - 2, 4: 2 ** 31 - 16, 30: 2 ** 30}[s] == m
    # just below the half: down; at the half: up
    h = 1 << (s - 1)
    assert S.snap([h - 1, h, -h, -h - 1], s).tolist() == [0, 1 << s, 0, -(1 << s)]
    assert S.snap([5, -7, MAX, MIN], 0).tolist() == [5, -7, MAX, MIN]
    # a line between the extremes keeps its two ends
    ring, xy = S.simplify_ref(np.array([1], np.uint8), *_col([0, 1], [0, 1], [0, 4], [MAX, MIN, MAX - h, MIN, -1, -1, 0, 0]), s)
    assert ring.tolist() == [0, 2] and xy.tolist() == [[m, MIN], [0, 0]]


def _properties(types, geo, part, ring, xy, s):
    """The properties of the definition on one column -> (coordinates removed, rings collapsed, polygon rings
    standing)."""
    out_ring, out_xy = S.simplify_ref(types, geo, part, ring, xy, s)
    t, _ = S.ring_types(types, geo, part)
    k_in, k = np.diff(np.asarray(ring, np.int64)), np.diff(out_ring.astype(np.int64))
    assert out_ring[0] == 0 and out_ring[-1] == out_xy.shape[0] and (k >= 0).all() and (k <= k_in).all()
    poly, line, pts = np.isin(t, S.POLYGONS), np.isin(t, S.LINES), np.isin(t, S.POINTS)
    assert ((k[poly] == 0) | (k[poly] >= 4)).all() and ((k[line] == 0) | (k[line] >= 2)).all()
    assert (k[pts] == k_in[pts]).all()
    # closed rings stay closed: a standing ring whose input was closed
    xy = np.asarray(xy).reshape(-1, 2)
    for r in np.flatnonzero(poly & (k > 0)):
        a, b = int(ring[r]), int(ring[r + 1])
        if (xy[a] == xy[b - 1]).all():
            assert (out_xy[out_ring[r]] == out_xy[out_ring[r + 1] - 1]).all(), r
    # no two equal neighbours inside a ring of lines or polygons
    same = np.flatnonzero((out_xy[1:] == out_xy[:-1]).all(axis=1)) + 1
    heads = set(out_ring[:-1][k > 0].tolist())
    owner = np.repeat(np.arange(k.size), k)
    assert all(i in heads or pts[owner[i]] for i in same.tolist())
    # idempotence
    again_ring, again_xy = S.simplify_ref(types, geo, part, out_ring, out_xy, s)
    assert again_ring.tobytes() == out_ring.tobytes() and again_xy.tobytes() == out_xy.tobytes()
    return int(k_in.sum() - k.sum()), int(((k == 0) & (k_in > 0)).sum()), int((poly & (k > 0)).sum())


def test_properties_on_synthetic_columns(oracle):
    rng = np.random.default_rng(43)
    cols = [A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2)) for i, n in enumerate([0, 1, 5, 64, 200, 700])]
    cols.append(A.synth_column(rng, 3, False, False, big=True))
    removed = 0
    for ci, col in enumerate(cols):
        st, geo, part, ring, xy = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"],
                                                           col["vb"], col["closed"], A.caps(col))
        assert st == 0, ci
        for s in (0, 3, 9, 30):
            removed += _properties(col["types"], geo, part, ring, xy, s)[0]
    assert removed > 1000


def test_fixture_tiles_properties_and_not_vacuous(oracle):
    """Over the oracle's assembly of every fixture tile at FIXTURE_SHIFT = 4 (a grid of 16 tile pixels, a z14 tile
    drawn at z10): the properties hold, and the reference removes coordinates, collapses rings and leaves polygon
    rings standing, so the GPU test that compares against it on the same tiles is not vacuous."""
    removed = collapsed = standing = n_cols = 0
    for path in tile_paths():
        tile = open(path, "rb").read()
        for L, oc in A.oracle_tile_columns(oracle, tile).items():
            if oc["asm"] is None or oc["asm"][0]:
                continue
            a, b, c = _properties(oc["types"], *oc["asm"][1:], FIXTURE_SHIFT)
            removed, collapsed, standing, n_cols = removed + a, collapsed + b, standing + c, n_cols + 1
    assert n_cols >= 700
    assert removed >= 1 and collapsed >= 1 and standing >= 1, (removed, collapsed, standing)


def test_layout_rule_under_sanitizers(tmp_path):
    """The host-side layout code (covt_simplify_plan.h) in a stand-alone program built with AddressSanitizer and
    UndefinedBehaviorSanitizer, on the CPU."""
    exe = str(tmp_path / "simplify_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "simplify_layout", "simplify_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])

"""CPU: the reference measures of tests/covt_measures.py (the definition the GPU pass of covt_measures.hip is
held to, include/covt.h "Geometry measures"), and the layout rule of covt_measures_plan.h.

1. known answers: squares of both windings, a shell with a hole, a two-part multipolygon, a 3-4-5 segment,
   degenerate rings and parts, a ring whose doubled area wraps mod 2^64;
2. the three references (nested loops, vectorised, from the WKB values) agree on the oracle's assembly of
   every fixture tile and on synthetic columns: area and num_coords equal, length within the header's bound;
3. the layout rule in a stand-alone program under AddressSanitizer + UBSan.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_measures as M
import covt_wkb as W
from conftest import tile_key, tile_paths

H = (1 << 31) - 1


def _col(geo, part, ring, coords):
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return i32(geo), i32(part), i32(ring), i32(coords).reshape(-1, 2)


SQ_CCW = [0, 0, 1, 0, 1, 1, 0, 1, 0, 0]
SQ_CW = [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
SHELL10 = [0, 0, 10, 0, 10, 10, 0, 10, 0, 0]
HOLE2 = [4, 4, 4, 6, 6, 6, 6, 4, 4, 4]
TRI = [0, 0, 4, 0, 0, 3, 0, 0]
SQ4 = [10, 10, 14, 10, 14, 14, 10, 14, 10, 10]
HOLE1 = [11, 11, 11, 12, 12, 12, 12, 11, 11, 11]
BIG = [-H, -H, H, -H, H, H, -H, H, -H, -H]
# (name, types, (geo, part, ring, coords), rows of (area, length, num_coords))
KATS = [
    ("unit square CCW", [2], _col([0, 1], [0, 1], [0, 5], SQ_CCW), [(1.0, 4.0, 5)]),
    ("unit square CW", [2], _col([0, 1], [0, 1], [0, 5], SQ_CW), [(1.0, 4.0, 5)]),
    ("shell with a hole", [2], _col([0, 1], [0, 2], [0, 5, 10], SHELL10 + HOLE2), [(96.0, 48.0, 10)]),
    ("shell with a hole of the shell's winding", [2],
     _col([0, 1], [0, 2], [0, 5, 10], SHELL10 + [4, 4, 6, 4, 6, 6, 4, 6, 4, 4]), [(96.0, 48.0, 10)]),
    ("hole larger than its shell", [2], _col([0, 1], [0, 2], [0, 5, 10], HOLE2 + SHELL10), [(-96.0, 48.0, 10)]),
    ("two-part multipolygon", [5], _col([0, 2], [0, 1, 3], [0, 4, 9, 14], TRI + SQ4 + HOLE1), [(21.0, 32.0, 14)]),
    ("3-4-5 segment", [1], _col([0, 1], [0, 1], [0, 2], [0, 0, 3, 4]), [(0.0, 5.0, 2)]),
    ("closed path of a LINESTRING", [1], _col([0, 1], [0, 1], [0, 5], SHELL10), [(0.0, 40.0, 5)]),
    ("MULTILINESTRING", [4], _col([0, 2], [0, 1, 2], [0, 2, 5], [0, 0, 3, 4] + [0, 0, 0, 5, 12, 5]), [(0.0, 22.0, 5)]),
    ("POINT", [0], _col([0, 1], [0, 1], [0, 1], [7, -9]), [(0.0, 0.0, 1)]),
    ("MULTIPOINT", [3], _col([0, 3], [0, 1, 2, 3], [0, 1, 2, 3], [1, 2, -5, 6, 3, -7]), [(0.0, 0.0, 3)]),
    ("1-vertex ring, empty ring, empty part", [5], _col([0, 3], [0, 2, 2, 3], [0, 1, 1, 6], [9, 9] + SQ_CW),
     [(1.0, 4.0, 6)]),
    ("empty features", [3, 1, 2, 5], _col([0, 0, 1, 2, 3], [0, 1, 3, 3], [0, 0, 0, 0], []),
     [(0.0, 0.0, 0)] * 4),
    # S = 8 H^2 = 2^65 - 2^35 + 8, which is -(2^35 - 8) mod 2^64: the area as defined is (2^35 - 8) / 2
    ("corners at +-(2^31 - 1)", [2], _col([0, 1], [0, 1], [0, 5], BIG), [(17179869180.0, 8.0 * H, 5)]),
    ("polygon between others", [1, 2, 0], _col([0, 1, 2, 3], [0, 1, 2, 3], [0, 2, 7, 8], [0, 0, 3, 4] + SQ_CCW + [5, 5]),
     [(0.0, 5.0, 2), (1.0, 4.0, 5), (0.0, 0.0, 1)]),
]


@pytest.mark.parametrize("name,types,col,rows", KATS, ids=[k[0] for k in KATS])
def test_known_answers(name, types, col, rows):
    types = np.asarray(types, np.uint8)
    want = (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32))
    offs, data = W.write_plain(types, *col)
    for fn, got in (("plain", M.measures_plain(types, *col)), ("numpy", M.measures_numpy(types, *col)),
                    ("wkb", M.wkb_measures(offs, data))):
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (fn, got)  # (+0.0, never -0.0)


def test_wraparound_value_is_the_mod_2_64_arithmetic():
    s, seg = M.ring_terms(list(zip(BIG[0::2], BIG[1::2])))
    assert s == (8 * H * H) % (1 << 64) == (1 << 64) - ((1 << 35) - 8)
    assert seg == [2.0 * H] * 4


def _agree(types, geo, part, ring, xy, wkb=True, parse=True):
    """The references agree on one column.  wkb: also those over its WKB values; parse: also the slow reader
    that goes through covt_wkb.parse (else only wkb_nested's, which the other columns pin to it)."""
    plain = M.measures_plain(types, geo, part, ring, xy)
    m = M.segments(geo, part, ring)
    assert M.same(M.measures_numpy(types, geo, part, ring, xy), plain, m)
    exact = M.measures_numpy(types, geo, part, ring, xy, fsum=True)
    assert M.same(exact, plain, m) and exact[1].tobytes() == plain[1].tobytes()
    if wkb:
        offs, data = W.write_numpy(types, geo, part, ring, xy)
        fast = M.wkb_measures(offs, data, with_segments=True, parse=False)
        assert M.same(fast, plain, m) and fast[1].tobytes() == plain[1].tobytes() and np.array_equal(fast[3], m)
        if parse:
            got = M.wkb_measures(offs, data, with_segments=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, fast))  # (the same terms through fsum)
    return plain, m


def test_references_agree_on_synthetic_columns(oracle):
    rng = np.random.default_rng(41)
    cols = [A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2)) for i, n in enumerate([0, 1, 5, 64, 200, 700])]
    cols.append(A.synth_column(rng, 3, False, False, big=True))
    for t in range(6):  # one-type columns: runs of empty parts / rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 150, bool(t & 1), False, probs=probs))
    n_area = n_len = 0
    for ci, col in enumerate(cols):
        st, geo, part, ring, xy = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"],
                                                           col["vb"], col["closed"], A.caps(col))
        assert st == 0, ci
        plain, m = _agree(col["types"], geo, part, ring, xy, wkb=xy.shape[0] < 50000)
        poly, line = np.isin(col["types"], M.POLYGONAL), np.isin(col["types"], M.LINEAR)
        assert (plain[0][~poly].view(np.uint64) == 0).all() and (plain[1][~line].view(np.uint64) == 0).all()
        assert int(plain[2].sum()) == xy.shape[0] and (plain[1] >= 0).all()
        n_area += int((plain[0] != 0).sum())
        n_len += int((plain[1] > 0).sum())
    assert n_area > 100 and n_len > 300


def test_references_agree_on_fixture_tiles(oracle):
    n_cols = n_rows = 0
    for ti, path in enumerate(tile_paths()):
        tile = open(path, "rb").read()
        for L, oc in A.oracle_tile_columns(oracle, tile).items():
            if oc["asm"] is None or oc["asm"][0]:
                continue
            # (every tile through the fast WKB reader, every fourth through covt_wkb.parse as well: a Python
            # loop per point over 5.8 M coordinates otherwise)
            plain, m = _agree(oc["types"], *oc["asm"][1:], parse=ti % 4 == 0)
            # real tiles lie inside the bound the header names (a POLYGON some encoder gave several outer
            # rings is negative where the later ones outweigh the first: shell minus holes as defined)
            assert (np.abs(plain[0]) < 2.0 ** 53).all(), (tile_key(path), L)
            n_cols += 1
            n_rows += oc["types"].size
    assert n_cols >= 700 and n_rows > 10000


def test_layout_rule_under_sanitizers(tmp_path):
    """The host-side layout code (covt_measures_plan.h) in a stand-alone program built with AddressSanitizer
    and UndefinedBehaviorSanitizer, on the CPU."""
    import os
    import subprocess

    from conftest import ROOT

    exe = str(tmp_path / "measures_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "measures_layout", "measures_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])

"""CPU: the WKB reference writers and parser of tests/covt_wkb.py (the definition the GPU pass of
covt_wkb.hip is held to, include/covt.h "Geometry as WKB"), and the plan's WKB layout (C-ABI, no GPU).

1. known answers: hand-written ISO WKB hex of every geometry type, an empty LINESTRING, INT32_MIN / MAX;
2. the vectorised writer equals the nested-loop writer on synthetic columns assembled by the oracle;
3. the parser turns written columns back into ``covt_asm.to_features`` of the same assembly (fixtures);
4. covt_plan_wkb_columns / covt_plan_wkb_descs: capacities, aligned disjoint slices, descriptor order.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_wkb as W
from conftest import tile_paths

D = {0: "0000000000000000", 1: "000000000000f03f", 2: "0000000000000040", 3: "0000000000000840",
     4: "0000000000001040"}


def _xy(*v):
    return "".join(D[x] for x in v)


def _col(types, geo, part, ring, coords):
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return np.asarray(types, np.uint8), i32(geo), i32(part), i32(ring), i32(coords).reshape(-1, 2)


TRI = [0, 0, 1, 0, 0, 1, 0, 0]
KATS = [
    ("POINT(1 2)", _col([0], [0, 1], [0, 1], [0, 1], [1, 2]), "0101000000" + _xy(1, 2)),
    ("LINESTRING(1 2,3 4)", _col([1], [0, 1], [0, 1], [0, 2], [1, 2, 3, 4]),
     "0102000000" "02000000" + _xy(1, 2, 3, 4)),
    ("POLYGON((0 0,1 0,0 1,0 0))", _col([2], [0, 1], [0, 1], [0, 4], TRI),
     "0103000000" "01000000" "04000000" + _xy(*TRI)),
    ("MULTIPOINT(1 2,3 4)", _col([3], [0, 2], [0, 1, 2], [0, 1, 2], [1, 2, 3, 4]),
     "0104000000" "02000000" "0101000000" + _xy(1, 2) + "0101000000" + _xy(3, 4)),
    ("MULTILINESTRING((1 2,3 4))", _col([4], [0, 1], [0, 1], [0, 2], [1, 2, 3, 4]),
     "0105000000" "01000000" "0102000000" "02000000" + _xy(1, 2, 3, 4)),
    ("MULTIPOLYGON(((0 0,1 0,0 1,0 0)))", _col([5], [0, 1], [0, 1], [0, 4], TRI),
     "0106000000" "01000000" "0103000000" "01000000" "04000000" + _xy(*TRI)),
    ("LINESTRING EMPTY", _col([1], [0, 1], [0, 1], [0, 0], []), "010200000000000000"),
    ("POINT(INT32_MIN INT32_MAX)", _col([0], [0, 1], [0, 1], [0, 1], [-(1 << 31), (1 << 31) - 1]),
     "0101000000" "000000000000e0c1" "0000c0ffffffdf41"),
    # empty parts and rings keep their headers: a polygon of one empty ring, a multipolygon of one part
    # without rings, an empty multilinestring
    ("POLYGON(EMPTY ring)", _col([2], [0, 1], [0, 1], [0, 0], []), "0103000000" "01000000" "00000000"),
    ("MULTIPOLYGON(EMPTY part)", _col([5], [0, 1], [0, 0], [0], []), "0106000000" "01000000" "0103000000" "00000000"),
    ("MULTILINESTRING EMPTY", _col([4], [0, 0], [0], [0], []), "0105000000" "00000000"),
]


@pytest.mark.parametrize("name,col,hexv", KATS, ids=[k[0] for k in KATS])
def test_known_answers(name, col, hexv):
    offs, data = W.write_plain(*col)
    assert data.hex() == hexv and offs.tolist() == [0, len(hexv) // 2]
    noffs, ndata = W.write_numpy(*col)
    assert ndata.tobytes().hex() == hexv and noffs.tolist() == offs.tolist()
    cls, parts = W.parse(data)
    assert cls == {0: 1, 3: 1, 1: 2, 4: 2, 2: 3, 5: 3}[int(col[0][0])]
    assert A.to_features(*col) == [(cls, [p[:-1] if cls == 3 and p else p for p in parts])]


def test_parser_rejects_malformed():
    for bad in ("00" + "01000000" + _xy(1, 2),            # big-endian byte order
                "0107000000" "00000000",                  # GEOMETRYCOLLECTION
                "0101000000" + _xy(1, 2) + "00",          # trailing byte
                "0104000000" "01000000" "0102000000" "00000000"):  # a line inside a MULTIPOINT
        with pytest.raises(ValueError):
            W.parse(bytes.fromhex(bad))


def _synth_cases():
    rng = np.random.default_rng(21)
    cols = [A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2)) for i, n in enumerate([0, 1, 5, 64, 200, 700])]
    cols.append(A.synth_column(rng, 3, False, False, big=True))
    for t in range(6):  # one-type columns: runs of empty parts / rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 150, bool(t & 1), False, probs=probs))
    return cols


def test_numpy_writer_matches_plain_writer(oracle):
    total = 0
    for ci, col in enumerate(_synth_cases()):
        st, geo, part, ring, xy = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"],
                                                           col["vb"], col["closed"], A.caps(col))
        assert st == 0, ci
        offs, data = W.write_plain(col["types"], geo, part, ring, xy)
        noffs, ndata = W.write_numpy(col["types"], geo, part, ring, xy)
        assert np.array_equal(offs, noffs), ci
        assert ndata.tobytes() == data, ci
        # the capacity the plan sizes a slice with bounds the bytes
        pcap, rcap, ccap = A.caps(col)
        assert len(data) <= 9 * (col["types"].size + pcap) + 4 * rcap + 16 * ccap, ci
        feats = W.parse_column(offs, data, unclose=True)
        assert feats == A.to_features(col["types"], geo, part, ring, xy), ci
        total += len(data)
    assert total > 100000


def test_parser_round_trip_on_fixture_tiles(oracle):
    n_cols = 0
    for p in tile_paths(("omt",))[:2] + tile_paths(("bing",))[:1] + tile_paths(("amazon",))[:1]:
        for L, c in A.oracle_tile_columns(oracle, open(p, "rb").read()).items():
            if c["asm"] is None or c["asm"][0] != 0:
                continue
            geo, part, ring, xy = c["asm"][1:]
            offs, data = W.write_numpy(c["types"], geo, part, ring, xy)
            assert W.parse_column(offs, data, unclose=True) == A.to_features(c["types"], geo, part, ring, xy), (p, L)
            n_cols += 1
    assert n_cols >= 10


def test_plan_wkb_layout(covt, decodable_tiles):
    """covt_plan_wkb_columns / _descs / _bytes: one record per geometry column in tile order, the capacity
    rule, 16-byte aligned disjoint slices inside the buffer, descriptors at the geometry descriptors' rows."""
    plan = covt.Plan.from_tiles([t for _, t in decodable_tiles[:40]])
    g, w, d = plan.geom, plan.wkb, plan.wdescs
    assert w.size == d.size == g.size > 0 and w.dtype == covt.WKB_INFO_DTYPE
    assert np.array_equal(w["tile"], g["tile"]) and np.array_equal(w["layer"], g["layer"])
    assert np.array_equal(w["desc_index"], g["desc_index"]) and np.array_equal(w["n_features"], g["n_features"])
    cap = 9 * (g["n_features"].astype(np.int64) + g["part_cap"]) + 4 * g["ring_cap"].astype(np.int64) \
        + 16 * g["coord_cap"].astype(np.int64)
    assert np.array_equal(w["byte_cap"], cap) and (w["flags"] == 0).all()
    assert (w["offsets_off"] % 16 == 0).all() and (w["bytes_off"] % 16 == 0).all()
    spans = sorted([(int(r["offsets_off"]), int(r["offsets_off"]) + 4 * (int(r["n_features"]) + 1)) for r in w]
                   + [(int(r["bytes_off"]), int(r["bytes_off"]) + int(r["byte_cap"])) for r in w])
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] <= plan.wkb_bytes <= spans[-1][1] + 15
    for f in ("offsets_off", "bytes_off", "byte_cap", "n_features", "flags"):
        assert np.array_equal(d[f][w["desc_index"]], w[f]), f


def test_layout_rule_under_sanitizers(tmp_path):
    """The host-side layout code (covt_wkb_plan.h: capacity, slices, the INT32_MAX check) in a stand-alone
    program built with AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU."""
    import os
    import subprocess

    from conftest import ROOT

    exe = str(tmp_path / "wkb_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "wkb_layout", "wkb_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])

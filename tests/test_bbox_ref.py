"""CPU: the reference bounding boxes of tests/covt_bbox.py (the definition the GPU pass of covt_bbox.hip is
held to, include/covt.h "Geometry bounding boxes"), and the plan's bounding-box layout (C-ABI, no GPU).

1. known answers: hand-written columns of every geometry type, an empty feature of each kind, a single
   point, negative and INT32_MIN / INT32_MAX coordinates;
2. the vectorised reference equals the nested-loop one on synthetic columns assembled by the oracle;
3. the box of a feature is the bounds of its parsed WKB value;
4. covt_plan_bbox_columns / covt_plan_bbox_descs: 32 bytes per feature, aligned disjoint slices, descriptor
   order; the layout rule itself in a stand-alone program under AddressSanitizer + UBSan.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_bbox as B
import covt_wkb as W

NAN = float("nan")
LO, HI = -(1 << 31), (1 << 31) - 1


def _col(geo, part, ring, coords):
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return i32(geo), i32(part), i32(ring), i32(coords).reshape(-1, 2)


TRI = [0, 0, 4, 0, 0, 3, 0, 0]
# (name, types, (geo, part, ring, coords), rows of (xmin, ymin, xmax, ymax), n_empty)
KATS = [
    ("POINT", [0], _col([0, 1], [0, 1], [0, 1], [7, -9]), [(7, -9, 7, -9)], 0),
    ("LINESTRING", [1], _col([0, 1], [0, 1], [0, 3], [5, 2, -3, 8, 1, -4]), [(-3, -4, 5, 8)], 0),
    ("POLYGON", [2], _col([0, 1], [0, 1], [0, 4], TRI), [(0, 0, 4, 3)], 0),
    ("POLYGON with a hole", [2], _col([0, 1], [0, 2], [0, 4, 8], [0, 0, 9, 0, 0, 9, 0, 0, 1, 1, 2, 1, 1, 2, 1, 1]),
     [(0, 0, 9, 9)], 0),
    ("MULTIPOINT", [3], _col([0, 3], [0, 1, 2, 3], [0, 1, 2, 3], [1, 2, -5, 6, 3, -7]), [(-5, -7, 3, 6)], 0),
    ("MULTILINESTRING", [4], _col([0, 2], [0, 1, 2], [0, 2, 4], [1, 2, 3, 4, -1, 10, 0, 0]), [(-1, 0, 3, 10)], 0),
    ("MULTIPOLYGON", [5], _col([0, 2], [0, 1, 2], [0, 4, 8], TRI + [10, 10, 12, 10, 10, 11, 10, 10]),
     [(0, 0, 12, 11)], 0),
    ("MULTIPOINT EMPTY", [3], _col([0, 0], [0], [0], []), [(NAN,) * 4], 1),
    ("LINESTRING EMPTY", [1], _col([0, 1], [0, 1], [0, 0], []), [(NAN,) * 4], 1),
    ("POLYGON of empty rings", [2], _col([0, 1], [0, 2], [0, 0, 0], []), [(NAN,) * 4], 1),
    ("MULTIPOLYGON of a part without rings", [5], _col([0, 1], [0, 0], [0], []), [(NAN,) * 4], 1),
    ("INT32 extremes", [1], _col([0, 1], [0, 1], [0, 2], [LO, HI, HI, LO]), [(LO, LO, HI, HI)], 0),
    ("negative", [0, 0], _col([0, 1, 2], [0, 1, 2], [0, 1, 2], [-1, -2, LO, -1]), [(-1, -2, -1, -2), (LO, -1, LO, -1)], 0),
    ("empty between full", [1, 4, 0], _col([0, 1, 1, 2], [0, 1, 2], [0, 2, 3], [1, 1, 2, 2, 9, -9]),
     [(1, 1, 2, 2), (NAN,) * 4, (9, -9, 9, -9)], 1),
]


@pytest.mark.parametrize("name,types,col,rows,n_empty", KATS, ids=[k[0] for k in KATS])
def test_known_answers(name, types, col, rows, n_empty):
    want = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    for fn in (B.bbox_plain, B.bbox_numpy):
        xmin, ymin, xmax, ymax, extent, ne = fn(*col)
        got = np.stack([xmin, ymin, xmax, ymax], axis=1)
        assert got.tobytes() == want.tobytes(), (fn.__name__, got)
        assert ne == n_empty
        full = want[~np.isnan(want[:, 0])]
        if full.size:
            assert extent.tolist() == [full[:, 0].min(), full[:, 1].min(), full[:, 2].max(), full[:, 3].max()]
        else:
            assert extent.view(np.uint64).tolist() == [B.NAN_BITS] * 4
    # and the box describes the WKB value of the same feature
    offs, data = W.write_plain(np.asarray(types, np.uint8), *col)
    assert B.same(B.wkb_bounds(W.parse_column(offs, data)), B.bbox_plain(*col))


def _synth_cases():
    rng = np.random.default_rng(31)
    cols = [A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2)) for i, n in enumerate([0, 1, 5, 64, 200, 700])]
    cols.append(A.synth_column(rng, 3, False, False, big=True))
    for t in range(6):  # one-type columns: runs of empty parts / rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 150, bool(t & 1), False, probs=probs))
    return cols


def test_numpy_reference_matches_plain_and_wkb_bounds(oracle):
    n_empty = n_rows = 0
    for ci, col in enumerate(_synth_cases()):
        st, geo, part, ring, xy = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"],
                                                           col["vb"], col["closed"], A.caps(col))
        assert st == 0, ci
        plain = B.bbox_plain(geo, part, ring, xy)
        assert B.same(plain, B.bbox_numpy(geo, part, ring, xy)), ci
        if col["types"].size <= 700 and xy.shape[0] < 50000:  # (the parser is a Python loop)
            offs, data = W.write_plain(col["types"], geo, part, ring, xy)
            assert B.same(plain, B.wkb_bounds(W.parse_column(offs, data))), ci
            assert B.same(plain, B.wkb_column_bounds(offs, np.frombuffer(data, np.uint8))), ci
        # the extent covers every coordinate of the column
        if xy.shape[0]:
            assert plain[4].tolist() == [xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()], ci
        n_empty += plain[5]
        n_rows += col["types"].size
    assert n_empty > 50 and n_rows > 1500


def test_plan_bbox_layout(covt, decodable_tiles):
    """covt_plan_bbox_columns / _descs / _bytes: one record per geometry column in tile order, 32 bytes per
    feature, 16-byte aligned disjoint slices inside the buffer, descriptors at the geometry descriptors' rows."""
    plan = covt.Plan.from_tiles([t for _, t in decodable_tiles[:40]])
    g, b, d = plan.geom, plan.bbox, plan.bdescs
    assert b.size == d.size == g.size > 0 and b.dtype == covt.BBOX_INFO_DTYPE and d.dtype == covt.BBOX_DESC_DTYPE
    assert np.array_equal(b["tile"], g["tile"]) and np.array_equal(b["layer"], g["layer"])
    assert np.array_equal(b["desc_index"], g["desc_index"]) and np.array_equal(b["n_features"], g["n_features"])
    assert (b["flags"] == 0).all() and (b["reserved"] == 0).all() and (b["off"] % 16 == 0).all()
    spans = [(int(r["off"]), int(r["off"]) + 32 * int(r["n_features"])) for r in b]
    assert spans == sorted(spans)  # tile order is buffer order
    assert spans[0][0] == 0 and all(x[1] <= y[0] < x[1] + 16 for x, y in zip(spans, spans[1:]))
    assert spans[-1][1] <= plan.bbox_bytes <= spans[-1][1] + 15
    for f in ("off", "n_features", "flags"):
        assert np.array_equal(d[f][b["desc_index"]], b[f]), f
    # a column read out of a buffer: four views of n values each, back to back
    buf = np.arange(plan.bbox_bytes, dtype=np.uint64).astype(np.uint8)
    res = np.zeros(b.size, dtype=covt.BBOX_RESULT_DTYPE)
    c = int(np.argmax(b["n_features"]))
    col = plan.bbox_column(buf, res, c)
    n, o = int(b["n_features"][c]), int(b["off"][c])
    assert len(col) == n > 0 and col.as_struct().shape == (n, 4)
    assert col.ymin.tobytes() == buf[o + 8 * n:o + 16 * n].tobytes() and col.ymax.tobytes() == buf[o + 24 * n:o + 32 * n].tobytes()


def test_layout_rule_under_sanitizers(tmp_path):
    """The host-side layout code (covt_bbox_plan.h) in a stand-alone program built with AddressSanitizer and
    UndefinedBehaviorSanitizer, on the CPU."""
    import os
    import subprocess

    from conftest import ROOT

    exe = str(tmp_path / "bbox_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "bbox_layout", "bbox_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])

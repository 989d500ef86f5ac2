"""CPU: the georeferencing transform (include/covt.h "Georeferenced geometry") on the host.
covt_geo_transform against the plain-Python table of tests/covt_geo.py bit for bit, known answers, the seam
between neighbouring tiles, rejected arguments, and the plan's side of it: covt_plan_geometry_extents against
the oracle's walk (Gen C) and against what oracle/gend.py wrote (Gen D), covt_plan_geo_transforms' launch-order
placement and `kinds`.
"""
import ctypes as C

import numpy as np
import pytest

import covt_geo as G
from conftest import tile_key, tile_paths

ZS = [0, 1, 5, 14, 22, 30]
EXTENTS = [256, 4096, 8192, 4095, 1000]
CRSS = [G.CRS_TILE, G.CRS_WEB_MERCATOR, G.CRS_CRS84]


def _addresses(rng, z):
    hi = (1 << z) - 1
    pts = {(0, 0), (hi, 0), (0, hi), (hi, hi)}
    for _ in range(6):
        pts.add((int(rng.integers(0, hi + 1)), int(rng.integers(0, hi + 1))))
    return sorted(pts)


def test_transform_equals_table_bit_for_bit(covt):
    rng = np.random.default_rng(7)
    n = 0
    for crs in CRSS:
        for z in ZS:
            for x, y in _addresses(rng, z):
                for e in EXTENTS:
                    got = covt.geo_transform(crs, z, x, y, e)
                    want = G.record(crs, z, x, y, e)
                    assert got.tobytes() == want.tobytes(), (crs, z, x, y, e, got, want)
                    n += 1
    assert n > 500
    assert covt.GEO_XFORM_DTYPE == G.XFORM_DTYPE


def test_known_answers_web_mercator(covt):
    xf = covt.geo_transform(covt.CRS_WEB_MERCATOR, 0, 0, 0, 4096)
    assert int(xf["kind"]) == covt.GEO_AFFINE
    out = G.apply(xf, np.array([[0, 0], [4096, 4096], [2048, 2048]], np.int32))
    assert out[0, 0] == -G.W and out[1, 0] == G.W and out[2, 0] == 0.0
    assert out[0, 1] == G.W and out[1, 1] == -G.W and out[2, 1] == 0.0


def test_known_answers_crs84(covt):
    xf = covt.geo_transform(covt.CRS_CRS84, 0, 0, 0, 4096)
    assert int(xf["kind"]) == covt.GEO_AFFINE_LAT
    out = G.apply(xf, np.array([[0, 0], [4096, 4096], [2048, 2048]], np.int32))
    assert out[0, 0] == -180.0 and out[1, 0] == 180.0 and out[2, 0] == 0.0
    assert abs(out[0, 1] - 85.0511287798066) < 1e-9 and abs(out[1, 1] + 85.0511287798066) < 1e-9
    assert abs(out[2, 1]) < 1e-9


def test_identity(covt):
    xf = covt.geo_transform(covt.CRS_TILE, 14, 8296, 10749, 4096)
    assert xf.tobytes() == np.zeros(1, covt.GEO_XFORM_DTYPE).tobytes()
    xy = np.array([[-5, 4100], [0, 0], [-(1 << 31), (1 << 31) - 1]], np.int32)
    assert G.apply(xf, xy).tobytes() == xy.astype(np.float64).tobytes()


def test_seam_between_neighbouring_tiles(covt):
    """The right / bottom edge (px = E) of tile (x, y) and the left / top edge (px = 0) of tile (x + 1, y + 1):
    Web Mercator within 4 ulp of W (the reference formulas give at most 2 over 50,000 random cases),
    longitude exactly."""
    rng = np.random.default_rng(11)
    ulp_w = np.spacing(G.W)
    worst = 0.0
    for _ in range(4000):
        z = int(rng.integers(1, 31))
        x, y = (int(v) for v in rng.integers(0, (1 << z) - 1, size=2))
        e = int(rng.choice(EXTENTS))
        a = covt.geo_transform(covt.CRS_WEB_MERCATOR, z, x, y, e)
        b = covt.geo_transform(covt.CRS_WEB_MERCATOR, z, x + 1, y + 1, e)
        pa, pb = G.apply(a, np.array([e, e], np.int32)), G.apply(b, np.array([0, 0], np.int32))
        worst = max(worst, abs(pa[0] - pb[0]), abs(pa[1] - pb[1]))
        a = covt.geo_transform(covt.CRS_CRS84, z, x, y, e)
        b = covt.geo_transform(covt.CRS_CRS84, z, x + 1, y + 1, e)
        la, lb = G.apply(a, np.array([e, e], np.int32)), G.apply(b, np.array([0, 0], np.int32))
        assert la[0] == lb[0], (z, x, y, e, la[0], lb[0])
    assert worst <= 4 * ulp_w, (worst, worst / ulp_w)
    assert 4 * ulp_w < 1.5e-8


@pytest.mark.parametrize("args", [(1, -1, 0, 0, 4096), (1, 31, 0, 0, 4096), (1, 5, 32, 0, 4096), (2, 5, 0, -1, 4096),
                                  (2, 5, 0, 32, 4096), (1, 0, 1, 0, 4096), (1, 5, 3, 3, 0), (2, 5, 3, 3, -7),
                                  (3, 5, 3, 3, 4096), (-1, 5, 3, 3, 4096)])
def test_rejected_arguments(covt, args):
    out = np.zeros(1, covt.GEO_XFORM_DTYPE)
    assert covt.lib().covt_geo_transform(*args, out.ctypes.data) == covt.ERR_INVALID_ARG
    with pytest.raises(covt.IllegalArgumentException):
        covt.geo_transform(*args)
    assert covt.lib().covt_geo_transform(1, 0, 0, 0, 4096, None) == covt.ERR_INVALID_ARG


def test_plan_extents_equal_the_oracle_walk_genc(covt, oracle):
    """covt_plan_geometry_extents over every fixture tile: the `extent` field of the oracle walk's records,
    column for column."""
    paths = tile_paths()
    tiles = [open(p, "rb").read() for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    assert plan.geometry_extents.size == plan.num_geometry_columns > 700
    c = 0
    for t, tile in enumerate(tiles):
        if int(plan.tile_status[t]):
            continue
        st, ss = oracle.walk_tile(tile, 0)
        assert st == 0
        by_layer = {}
        for s in ss:
            if s.column_kind == 1:
                by_layer[s.layer] = s.extent
        for layer in sorted(by_layer):
            assert (int(plan.geom["tile"][c]), int(plan.geom["layer"][c])) == (t, layer), tile_key(paths[t])
            assert int(plan.geometry_extents[c]) == by_layer[layer], (tile_key(paths[t]), layer)
            c += 1
    assert c == plan.num_geometry_columns
    assert covt.lib().covt_plan_geometry_extents(None, None) == covt.ERR_INVALID_ARG
    assert covt.lib().covt_plan_geometry_extents(plan._h, None) == covt.ERR_INVALID_ARG


def _gend_tile(extents):
    """A Gen D tile with one POINT layer per extent (a layer without a geometry column in between)."""
    import oracle.gend as D

    layers = []
    for k, e in enumerate(extents):
        n = 3 + k
        cols = [D.id_column(np.arange(n)), D.geometry_column(np.zeros(n, np.uint8), vertices=np.arange(2 * n).reshape(-1, 2))]
        layers.append(D.layer("l%d" % k, e, n, cols))
        if k == 0:
            layers.append(D.layer("ids_only", 512, 2, [D.id_column(np.arange(2))]))
    return D.tile(layers)


def test_plan_extents_gend(covt, oracle):
    tiles = [_gend_tile([4096, 1000]), _gend_tile([1000]), _gend_tile([8192, 4096, 1000])]
    plan = covt.Plan.from_tiles(tiles, covt.FORMAT_GEND)
    assert (plan.tile_status == 0).all()
    assert plan.geometry_extents.tolist() == [4096, 1000, 1000, 8192, 4096, 1000]
    assert plan.geom["layer"].tolist() == [0, 2, 0, 0, 2, 3]  # (layer 1 of a tile holds ids only)


def test_plan_geo_transforms_are_in_launch_order(covt):
    """Column c's transform lies at desc_index[c]; a batch whose tiles differ in z (and whose launch order is
    not its tile order) catches a tile-order / launch-order mix-up."""
    keys = ["omt/5_16_20", "omt/14_8298_10748", "bing/4-8-5"]
    paths = {tile_key(p): p for p in tile_paths()}
    tiles = [open(paths[k], "rb").read() for k in keys]
    zxy = [G.zxy_of_key(k) for k in keys]
    plan = covt.Plan.from_tiles(tiles)
    di = plan.geom["desc_index"]
    assert not np.array_equal(di, np.arange(di.size))  # the launch order is not the tile order
    for crs, kind in ((covt.CRS_WEB_MERCATOR, covt.GEO_AFFINE), (covt.CRS_CRS84, covt.GEO_AFFINE_LAT),
                      (covt.CRS_TILE, covt.GEO_IDENTITY)):
        table, kinds = plan.geo_transforms(crs, zxy)
        assert kinds == 1 << kind and table.size == plan.num_geometry_columns
        for c in range(plan.num_geometry_columns):
            z, x, y = zxy[int(plan.geom["tile"][c])]
            want = G.record(crs, z, x, y, int(plan.geometry_extents[c]))
            assert table[int(di[c])].tobytes() == want.tobytes(), (crs, c)
    table, kinds = plan.geo_transforms(covt.CRS_TILE)  # tile-local needs no addresses
    assert kinds == 1 and table.tobytes() == np.zeros(table.size, covt.GEO_XFORM_DTYPE).tobytes()
    # an invalid address of any tile, a missing table of addresses, an unknown CRS, a short list
    for bad in ([(5, 16, 20), (31, 0, 0), (4, 8, 5)], [(5, 16, 20), (14, 1 << 14, 0), (4, 8, 5)], [(5, 16, -1)] * 3):
        with pytest.raises(covt.IllegalArgumentException):
            plan.geo_transforms(covt.CRS_WEB_MERCATOR, bad)
    with pytest.raises(covt.IllegalArgumentException):
        plan.geo_transforms(covt.CRS_CRS84)
    with pytest.raises(covt.IllegalArgumentException):
        plan.geo_transforms(7, zxy)
    with pytest.raises(covt.IllegalArgumentException):
        plan.geo_transforms(covt.CRS_CRS84, zxy[:2])
    kinds = C.c_uint32(0)
    assert covt.lib().covt_plan_geo_transforms(None, 1, None, None, C.byref(kinds)) == covt.ERR_INVALID_ARG
    assert covt.lib().covt_plan_geo_transforms(plan._h, 1, None, None, None) == covt.ERR_INVALID_ARG


def test_plan_geo_transforms_reject_a_layer_without_extent(covt):
    plan = covt.Plan.from_tiles([_gend_tile([4096, 0])], covt.FORMAT_GEND)
    assert plan.geometry_extents.tolist() == [4096, 0]
    with pytest.raises(covt.IllegalArgumentException):
        plan.geo_transforms(covt.CRS_WEB_MERCATOR, [(3, 1, 1)])


def test_transform_header_in_a_host_only_program_under_sanitizers(tmp_path):
    """covt_geo_plan.h compiled by the host compiler alone into a stand-alone program with AddressSanitizer and
    UndefinedBehaviorSanitizer: the coefficients and the transformed pixels equal the Python table bit for bit
    (the latitude, which goes through the host libm, within 1e-9 degrees), invalid arguments are refused."""
    import os
    import subprocess

    from conftest import ROOT

    exe = str(tmp_path / "geo_plan_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "geo_plan", "geo_plan_check.cc")])
    rng = np.random.default_rng(23)
    cases = []
    for crs in CRSS:
        for z in ZS:
            for x, y in _addresses(rng, z)[:5]:
                for e in EXTENTS:
                    px, py = (int(v) for v in rng.integers(-e // 4, e + e // 4 + 1, size=2))
                    cases.append((crs, z, x, y, e, px, py))
    cases += [(1, 3, 1, 1, 4096, -(1 << 31), (1 << 31) - 1), (1, 31, 0, 0, 4096, 0, 0), (2, 3, 8, 0, 4096, 0, 0),
              (2, 3, 0, 0, 0, 0, 0), (5, 3, 0, 0, 4096, 0, 0)]
    p = subprocess.run([exe], input="".join("%d %d %d %d %d %d %d\n" % c for c in cases), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines()]
    assert len(rows) == len(cases)
    f64 = lambda h: np.array([int(h, 16)], np.uint64).view(np.float64)[0]  # noqa: E731
    for c, r in zip(cases, rows):
        if not G.valid(*c[:5]):
            assert int(r[0]) == -6, c
            continue
        want = G.record(*c[:5])
        assert int(r[0]) == 0 and int(r[5]) == int(want["kind"]), c
        assert [int(h, 16) for h in r[1:5]] == [int(np.float64(want[k]).view(np.uint64)) for k in ("sx", "ox", "sy", "oy")], c
        xy = G.apply(want, np.array([c[5], c[6]], np.int32))
        assert int(r[6], 16) == int(xy[0].view(np.uint64)), c
        if int(want["kind"]) == G.AFFINE_LAT:
            assert abs(f64(r[7]) - xy[1]) <= 1e-9, c
        else:
            assert int(r[7], 16) == int(xy[1].view(np.uint64)), c

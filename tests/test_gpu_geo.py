"""GPU: the projected WKB and bounding-box passes (include/covt.h "Georeferenced geometry") against the
reference transform of tests/covt_geo.py, through the C-ABI: covt_assemble_geometry_device +
covt_geometry_wkb_projected_device / covt_geometry_bbox_projected_device on synthetic columns, the
_projected_host entry points on the fixture tiles, the DeviceBatch / DevicePlan paths, decode_covt, a
HIP-graph replay and the Java overloads through a fake VM.

What is exact and what is not: IDENTITY and AFFINE coordinates and the x of AFFINE_LAT equal the numpy
reference bit for bit; the y of AFFINE_LAT goes through the device's sinh and atan and is held to 1e-9
degrees (the smallest pixel of this project's data, z14 at extent 8192, spans 2.7e-6 degrees; float64
spacing at 90 degrees is 1.4e-14).
"""
import struct

import numpy as np
import pytest

import covt_asm as A
import covt_bbox as B
import covt_geo as G
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
LAT_TOL = 1e-9
NAN4 = np.full(4, np.nan).tobytes()
CRS_OF_KIND = {G.IDENTITY: G.CRS_TILE, G.AFFINE: G.CRS_WEB_MERCATOR, G.AFFINE_LAT: G.CRS_CRS84}


def _a16(x):
    return (x + 15) & ~15


def _wkb_cap(col):
    pcap, rcap, ccap = col.get("caps") or A.caps(col)
    return 9 * (col["types"].size + pcap) + 4 * rcap + 16 * ccap


def _layouts(covt, cols, bflags=None):
    """WKB and bounding-box descriptors (the plan's layout rules, a gap after every slice)."""
    wd = np.zeros(len(cols), dtype=covt.WKB_DESC_DTYPE)
    bd = np.zeros(len(cols), dtype=covt.BBOX_DESC_DTYPE)
    woff = boff = 0
    for ci, col in enumerate(cols):
        n = col["types"].size
        wd[ci]["offsets_off"] = woff
        woff = _a16(woff + 4 * (n + 1)) + 16
        wd[ci]["bytes_off"] = woff
        wd[ci]["byte_cap"] = _wkb_cap(col)
        woff = _a16(woff + _wkb_cap(col)) + 16
        wd[ci]["n_features"] = n
        bd[ci]["off"] = boff
        bd[ci]["n_features"] = n
        bd[ci]["flags"] = bflags[ci] if bflags else 0
        boff = _a16(boff + 32 * n) + 16
    return wd, max(woff, 16), bd, max(boff, 16)


def _tables(cols, kinds_of, rng, z_choices=(0, 1, 5, 14, 22, 30), extents=(256, 4096, 8192, 4095, 1000)):
    """One transform per column, kinds as given, tile addresses and extents pairwise different."""
    table = np.zeros(len(cols), dtype=G.XFORM_DTYPE)
    seen = set()
    for ci in range(len(cols)):
        while True:
            z = int(z_choices[int(rng.integers(0, len(z_choices)))]) if ci >= len(z_choices) else int(z_choices[ci])
            x, y = (int(rng.integers(0, 1 << z)) for _ in range(2))
            e = int(extents[int(rng.integers(0, len(extents)))])
            if (z, x, y, e) not in seen:
                seen.add((z, x, y, e))
                break
        table[ci] = G.record(CRS_OF_KIND[kinds_of[ci]], z, x, y, e)
        if kinds_of[ci] != G.IDENTITY:
            cols[ci]["extent"] = e
    return table


def _run(covt, cols, table=None, kinds=0, products=("wkb", "bbox"), flags_extra=None, in_res=None, dres=None,
         bflags=None, expect=0):
    """covt_assemble_geometry_device, then the plain passes (table None) or the projected ones, over synthetic
    columns; every output buffer is poisoned with FILL first."""
    import torch

    dec, desc, asm_bytes, _ = A.pack_columns(covt, cols, flags_extra, in_res)
    wd, wkb_bytes, bd, bbox_bytes = _layouts(covt, cols, bflags)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_dec, d_desc, d_wdesc, d_bdesc = up(dec), up(desc), up(wd), up(bd)
    d_asm = torch.full((asm_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_gres = torch.zeros(4 * len(cols), dtype=torch.int32, device=dev)
    d_res = torch.from_numpy(np.zeros(2, np.int32) if dres is None else np.asarray(dres, np.int32)).to(dev)
    d_xf = up(table) if table is not None else None
    s = torch.cuda.current_stream(dev).cuda_stream
    L = covt.lib()
    n = len(cols)
    assert L.covt_assemble_geometry_device(d_dec.data_ptr(), d_res.data_ptr(), d_desc.data_ptr(), n,
                                           d_asm.data_ptr(), d_gres.data_ptr(), s) == 0
    out = {"wd": wd, "bd": bd}
    if "wkb" in products:
        d_wkb = torch.full((wkb_bytes,), FILL, dtype=torch.uint8, device=dev)
        d_wres = torch.full((16 * n,), FILL, dtype=torch.uint8, device=dev)
        a = (d_dec.data_ptr(), d_desc.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(), d_wdesc.data_ptr(), n,
             d_wkb.data_ptr(), d_wres.data_ptr())
        st = L.covt_geometry_wkb_device(*a, s) if table is None else \
            L.covt_geometry_wkb_projected_device(*a, d_xf.data_ptr(), kinds, s)
        assert st == expect
    if "bbox" in products:
        d_bbox = torch.full((bbox_bytes,), FILL, dtype=torch.uint8, device=dev)
        d_bres = torch.full((40 * n,), FILL, dtype=torch.uint8, device=dev)
        a = (d_desc.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(), d_bdesc.data_ptr(), n, d_bbox.data_ptr(),
             d_bres.data_ptr())
        st = L.covt_geometry_bbox_device(*a, s) if table is None else \
            L.covt_geometry_bbox_projected_device(*a, d_xf.data_ptr(), kinds, s)
        assert st == expect
    torch.cuda.synchronize()
    if "wkb" in products:
        out["wkb"], out["wres"] = d_wkb.cpu().numpy(), d_wres.cpu().numpy().view(covt.WKB_RESULT_DTYPE)
    if "bbox" in products:
        out["bbox"], out["bres"] = d_bbox.cpu().numpy(), d_bres.cpu().numpy().view(covt.BBOX_RESULT_DTYPE)
    out["gres"] = d_gres.cpu().numpy().view(covt.GEOM_RESULT_DTYPE)
    return out


def _assembly(oracle, col, cache):
    """(status, geo, part, ring, coords) of the oracle's assembly, cached per column object."""
    if id(col) not in cache:
        cache[id(col)] = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"], col["vb"],
                                                  col["closed"], col.get("caps") or A.caps(col))
    return cache[id(col)]


def _int_boxes(oracle, col, cache):
    key = ("bbox", id(col))
    if key not in cache:
        cache[key] = B.bbox_numpy(*_assembly(oracle, col, cache)[1:])
    return cache[key]


def coord_positions(offsets, data):
    """Byte positions of every coordinate (x double; y follows) of a column's WKB values, in order."""
    buf = bytes(data)
    u32 = struct.Struct("<I").unpack_from
    runs = []

    def value(pos):
        code = u32(buf, pos + 1)[0]
        pos += 5
        if code == 1:
            runs.append((pos, 1))
            return pos + 16
        if code in (2, 3):
            rings = 1
            if code == 3:
                rings = u32(buf, pos)[0]
                pos += 4
            for _ in range(rings):
                k = u32(buf, pos)[0]
                pos += 4
                if k:
                    runs.append((pos, k))
                pos += 16 * k
            return pos
        parts = u32(buf, pos)[0]
        pos += 4
        for _ in range(parts):
            pos = value(pos)
        return pos

    offs = np.asarray(offsets).tolist()
    for f in range(len(offs) - 1):
        assert value(offs[f]) == offs[f + 1]
    if not runs:
        return np.zeros(0, np.int64)
    return np.concatenate([p + 16 * np.arange(k, dtype=np.int64) for p, k in runs])


def _same_y(got, want, kind, what):
    """y values: bit for bit unless the kind maps them through the device libm."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if kind != G.AFFINE_LAT:
        assert got.tobytes() == want.tobytes(), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert (got[nan].view(np.uint64) == G.NAN_BITS).all(), what
    if (~nan).any():
        d = np.abs(got[~nan] - want[~nan])
        assert np.nanmax(d) <= LAT_TOL, (what, float(np.nanmax(d)))


def _check_wkb_column(plain_off, plain_data, got_off, got_data, xf, coords, what, pos=None):
    """A projected column against the plain one: offsets and every non-coordinate byte equal, the coordinates
    apply(xf, assembled coordinates).  pos: coord_positions of the plain column, if the caller has them."""
    assert np.array_equal(plain_off, got_off), what
    assert plain_data.size == got_data.size, what
    pos = coord_positions(plain_off, plain_data) if pos is None else pos
    assert pos.size == coords.shape[0], what
    mask = np.ones(plain_data.size, dtype=bool)
    idx = (pos[:, None] + np.arange(16)[None, :]).reshape(-1)
    mask[idx] = False
    assert np.array_equal(plain_data[mask], got_data[mask]), what
    if pos.size == 0:
        return
    as_f64 = lambda d: np.ascontiguousarray(d[idx].reshape(-1, 16)).view(np.float64)  # noqa: E731  [n, 2]
    assert as_f64(plain_data).tobytes() == coords.astype(np.float64).tobytes(), what  # (the plain pass: the pixels)
    got, want = as_f64(got_data), G.apply(xf, coords)
    assert got[:, 0].tobytes() == want[:, 0].tobytes(), what
    _same_y(got[:, 1], want[:, 1], int(xf["kind"]), what)


def _check_bbox_column(got, want, kind, what):
    """(xmin, ymin, xmax, ymax, extent, n_empty) against the transformed reference."""
    for k in (0, 2):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (what, k)
    for k in (1, 3):
        _same_y(got[k], want[k], kind, (what, k))
    assert np.asarray(got[4])[[0, 2]].tobytes() == np.asarray(want[4])[[0, 2]].tobytes(), (what, got[4], want[4])
    _same_y(np.asarray(got[4])[[1, 3]], np.asarray(want[4])[[1, 3]], kind, (what, "extent"))
    assert int(got[5]) == int(want[5]), what
    ok = ~np.isnan(np.asarray(got[1]))
    assert (np.asarray(got[0])[ok] <= np.asarray(got[2])[ok]).all() and (np.asarray(got[1])[ok] <= np.asarray(got[3])[ok]).all()


def _bbox_of(buf, bres, bd, ci, n):
    o = int(bd["off"][ci])
    a = buf[o:o + 32 * n].view(np.float64)
    return a[:n], a[n:2 * n], a[2 * n:3 * n], a[3 * n:], bres["extent"][ci], int(bres["n_empty"][ci])


def _wkb_of(buf, wres, wd, ci, n):
    oo, bo = int(wd["offsets_off"][ci]), int(wd["bytes_off"][ci])
    return buf[oo:oo + 4 * (n + 1)].view(np.int32), buf[bo:bo + int(wres["n_bytes"][ci])]


def _tile_local(rng, col, extent):
    """Coordinates as a tile holds them: inside the extent, in the buffer around it (negative, past the extent)."""
    col["vb"] = rng.integers(-(extent // 4), extent + extent // 4 + 1, size=col["vb"].size, dtype=np.int64).astype(np.int32)


def _mixed_columns(rng):
    cols = []
    for i in range(36):
        n = [0, 1, 63, 64, 65, 1000][i % 6]
        cols.append(A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2)))
    for t in range(6):  # one-type columns: runs of empty parts and rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 400, bool(t & 1), False, probs=probs))
    return cols


@pytest.fixture(scope="module")
def mixed(covt, oracle, gpu_available):
    """The mixed batch once: its columns, transforms, the plain and the projected passes' outputs."""
    rng = np.random.default_rng(31)
    cols = _mixed_columns(rng)
    kinds_of = [(i + i // 6) % 3 for i in range(len(cols))]  # every kind meets every feature count and type
    table = _tables(cols, kinds_of, rng)
    for ci, col in enumerate(cols):
        if ci % 5:  # (every fifth column keeps its full-range int32 coordinates)
            _tile_local(rng, col, int(col.get("extent", 4096)))
    plain = _run(covt, cols)
    proj = _run(covt, cols, table, 7)
    return cols, table, plain, proj, {}


def test_mixed_batch_wkb(covt, oracle, mixed):
    cols, table, plain, proj, cache = mixed
    assert (proj["gres"]["status"] == 0).all() and (proj["wres"]["status"] == 0).all()
    assert proj["wres"].tobytes() == plain["wres"].tobytes()
    written = np.zeros(proj["wkb"].size, dtype=bool)
    for ci, col in enumerate(cols):
        n = col["types"].size
        po, pdata = _wkb_of(plain["wkb"], plain["wres"], plain["wd"], ci, n)
        go, gdata = _wkb_of(proj["wkb"], proj["wres"], proj["wd"], ci, n)
        coords = np.asarray(_assembly(oracle, col, cache)[4]).reshape(-1, 2)
        _check_wkb_column(po, pdata, go, gdata, table[ci], coords, ci)
        oo, bo = int(proj["wd"]["offsets_off"][ci]), int(proj["wd"]["bytes_off"][ci])
        written[oo:oo + 4 * (n + 1)] = True
        written[bo:bo + gdata.size] = True
    assert (proj["wkb"][~written] == FILL).all()


def test_mixed_batch_bbox(covt, oracle, mixed):
    cols, table, plain, proj, cache = mixed
    assert (proj["bres"]["status"] == 0).all()
    written = np.zeros(proj["bbox"].size, dtype=bool)
    for ci, col in enumerate(cols):
        n = col["types"].size
        want = G.apply_boxes(table[ci], _int_boxes(oracle, col, cache))
        _check_bbox_column(_bbox_of(proj["bbox"], proj["bres"], proj["bd"], ci, n), want, int(table[ci]["kind"]), ci)
        o = int(proj["bd"]["off"][ci])
        written[o:o + 32 * n] = True
    assert (proj["bbox"][~written] == FILL).all()
    assert np.array_equal(proj["bres"]["n_empty"], plain["bres"]["n_empty"])


def test_mixed_batch_two_products_agree(covt, mixed):
    """Every projected box is the bounds of the projected WKB value beside it."""
    cols, table, plain, proj, cache = mixed
    for ci, col in enumerate(cols):
        n = col["types"].size
        offs, data = _wkb_of(proj["wkb"], proj["wres"], proj["wd"], ci, n)
        want = B.wkb_column_bounds(offs, data)
        _check_bbox_column(_bbox_of(proj["bbox"], proj["bres"], proj["bd"], ci, n), want, int(table[ci]["kind"]), ci)


def test_identity_only_equals_the_plain_passes(covt, mixed):
    """A table of IDENTITY transforms (kinds = 1): both projected passes' buffers and results equal the plain
    passes' byte for byte."""
    cols, table, plain, proj, cache = mixed
    ident = np.zeros(len(cols), dtype=G.XFORM_DTYPE)
    got = _run(covt, cols, ident, 1)
    for k in ("wkb", "wres", "bbox", "bres"):
        assert got[k].tobytes() == plain[k].tobytes(), k


def test_bbox_store_sites_under_a_flip(covt, oracle, gpu_available):
    """The four store sites of the bounding-box pass under AFFINE with sy < 0: a feature ending 2047 / 2048 /
    2049 coordinates past its owner's run (the wave finishes it / the workgroup does), a 300,000-coordinate
    feature with its extremes first and last, features ending at chunk edges, and the column extent; once
    with up to 64 workgroups per column and once padded to 4097 columns (one workgroup each).  ymin <= ymax
    everywhere and equality with the reference show the flip at every site."""
    from test_gpu_bbox import _long_feature_columns

    rng = np.random.default_rng(16)
    cols = _long_feature_columns(rng)
    cache = {}

    def check(cols):
        table = np.zeros(len(cols), dtype=G.XFORM_DTYPE)
        for ci in range(len(cols)):  # pairwise different addresses at z 14
            table[ci] = G.record(G.CRS_WEB_MERCATOR, 14, 5000 + ci, 16000 - ci, 4096)
        assert (table["sy"] < 0).all()
        got = _run(covt, cols, table, 2, products=("bbox",))
        assert (got["bres"]["status"] == 0).all()
        for ci, col in enumerate(cols):
            n = col["types"].size
            box = _bbox_of(got["bbox"], got["bres"], got["bd"], ci, n)
            _check_bbox_column(box, G.apply_boxes(table[ci], _int_boxes(oracle, col, cache)), G.AFFINE, ci)
            assert box[4][1] <= box[4][3]
        return got, table

    got, table = check(cols)
    lo, hi = -(1 << 31), (1 << 31) - 1
    ends = G.apply(table[3], np.array([[lo, lo], [hi, hi]], np.int32))
    assert got["bres"]["extent"][3].tolist() == [ends[0, 0], ends[1, 1], ends[1, 0], ends[0, 1]]  # (y flipped)
    tiny = A.synth_column(rng, 1, False, False)
    check(cols + [tiny] * (4097 - len(cols)))


def _multipoints(rng, counts):
    k = int(sum(counts))
    return {"types": np.full(len(counts), 3, np.uint8), "go": np.asarray(counts, np.int32), "po": np.zeros(0, np.int32),
            "ro": np.zeros(0, np.int32), "vo": None,
            "vb": rng.integers(-1000, 5000, size=2 * k, dtype=np.int64).astype(np.int32), "closed": False}


def test_empty_features_and_all_empty_columns(covt, oracle, gpu_available):
    """Runs of empty features and columns of nothing else under every kind: the quiet NaN's bits, n_empty, a
    NaN extent; the WKB values of the empty features are those of the plain pass."""
    rng = np.random.default_rng(19)
    runs = [0, 1, 63, 64, 65, 700]
    cols = []
    for kind in range(3):
        cols += [_multipoints(rng, [0] * r + [1] * 100 + [0] * r + [2] * 100 + [0] * r) for r in runs]
        cols.append(_multipoints(rng, [0] * 700))
    kinds_of = [ci // (len(runs) + 1) for ci in range(len(cols))]
    table = _tables(cols, kinds_of, rng)
    plain = _run(covt, cols)
    got = _run(covt, cols, table, 7)
    cache = {}
    for ci, col in enumerate(cols):
        n = col["types"].size
        box = _bbox_of(got["bbox"], got["bres"], got["bd"], ci, n)
        _check_bbox_column(box, G.apply_boxes(table[ci], _int_boxes(oracle, col, cache)), kinds_of[ci], ci)
        empty = np.asarray(col["go"]) == 0
        for k in range(4):
            assert (box[k][empty].view(np.uint64) == G.NAN_BITS).all() and not np.isnan(box[k][~empty]).any()
        assert box[5] == int(empty.sum())
        po, pdata = _wkb_of(plain["wkb"], plain["wres"], plain["wd"], ci, n)
        go, gdata = _wkb_of(got["wkb"], got["wres"], got["wd"], ci, n)
        coords = np.asarray(_assembly(oracle, col, cache)[4]).reshape(-1, 2)
        _check_wkb_column(po, pdata, go, gdata, table[ci], coords, ci)
    for ci in (len(runs), 2 * len(runs) + 1, 3 * len(runs) + 2):  # the all-empty columns
        assert got["bres"]["extent"][ci].tobytes() == NAN4 and int(got["bres"]["n_empty"][ci]) == 700


def test_status_paths(covt, oracle, gpu_available):
    rng = np.random.default_rng(18)
    ok = A.synth_column(rng, 50, False, False)
    _tile_local(rng, ok, 4096)
    cols = [ok] * 7
    # 0: fine  1: source stream failed  2: COVT_GEOM_TOO_LARGE  3: kind 3  4: a kind whose bit `kinds` lacks
    # 5: fine (IDENTITY)  6: fine
    table = np.zeros(7, dtype=G.XFORM_DTYPE)
    for ci in range(7):
        table[ci] = G.record(G.CRS_WEB_MERCATOR, 5, 3 + ci, 9, 4096)
    table[3]["kind"] = 3
    table[4] = G.record(G.CRS_CRS84, 5, 1, 2, 4096)
    table[5] = G.record(G.CRS_TILE, 5, 1, 3, 4096)
    got = _run(covt, cols, table, 0b011, flags_extra=[0, 0, 0x80000000, 0, 0, 0, 0],
               in_res=[[-1] * 6, [0, -1, -1, -1, -1, 1]] + [[-1] * 6] * 5, dres=[0, 5, covt.ERR_TRUNCATED, 7])
    bad = covt.ERR_INVALID_ARG
    want = [0, covt.ERR_TRUNCATED, bad, bad, bad, 0, 0]
    assert got["wres"]["status"].tolist() == want and got["bres"]["status"].tolist() == want
    n = 50
    for ci in (1, 2, 3, 4):  # failed columns: n_bytes 0 / n_empty 0, extent NaN, slices untouched
        assert int(got["wres"]["n_bytes"][ci]) == 0 and int(got["wres"]["reserved"][ci]) == 0
        assert int(got["bres"]["n_empty"][ci]) == 0 and got["bres"]["extent"][ci].tobytes() == NAN4
        o = int(got["bd"]["off"][ci])
        assert (got["bbox"][o:o + 32 * n + 16] == FILL).all(), ci
        oo, bo = int(got["wd"]["offsets_off"][ci]), int(got["wd"]["bytes_off"][ci])
        assert (got["wkb"][oo:oo + 4 * (n + 1)] == FILL).all() and (got["wkb"][bo:bo + _wkb_cap(ok)] == FILL).all(), ci
    cache = {}
    plain = _run(covt, [ok])
    po, pdata = _wkb_of(plain["wkb"], plain["wres"], plain["wd"], 0, n)
    coords = np.asarray(_assembly(oracle, ok, cache)[4]).reshape(-1, 2)
    for ci in (0, 5, 6):  # the neighbours are exact
        go, gdata = _wkb_of(got["wkb"], got["wres"], got["wd"], ci, n)
        _check_wkb_column(po, pdata, go, gdata, table[ci], coords, ci)
        _check_bbox_column(_bbox_of(got["bbox"], got["bres"], got["bd"], ci, n),
                           G.apply_boxes(table[ci], _int_boxes(oracle, ok, cache)), int(table[ci]["kind"]), ci)
    # `kinds` with a bit above bit 2: the call itself is rejected and nothing is written
    got = _run(covt, cols, table, 0b1011, expect=bad)
    assert (got["wkb"] == FILL).all() and (got["bbox"] == FILL).all()
    assert (got["wres"].view(np.uint8) == FILL).all() and (got["bres"].view(np.uint8) == FILL).all()


# ---- the fixture tiles through the plan ----------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_geo(covt, oracle, gpu_available):
    """The OMT and Bing fixture tiles (their names are z/x/y), the oracle's assembly of every column, the plain
    WKB of the plan and, per column, where its coordinates lie -- once for the tests below."""
    paths = tile_paths(("omt", "bing"))
    tiles = [open(p, "rb").read() for p in paths]
    zxy = [G.zxy_of_key(tile_key(p)) for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    wbuf, wres = plan.wkb_host()
    cols = {}
    per_tile = {}
    for c in range(plan.num_geometry_columns):
        t, L = int(plan.geom["tile"][c]), int(plan.geom["layer"][c])
        if t not in per_tile:
            per_tile[t] = A.oracle_tile_columns(oracle, tiles[t])
        oc = per_tile[t][L]
        if oc["asm"] is None:
            assert int(wres["status"][c]) != 0
            continue
        assert int(wres["status"][c]) == 0
        w = plan.wkb_column(wbuf, wres, c)
        coords = np.asarray(oc["asm"][4]).reshape(-1, 2)
        cols[c] = (w, coords, B.bbox_numpy(*oc["asm"][1:]), coord_positions(w.offsets, w.data))
    assert len(cols) >= 600
    return paths, tiles, zxy, plan, wres, cols


@pytest.mark.parametrize("crs", [G.CRS_WEB_MERCATOR, G.CRS_CRS84])
def test_fixture_tiles_projected(covt, fixture_geo, crs):
    """Plan.wkb_host / bbox_host with a CRS over the fixture tiles against apply() over the oracle's assembly."""
    paths, tiles, zxy, plan, wres0, cols = fixture_geo
    table, kinds = plan.geo_transforms(crs, zxy)
    wbuf, wres = plan.wkb_host(crs=crs, tile_zxy=zxy)
    bbuf, bres = plan.bbox_host(crs=crs, tile_zxy=zxy)
    assert wres.tobytes() == wres0.tobytes()
    kind = G.AFFINE if crs == G.CRS_WEB_MERCATOR else G.AFFINE_LAT
    assert kinds == 1 << kind
    for c, (w, coords, boxes, pos) in cols.items():
        xf = table[int(plan.geom["desc_index"][c])]
        z, x, y = zxy[int(plan.geom["tile"][c])]
        assert xf.tobytes() == G.record(crs, z, x, y, int(plan.geometry_extents[c])).tobytes()
        g = plan.wkb_column(wbuf, wres, c)
        _check_wkb_column(w.offsets, w.data, g.offsets, g.data, xf, coords, (tile_key(paths[int(plan.geom["tile"][c])]), c),
                          pos)
        col = plan.bbox_column(bbuf, bres, c)
        _check_bbox_column((col.xmin, col.ymin, col.xmax, col.ymax, col.extent, col.n_empty), G.apply_boxes(xf, boxes),
                           kind, c)
    for c in range(plan.num_geometry_columns):
        if c not in cols:
            assert int(bres["status"][c]) != 0 and bres["extent"][c].tobytes() == NAN4


def _same_slices(plan, res, x, y, kind):
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(res["status"][c]):
            continue
        if kind == "bbox":
            o, n = int(plan.bbox["off"][c]), int(plan.bbox["n_features"][c])
            assert x[o:o + 32 * n].tobytes() == y[o:o + 32 * n].tobytes(), c
        else:
            o, n, b = int(plan.wkb["offsets_off"][c]), int(plan.wkb["n_features"][c]), int(plan.wkb["bytes_off"][c])
            assert x[o:o + 4 * (n + 1)].tobytes() == y[o:o + 4 * (n + 1)].tobytes(), c
            assert x[b:b + int(res["n_bytes"][c])].tobytes() == y[b:b + int(res["n_bytes"][c])].tobytes(), c
        n_ok += 1
    return n_ok


@pytest.mark.parametrize("crs", [G.CRS_WEB_MERCATOR, G.CRS_CRS84])
def test_device_paths_match_host_path(covt, gpu_available, crs):
    """30 tiles through DeviceBatch (xf=) and through DevicePlan with a supplied table: the host path's bytes."""
    import torch

    paths = tile_paths(("omt",))[:30]
    tiles = [open(p, "rb").read() for p in paths]
    zxy = [G.zxy_of_key(tile_key(p)) for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    wbuf_h, wres_h = plan.wkb_host(crs=crs, tile_zxy=zxy)
    bbuf_h, bres_h = plan.bbox_host(crs=crs, tile_zxy=zxy)
    assert (bres_h["status"] == 0).any()
    xf = plan.geo_transforms(crs, zxy)
    b = covt.DeviceBatch(plan, "cuda:0")
    b.decode()
    b.assemble()
    b.wkb(xf=xf)
    b.bbox(xf=xf)
    d_xf = b.d_xf
    b.bbox(xf=xf)  # (the table is uploaded once and kept)
    assert b.d_xf is d_xf
    torch.cuda.synchronize()
    wbuf_d, wres_d = b.wkb_results()
    bbuf_d, bres_d = b.bbox_results()
    assert wres_h.tobytes() == wres_d.tobytes() and bres_h.tobytes() == bres_d.tobytes()
    assert _same_slices(plan, wres_h, wbuf_h, wbuf_d, "wkb") > 0 and _same_slices(plan, bres_h, bbuf_h, bbuf_d, "bbox") > 0
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_wkb, d_wres = dp.alloc_wkb()
    d_bbox, d_bres = dp.alloc_bbox()
    gi, _ = dp.geometry_copy()
    assert gi.tobytes() == plan.geom.tobytes()  # (so the host plan's table is in this plan's launch order)
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.wkb(d_out, d_res, d_asm, d_gres, d_wkb, d_wres, d_xf=d_xf, kinds=xf[1])
    dp.bbox(d_asm, d_gres, d_bbox, d_bres, d_xf=d_xf, kinds=xf[1])
    torch.cuda.synchronize()
    ng = plan.num_geometry_columns
    wres_p = d_wres.cpu().numpy().view(np.uint8)[:16 * ng].view(covt.WKB_RESULT_DTYPE)[plan.wkb["desc_index"]]
    bres_p = d_bres.cpu().numpy().view(np.uint8)[:40 * ng].view(covt.BBOX_RESULT_DTYPE)[plan.bbox["desc_index"]]
    assert wres_h.tobytes() == wres_p.tobytes() and bres_h.tobytes() == bres_p.tobytes()
    _same_slices(plan, wres_h, wbuf_h, d_wkb.cpu().numpy().view(np.uint8)[:plan.wkb_bytes], "wkb")
    _same_slices(plan, bres_h, bbuf_h, d_bbox.cpu().numpy().view(np.uint8)[:plan.bbox_bytes], "bbox")


def test_decode_covt_in_a_crs(covt, gpu_available):
    """decode_covt(tile, tile_id=, crs=) yields wkb / bbox in that CRS; the layers of a z14 OMT tile lie inside
    the tile's own lon/lat bounds (closed form, independent of the transform table) widened by its buffer."""
    import math

    key = "omt/14_8298_10748"
    path = [p for p in tile_paths(("omt",)) if tile_key(p) == key][0]
    tile = open(path, "rb").read()
    z, x, y = G.zxy_of_key(key)
    plain = covt.CovtParser.decode_covt(tile)
    assert all(lc.crs == covt.CRS_TILE for lc in plain)
    with pytest.raises(covt.IllegalArgumentException):
        covt.CovtParser.decode_covt(tile, crs=covt.CRS_CRS84)
    n = 1 << z
    lon = [x / n * 360.0 - 180.0, (x + 1) / n * 360.0 - 180.0]
    lat = [math.degrees(math.atan(math.sinh(math.pi * (1 - 2 * (y + 1) / n)))),
           math.degrees(math.atan(math.sinh(math.pi * (1 - 2 * y / n))))]
    for crs in (covt.CRS_CRS84, covt.CRS_WEB_MERCATOR):
        layers = covt.CovtParser.decode_covt(tile, tile_id=(z, x, y), crs=crs)
        plan = covt.Plan.from_tiles([tile])
        wbuf, wres = plan.wkb_host(crs=crs, tile_zxy=[(z, x, y)])
        bbuf, bres = plan.bbox_host(crs=crs, tile_zxy=[(z, x, y)])
        by_layer = {int(plan.geom["layer"][c]): c for c in range(plan.num_geometry_columns)}
        assert layers and len(layers) == len(plain)
        for lc, pl in zip(layers, plain):
            assert lc.crs == crs and lc.wkb is not None and lc.bbox is not None
            c = by_layer[lc.layer]
            w, bb = plan.wkb_column(wbuf, wres, c), plan.bbox_column(bbuf, bres, c)
            assert lc.wkb.data.tobytes() == w.data.tobytes() and np.array_equal(lc.wkb.offsets, w.offsets)
            assert lc.bbox.as_struct().tobytes() == bb.as_struct().tobytes()
            assert lc.bbox.extent.tobytes() == bb.extent.tobytes()
            assert np.array_equal(lc.wkb.offsets, pl.wkb.offsets)
            if crs != covt.CRS_CRS84 or np.isnan(lc.bbox.extent[0]):
                continue
            e = int(plan.geometry_extents[c])
            over = max(0.0, -pl.bbox.extent[0], -pl.bbox.extent[1], pl.bbox.extent[2] - e, pl.bbox.extent[3] - e) / e
            assert over < 0.5  # (the layer's own buffer, in tiles)
            w_lon, w_lat = (lon[1] - lon[0]) * (over + 1e-6), (lat[1] - lat[0]) * (over + 1e-6) * 1.01
            ext = lc.bbox.extent
            assert lon[0] - w_lon <= ext[0] <= ext[2] <= lon[1] + w_lon, (lc.layer, ext, lon)
            assert lat[0] - w_lat <= ext[1] <= ext[3] <= lat[1] + w_lat, (lc.layer, ext, lat)


def test_projected_passes_replay_in_a_hip_graph(covt, gpu_available, decodable_tiles):
    """decode + assemble + projected WKB + projected bbox captured in one HIP graph and replayed three times
    into poisoned buffers: the eager bytes each time (the passes hold no scratch; the table is on the device
    before the capture)."""
    import torch

    tiles = [t for _, t in decodable_tiles]
    zxy = [G.zxy_of_key(k) for k, _ in decodable_tiles]
    plan = covt.Plan.from_tiles(tiles)
    crs = covt.CRS_CRS84
    wbuf_h, wres_h = plan.wkb_host(crs=crs, tile_zxy=zxy)
    bbuf_h, bres_h = plan.bbox_host(crs=crs, tile_zxy=zxy)
    assert (bres_h["status"] == 0).all() and (wres_h["status"] == 0).all()
    xf = plan.geo_transforms(crs, zxy)
    dev = torch.device("cuda:0")
    b = covt.DeviceBatch(plan, dev)
    s = torch.cuda.Stream(dev)

    def launch():
        b.decode(s)
        b.assemble(s)
        b.wkb(s, xf=xf)
        b.bbox(s, xf=xf)

    with torch.cuda.stream(s):
        launch()  # fork streams, events, the assembly scratch and the table exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for _ in range(3):
        for t in (b.d_bbox, b.d_wkb, b.d_asm):
            t.fill_(FILL)
        b.d_bres.fill_(0x5A5A5A5A5A5A5A5A)
        b.d_wres.fill_(0x5A5A5A5A5A5A5A5A)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        wbuf, wres = b.wkb_results()
        bbuf, bres = b.bbox_results()
        assert wres.tobytes() == wres_h.tobytes() and bres.tobytes() == bres_h.tobytes()
        assert _same_slices(plan, wres_h, wbuf_h, wbuf, "wkb") == plan.num_geometry_columns
        assert _same_slices(plan, bres_h, bbuf_h, bbuf, "bbox") == plan.num_geometry_columns
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


# ---- GpuCovtBatch.geometryWkb / geometryBbox with a CRS through the JNI shim and a fake VM ----------------
@pytest.fixture(scope="module")
def geo_shim(covt):
    """tests/jni_geo/jni_geo_test: the shim compiled against the stand-in tests/jni/jni.h with the compiler
    line of tests/jni/Makefile."""
    import os
    import subprocess

    from conftest import ROOT

    covt.lib()
    src = os.path.join(ROOT, "tests", "jni_geo", "jni_geo_test.cc")
    exe = src[:-3]
    lib_dir = os.path.join(ROOT, "cov-tiles_amd")
    deps = [src, os.path.join(ROOT, "tests", "jni", "jni.h"), os.path.join(lib_dir, "jni", "covt_jni.cc"),
            os.path.join(ROOT, "include", "covt.h"), os.path.join(lib_dir, "libcovt.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall",
                               "-I" + os.path.join(ROOT, "tests", "jni"), "-I" + os.path.join(ROOT, "include"),
                               "-o", exe, src, os.path.join(lib_dir, "jni", "covt_jni.cc"), "-L" + lib_dir, "-lcovt",
                               "-Wl,-rpath,$ORIGIN/../../cov-tiles_amd", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


JNI_KEYS = ["omt/5_16_20", "omt/14_8298_10748", "bing/4-8-5"]


def _jni_case(mode, crs, zxy):
    import os

    from conftest import ROOT

    tiles = [open(os.path.join(ROOT, "tests", "golden", "tiles", k + ".covt"), "rb").read() for k in JNI_KEYS]
    nums = [len(t) for t in tiles] + [v for a in zxy for v in a]
    return tiles, "%s %d %d %s | %s" % (mode, crs, len(tiles), " ".join(str(v) for v in nums), b"".join(tiles).hex())


def _shim_run(exe, case):
    import subprocess

    p = subprocess.run([exe], input=case + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    (out,) = p.stdout.splitlines()
    return out.split()


@pytest.mark.parametrize("crs", [G.CRS_WEB_MERCATOR, G.CRS_CRS84])
def test_projected_geometry_through_jni(geo_shim, covt, gpu_available, crs):
    """Both overloads into direct buffers: the returned rows and the buffers equal Plan.*_host(crs=...)'s."""
    zxy = [G.zxy_of_key(k) for k in JNI_KEYS]
    tiles, case = _jni_case("wkb", crs, zxy)
    plan = covt.Plan.from_tiles(tiles)
    kind, nb, res_hex, out_hex = _shim_run(geo_shim, case)
    wbuf, wres = plan.wkb_host(crs=crs, tile_zxy=zxy)
    assert kind == "ok" and int(nb) == plan.wkb_bytes
    res = np.frombuffer(bytes.fromhex(res_hex), "<i8").reshape(-1, 2)
    assert np.array_equal(res[:, 0], wres["status"]) and np.array_equal(res[:, 1], wres["n_bytes"])
    assert _same_slices(plan, wres, wbuf, np.frombuffer(bytes.fromhex(out_hex), np.uint8), "wkb") >= 10
    _, case = _jni_case("bbox", crs, zxy)
    kind, nb, res_hex, out_hex = _shim_run(geo_shim, case)
    bbuf, bres = plan.bbox_host(crs=crs, tile_zxy=zxy)
    assert kind == "ok" and int(nb) == plan.bbox_bytes
    res = np.frombuffer(bytes.fromhex(res_hex), "<i8").reshape(-1, 6)
    assert np.array_equal(res[:, 0], bres["status"]) and np.array_equal(res[:, 1], bres["n_empty"])
    assert res[:, 2:].tobytes() == np.ascontiguousarray(bres["extent"]).tobytes()  # (the doubles' bits)
    assert _same_slices(plan, bres, bbuf, np.frombuffer(bytes.fromhex(out_hex), np.uint8), "bbox") >= 10
    plain, _ = plan.bbox_host()
    assert plain.tobytes() != bbuf.tobytes()


@pytest.mark.parametrize("mode", ["wkb", "bbox"])
@pytest.mark.parametrize("bad", ["length", "z31"])
def test_projected_jni_rejects_bad_addresses(geo_shim, gpu_available, mode, bad):
    """A tileZxy of the wrong length, and z = 31: IllegalArgumentException."""
    zxy = [list(G.zxy_of_key(k)) for k in JNI_KEYS]
    if bad == "length":
        zxy[-1] = zxy[-1][:2]
    else:
        zxy[1] = [31, 0, 0]
    _, case = _jni_case(mode, G.CRS_WEB_MERCATOR, zxy)
    assert _shim_run(geo_shim, case) == ["exc", "java/lang/IllegalArgumentException"]

"""The mvt entry points as a C caller sees them: raw ctypes calls on libcovt.so with caller-owned structs and
buffers (tests/test_capi_simplify.py drives the simplification the same way).  CPU only: struct sizes, exported
and bound symbols, the plan's records and descriptors on every fixture tile against the rule written out here,
the too-large flag where the WKB flag is, option validation, null and negative arguments, the host tile writer."""
import ctypes as C
import os

import numpy as np
import pytest

import covt_geom as G
import covt_props as P
from conftest import ROOT, tile_key, tile_paths


class MvtInfo(C.Structure):  # covt_mvt_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("n_features", C.c_int32), ("desc_index", C.c_int32),
                ("off", C.c_int64), ("byte_cap", C.c_int64), ("flags", C.c_int32), ("ring_cap", C.c_int32),
                ("coord_cap", C.c_int32), ("reserved", C.c_int32)]


class MvtDesc(C.Structure):  # covt_mvt_desc
    _fields_ = [("off", C.c_int64), ("byte_cap", C.c_int64), ("n_features", C.c_int32), ("flags", C.c_int32),
                ("ring_cap", C.c_int32), ("coord_cap", C.c_int32)]


class MvtResult(C.Structure):  # covt_mvt_result
    _fields_ = [("status", C.c_int32), ("n_empty", C.c_int32), ("n_bytes", C.c_int64)]


class MvtOptions(C.Structure):  # covt_mvt_options
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("shift", C.c_int32), ("reserved", C.c_int32)]


TILE = os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt")
NAMES = ["covt_mvt_options_init", "covt_plan_mvt_bytes", "covt_plan_mvt_columns", "covt_plan_mvt_descs",
         "covt_geometry_mvt_device", "covt_plan_mvt_host", "covt_device_plan_mvt_bytes",
         "covt_device_plan_mvt_descs_device", "covt_device_plan_mvt_copy", "covt_device_plan_mvt"]
CHUNK = 1024  # COVT_MVT_CHUNK


def a16(x):
    return (x + 15) & ~15


def slice_bytes(n, byte_cap, ring_cap, coord_cap):
    """type | offsets | bytes | ring records (16 bytes) | ring bases | chunk totals."""
    return (a16(n) + a16(4 * (n + 1)) + a16(byte_cap) + a16(16 * ring_cap) + a16(4 * ring_cap)
            + a16(4 * ((coord_cap + CHUNK - 1) // CHUNK + 1)))


def _plan(L, tile):
    buf = (C.c_uint8 * (len(tile) + 4096)).from_buffer_copy(tile + bytes(4096))
    off, size = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(tile))
    h = C.c_void_p()
    assert L.covt_plan_create(C.cast(buf, C.POINTER(C.c_uint8)), off, size, 1, 0, 0, C.byref(h)) == 0
    return h, buf


def test_struct_sizes_and_bindings(covt):
    assert (C.sizeof(MvtInfo), C.sizeof(MvtDesc), C.sizeof(MvtResult), C.sizeof(MvtOptions)) == (48, 32, 16, 16)
    assert C.sizeof(covt.MvtOptions) == 16 and covt.MVT_TOO_LARGE == 1 and covt.MVT_ORIENT == 1 and covt.MVT_MAX_SHIFT == 30
    for struct, dtype in ((MvtInfo, covt.MVT_INFO_DTYPE), (MvtDesc, covt.MVT_DESC_DTYPE), (MvtResult, covt.MVT_RESULT_DTYPE)):
        assert dtype.itemsize == C.sizeof(struct)
        for f, _ in struct._fields_:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    header = open(os.path.join(ROOT, "include", "covt.h")).read()
    for n in NAMES:
        assert n in covt.EXPORTED_SYMBOLS and n + "(" in header and hasattr(covt.lib(), n), n
    assert "mvt" in covt._PRODUCTS and "Geometry as MVT" in header
    for flag in ("COVT_MVT_TOO_LARGE", "COVT_MVT_ORIENT", "COVT_MVT_MAX_SHIFT"):
        assert "#define " + flag in header
    q = covt._PRODUCTS["mvt"]
    assert q.res_dtype == covt.MVT_RESULT_DTYPE and q.res_words == ("int64", 2)
    for owner, names in ((covt.Plan, ("mvt_host", "mvt_column")), (covt.DeviceBatch, ("mvt", "mvt_results")),
                         (covt.DevicePlan, ("mvt_copy", "alloc_mvt", "mvt"))):
        for name in names:
            assert hasattr(owner, name), name
    # the build id covers the new files
    assert "csrc/covt_mvt.hip" in covt._BUILD_SOURCES and "csrc/covt_mvt_plan.h" in covt._BUILD_SOURCES
    assert covt.source_build_id() in covt.version()
    mk = open(os.path.join(ROOT, "cov-tiles_amd", "Makefile")).read()
    assert "csrc/covt_mvt.hip" in mk and "csrc/covt_mvt_plan.h" in mk


def test_options(covt):
    L = covt.lib()
    o = MvtOptions(1, 2, 3, 4)
    L.covt_mvt_options_init(C.byref(o))
    assert (o.size, o.flags, o.shift, o.reserved) == (16, 0, 0, 0)
    L.covt_mvt_options_init(None)  # (ignored)
    p = covt.MvtOptions()
    assert (p.size, p.flags, p.shift, p.reserved) == (16, 0, 0, 0)
    p = covt.MvtOptions(orient=True, shift=4)
    assert (p.size, p.flags, p.shift) == (16, covt.MVT_ORIENT, 4)


BAD_OPTIONS = [("shift -1", (16, 0, -1)), ("shift 31", (16, 0, 31)), ("shift INT32_MIN", (16, 0, -2 ** 31)),
               ("shift INT32_MAX", (16, 0, 2 ** 31 - 1)), ("flag bit 1", (16, 2, 0)), ("flag bit 31", (16, 1 << 31, 0)),
               ("all flag bits", (16, 0xFFFFFFFF, 0)), ("size 0", (0, 0, 0)), ("size 12", (12, 0, 0)),
               ("size 32", (32, 0, 0))]


@pytest.mark.parametrize("name,fields", BAD_OPTIONS, ids=[b[0] for b in BAD_OPTIONS])
def test_option_validation(covt, name, fields):
    """A shift outside [0, 30], an unknown flag bit or a wrong size: COVT_ERR_INVALID_ARG from the device entry
    point (before it looks at its pointers: 0 columns would otherwise be nothing to do) and from the whole-plan
    call, before any device work."""
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    o = MvtOptions(fields[0], fields[1], fields[2], 0)
    assert L.covt_geometry_mvt_device(None, None, None, None, None, 0, C.byref(o), None, None, None) == I
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        out = (C.c_uint8 * L.covt_plan_mvt_bytes(h))()
        res = (MvtResult * n)()
        assert L.covt_plan_mvt_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), C.byref(o), out, res) == I
        assert not any(bytes(out)) and not any(bytes(res))
    finally:
        L.covt_plan_destroy(h)


def test_mvt_entry_points_check_their_arguments(covt):
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    ok = MvtOptions(16, 1, 30, 0)
    assert L.covt_plan_mvt_bytes(None) == 0
    assert L.covt_plan_mvt_columns(None, None) == I and L.covt_plan_mvt_descs(None, None) == I
    assert L.covt_plan_mvt_host(None, None, 0, C.byref(ok), None, None) == I
    assert L.covt_geometry_mvt_device(None, None, None, None, None, -1, C.byref(ok), None, None, None) == I
    assert L.covt_geometry_mvt_device(None, None, None, None, None, 3, C.byref(ok), None, None, None) == I
    assert L.covt_geometry_mvt_device(None, None, None, None, None, 0, None, None, None, None) == I  # no options
    assert L.covt_geometry_mvt_device(None, None, None, None, None, 0, C.byref(ok), None, None, None) == 0  # nothing to do
    assert L.covt_device_plan_mvt_bytes(None) == 0 and not L.covt_device_plan_mvt_descs_device(None)
    assert L.covt_device_plan_mvt_copy(None, None, None) == I
    assert L.covt_device_plan_mvt(None, None, None, None, 0, C.byref(ok), None, None, None) == I
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        assert L.covt_plan_mvt_bytes(h) > 0 and L.covt_plan_mvt_columns(h, None) == I and L.covt_plan_mvt_descs(h, None) == I
        out = (C.c_uint8 * L.covt_plan_mvt_bytes(h))()
        res = (MvtResult * n)()
        tiles = C.cast(buf, C.POINTER(C.c_uint8))
        # no options, a tile past the caller's buffer, a missing output buffer, missing results, missing tiles: all
        # refused before any device work
        assert L.covt_plan_mvt_host(h, tiles, len(tile), None, out, res) == I
        assert L.covt_plan_mvt_host(h, tiles, len(tile) - 1, C.byref(ok), out, res) == I
        assert L.covt_plan_mvt_host(h, tiles, len(tile), C.byref(ok), None, res) == I
        assert L.covt_plan_mvt_host(h, tiles, len(tile), C.byref(ok), out, None) == I
        assert L.covt_plan_mvt_host(h, None, len(tile), C.byref(ok), out, res) == I
    finally:
        L.covt_plan_destroy(h)


def test_records_and_descriptors_on_every_fixture_tile(covt):
    """Offsets 16-byte aligned, slices disjoint, in tile order and inside covt_plan_mvt_bytes, sized by the rule
    from the geometry column's capacities; descriptors are the records at desc_index; COVT_MVT_TOO_LARGE exactly
    where COVT_WKB_TOO_LARGE is."""
    n_cols = 0
    for path in tile_paths():
        plan = covt.Plan.from_tiles([open(path, "rb").read()])
        if int(plan.tile_status[0]):
            plan.close()
            continue
        end = 0
        for c in range(plan.num_geometry_columns):
            g, q, w = plan.geom[c], plan.mvt[c], plan.wkb[c]
            key = (tile_key(path), c)
            assert (int(q["tile"]), int(q["layer"]), int(q["desc_index"])) == (int(g["tile"]), int(g["layer"]), int(g["desc_index"]))
            assert bool(q["flags"] & covt.MVT_TOO_LARGE) == bool(w["flags"] & 1), key
            if q["flags"]:
                assert (int(q["n_features"]), int(q["byte_cap"]), int(q["ring_cap"]), int(q["coord_cap"])) == (0, 0, 0, 0), key
            else:
                n, rc, cc = int(g["n_features"]), int(g["ring_cap"]), int(g["coord_cap"])
                assert (int(q["n_features"]), int(q["ring_cap"]), int(q["coord_cap"])) == (n, rc, cc), key
                assert int(q["byte_cap"]) == 10 * cc + 7 * rc + 5 * n <= 2 ** 31 - 1, key
            assert int(q["off"]) == end and end % 16 == 0, key
            end += slice_bytes(int(q["n_features"]), int(q["byte_cap"]), int(q["ring_cap"]), int(q["coord_cap"]))
            d = plan.mvdescs[int(q["desc_index"])]
            assert all(int(d[f]) == int(q[f]) for f in ("off", "byte_cap", "n_features", "flags", "ring_cap", "coord_cap")), key
            n_cols += 1
        assert plan.mvt_bytes == end
        plan.close()
    assert n_cols >= 700


def _prop(covt, name, ptype, values):
    """A PropertyColumn built by hand: values[i] None -> absent."""
    n = len(values)
    validity = np.zeros((n + 7) // 8, np.uint8)
    for i, v in enumerate(values):
        if v is not None:
            validity[i >> 3] |= 1 << (i & 7)
    d_off = d_bytes = None
    if ptype == covt.PROP_BOOLEAN:
        vals = np.zeros((n + 7) // 8, np.uint8)
        for i, v in enumerate(values):
            if v:
                vals[i >> 3] |= 1 << (i & 7)
    elif ptype == covt.PROP_INT64:
        vals = np.array([v or 0 for v in values], np.int64)
    elif ptype == covt.PROP_FLOAT:
        vals = np.array([v or 0 for v in values], np.float32)
    else:
        words = sorted({v for v in values if v is not None})
        vals = np.array([words.index(v) if v is not None else 0 for v in values], np.int32)
        enc = [w.encode() for w in words]
        d_off = np.cumsum([0] + [len(e) for e in enc]).astype(np.int32)
        d_bytes = np.frombuffer(b"".join(enc), np.uint8)
    return covt.PropertyColumn(name, ptype, n, validity, vals, d_off, d_bytes, sum(v is not None for v in values))


def test_tile_writer(covt):
    """mvt_layer_bytes around a hand-made MvtColumn: field order, ids, tags, value kinds and their deduplication,
    empty features left out, index; read back by the two independent MVT readers of the tests."""
    vals = [bytes([9, 50, 34]), b"", bytes([9, 4, 4, 18, 0, 16, 16, 0]), bytes([9, 6, 12, 18, 10, 12, 24, 44, 15])]
    offs = np.cumsum([0] + [len(v) for v in vals]).astype(np.int32)
    col = covt.MvtColumn(np.array([1, 2, 2, 3], np.uint8), offs, np.frombuffer(b"".join(vals), np.uint8), 1)
    assert len(col) == 4 and [col.feature(i) for i in range(4)] == vals
    props = {"name": _prop(covt, "name", covt.PROP_STRING, ["a", "b", None, "a"]),
             "rank": _prop(covt, "rank", covt.PROP_INT64, [7, 7, -3, None]),
             "h": _prop(covt, "h", covt.PROP_FLOAT, [1.5, None, 1.5, 0.0]),
             "ok": _prop(covt, "ok", covt.PROP_BOOLEAN, [True, False, None, False])}
    ids = np.array([10, 11, 2 ** 40, 13], np.int64)
    rec = covt.mvt_layer_bytes("roads", 4096, col, ids=ids, properties=props)
    # the record: field 3, then version, name, features, keys, values, extent in this order
    assert rec[0] == 0x1A
    fields = [(f, v) for f, _, v in G._fields(next(G._fields(rec))[2])]
    assert [f for f, _ in fields] == [15, 1] + [2] * 3 + [3] * 4 + [4] * 7 + [5]
    assert fields[0][1] == 2 and fields[1][1] == b"roads" and fields[-1][1] == 4096
    assert [v for f, v in fields if f == 3] == [b"name", b"rank", b"h", b"ok"]
    # values in first-use order, deduplicated by kind and exact value: "a", 7, 1.5f, true | -3 | 0.0f, false
    assert [v for f, v in fields if f == 4] == [b"\x0a\x01a", b"\x28\x07", b"\x15\x00\x00\xc0\x3f", b"\x38\x01",
                                                b"\x30\x05", b"\x15\x00\x00\x00\x00", b"\x38\x00"]
    feats = G.mvt_layers(rec)["roads"]
    assert feats["extent"] == 4096
    assert [(i, c) for i, c, _ in feats["features"]] == [(10, 1), (2 ** 40, 2), (13, 3)]  # the empty one left out
    assert feats["features"][0][2] == [((25, 17),)] and feats["features"][1][2] == [((2, 2), (2, 10), (10, 10))]
    assert P.mvt_properties(rec)["roads"] == [{"name": "a", "rank": 7, "h": 1.5, "ok": True}, {"rank": -3, "h": 1.5},
                                              {"name": "a", "h": 0.0, "ok": False}]
    # index restricts and orders; without ids and properties a feature is type + geometry
    rec = covt.mvt_layer_bytes("r", 512, col, index=np.array([3, 1, 0], np.int32))
    feats = G.mvt_layers(rec)["r"]
    assert feats["extent"] == 512 and [c for _, c, _ in feats["features"]] == [3, 1]
    assert covt.mvt_tile_bytes([rec, rec]) == rec + rec

"""The simplify entry points as a C caller sees them: raw ctypes calls on libcovt.so with caller-owned structs and
buffers (tests/test_capi_select.py drives the selection the same way).  CPU only: struct sizes, exported and
bound symbols, the plan's layout and the retargeted descriptor table on every fixture tile against the rule
written out here, null and negative arguments, shift validation, covt_plan_set_simplify on and off."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, tile_key, tile_paths


class SimplifyInfo(C.Structure):  # covt_simplify_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("n_features", C.c_int32), ("desc_index", C.c_int32),
                ("off", C.c_int64), ("flags", C.c_int32), ("part_cap", C.c_int32), ("ring_cap", C.c_int32),
                ("coord_cap", C.c_int32)]


class SimplifyDesc(C.Structure):  # covt_simplify_desc
    _fields_ = [("off", C.c_int64), ("n_features", C.c_int32), ("flags", C.c_int32), ("part_cap", C.c_int32),
                ("ring_cap", C.c_int32), ("coord_cap", C.c_int32), ("reserved", C.c_int32)]


class GeomResult(C.Structure):  # covt_geom_result
    _fields_ = [("status", C.c_int32), ("num_parts", C.c_int32), ("num_rings", C.c_int32), ("num_coords", C.c_int32)]


TILE = os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt")
NAMES = ["covt_plan_simplify_bytes", "covt_plan_simplify_columns", "covt_plan_simplify_descs",
         "covt_plan_simplified_geometry_descs", "covt_plan_simplify_shifts", "covt_geometry_simplify_device",
         "covt_plan_simplify_host", "covt_plan_set_simplify", "covt_device_plan_simplify_bytes",
         "covt_device_plan_simplify_descs_device", "covt_device_plan_simplify_copy",
         "covt_device_plan_simplified_geometry_descs_device", "covt_device_plan_simplify"]
CHUNK = 1024  # COVT_SIMPLIFY_CHUNK


def a16(x):
    return (x + 15) & ~15


def member_offsets(n, part_cap, ring_cap, coord_cap):
    """(geometry_offsets, part_offsets, ring_offsets, coords, ring scratch, chunk scratch, slice bytes)."""
    part = a16(4 * (n + 1))
    ring = part + a16(4 * (part_cap + 1))
    xy = ring + a16(4 * (ring_cap + 1))
    rk = xy + a16(8 * coord_cap)
    ck = rk + a16(4 * ring_cap)
    return 0, part, ring, xy, rk, ck, ck + a16(4 * ((coord_cap + CHUNK - 1) // CHUNK + 1))


def _plan(L, tile):
    buf = (C.c_uint8 * (len(tile) + 4096)).from_buffer_copy(tile + bytes(4096))
    off, size = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(tile))
    h = C.c_void_p()
    assert L.covt_plan_create(C.cast(buf, C.POINTER(C.c_uint8)), off, size, 1, 0, 0, C.byref(h)) == 0
    return h, buf


def test_struct_sizes_and_bindings(covt):
    assert C.sizeof(SimplifyInfo) == 40 and C.sizeof(SimplifyDesc) == 32 and C.sizeof(GeomResult) == 16
    assert covt.SIMPLIFY_INFO_DTYPE.itemsize == 40 and covt.SIMPLIFY_DESC_DTYPE.itemsize == 32
    assert covt.SIMPLIFY_TOO_LARGE == 1 and covt.SIMPLIFY_MAX_SHIFT == 30
    for struct, dtype in ((SimplifyInfo, covt.SIMPLIFY_INFO_DTYPE), (SimplifyDesc, covt.SIMPLIFY_DESC_DTYPE)):
        for f, _ in struct._fields_:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    header = open(os.path.join(ROOT, "include", "covt.h")).read()
    for n in NAMES:
        assert n in covt.EXPORTED_SYMBOLS and n + "(" in header and hasattr(covt.lib(), n), n
    assert "simplify" in covt._PRODUCTS and "Geometry simplification" in header
    for flag in ("COVT_SIMPLIFY_TOO_LARGE", "COVT_SIMPLIFY_MAX_SHIFT"):
        assert "#define " + flag in header
    q = covt._PRODUCTS["simplify"]
    assert q.res_dtype == covt.GEOM_RESULT_DTYPE and q.res_words == ("int32", 4)
    for name in ("simplify_host", "simplified_arrays", "set_simplify", "simplify_shifts"):
        assert hasattr(covt.Plan, name), name
    for name in ("simplify", "simplify_results"):
        assert hasattr(covt.DeviceBatch, name), name
    for name in ("simplify_copy", "alloc_simplify", "simplify"):
        assert hasattr(covt.DevicePlan, name), name
    # the build id covers the new files
    assert "csrc/covt_simplify.hip" in covt._BUILD_SOURCES and "csrc/covt_simplify_plan.h" in covt._BUILD_SOURCES
    assert covt.source_build_id() in covt.version()


def test_simplify_entry_points_check_their_arguments(covt):
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    assert L.covt_plan_simplify_bytes(None) == 0
    assert L.covt_plan_simplify_columns(None, None) == I and L.covt_plan_simplify_descs(None, None) == I
    assert L.covt_plan_simplified_geometry_descs(None, None) == I and L.covt_plan_simplify_shifts(None, None, None) == I
    assert L.covt_plan_simplify_host(None, None, 0, 0, None, None, None) == I
    assert L.covt_plan_set_simplify(None, 1, 0, None) == I
    assert L.covt_geometry_simplify_device(None, None, None, None, None, -1, 0, None, None, None, None) == I
    assert L.covt_geometry_simplify_device(None, None, None, None, None, 3, 0, None, None, None, None) == I
    assert L.covt_geometry_simplify_device(None, None, None, None, None, 0, 0, None, None, None, None) == 0  # nothing to do
    assert L.covt_device_plan_simplify_bytes(None) == 0 and not L.covt_device_plan_simplify_descs_device(None)
    assert not L.covt_device_plan_simplified_geometry_descs_device(None)
    assert L.covt_device_plan_simplify_copy(None, None, None) == I
    assert L.covt_device_plan_simplify(None, None, None, None, 0, None, None, None, None) == I
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        assert L.covt_plan_simplify_bytes(h) > 0 and L.covt_plan_simplify_columns(h, None) == I
        assert L.covt_plan_simplify_descs(h, None) == I and L.covt_plan_simplified_geometry_descs(h, None) == I
        shifts = (C.c_int32 * 1)(3)
        cols = (C.c_int32 * n)()
        assert L.covt_plan_simplify_shifts(h, None, cols) == I and L.covt_plan_simplify_shifts(h, shifts, None) == I
        assert L.covt_plan_simplify_shifts(h, shifts, cols) == 0 and list(cols) == [3] * n
        out = (C.c_uint8 * L.covt_plan_simplify_bytes(h))()
        res = (GeomResult * n)()
        tiles = C.cast(buf, C.POINTER(C.c_uint8))
        # a tile past the caller's buffer, a missing output buffer, missing results, missing tiles: all refused
        # before any device work
        assert L.covt_plan_simplify_host(h, tiles, len(tile) - 1, 0, None, out, res) == I
        assert L.covt_plan_simplify_host(h, tiles, len(tile), 0, None, None, res) == I
        assert L.covt_plan_simplify_host(h, tiles, len(tile), 0, None, out, None) == I
        assert L.covt_plan_simplify_host(h, None, len(tile), 0, None, out, res) == I
    finally:
        L.covt_plan_destroy(h)


@pytest.mark.parametrize("shift", [-1, 31, 32, 64, -2 ** 31, 2 ** 31 - 1])
def test_shift_validation(covt, shift):
    """A uniform shift outside [0, 30]: COVT_ERR_INVALID_ARG from the device entry point (before it looks at its
    pointers: 0 columns would otherwise be nothing to do), from the whole-plan call and from set_simplify."""
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    assert L.covt_geometry_simplify_device(None, None, None, None, None, 0, shift, None, None, None, None) == I
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        out = (C.c_uint8 * L.covt_plan_simplify_bytes(h))()
        res = (GeomResult * n)()
        assert L.covt_plan_simplify_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), shift, None, out, res) == I
        assert L.covt_plan_set_simplify(h, 1, shift, None) == I
        assert L.covt_plan_set_simplify(h, 1, 0, (C.c_int32 * 1)(shift)) == I
        assert L.covt_plan_set_simplify(h, 0, shift, None) == 0  # (unsetting reads no shift)
    finally:
        L.covt_plan_destroy(h)
    plan = covt.Plan.from_tiles([tile])
    with pytest.raises(covt.IllegalArgumentException):
        plan.simplify_host(shift)
    with pytest.raises(covt.IllegalArgumentException):
        plan.set_simplify(shift)
    plan.close()


def test_set_simplify_on_and_off(covt):
    L = covt.lib()
    tile = open(TILE, "rb").read()
    h, _ = _plan(L, tile)
    try:
        for s in (0, 4, 30):
            assert L.covt_plan_set_simplify(h, 1, s, None) == 0
        assert L.covt_plan_set_simplify(h, 1, 99, (C.c_int32 * 1)(7)) == 0  # (per-tile shifts: `shift` is not read)
        assert L.covt_plan_set_simplify(h, 0, 0, None) == 0 and L.covt_plan_set_simplify(h, 0, 0, None) == 0
    finally:
        L.covt_plan_destroy(h)
    plan = covt.Plan.from_tiles([tile, tile])
    plan.set_simplify(4)
    plan.set_simplify([0, 30])
    plan.set_simplify(None)
    with pytest.raises(covt.IllegalArgumentException):
        plan.set_simplify([1, 2, 3])  # one per tile
    ts = plan.simplify_shifts([5, 9])
    assert ts.dtype == np.int32 and ts[plan.geom["desc_index"]].tolist() == [5 if t == 0 else 9 for t in plan.geom["tile"]]
    plan.close()


def test_plan_simplify_layout_on_every_fixture_tile(covt):
    """covt_plan_simplify_columns / _descs: slices in tile order, back to back and 16-byte aligned, sized by the
    geometry column's capacities; each descriptor at its desc_index, the geometry descriptors' order.
    covt_plan_simplified_geometry_descs: the geometry descriptors with out_off[0..3] at the slice's members and
    everything else unchanged."""
    n_cols = 0
    gd_dtype = np.dtype([("in_off", np.int64, 6), ("in_len", np.int32, 6), ("in_res", np.int32, 6),
                         ("out_off", np.int64, 6), ("part_cap", np.int32), ("ring_cap", np.int32),
                         ("coord_cap", np.int32), ("flags", np.int32)])
    assert gd_dtype.itemsize == 160
    for path in tile_paths():
        tile = open(path, "rb").read()
        plan = covt.Plan.from_tiles([tile])
        if int(plan.tile_status[0]):
            continue
        s, d, g = plan.simplify, plan.spdescs, plan.geom
        assert s.dtype == covt.SIMPLIFY_INFO_DTYPE and d.dtype == covt.SIMPLIFY_DESC_DTYPE, tile_key(path)
        gd = np.asarray(plan.gdescs).view(np.uint8).reshape(-1).view(gd_dtype)
        sg = plan.sgdescs.view(gd_dtype)
        assert gd.size == sg.size == plan.num_geometry_columns
        end = 0
        for c in range(plan.num_geometry_columns):
            refused = bool(int(g["flags"][c]) & 0x80000000)
            n, pc, rc, cc = (0, 0, 0, 0) if refused else (int(g[f][c]) for f in ("n_features", "part_cap", "ring_cap", "coord_cap"))
            assert (s["tile"][c], s["layer"][c], s["n_features"][c], s["desc_index"][c]) == \
                (g["tile"][c], g["layer"][c], n, g["desc_index"][c]), (tile_key(path), c)
            assert (int(s["part_cap"][c]), int(s["ring_cap"][c]), int(s["coord_cap"][c])) == (pc, rc, cc)
            assert int(s["flags"][c]) == (covt.SIMPLIFY_TOO_LARGE if refused else 0)
            assert int(s["off"][c]) == end and end % 16 == 0
            m = member_offsets(n, pc, rc, cc)
            end += m[6]
            k = int(s["desc_index"][c])
            assert sg["out_off"][k][:4].tolist() == [int(s["off"][c]) + o for o in m[:4]]
            assert sg["out_off"][k][4:].tolist() == gd["out_off"][k][4:].tolist()
            for f in ("in_off", "in_len", "in_res", "part_cap", "ring_cap", "coord_cap", "flags"):
                assert np.array_equal(sg[f][k], gd[f][k]), (tile_key(path), c, f)
            n_cols += 1
        assert end == plan.simplify_bytes == covt.lib().covt_plan_simplify_bytes(plan._h), tile_key(path)
        for f in ("off", "n_features", "flags", "part_cap", "ring_cap", "coord_cap"):
            assert np.array_equal(d[f][s["desc_index"]], s[f]), (tile_key(path), f)
        assert (d["reserved"] == 0).all()
        plan.close()
    assert n_cols >= 700


def test_simplified_arrays_reads_the_members(covt):
    """Plan.simplified_arrays on a hand-filled buffer: the four arrays are views at the rule's offsets."""
    plan = covt.Plan.from_tiles([open(TILE, "rb").read()])
    c = int(np.argmax(plan.simplify["coord_cap"]))
    q = plan.simplify[c]
    n, o = int(q["n_features"]), int(q["off"])
    m = member_offsets(n, int(q["part_cap"]), int(q["ring_cap"]), int(q["coord_cap"]))
    buf = np.full(plan.simplify_bytes, 0xEE, np.uint8)
    buf[o + m[1]:o + m[1] + 12].view(np.int32)[:] = [0, 1, 2]
    buf[o + m[2]:o + m[2] + 12].view(np.int32)[:] = [0, 2, 3]
    buf[o + m[3]:o + m[3] + 24].view(np.int32)[:] = [1, 2, 3, 4, 5, 6]
    res = np.zeros(plan.num_geometry_columns, covt.GEOM_RESULT_DTYPE)
    res[c] = (0, 2, 2, 3)
    col = plan.simplified_arrays(buf, res, c)
    assert col.geometry_offsets.size == n + 1 and col.part_offsets.tolist() == [0, 1, 2]
    assert col.ring_offsets.tolist() == [0, 2, 3] and col.coords.tolist() == [[1, 2], [3, 4], [5, 6]]
    res[c]["status"] = covt.ERR_TRUNCATED
    with pytest.raises(covt.ArrayIndexOutOfBoundsException):
        plan.simplified_arrays(buf, res, c)
    plan.close()

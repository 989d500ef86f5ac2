"""The measures entry points as a C caller sees them: raw ctypes calls on libcovt.so with caller-owned structs
and buffers, no Python mirror classes (tests/test_capi_bbox.py drives the bounding boxes the same way).  CPU:
struct sizes, argument checks, the plan's layout.  GPU: covt_plan_create -> covt_plan_measures_bytes /
_columns -> covt_plan_measures_host, the values read back with nothing but the header's struct layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import covt_asm as A
import covt_measures as M
from conftest import ROOT


class MeasuresInfo(C.Structure):  # covt_measures_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("n_features", C.c_int32), ("desc_index", C.c_int32),
                ("off", C.c_int64), ("flags", C.c_int32), ("ring_cap", C.c_int32)]


class MeasuresDesc(C.Structure):  # covt_measures_desc
    _fields_ = [("off", C.c_int64), ("n_features", C.c_int32), ("flags", C.c_int32), ("ring_cap", C.c_int32),
                ("reserved", C.c_int32)]


class MeasuresResult(C.Structure):  # covt_measures_result
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32)]


class GeomInfo(C.Structure):  # covt_geom_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("column_type", C.c_int32), ("n_features", C.c_int32),
                ("stream", C.c_int32 * 6), ("part_cap", C.c_int32), ("ring_cap", C.c_int32), ("coord_cap", C.c_int32),
                ("flags", C.c_int32), ("desc_index", C.c_int32), ("reserved", C.c_int32), ("out_off", C.c_int64 * 6)]


TILE = os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt")


def _plan(L, tile):
    buf = (C.c_uint8 * (len(tile) + 4096)).from_buffer_copy(tile + bytes(4096))
    off, size = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(tile))
    h = C.c_void_p()
    assert L.covt_plan_create(C.cast(buf, C.POINTER(C.c_uint8)), off, size, 1, 0, 0, C.byref(h)) == 0
    return h, buf


def _slice_bytes(n, ring_cap):  # include/covt.h "Geometry measures": the three arrays, the count padded, the scratch
    return 16 * n + (4 * n + 15) // 16 * 16 + 16 * ring_cap


def test_struct_sizes_and_bindings(covt):
    assert C.sizeof(MeasuresInfo) == 32 and C.sizeof(MeasuresDesc) == 24 and C.sizeof(MeasuresResult) == 8
    assert covt.MEASURES_INFO_DTYPE.itemsize == 32 and covt.MEASURES_DESC_DTYPE.itemsize == 24
    assert covt.MEASURES_RESULT_DTYPE.itemsize == 8 and covt.MEASURES_TOO_LARGE == 1
    for f, _ in MeasuresInfo._fields_:
        assert covt.MEASURES_INFO_DTYPE.fields[f][1] == getattr(MeasuresInfo, f).offset, f
    for f, _ in MeasuresDesc._fields_:
        assert covt.MEASURES_DESC_DTYPE.fields[f][1] == getattr(MeasuresDesc, f).offset, f
    names = ["covt_plan_measures_bytes", "covt_plan_measures_columns", "covt_plan_measures_descs",
             "covt_geometry_measures_device", "covt_plan_measures_host", "covt_device_plan_measures_bytes",
             "covt_device_plan_measures_descs_device", "covt_device_plan_measures_copy", "covt_device_plan_measures"]
    header = open(os.path.join(ROOT, "include", "covt.h")).read()
    for n in names:
        assert n in covt.EXPORTED_SYMBOLS and n + "(" in header and hasattr(covt.lib(), n), n
    assert "measures" in covt._PRODUCTS


def test_measures_entry_points_check_their_arguments(covt):
    L = covt.lib()
    assert L.covt_plan_measures_bytes(None) == 0
    assert L.covt_plan_measures_columns(None, None) == covt.ERR_INVALID_ARG
    assert L.covt_plan_measures_descs(None, None) == covt.ERR_INVALID_ARG
    assert L.covt_plan_measures_host(None, None, 0, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_measures_device(None, None, None, None, None, -1, None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_measures_device(None, None, None, None, None, 3, None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_measures_device(None, None, None, None, None, 0, None, None, None) == 0  # nothing to do
    assert L.covt_device_plan_measures_bytes(None) == 0 and not L.covt_device_plan_measures_descs_device(None)
    assert L.covt_device_plan_measures_copy(None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_device_plan_measures(None, None, None, None, None, None, None) == covt.ERR_INVALID_ARG
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        assert L.covt_plan_measures_bytes(h) > 0 and L.covt_plan_measures_columns(h, None) == covt.ERR_INVALID_ARG
        assert L.covt_plan_measures_descs(h, None) == covt.ERR_INVALID_ARG
        # a tile past the caller's buffer, a missing output buffer, missing results
        out = (C.c_uint8 * L.covt_plan_measures_bytes(h))()
        res = (MeasuresResult * n)()
        tiles = C.cast(buf, C.POINTER(C.c_uint8))
        assert L.covt_plan_measures_host(h, tiles, len(tile) - 1, out, res) == covt.ERR_INVALID_ARG
        assert L.covt_plan_measures_host(h, tiles, len(tile), None, res) == covt.ERR_INVALID_ARG
        assert L.covt_plan_measures_host(h, tiles, len(tile), out, None) == covt.ERR_INVALID_ARG
        assert L.covt_plan_measures_host(h, None, len(tile), out, res) == covt.ERR_INVALID_ARG
    finally:
        L.covt_plan_destroy(h)


def test_plan_measures_layout(covt):
    """covt_plan_measures_columns / _descs on omt/5_16_20: slices in tile order, back to back and 16-byte
    aligned, sized from n_features and the geometry column's ring_cap; each descriptor at its desc_index."""
    L = covt.lib()
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        info, descs, ginfo = (MeasuresInfo * n)(), (MeasuresDesc * n)(), (GeomInfo * n)()
        assert n > 0 and L.covt_plan_measures_columns(h, info) == 0 and L.covt_plan_measures_descs(h, descs) == 0
        assert L.covt_plan_geometry_columns(h, ginfo) == 0
        end = 0
        for c in range(n):
            m, g, d = info[c], ginfo[c], descs[info[c].desc_index]
            assert (m.tile, m.layer, m.n_features, m.desc_index, m.ring_cap) == (g.tile, g.layer, g.n_features,
                                                                                 g.desc_index, g.ring_cap)
            assert m.off == (end + 15) // 16 * 16 and m.flags == 0
            assert (d.off, d.n_features, d.flags, d.ring_cap, d.reserved) == (m.off, m.n_features, 0, m.ring_cap, 0)
            end = m.off + _slice_bytes(m.n_features, m.ring_cap)
        assert end <= L.covt_plan_measures_bytes(h) <= end + 15
        assert sorted(info[c].desc_index for c in range(n)) == list(range(n))
    finally:
        L.covt_plan_destroy(h)
    # the same through the Python plan, and a column read out of a buffer: three views of n values each
    plan = covt.Plan.from_tiles([tile])
    assert plan.measures.dtype == covt.MEASURES_INFO_DTYPE and plan.mdescs.dtype == covt.MEASURES_DESC_DTYPE
    assert plan.measures_bytes == L.covt_plan_measures_bytes(plan._h)
    assert np.array_equal(plan.measures["ring_cap"], plan.geom["ring_cap"])
    for f in ("off", "n_features", "flags", "ring_cap"):
        assert np.array_equal(plan.mdescs[f][plan.measures["desc_index"]], plan.measures[f]), f
    bufn = np.arange(plan.measures_bytes, dtype=np.uint64).astype(np.uint8)
    c = int(np.argmax(plan.measures["n_features"]))
    col = plan.measures_column(bufn, np.zeros(plan.num_geometry_columns, dtype=covt.MEASURES_RESULT_DTYPE), c)
    k, o = int(plan.measures["n_features"][c]), int(plan.measures["off"][c])
    assert len(col) == k > 0 and col.area.dtype == col.length.dtype == np.float64 and col.num_coords.dtype == np.int32
    assert col.area.tobytes() == bufn[o:o + 8 * k].tobytes() and col.length.tobytes() == bufn[o + 8 * k:o + 16 * k].tobytes()
    assert col.num_coords.tobytes() == bufn[o + 16 * k:o + 20 * k].tobytes()


@pytest.mark.gpu
def test_c_caller_reads_measures(covt, oracle, gpu_available):
    L = covt.lib()
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        info = (MeasuresInfo * n)()
        assert n > 0 and L.covt_plan_measures_columns(h, info) == 0
        out = (C.c_uint8 * L.covt_plan_measures_bytes(h))()
        res = (MeasuresResult * n)()
        assert L.covt_plan_measures_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), out, res) == 0
        raw = bytes(out)
        cols = A.oracle_tile_columns(oracle, tile)
        for c in range(n):
            m, r = info[c], res[c]
            oc = cols[m.layer]
            assert r.status == 0 and m.tile == 0 and m.n_features == oc["types"].size
            k = m.n_features
            got = (np.frombuffer(raw, "<f8", k, m.off), np.frombuffer(raw, "<f8", k, m.off + 8 * k),
                   np.frombuffer(raw, "<i4", k, m.off + 16 * k))
            ref = M.measures_plain(oc["types"], *oc["asm"][1:])
            assert M.same(got, ref, M.segments(*oc["asm"][1:4])), m.layer
    finally:
        L.covt_plan_destroy(h)

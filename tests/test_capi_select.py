"""The select entry points as a C caller sees them: raw ctypes calls on libcovt.so with caller-owned structs and
buffers (tests/test_capi_measures.py drives the measures the same way).  CPU only: struct sizes, exported and
bound symbols, the plan's layout on every fixture tile against the rule written out here, null and negative
arguments, the predicate's validation."""
import ctypes as C
import os

import numpy as np
import pytest

import covt_select as S
from conftest import ROOT, tile_key, tile_paths


class SelectInfo(C.Structure):  # covt_select_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("n_features", C.c_int32), ("desc_index", C.c_int32),
                ("off", C.c_int64), ("byte_cap", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32)]


class SelectDesc(C.Structure):  # covt_select_desc
    _fields_ = [("off", C.c_int64), ("byte_cap", C.c_int64), ("n_features", C.c_int32), ("flags", C.c_int32)]


class SelectResult(C.Structure):  # covt_select_result
    _fields_ = [("status", C.c_int32), ("n_selected", C.c_int32), ("n_bytes", C.c_int64)]


class SelectPred(C.Structure):  # covt_select_pred
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_double * 4), ("min_area", C.c_double),
                ("min_length", C.c_double)]


TILE = os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt")
NAMES = ["covt_select_pred_init", "covt_plan_select_bytes", "covt_plan_select_columns", "covt_plan_select_descs",
         "covt_select_predicate_device", "covt_geometry_select_device", "covt_plan_select_host",
         "covt_device_plan_select_bytes", "covt_device_plan_select_descs_device", "covt_device_plan_select_copy",
         "covt_device_plan_select"]


def _plan(L, tile):
    buf = (C.c_uint8 * (len(tile) + 4096)).from_buffer_copy(tile + bytes(4096))
    off, size = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(tile))
    h = C.c_void_p()
    assert L.covt_plan_create(C.cast(buf, C.POINTER(C.c_uint8)), off, size, 1, 0, 0, C.byref(h)) == 0
    return h, buf


def test_struct_sizes_and_bindings(covt):
    assert C.sizeof(SelectInfo) == 40 and C.sizeof(SelectDesc) == 24 and C.sizeof(SelectResult) == 16
    assert C.sizeof(SelectPred) == 56 and C.sizeof(covt.SelectPred) == 56
    assert covt.SELECT_INFO_DTYPE.itemsize == 40 and covt.SELECT_DESC_DTYPE.itemsize == 24
    assert covt.SELECT_RESULT_DTYPE.itemsize == 16 and covt.SELECT_TOO_LARGE == 1
    assert (covt.SELECT_WINDOW, covt.SELECT_MIN_SIZE, covt.SELECT_KEEP_EMPTY) == (S.WINDOW, S.MIN_SIZE, S.KEEP_EMPTY) == (1, 2, 4)
    for struct, dtype in ((SelectInfo, covt.SELECT_INFO_DTYPE), (SelectDesc, covt.SELECT_DESC_DTYPE),
                          (SelectResult, covt.SELECT_RESULT_DTYPE)):
        for f, _ in struct._fields_:
            assert dtype.fields[f][1] == getattr(struct, f).offset, f
    for f, _ in SelectPred._fields_:
        assert getattr(covt.SelectPred, f).offset == getattr(SelectPred, f).offset, f
    header = open(os.path.join(ROOT, "include", "covt.h")).read()
    for n in NAMES:
        assert n in covt.EXPORTED_SYMBOLS and n + "(" in header and hasattr(covt.lib(), n), n
    assert "select" in covt._PRODUCTS and "Feature selection" in header
    for flag in ("COVT_SELECT_TOO_LARGE", "COVT_SELECT_WINDOW", "COVT_SELECT_MIN_SIZE", "COVT_SELECT_KEEP_EMPTY"):
        assert "#define " + flag in header


def test_pred_init_and_python_pred(covt):
    L = covt.lib()
    p = SelectPred()
    C.memset(C.byref(p), 0xEE, C.sizeof(p))
    L.covt_select_pred_init(C.byref(p))
    assert (p.size, p.flags, list(p.window), p.min_area, p.min_length) == (56, 0, [0.0] * 4, 0.0, 0.0)
    L.covt_select_pred_init(None)  # (ignored)
    q = covt.SelectPred()
    assert (q.size, q.flags) == (56, 0)
    q = covt.SelectPred(window=(1, 2, 3, 4), min_area=4.0, keep_empty=True)
    assert q.flags == 7 and list(q.window) == [1.0, 2.0, 3.0, 4.0] and q.min_area == 4.0 and q.min_length == np.inf
    q = covt.SelectPred(min_length=8)
    assert q.flags == covt.SELECT_MIN_SIZE and q.min_area == np.inf and q.min_length == 8.0


def test_select_entry_points_check_their_arguments(covt):
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    pred = SelectPred()
    L.covt_select_pred_init(C.byref(pred))
    assert L.covt_plan_select_bytes(None) == 0
    assert L.covt_plan_select_columns(None, None) == I and L.covt_plan_select_descs(None, None) == I
    assert L.covt_plan_select_host(None, None, 0, 0, None, C.byref(pred), None, None) == I
    assert L.covt_geometry_select_device(None, None, None, None, -1, None, None, None) == I
    assert L.covt_geometry_select_device(None, None, None, None, 3, None, None, None) == I
    assert L.covt_geometry_select_device(None, None, None, None, 0, None, None, None) == 0  # nothing to do
    assert L.covt_select_predicate_device(None, None, None, None, None, None, None, -1, C.byref(pred), None, None) == I
    assert L.covt_select_predicate_device(None, None, None, None, None, None, None, 3, C.byref(pred), None, None) == I
    assert L.covt_select_predicate_device(None, None, None, None, None, None, None, 0, C.byref(pred), None, None) == 0
    assert L.covt_select_predicate_device(None, None, None, None, None, None, None, 0, None, None, None) == I
    assert L.covt_device_plan_select_bytes(None) == 0 and not L.covt_device_plan_select_descs_device(None)
    assert L.covt_device_plan_select_copy(None, None, None) == I
    assert L.covt_device_plan_select(None, None, None, None, None, None) == I
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        assert L.covt_plan_select_bytes(h) > 0 and L.covt_plan_select_columns(h, None) == I
        assert L.covt_plan_select_descs(h, None) == I
        out = (C.c_uint8 * L.covt_plan_select_bytes(h))()
        res = (SelectResult * n)()
        tiles = C.cast(buf, C.POINTER(C.c_uint8))
        # a tile past the caller's buffer, a missing output buffer, missing results, tiles, predicate, an unknown
        # CRS, a CRS without the tiles' addresses: all refused before any device work
        assert L.covt_plan_select_host(h, tiles, len(tile) - 1, 0, None, C.byref(pred), out, res) == I
        assert L.covt_plan_select_host(h, tiles, len(tile), 0, None, C.byref(pred), None, res) == I
        assert L.covt_plan_select_host(h, tiles, len(tile), 0, None, C.byref(pred), out, None) == I
        assert L.covt_plan_select_host(h, None, len(tile), 0, None, C.byref(pred), out, res) == I
        assert L.covt_plan_select_host(h, tiles, len(tile), 0, None, None, out, res) == I
        assert L.covt_plan_select_host(h, tiles, len(tile), 7, None, C.byref(pred), out, res) == I
        assert L.covt_plan_select_host(h, tiles, len(tile), covt.CRS_CRS84, None, C.byref(pred), out, res) == I
    finally:
        L.covt_plan_destroy(h)


def _bad_preds(L):
    def fresh():
        p = SelectPred()
        L.covt_select_pred_init(C.byref(p))
        return p

    nan = float("nan")
    for k in range(4):
        p = fresh()
        p.flags = S.WINDOW
        p.window[k] = nan
        yield "window[%d] NaN" % k, p
    for f in ("min_area", "min_length"):
        p = fresh()
        setattr(p, f, nan)  # (refused whether or not the flag asks for the field)
        yield f + " NaN", p
    for size in (0, 48, 55, 57, 64):
        p = fresh()
        p.size = size
        yield "size %d" % size, p
    for bit in (0x8, 0x10, 0x80000000):
        p = fresh()
        p.flags = S.WINDOW | bit
        yield "flag %#x" % bit, p


def test_predicate_validation(covt):
    """A NaN in window or min_*, a wrong size, an unknown flag bit: COVT_ERR_INVALID_ARG from the device entry point
    (before it looks at its pointers: 0 columns would otherwise be nothing to do) and from the whole-plan call."""
    L = covt.lib()
    tile = open(TILE, "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        out = (C.c_uint8 * L.covt_plan_select_bytes(h))()
        res = (SelectResult * n)()
        tiles = C.cast(buf, C.POINTER(C.c_uint8))
        seen = 0
        for what, p in _bad_preds(L):
            assert L.covt_select_predicate_device(None, None, None, None, None, None, None, 0, C.byref(p), None,
                                                  None) == covt.ERR_INVALID_ARG, what
            assert L.covt_plan_select_host(h, tiles, len(tile), 0, None, C.byref(p), out, res) == covt.ERR_INVALID_ARG, what
            seen += 1
        assert seen == 14
        ok = SelectPred()
        L.covt_select_pred_init(C.byref(ok))
        ok.flags = 7
        ok.window[:] = [float("-inf"), -1.0, float("inf"), 1.0]  # infinities are values
        assert L.covt_select_predicate_device(None, None, None, None, None, None, None, 0, C.byref(ok), None, None) == 0
    finally:
        L.covt_plan_destroy(h)
    plan = covt.Plan.from_tiles([tile])
    bad = covt.SelectPred(window=(0, 0, float("nan"), 1))
    with pytest.raises(covt.IllegalArgumentException):
        plan.select_host(bad)


def _wkb_capacity(g):  # include/covt.h "Geometry as WKB"
    return 9 * (int(g["n_features"]) + int(g["part_cap"])) + 4 * int(g["ring_cap"]) + 16 * int(g["coord_cap"])


def test_plan_select_layout_on_every_fixture_tile(covt):
    """covt_plan_select_columns / _descs: slices in tile order, back to back and 16-byte aligned, mask | sel |
    offsets | bytes with every member padded to 16 bytes, byte_cap the WKB column's; each descriptor at its
    desc_index, the geometry descriptors' order."""
    n_cols = 0
    for path in tile_paths():
        tile = open(path, "rb").read()
        plan = covt.Plan.from_tiles([tile])
        if int(plan.tile_status[0]):
            continue
        s, d, g, w = plan.select, plan.sdescs, plan.geom, plan.wkb
        assert s.dtype == covt.SELECT_INFO_DTYPE and d.dtype == covt.SELECT_DESC_DTYPE, tile_key(path)
        end = 0
        for c in range(plan.num_geometry_columns):
            refused = bool(int(w["flags"][c]) & covt.WKB_TOO_LARGE)
            n = 0 if refused else int(g["n_features"][c])
            assert (s["tile"][c], s["layer"][c], s["n_features"][c], s["desc_index"][c]) == \
                (g["tile"][c], g["layer"][c], n, g["desc_index"][c]), (tile_key(path), c)
            assert int(s["byte_cap"][c]) == int(w["byte_cap"][c]) == (0 if refused else _wkb_capacity(g[c]))
            assert int(s["flags"][c]) == (covt.SELECT_TOO_LARGE if refused else 0)
            assert int(s["reserved"][c]) == 0 and int(s["off"][c]) == S.a16(end)
            end = int(s["off"][c]) + S.member_offsets(n)[3] + int(s["byte_cap"][c])
            n_cols += 1
        assert end <= plan.select_bytes <= end + 15, tile_key(path)
        for f in ("off", "byte_cap", "n_features", "flags"):
            assert np.array_equal(d[f][s["desc_index"]], s[f]), (tile_key(path), f)
        assert sorted(s["desc_index"].tolist()) == list(range(plan.num_geometry_columns))
        assert plan.select_bytes == covt.lib().covt_plan_select_bytes(plan._h)
        plan.close()
    assert n_cols >= 700


def test_select_column_reads_the_members(covt):
    """Plan.select_column on a hand-filled buffer: index and the WKB column are views at the rule's offsets."""
    plan = covt.Plan.from_tiles([open(TILE, "rb").read()])
    c = int(np.argmax(plan.select["n_features"]))
    n, o = int(plan.select["n_features"][c]), int(plan.select["off"][c])
    assert n >= 3
    _, m_sel, m_off, m_bytes = S.member_offsets(n)
    buf = np.full(plan.select_bytes, 0xEE, np.uint8)
    buf[o + m_sel:o + m_sel + 8].view(np.int32)[:] = [1, n - 1]
    buf[o + m_off:o + m_off + 12].view(np.int32)[:] = [0, 2, 5]
    buf[o + m_bytes:o + m_bytes + 5] = [9, 8, 7, 6, 5]
    res = np.zeros(plan.num_geometry_columns, covt.SELECT_RESULT_DTYPE)
    res[c] = (0, 2, 5)
    col = plan.select_column(buf, res, c)
    assert len(col) == 2 and col.index.dtype == np.int32 and col.index.tolist() == [1, n - 1]
    assert len(col.wkb) == 2 and col.wkb.feature(0) == bytes([9, 8]) and col.wkb.feature(1) == bytes([7, 6, 5])
    res[c]["status"] = covt.ERR_TRUNCATED
    with pytest.raises(covt.ArrayIndexOutOfBoundsException):
        plan.select_column(buf, res, c)
    empty = plan.select_column(buf, np.zeros(plan.num_geometry_columns, covt.SELECT_RESULT_DTYPE), c)
    assert len(empty) == 0 and len(empty.wkb) == 0 and empty.wkb.offsets.tolist() == [0] and empty.wkb.data.size == 0

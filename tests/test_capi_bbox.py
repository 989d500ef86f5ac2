"""The bounding-box entry points as a C caller sees them: raw ctypes calls on libcovt.so with caller-owned
structs and buffers, no Python mirror classes (tests/test_capi.py drives the C-ABI the same way).  CPU:
argument checks.  GPU: covt_plan_create -> covt_plan_bbox_bytes / _columns -> covt_plan_bbox_host, the values
read back with nothing but the header's struct layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import covt_asm as A
import covt_bbox as B
from conftest import ROOT


class BboxInfo(C.Structure):  # covt_bbox_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("n_features", C.c_int32), ("desc_index", C.c_int32),
                ("off", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32)]


class BboxDesc(C.Structure):  # covt_bbox_desc
    _fields_ = [("off", C.c_int64), ("n_features", C.c_int32), ("flags", C.c_int32)]


class BboxResult(C.Structure):  # covt_bbox_result
    _fields_ = [("status", C.c_int32), ("n_empty", C.c_int32), ("extent", C.c_double * 4)]


def _plan(L, tile):
    buf = (C.c_uint8 * (len(tile) + 4096)).from_buffer_copy(tile + bytes(4096))
    off, size = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(tile))
    h = C.c_void_p()
    assert L.covt_plan_create(C.cast(buf, C.POINTER(C.c_uint8)), off, size, 1, 0, 0, C.byref(h)) == 0
    return h, buf


def test_bbox_entry_points_check_their_arguments(covt):
    assert C.sizeof(BboxInfo) == 32 and C.sizeof(BboxDesc) == 16 and C.sizeof(BboxResult) == 40
    L = covt.lib()
    assert L.covt_plan_bbox_bytes(None) == 0
    assert L.covt_plan_bbox_columns(None, None) == covt.ERR_INVALID_ARG
    assert L.covt_plan_bbox_descs(None, None) == covt.ERR_INVALID_ARG
    assert L.covt_plan_bbox_host(None, None, 0, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_bbox_device(None, None, None, None, -1, None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_bbox_device(None, None, None, None, 3, None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_bbox_device(None, None, None, None, 0, None, None, None) == 0  # nothing to do
    assert L.covt_device_plan_bbox_bytes(None) == 0 and not L.covt_device_plan_bbox_descs_device(None)
    assert L.covt_device_plan_bbox_copy(None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_device_plan_bbox(None, None, None, None, None, None) == covt.ERR_INVALID_ARG
    tile = open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        assert L.covt_plan_bbox_bytes(h) > 0 and L.covt_plan_bbox_columns(h, None) == covt.ERR_INVALID_ARG
        info, descs = (BboxInfo * n)(), (BboxDesc * n)()
        assert L.covt_plan_bbox_columns(h, info) == 0 and L.covt_plan_bbox_descs(h, descs) == 0
        end = 0
        for c in range(n):  # tile order: slices back to back, 16-byte aligned; the descriptor at desc_index
            b, d = info[c], descs[info[c].desc_index]
            assert b.off == (end + 15) // 16 * 16 and (d.off, d.n_features, d.flags) == (b.off, b.n_features, b.flags)
            end = b.off + 32 * b.n_features
        assert end <= L.covt_plan_bbox_bytes(h) <= end + 15
        # a tile past the caller's buffer, a missing output buffer
        out = (C.c_uint8 * L.covt_plan_bbox_bytes(h))()
        res = (BboxResult * n)()
        assert L.covt_plan_bbox_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile) - 1, out, res) == covt.ERR_INVALID_ARG
        assert L.covt_plan_bbox_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), None, res) == covt.ERR_INVALID_ARG
    finally:
        L.covt_plan_destroy(h)


@pytest.mark.gpu
def test_c_caller_reads_bboxes(covt, oracle, gpu_available):
    L = covt.lib()
    tile = open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        info = (BboxInfo * n)()
        assert n > 0 and L.covt_plan_bbox_columns(h, info) == 0
        out = (C.c_uint8 * L.covt_plan_bbox_bytes(h))()
        res = (BboxResult * n)()
        assert L.covt_plan_bbox_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), out, res) == 0
        raw = bytes(out)
        cols = A.oracle_tile_columns(oracle, tile)
        for c in range(n):
            b, r = info[c], res[c]
            oc = cols[b.layer]
            assert r.status == 0 and b.tile == 0 and b.n_features == oc["types"].size
            k = b.n_features
            arrays = [np.frombuffer(raw, "<f8", k, b.off + 8 * k * i) for i in range(4)]
            got = (*arrays, np.array(list(r.extent), dtype=np.float64), r.n_empty)
            assert B.same(got, B.bbox_plain(*oc["asm"][1:])), b.layer
    finally:
        L.covt_plan_destroy(h)

"""The WKB entry points as a C caller sees them: raw ctypes calls on libcovt.so with caller-owned structs
and buffers, no Python mirror classes (tests/test_capi.py drives the C-ABI the same way).  CPU: argument
checks.  GPU: covt_plan_create -> covt_plan_wkb_bytes / _columns -> covt_plan_wkb_host, the values read
back with nothing but the header's struct layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import covt_asm as A
import covt_wkb as W
from conftest import ROOT


class WkbInfo(C.Structure):  # covt_wkb_info
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("n_features", C.c_int32), ("desc_index", C.c_int32),
                ("offsets_off", C.c_int64), ("bytes_off", C.c_int64), ("byte_cap", C.c_int64),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class WkbResult(C.Structure):  # covt_wkb_result
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("n_bytes", C.c_int64)]


def _plan(L, tile):
    buf = (C.c_uint8 * (len(tile) + 4096)).from_buffer_copy(tile + bytes(4096))
    off, size = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(tile))
    h = C.c_void_p()
    assert L.covt_plan_create(C.cast(buf, C.POINTER(C.c_uint8)), off, size, 1, 0, 0, C.byref(h)) == 0
    return h, buf


def test_wkb_entry_points_check_their_arguments(covt):
    L = covt.lib()
    assert L.covt_plan_wkb_bytes(None) == 0
    assert L.covt_plan_wkb_columns(None, None) == covt.ERR_INVALID_ARG
    assert L.covt_plan_wkb_descs(None, None) == covt.ERR_INVALID_ARG
    assert L.covt_plan_wkb_host(None, None, 0, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_wkb_device(None, None, None, None, None, -1, None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_wkb_device(None, None, None, None, None, 3, None, None, None) == covt.ERR_INVALID_ARG
    assert L.covt_geometry_wkb_device(None, None, None, None, None, 0, None, None, None) == 0  # nothing to do
    tile = open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()
    h, buf = _plan(L, tile)
    try:
        assert L.covt_plan_wkb_bytes(h) > 0 and L.covt_plan_wkb_columns(h, None) == covt.ERR_INVALID_ARG
        # a tile past the caller's buffer, a missing output buffer
        out = (C.c_uint8 * L.covt_plan_wkb_bytes(h))()
        res = (WkbResult * L.covt_plan_num_geometry_columns(h))()
        assert L.covt_plan_wkb_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile) - 1, out, res) == covt.ERR_INVALID_ARG
        assert L.covt_plan_wkb_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), None, res) == covt.ERR_INVALID_ARG
    finally:
        L.covt_plan_destroy(h)


@pytest.mark.gpu
def test_c_caller_reads_wkb(covt, oracle, gpu_available):
    L = covt.lib()
    tile = open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()
    h, buf = _plan(L, tile)
    try:
        n = L.covt_plan_num_geometry_columns(h)
        info = (WkbInfo * n)()
        assert n > 0 and L.covt_plan_wkb_columns(h, info) == 0
        out = (C.c_uint8 * L.covt_plan_wkb_bytes(h))()
        res = (WkbResult * n)()
        assert L.covt_plan_wkb_host(h, C.cast(buf, C.POINTER(C.c_uint8)), len(tile), out, res) == 0
        raw = bytes(out)
        cols = A.oracle_tile_columns(oracle, tile)
        for c in range(n):
            w, r = info[c], res[c]
            oc = cols[w.layer]
            assert r.status == 0 and w.tile == 0 and w.n_features == oc["types"].size
            offs = np.frombuffer(raw, "<i4", w.n_features + 1, w.offsets_off)
            assert offs[0] == 0 and offs[-1] == r.n_bytes <= w.byte_cap
            feats = [W.parse(raw[w.bytes_off + offs[i]:w.bytes_off + offs[i + 1]], unclose=True)
                     for i in range(w.n_features)]
            assert feats == A.to_features(oc["types"], *oc["asm"][1:]), w.layer
    finally:
        L.covt_plan_destroy(h)

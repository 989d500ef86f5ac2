"""The query entry points as a C caller sees them (include/covt.h "Geometry queries"): raw ctypes calls on
libcovt.so.  CPU only: the struct's size and field offsets, exported and bound symbols, covt_select_query_init,
every refusal of the argument rule, null and negative arguments of the device and host entry points -- all
refused before any device work -- and the Python SelectQuery."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["covt_select_query_init", "covt_select_query_device", "covt_plan_select_query_host"]
TILE = os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt")


class Query(C.Structure):  # covt_select_query as the header spells it
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("relation", C.c_int32), ("reserved", C.c_int32),
                ("window", C.c_int32 * 4)]


def _new(L):
    q = Query()
    C.memset(C.byref(q), 0xEE, C.sizeof(q))
    L.covt_select_query_init(C.byref(q))
    return q


def test_struct_size_offsets_and_bindings(covt):
    assert C.sizeof(Query) == C.sizeof(covt.SelectQuery) == 32
    assert [(f, getattr(Query, f).offset) for f, _ in Query._fields_] == [
        ("size", 0), ("flags", 4), ("relation", 8), ("reserved", 12), ("window", 16)]
    for f, _ in Query._fields_:
        assert getattr(Query, f).offset == getattr(covt.SelectQuery, f).offset, f
    header = open(os.path.join(ROOT, "include", "covt.h")).read()
    for n in NAMES:
        assert n in covt.EXPORTED_SYMBOLS and n + "(" in header and hasattr(covt.lib(), n), n
    assert header.index("Property predicates") < header.index("Geometry queries") < header.index("Device-side plan")
    assert covt.QUERY_INTERSECTS == 0 and covt.QUERY_WITHIN == 1
    assert "#define COVT_QUERY_INTERSECTS 0" in header and "#define COVT_QUERY_WITHIN 1" in header
    assert "csrc/covt_query.hip" in covt._BUILD_SOURCES and "csrc/covt_query_plan.h" in covt._BUILD_SOURCES
    mk = open(os.path.join(ROOT, "cov-tiles_amd", "Makefile")).read()
    assert "csrc/covt_query.hip" in mk and "csrc/covt_query_plan.h" in mk
    assert covt.version().endswith(covt.source_build_id())


def test_query_init(covt):
    L = covt.lib()
    q = _new(L)
    assert (q.size, q.flags, q.relation, q.reserved, tuple(q.window)) == (32, 0, 0, 0, (0, 0, 0, 0))
    L.covt_select_query_init(None)  # (ignored)


def _device(L, q, mode=0, n=1, ptrs=(16,) * 6, status=None):
    dec, gdesc, asm, gres, sdesc, sel = ptrs
    return L.covt_select_query_device(dec, gdesc, asm, gres, sdesc, n, C.byref(q) if q is not None else None, mode, sel,
                                      status, None)


def test_argument_rule(covt):
    """A wrong size, a nonzero flags, a nonzero reserved, an unknown relation, an unknown mode: each refused by
    the device call and by the host call, before any device work (the pointers are not dereferenced)."""
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    tile = open(TILE, "rb").read()
    plan = covt.Plan.from_tiles([tile])
    blob = plan.blob.ctypes.data_as(C.POINTER(C.c_uint8))
    sel = np.zeros(max(plan.select_bytes, 1), np.uint8)
    res = np.zeros(max(plan.num_geometry_columns, 1), covt.SELECT_RESULT_DTYPE)
    g = L.covt_plan_select_query_host

    def host(q):
        return g(plan._h, blob, plan.blob.size, 0, None, None, None, C.byref(q), sel.ctypes.data, res.ctypes.data, None, None)

    for field, values in (("size", (0, 31, 33, 56)), ("flags", (1, 0x80000000)), ("reserved", (1, -1)),
                          ("relation", (-1, 2, 1 << 30))):
        for v in values:
            q = _new(L)
            setattr(q, field, v)
            assert _device(L, q) == I, (field, v)
            assert _device(L, q, n=0) == I, (field, v)  # (even with nothing to do)
            assert host(q) == I, (field, v)
    q = _new(L)
    for mode in (-1, 2, 7):
        assert _device(L, q, mode=mode) == I
    # every window is a query: inverted, a point, the whole plane
    for w in ((5, 5, 0, 0), (3, 3, 3, 3), (-2**31, -2**31, 2**31 - 1, 2**31 - 1)):
        q.window = (C.c_int32 * 4)(*w)
        for rel in (0, 1):
            q.relation = rel
            assert _device(L, q, n=0) == 0


def test_null_and_negative_arguments(covt):
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    q = _new(L)
    assert _device(L, q, n=0, ptrs=(None,) * 6) == 0  # nothing to do
    assert _device(L, None, n=0, ptrs=(None,) * 6) == I
    assert _device(L, q, n=-1) == I
    assert _device(L, q, n=2**31) == I
    for k in range(6):
        ptrs = [16] * 6
        ptrs[k] = None
        assert _device(L, q, ptrs=tuple(ptrs)) == I, k
    assert _device(L, q, ptrs=(16, 16, 16, 16, 16, 24)) == I  # the select buffer: 16-byte aligned
    # the whole-plan call
    tile = open(TILE, "rb").read()
    plain = covt.Plan.from_tiles([tile])
    blob = plain.blob.ctypes.data_as(C.POINTER(C.c_uint8))
    n = plain.blob.size
    sel = np.zeros(max(plain.select_bytes, 1), np.uint8)
    res = np.zeros(max(plain.num_geometry_columns, 1), covt.SELECT_RESULT_DTYPE)
    g = L.covt_plan_select_query_host
    pred = covt.SelectPred()
    w = covt.Where(("class", "==", "motorway"))
    qp = C.byref(q)
    assert g(None, blob, n, 0, None, None, None, qp, sel.ctypes.data, res.ctypes.data, None, None) == I
    assert g(plain._h, blob, n, 0, None, None, None, None, sel.ctypes.data, res.ctypes.data, None, None) == I  # no stage
    assert g(plain._h, None, n, 0, None, None, None, qp, sel.ctypes.data, res.ctypes.data, None, None) == I
    assert g(plain._h, blob, n, 7, None, None, None, qp, sel.ctypes.data, res.ctypes.data, None, None) == I
    assert g(plain._h, blob, n, covt.CRS_CRS84, None, None, None, qp, sel.ctypes.data, res.ctypes.data, None, None) == I
    assert g(plain._h, blob, n, 0, None, None, None, qp, None, res.ctypes.data, None, None) == I
    assert g(plain._h, blob, n, 0, None, None, None, qp, sel.ctypes.data, None, None, None) == I
    # a where needs the property plan; a predicate must be valid
    assert g(plain._h, blob, n, 0, None, None, C.byref(w), qp, sel.ctypes.data, res.ctypes.data, None, None) == I
    pred.flags = 8
    assert g(plain._h, blob, n, 0, None, C.byref(pred), None, qp, sel.ctypes.data, res.ctypes.data, None, None) == I


def test_python_select_query(covt):
    q = covt.SelectQuery((1, -2, 3, 4))
    assert (q.size, q.flags, q.relation, q.reserved, tuple(q.window)) == (32, 0, covt.QUERY_INTERSECTS, 0, (1, -2, 3, 4))
    assert covt.SelectQuery((0, 0, 9, 9), "within").relation == covt.QUERY_WITHIN
    assert covt.SelectQuery((0, 0, 9, 9), relation=covt.QUERY_WITHIN).relation == covt.QUERY_WITHIN
    assert tuple(covt.SelectQuery().window) == (0, 0, 0, 0)
    assert tuple(covt.SelectQuery.at(100, 200).window) == (100, 200, 100, 200)
    at = covt.SelectQuery.at(100, 200, radius=8)
    assert tuple(at.window) == (92, 192, 108, 208) and at.relation == covt.QUERY_INTERSECTS
    assert covt.SelectQuery.at(1, 2, 3, "within").relation == covt.QUERY_WITHIN
    assert tuple(covt.SelectQuery.at(2**31 - 2, -2**31 + 1, 5).window) == (2**31 - 7, -2**31, 2**31 - 1, -2**31 + 6)
    assert bytes(memoryview(q)) == bytes(memoryview(Query(32, 0, 0, 0, (C.c_int32 * 4)(1, -2, 3, 4))))
    for bad in (dict(window=(0, 0, 1)), dict(window=(0, 0, 1, 2**31)), dict(window=(0, 0, 1, 1), relation="touches")):
        with pytest.raises(ValueError):
            covt.SelectQuery(**bad)
    # the plan refuses a call with no stage at all
    plan = covt.Plan.from_tiles([open(TILE, "rb").read()])
    with pytest.raises(ValueError):
        plan.select_host(None, where=covt.Where(("class", "==", "motorway")), query=q)  # (no property plan)

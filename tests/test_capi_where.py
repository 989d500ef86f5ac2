"""The property-predicate entry points as a C caller sees them: raw ctypes calls on libcovt.so with the structs of
tests/covt_where.py.  CPU only: struct sizes and field offsets, exported and bound symbols, the limits of
covt_where_add_clause (a refused add leaves the blob untouched), covt_plan_where_bind on every fixture tile
against a binding computed here from the plan's records, null and wrong arguments, the Python Where."""
import ctypes as C
import os

import numpy as np
import pytest

import covt_where as W
from conftest import ROOT, tile_paths

NAMES = ["covt_where_init", "covt_where_add_clause", "covt_where_valid", "covt_where_bind", "covt_plan_where_bind",
         "covt_where_dict_bound", "covt_select_where_device", "covt_plan_select_where_host"]
TILE = os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt")


def _lits(values):
    arr = (W.Literal * max(len(values), 1))()
    for k, L in enumerate(values):
        arr[k].kinds, arr[k].b, arr[k].i, arr[k].d = L["kinds"], L["b"], L["i"], L["d"]
        if L["kinds"] & W.STRING:
            arr[k].str, arr[k].str_len = L["s"], len(L["s"])
    return arr


def _add(L, w, name, op, flags, values):
    name = name.encode() if isinstance(name, str) else name
    return L.covt_where_add_clause(C.byref(w), name, len(name), op, flags, _lits(values), len(values))


def _refused(L, w, name, op, flags, values):
    before = bytes(memoryview(w))
    assert _add(L, w, name, op, flags, values) == -6
    assert bytes(memoryview(w)) == before


def _new(L):
    w = W.Blob()
    C.memset(C.byref(w), 0xEE, C.sizeof(w))
    L.covt_where_init(C.byref(w))
    return w


def test_struct_sizes_offsets_and_bindings(covt):
    assert (C.sizeof(W.Value), C.sizeof(W.Clause), C.sizeof(W.Blob)) == (32, 32, 2320)
    assert (C.sizeof(covt.WhereValue), C.sizeof(covt.WhereClause), C.sizeof(covt.Where)) == (32, 32, 2320)
    assert C.sizeof(covt.WhereLiteral) == C.sizeof(W.Literal) == 40
    assert [(f, getattr(W.Value, f).offset) for f, _ in W.Value._fields_] == [
        ("i", 0), ("d", 8), ("str_off", 16), ("str_len", 20), ("kinds", 24), ("b", 28)]
    assert [(f, getattr(W.Clause, f).offset) for f, _ in W.Clause._fields_] == [
        ("op", 0), ("flags", 4), ("first_value", 8), ("n_values", 12), ("name_off", 16), ("name_len", 20),
        ("reserved", 24)]
    assert [(f, getattr(W.Blob, f).offset) for f, _ in W.Blob._fields_] == [
        ("size", 0), ("n_clauses", 4), ("n_values", 8), ("text_len", 12), ("clauses", 16), ("values", 272),
        ("text", 1296)]
    for mine, theirs in ((W.Value, covt.WhereValue), (W.Clause, covt.WhereClause), (W.Blob, covt.Where),
                         (W.Literal, covt.WhereLiteral)):
        for f, _ in mine._fields_:
            assert getattr(mine, f).offset == getattr(theirs, f).offset, f
    header = open(os.path.join(ROOT, "include", "covt.h")).read()
    for n in NAMES:
        assert n in covt.EXPORTED_SYMBOLS and n + "(" in header and hasattr(covt.lib(), n), n
    assert "Property predicates" in header
    for name, value in (("MAX_CLAUSES", 8), ("MAX_VALUES", 32), ("MAX_TEXT", 1024), ("MAX_IN", 16), ("EQ", 0), ("NE", 1),
                        ("LT", 2), ("LE", 3), ("GT", 4), ("GE", 5), ("IN", 6), ("NOT_IN", 7), ("IS_NULL", 8),
                        ("NOT_NULL", 9), ("BOOL", 1), ("INT", 2), ("REAL", 4), ("STRING", 8), ("NULL_MATCHES", 1),
                        ("WRITE", 0), ("AND", 1)):
        assert getattr(covt, "WHERE_" + name) == getattr(W, name) == value
        assert "#define COVT_WHERE_" + name + " " in header
    assert "csrc/covt_where.hip" in covt._BUILD_SOURCES and "csrc/covt_where_plan.h" in covt._BUILD_SOURCES
    group, wave = covt.where_dict_bounds()
    assert group >= wave > 0 and group % 64 == 0 and wave % 64 == 0 and covt.lib().covt_where_dict_bound(2) == 0


def test_add_clause_limits(covt):
    L = covt.lib()
    w = _new(L)
    assert (w.size, w.n_clauses, w.n_values, w.text_len) == (2320, 0, 0, 0) and bytes(memoryview(w))[16:] == bytes(2304)
    assert L.covt_where_valid(C.byref(w)) == 1 and L.covt_where_valid(None) == 0
    L.covt_where_init(None)  # (ignored)
    one = [W.lit(1)]
    # the value counts: none for the null tests, exactly one for a comparison, 1 .. 16 for IN
    for op in range(10):
        lo, hi = (0, 0) if op >= W.IS_NULL else (1, 16) if op >= W.IN else (1, 1)
        for n in (0, 1, 2, 16, 17):
            x = _new(L)
            if lo <= n <= hi:
                assert _add(L, x, "c", op, 0, one * n) == 0 and x.n_clauses == 1 and x.n_values == n
            else:
                _refused(L, x, "c", op, 0, one * n)
    # an unknown op or flag, a value without a kind or with an unknown one, a NaN, bad strings
    for op, flags, values in ((-1, 0, one), (10, 0, one), (W.EQ, 2, one), (W.EQ, 0x80000000, one),
                              (W.EQ, 0, [W.lit(kinds=0, i=1)]), (W.EQ, 0, [W.lit(kinds=16, i=1)]),
                              (W.EQ, 0, [W.lit(kinds=W.REAL, d=float("nan"))]),
                              (W.IN, 0, [W.lit(2), W.lit(kinds=W.INT, i=1, d=float("nan"))])):
        _refused(L, w, "c", op, flags, values)
    bad = _lits([W.lit("abc")])
    bad[0].str_len = -1
    assert L.covt_where_add_clause(C.byref(w), b"c", 1, W.EQ, 0, bad, 1) == -6
    bad[0].str, bad[0].str_len = None, 3
    assert L.covt_where_add_clause(C.byref(w), b"c", 1, W.EQ, 0, bad, 1) == -6
    assert L.covt_where_add_clause(C.byref(w), None, 1, W.IS_NULL, 0, None, 0) == -6
    assert L.covt_where_add_clause(C.byref(w), b"c", -1, W.IS_NULL, 0, None, 0) == -6
    assert L.covt_where_add_clause(C.byref(w), b"c", 1, W.EQ, 0, None, 1) == -6
    assert L.covt_where_add_clause(None, b"c", 1, W.IS_NULL, 0, None, 0) == -6
    assert bytes(memoryview(w)) == bytes(memoryview(_new(L)))
    # what an accepted clause writes is make_blob's layout
    clauses = [("class", W.IN, 0, [W.lit("motorway"), W.lit("trunk"), W.lit("")]), ("rank", W.LE, 1, [W.lit(3)]),
               ("name:de", W.IS_NULL, 0, []), ("", W.NE, 0, [W.lit(True)]), ("w", W.EQ, 0, [W.lit(100.0)])]
    for c in clauses:
        assert _add(L, w, *c) == 0
    assert bytes(memoryview(w)) == bytes(memoryview(W.make_blob(clauses))) and L.covt_where_valid(C.byref(w)) == 1
    # a ninth clause
    x = _new(L)
    for _ in range(8):
        assert _add(L, x, "n", W.NOT_NULL, 0, []) == 0
    _refused(L, x, "n", W.NOT_NULL, 0, [])
    # a 33rd value
    x = _new(L)
    assert _add(L, x, "a", W.IN, 0, one * 16) == 0 and _add(L, x, "b", W.NOT_IN, 0, one * 15) == 0
    _refused(L, x, "c", W.IN, 0, one * 2)
    assert _add(L, x, "c", W.EQ, 0, one) == 0 and x.n_values == 32
    _refused(L, x, "d", W.EQ, 0, one)
    # text past 1024 bytes
    x = _new(L)
    assert _add(L, x, "name", W.EQ, 0, [W.lit("x" * 500)]) == 0 and x.text_len == 504
    _refused(L, x, "n", W.EQ, 0, [W.lit("z" * 520)])
    assert _add(L, x, "n", W.EQ, 0, [W.lit("y" * 519)]) == 0 and x.text_len == 1024
    _refused(L, x, "n", W.IS_NULL, 0, [])
    assert _add(L, x, "", W.IS_NULL, 0, []) == 0
    # a blob that is not valid takes no clause
    x = _new(L)
    x.size = 56
    _refused(L, x, "n", W.IS_NULL, 0, [])
    x = W.make_blob(clauses)
    x.values[1].kinds = 0
    assert L.covt_where_valid(C.byref(x)) == 0
    _refused(L, x, "n", W.IS_NULL, 0, [])


def test_python_where(covt):
    w = covt.Where(("class", "in", ["motorway", "trunk"]), ("rank", "<=", 3), ("name:de", "is null"),
                   ("max-text-width", "==", 100.0), ("class", "!=", "motorway", True))
    ref = W.make_blob([("class", W.IN, 0, [W.lit("motorway"), W.lit("trunk")]), ("rank", W.LE, 0, [W.lit(3)]),
                       ("name:de", W.IS_NULL, 0, []), ("max-text-width", W.EQ, 0, [W.lit(100.0)]),
                       ("class", W.NE, W.NULL_MATCHES, [W.lit("motorway")])])
    assert w.tobytes() == bytes(memoryview(ref)) and w.valid()
    kinds = lambda x: covt.Where(("c", "==", x)).values[0].kinds  # noqa: E731
    assert kinds(True) == W.BOOL and kinds(np.bool_(False)) == W.BOOL and kinds(3) == W.INT | W.REAL
    assert kinds(2 ** 53) == W.INT | W.REAL and kinds(2 ** 53 + 1) == W.INT and kinds(np.int64(-7)) == W.INT | W.REAL
    assert kinds(0.5) == W.REAL and kinds(100.0) == W.REAL | W.INT and kinds(float("inf")) == W.REAL
    assert kinds(2.0 ** 63) == W.REAL and kinds(-2.0 ** 63) == W.REAL | W.INT and kinds(np.float32(2.0)) == W.REAL | W.INT
    assert kinds("a") == W.STRING and kinds(b"a") == W.STRING
    for value in (True, 2 ** 53 + 1, -2 ** 63, 0.1, 100.0, "é", b"\x00\xff"):
        v, L = covt.Where(("c", "==", value)).values[0], W.lit(value)
        assert (v.kinds, v.b, v.i, v.d) == (L["kinds"], L["b"], L["i"], L["d"])
    assert covt.Where(("c", "not in", (1, 2, 3))).n_values == 3 and covt.Where(("c", "not null")).n_values == 0
    assert covt.Where().n_clauses == 0 and covt.Where().valid()
    for bad in (("c", "==", float("nan")), ("c", "~", 1), ("c", "==", None), ("c", "==", 2 ** 63), ("c", "<", [1, 2]),
                ("c", "in", []), ("c", "in", list(range(17))), ("c", "is null", 1), ("c", "==", "x" * 1024)):
        with pytest.raises(ValueError):
            covt.Where(bad)
    with pytest.raises(ValueError):
        covt.Where(*[("c", "not null")] * 9)


def _python_bind(plan, names):
    """The bind table from plan.props and plan.property_name: first record in tile order per (tile, layer, name)."""
    first = {}
    for c in range(plan.num_property_columns):
        p = plan.props[c]
        first.setdefault((int(p["tile"]), int(p["layer"]), plan.property_name(c)), int(p["desc_index"]))
    out = np.full((plan.num_geometry_columns, 8), -1, np.int32)
    for g in plan.geom:
        for k, name in enumerate(names):
            out[int(g["desc_index"]), k] = first.get((int(g["tile"]), int(g["layer"]), name), -1)
    return out


def test_plan_where_bind_on_every_fixture_tile(covt):
    tiles = [open(p, "rb").read() for p in tile_paths()]
    plan = covt.Plan.from_tiles(tiles, flags=covt.PLAN_PROPERTIES)
    names = ["class", "rank", "name:de", "max-text-width", "name", "name:", "no such column", "class"]
    w = covt.Where(*[(n, "not null") for n in names])
    got = plan.where_bind(w)
    want = _python_bind(plan, names)
    assert got.shape == want.shape and np.array_equal(got, want)
    bound = (got >= 0).sum(axis=0)
    assert bound[0] > 0 and bound[1] > 0 and bound[2] > 0 and bound[3] > 0 and bound[6] == 0
    assert np.array_equal(got[:, 0], got[:, 7]) and (got < plan.num_property_columns).all()
    # fewer clauses: the unused slots hold -1
    got2 = plan.where_bind(covt.Where(("rank", "<=", 3)))
    assert np.array_equal(got2[:, 0], want[:, 1]) and (got2[:, 1:] == -1).all()
    # covt_where_bind over the same records is the same table; with the names cut off nothing binds
    L = covt.lib()
    out = np.full_like(want, 77)
    blob = plan.blob
    assert L.covt_where_bind(C.byref(w), plan.geom.ctypes.data, plan.geom.size, plan.props.ctypes.data,
                             plan.props.size, blob.ctypes.data_as(C.POINTER(C.c_uint8)), blob.size,
                             out.ctypes.data) == 0
    assert np.array_equal(out, want)
    assert L.covt_where_bind(C.byref(w), plan.geom.ctypes.data, plan.geom.size, plan.props.ctypes.data,
                             plan.props.size, blob.ctypes.data_as(C.POINTER(C.c_uint8)), 0, out.ctypes.data) == 0
    assert (out[:, :4] == -1).all()


def test_where_entry_points_check_their_arguments(covt):
    L = covt.lib()
    I = covt.ERR_INVALID_ARG
    w = covt.Where(("class", "==", "motorway"))
    tile = open(TILE, "rb").read()
    plain = covt.Plan.from_tiles([tile])
    props = covt.Plan.from_tiles([tile], flags=covt.PLAN_PROPERTIES)
    out = np.zeros((max(plain.num_geometry_columns, 1), 8), np.int32)
    blob = props.blob.ctypes.data_as(C.POINTER(C.c_uint8))
    # a plan without properties, null arguments, a blob that is not valid
    assert L.covt_plan_where_bind(plain._h, blob, props.blob.size, C.byref(w), out.ctypes.data) == I
    with pytest.raises(ValueError):
        plain.where_bind(w)
    assert L.covt_plan_where_bind(None, blob, props.blob.size, C.byref(w), out.ctypes.data) == I
    assert L.covt_plan_where_bind(props._h, blob, props.blob.size, None, out.ctypes.data) == I
    assert L.covt_plan_where_bind(props._h, blob, props.blob.size, C.byref(w), None) == I
    assert L.covt_plan_where_bind(props._h, None, props.blob.size, C.byref(w), out.ctypes.data) == I
    assert L.covt_plan_where_bind(props._h, blob, props.blob.size, C.byref(w), out.ctypes.data) == 0
    broken = W.make_blob([("class", W.EQ, 0, [W.lit("motorway")])])
    broken.size = 0
    assert L.covt_plan_where_bind(props._h, blob, props.blob.size, C.byref(broken), out.ctypes.data) == I
    assert L.covt_where_bind(None, None, 0, None, 0, None, 0, None) == I
    assert L.covt_where_bind(C.byref(w), None, 0, None, 0, None, 0, None) == 0
    assert L.covt_where_bind(C.byref(w), None, 1, None, 0, None, 0, out.ctypes.data) == I
    assert L.covt_where_bind(C.byref(w), None, -1, None, 0, None, 0, None) == I
    # the device entry point: counts, mode, null pointers, alignment -- all refused before any device work
    f = L.covt_select_where_device
    assert f(None, None, None, 0, None, 0, None, None, 0, None, None, None) == 0  # nothing to do
    assert f(None, None, None, 0, None, -1, None, None, 0, None, None, None) == I
    assert f(None, None, None, -1, None, 0, None, None, 0, None, None, None) == I
    assert f(None, None, None, 0, None, 0, None, None, 2, None, None, None) == I
    assert f(None, None, None, 0, None, 3, None, None, 0, None, None, None) == I
    assert f(16, 16, 16, 1, 16, 3, None, 16, 0, 16, None, None) == I
    assert f(16, 16, 16, 1, 16, 3, 16, None, 0, 16, None, None) == I
    assert f(None, 16, 16, 1, 16, 3, 16, 16, 0, 16, None, None) == I
    assert f(16, 16, 16, 1, 16, 3, 16, 16, 0, 24, None, None) == I  # the select buffer: 16-byte aligned
    assert f(16, 16, 16, 1, 16, 3, 12, 16, 0, 16, None, None) == I  # the blob: 8-byte aligned
    # the whole-plan call: refused before any device work
    g = L.covt_plan_select_where_host
    sel = np.zeros(max(props.select_bytes, 1), np.uint8)
    res = np.zeros(max(props.num_geometry_columns, 1), covt.SELECT_RESULT_DTYPE)
    pred = covt.SelectPred()
    n = props.blob.size
    assert g(None, blob, n, 0, None, C.byref(pred), C.byref(w), sel.ctypes.data, res.ctypes.data, None) == I
    assert g(plain._h, blob, n, 0, None, C.byref(pred), C.byref(w), sel.ctypes.data, res.ctypes.data, None) == I
    assert g(props._h, blob, n, 0, None, C.byref(pred), None, sel.ctypes.data, res.ctypes.data, None) == I
    assert g(props._h, blob, n, 0, None, C.byref(pred), C.byref(broken), sel.ctypes.data, res.ctypes.data, None) == I
    assert g(props._h, None, n, 0, None, C.byref(pred), C.byref(w), sel.ctypes.data, res.ctypes.data, None) == I
    assert g(props._h, blob, n, 7, None, C.byref(pred), C.byref(w), sel.ctypes.data, res.ctypes.data, None) == I
    assert g(props._h, blob, n, covt.CRS_CRS84, None, None, C.byref(w), sel.ctypes.data, res.ctypes.data, None) == I
    assert g(props._h, blob, n, 0, None, None, C.byref(w), None, res.ctypes.data, None) == I
    assert g(props._h, blob, n, 0, None, None, C.byref(w), sel.ctypes.data, None, None) == I
    pred.flags = 8
    assert g(props._h, blob, n, 0, None, C.byref(pred), C.byref(w), sel.ctypes.data, res.ctypes.data, None) == I

"""covtiles_amd -- MI355X-native COVT Id/Geometry stream decoder (host side).

Python mirror of the reference's decoder API (springmeyer/cov-tiles, evaluation/java,
package ``com.covt.decoder``) over the C-ABI of ``libcovt.so`` (``include/covt.h``):

* ``DecodingUtils`` -- one static method per ``DecodingUtils.java`` method, same names, argument
  order and ``IntWrapper`` cursor semantics; errors raise the Python analogue of the Java exception.
* ``CovtParser.decode_covt`` -- the Id + Geometry part of ``CovtParser.decodeCovt`` for one tile.
* ``Plan`` / ``DeviceBatch`` -- the batch path: host metadata walk -> descriptor table -> one
  GPU launch over every stream of every tile, with device-resident inputs/outputs (torch tensors
  are used as device memory and for the HIP stream; they are plumbing, not the decoder).

The directory name contains a dash, so import it through ``load()`` below or
``importlib`` (``tests/conftest.py`` and ``bench.py`` do).  There is no CPU fallback: if
``libcovt.so`` is missing or no GPU is visible, the decode entry points raise.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, os.environ.get("COVT_LIB_VARIANT", "libcovt.so"))  # tools: libcovt_timing.so

OK = 0
ERR_UNSUPPORTED_ENCODING = -1
ERR_TRUNCATED = -2
ERR_COUNT_MISMATCH = -3
ERR_BAD_HEADER = -4
ERR_DEVICE = -5
ERR_INVALID_ARG = -6
INPUT_PADDING = 4096
FORMAT_GENC, FORMAT_GEND = 0, 1
FAMILY_RLE, FAMILY_VARINT, FAMILY_FASTPFOR, FAMILY_LANE, FAMILY_SPLIT, FAMILY_SPLIT_FPF, FAMILY_SPLIT_RLE = range(7)
NUM_FAMILIES = 7
DESC_LANE, DESC_SPLIT, DESC_SPLIT_PAD, DESC_SPLIT_FPF = 0x1, 0x2, 0x4, 0x8
DESC_SPLIT_RLE = 0x10
SPLIT_SLOTS = 8
ID_FORMAT, ID_JAVA = 0, 1
LAUNCH_AUTO, LAUNCH_FUSED, LAUNCH_FORKED = 0, 1, 2
LAUNCH_FPF_STREAM, LAUNCH_FPF_CLASSIC = 0x4, 0x8  # or-ed in: the FastPFOR family kernel variant (include/covt.h)

(OP_NONE, OP_BYTE_RLE_U8, OP_RLE_U64, OP_RLE_I32, OP_RLE_S64, OP_VARINT_I32, OP_VARINT_ZZ_I32,
 OP_VARINT_ZZ_DELTA_I32, OP_VARINT_ZZ_DELTA_XY, OP_VARINT_DELTA_MORTON, OP_FPF_ZZ_DELTA_I32, OP_FPF_ZZ_DELTA_XY,
 OP_FPF_DELTA_MORTON, OP_VARINT_U64, OP_VARINT_I32_AS_I64, OP_VARINT_ZZ_DELTA_I64, OP_BYTE_RLE_RAW,
 OP_VARINT_ZZ_I32_AS_I64, OP_VARINT_ZZ_S64, OP_VARINT_ZZ_DELTA_S64) = range(20)

# property columns (include/covt.h "Property columns")
PLAN_PROPERTIES = 0x1
RELEASE_PINNED = 0x2  # covt_release_scratch flag: also free blocks pinned by a graph capture
PROP_BOOLEAN, PROP_INT64, PROP_FLOAT, PROP_STRING = 0, 1, 2, 3
PROP_DICT_OWNER, PROP_DENSE_BOOL, PROP_UNSUPPORTED, PROP_DATA_SHORT, PROP_UNSUPPORTED_LATE = 0x1, 0x2, 0x4, 0x8, 0x10

# StreamType ordinals (converter/StreamType.java)
GEOMETRY_TYPES, GEOMETRY_OFFSETS, PART_OFFSETS, RING_OFFSETS, VERTEX_OFFSETS, VERTEX_BUFFER = range(4, 10)


# ---------------------------------------------------------------------------
# Java exception analogues (status -> exception), CovtParser.java:426 etc.
# ---------------------------------------------------------------------------
class CovtError(Exception):
    status = 0


class IllegalArgumentException(CovtError, ValueError):
    pass


class ArrayIndexOutOfBoundsException(CovtError, IndexError):
    pass


class DeviceError(CovtError, RuntimeError):
    pass


def _raise(status: int, what: str):
    if status == OK:
        return
    cls = {ERR_UNSUPPORTED_ENCODING: IllegalArgumentException, ERR_BAD_HEADER: IllegalArgumentException,
           ERR_INVALID_ARG: IllegalArgumentException, ERR_TRUNCATED: ArrayIndexOutOfBoundsException,
           ERR_COUNT_MISMATCH: ArrayIndexOutOfBoundsException}.get(status, DeviceError)
    e = cls("%s failed with status %d" % (what, status))
    e.status = status
    raise e


# ---------------------------------------------------------------------------
# C-ABI binding
# ---------------------------------------------------------------------------
class StreamDesc(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("avail", C.c_int32), ("num_values", C.c_int32),
                ("op", C.c_uint8), ("num_bits", C.c_uint8), ("flags", C.c_uint16), ("byte_length", C.c_int32)]


class StreamResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("consumed", C.c_int32)]


class StreamInfo(C.Structure):
    _fields_ = [("tile", C.c_int32), ("layer", C.c_int32), ("column_kind", C.c_int32), ("stream_type", C.c_int32),
                ("encoding", C.c_int32), ("column_type", C.c_int32), ("num_values", C.c_int32),
                ("byte_length", C.c_int32), ("num_bits", C.c_int32), ("op", C.c_int32), ("elem_bytes", C.c_int32),
                ("desc_index", C.c_int32), ("in_off", C.c_int64), ("out_off", C.c_int64),
                ("out_elems", C.c_int64)]


class GeomDesc(C.Structure):
    _fields_ = [("in_off", C.c_int64 * 6), ("in_len", C.c_int32 * 6), ("in_res", C.c_int32 * 6),
                ("out_off", C.c_int64 * 6), ("part_cap", C.c_int32), ("ring_cap", C.c_int32),
                ("coord_cap", C.c_int32), ("flags", C.c_int32)]


class GeomResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("num_parts", C.c_int32), ("num_rings", C.c_int32),
                ("num_coords", C.c_int32)]


GEOM_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("column_type", np.int32),
                            ("n_features", np.int32), ("stream", np.int32, (6,)), ("part_cap", np.int32),
                            ("ring_cap", np.int32), ("coord_cap", np.int32), ("flags", np.uint32),
                            ("desc_index", np.int32), ("reserved", np.int32), ("out_off", np.int64, (6,))])
GEOM_RESULT_DTYPE = np.dtype([("status", np.int32), ("num_parts", np.int32), ("num_rings", np.int32),
                              ("num_coords", np.int32)])
PROP_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("column", np.int32), ("type", np.int32),
                            ("column_type", np.int32), ("n_features", np.int32), ("n_data", np.int32),
                            ("n_dict", np.int32), ("lang", np.int32), ("name_len", np.int32), ("lang_len", np.int32),
                            ("dict_bytes", np.int32), ("stream", np.int32, (3,)), ("desc_index", np.int32),
                            ("name_off", np.int64), ("lang_off", np.int64), ("out_off", np.int64, (4,))])
PROP_DESC_DTYPE = np.dtype([("present_off", np.int64), ("data_off", np.int64), ("length_off", np.int64),
                            ("dict_in_off", np.int64), ("out_off", np.int64, (4,)), ("res", np.int32, (3,)),
                            ("n_features", np.int32), ("n_data", np.int32), ("n_dict", np.int32),
                            ("dict_bytes", np.int32), ("type", np.int16), ("flags", np.int16)])
PROP_RESULT_DTYPE = np.dtype([("status", np.int32), ("n_valid", np.int32)])
assert PROP_INFO_DTYPE.itemsize == 112 and PROP_DESC_DTYPE.itemsize == 96
GEOM_CLOSED_IN_STREAM = 0x1
GEOM_TOO_LARGE = 0x80000000
GEOM_MAX_CAP = 1 << 25
assert C.sizeof(GeomDesc) == 160 and GEOM_INFO_DTYPE.itemsize == 112
# geometry as WKB (include/covt.h "Geometry as WKB")
WKB_DESC_DTYPE = np.dtype([("offsets_off", np.int64), ("bytes_off", np.int64), ("byte_cap", np.int64),
                           ("n_features", np.int32), ("flags", np.int32)])
WKB_RESULT_DTYPE = np.dtype([("status", np.int32), ("reserved", np.int32), ("n_bytes", np.int64)])
WKB_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("n_features", np.int32),
                           ("desc_index", np.int32), ("offsets_off", np.int64), ("bytes_off", np.int64),
                           ("byte_cap", np.int64), ("flags", np.int32), ("reserved", np.int32)])
WKB_TOO_LARGE = 0x1
assert WKB_DESC_DTYPE.itemsize == 32 and WKB_RESULT_DTYPE.itemsize == 16 and WKB_INFO_DTYPE.itemsize == 48
# geometry bounding boxes (include/covt.h "Geometry bounding boxes")
BBOX_DESC_DTYPE = np.dtype([("off", np.int64), ("n_features", np.int32), ("flags", np.int32)])
BBOX_RESULT_DTYPE = np.dtype([("status", np.int32), ("n_empty", np.int32), ("extent", np.float64, (4,))])
BBOX_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("n_features", np.int32),
                            ("desc_index", np.int32), ("off", np.int64), ("flags", np.int32),
                            ("reserved", np.int32)])
BBOX_TOO_LARGE = 0x1
assert BBOX_DESC_DTYPE.itemsize == 16 and BBOX_RESULT_DTYPE.itemsize == 40 and BBOX_INFO_DTYPE.itemsize == 32
# geometry measures (include/covt.h "Geometry measures")
MEASURES_DESC_DTYPE = np.dtype([("off", np.int64), ("n_features", np.int32), ("flags", np.int32),
                                ("ring_cap", np.int32), ("reserved", np.int32)])
MEASURES_RESULT_DTYPE = np.dtype([("status", np.int32), ("reserved", np.int32)])
MEASURES_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("n_features", np.int32),
                                ("desc_index", np.int32), ("off", np.int64), ("flags", np.int32),
                                ("ring_cap", np.int32)])
MEASURES_TOO_LARGE = 0x1
assert (MEASURES_DESC_DTYPE.itemsize == 24 and MEASURES_RESULT_DTYPE.itemsize == 8
        and MEASURES_INFO_DTYPE.itemsize == 32)
# feature selection (include/covt.h "Feature selection")
SELECT_DESC_DTYPE = np.dtype([("off", np.int64), ("byte_cap", np.int64), ("n_features", np.int32), ("flags", np.int32)])
SELECT_RESULT_DTYPE = np.dtype([("status", np.int32), ("n_selected", np.int32), ("n_bytes", np.int64)])
SELECT_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("n_features", np.int32),
                              ("desc_index", np.int32), ("off", np.int64), ("byte_cap", np.int64),
                              ("flags", np.int32), ("reserved", np.int32)])
SELECT_TOO_LARGE = 0x1
SELECT_WINDOW, SELECT_MIN_SIZE, SELECT_KEEP_EMPTY = 0x1, 0x2, 0x4
assert SELECT_DESC_DTYPE.itemsize == 24 and SELECT_RESULT_DTYPE.itemsize == 16 and SELECT_INFO_DTYPE.itemsize == 40
# geometry simplification (include/covt.h "Geometry simplification")
SIMPLIFY_DESC_DTYPE = np.dtype([("off", np.int64), ("n_features", np.int32), ("flags", np.int32),
                                ("part_cap", np.int32), ("ring_cap", np.int32), ("coord_cap", np.int32),
                                ("reserved", np.int32)])
SIMPLIFY_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("n_features", np.int32),
                                ("desc_index", np.int32), ("off", np.int64), ("flags", np.int32),
                                ("part_cap", np.int32), ("ring_cap", np.int32), ("coord_cap", np.int32)])
SIMPLIFY_TOO_LARGE = 0x1
SIMPLIFY_MAX_SHIFT = 30
assert SIMPLIFY_DESC_DTYPE.itemsize == 32 and SIMPLIFY_INFO_DTYPE.itemsize == 40
# geometry as MVT command streams (include/covt.h "Geometry as MVT")
MVT_DESC_DTYPE = np.dtype([("off", np.int64), ("byte_cap", np.int64), ("n_features", np.int32), ("flags", np.int32),
                           ("ring_cap", np.int32), ("coord_cap", np.int32)])
MVT_RESULT_DTYPE = np.dtype([("status", np.int32), ("n_empty", np.int32), ("n_bytes", np.int64)])
MVT_INFO_DTYPE = np.dtype([("tile", np.int32), ("layer", np.int32), ("n_features", np.int32),
                           ("desc_index", np.int32), ("off", np.int64), ("byte_cap", np.int64), ("flags", np.int32),
                           ("ring_cap", np.int32), ("coord_cap", np.int32), ("reserved", np.int32)])
MVT_TOO_LARGE = 0x1
MVT_ORIENT = 0x1
MVT_MAX_SHIFT = 30
assert MVT_DESC_DTYPE.itemsize == 32 and MVT_INFO_DTYPE.itemsize == 48 and MVT_RESULT_DTYPE.itemsize == 16
# georeferenced geometry (include/covt.h "Georeferenced geometry")
CRS_TILE, CRS_WEB_MERCATOR, CRS_CRS84 = 0, 1, 2
GEO_IDENTITY, GEO_AFFINE, GEO_AFFINE_LAT = 0, 1, 2
GEO_XFORM_DTYPE = np.dtype([("sx", np.float64), ("ox", np.float64), ("sy", np.float64), ("oy", np.float64),
                            ("kind", np.int32), ("reserved", np.int32)])
assert GEO_XFORM_DTYPE.itemsize == 40

class PlanOptions(C.Structure):
    """covt_plan_options (include/covt.h): the plan-layout options.  ``PlanOptions()`` holds the
    library defaults (covt_plan_options_init); keyword arguments override fields, e.g.
    ``PlanOptions(split_min=-1)`` plans no split streams."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("split_min", C.c_int64), ("split_ratio", C.c_int64),
                ("split_chunk", C.c_int64), ("split_values", C.c_int64), ("fpf_split_weight", C.c_int32),
                ("lane_max_bytes", C.c_int32), ("lane_min_streams", C.c_int64), ("plan_threads", C.c_int32),
                ("host_prefault", C.c_int32), ("prefault_threads", C.c_int32), ("device_walk", C.c_int32),
                ("lane_max_values", C.c_int32), ("split_max_streams", C.c_int64),
                ("split_grow", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().covt_plan_options_init(C.byref(self))
        for k, v in kw.items():
            if k not in {f[0] for f in self._fields_} or k == "size":
                raise TypeError("unknown plan option %r" % k)
            setattr(self, k, v)

    def __repr__(self):
        return "PlanOptions(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f, _ in self._fields_[1:])


class SelectPred(C.Structure):
    """covt_select_pred (include/covt.h "Feature selection"): which features a selection keeps.  ``window`` =
    (xmin, ymin, xmax, ymax) in the space of the bounding boxes keeps the features whose box meets it;
    ``min_area`` / ``min_length`` (tile pixels) keep those that reach either, and everything without extent;
    ``keep_empty`` keeps the features without a coordinate.  ``SelectPred()`` keeps every non-empty feature."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_double * 4), ("min_area", C.c_double),
                ("min_length", C.c_double)]

    def __init__(self, window=None, min_area=None, min_length=None, keep_empty: bool = False):
        super().__init__()
        lib().covt_select_pred_init(C.byref(self))
        if window is not None:
            self.flags |= SELECT_WINDOW
            self.window = (C.c_double * 4)(*[float(v) for v in window])
        if min_area is not None or min_length is not None:
            self.flags |= SELECT_MIN_SIZE
            # (a minimum left out never admits a feature: nothing reaches +inf)
            self.min_area = float("inf") if min_area is None else float(min_area)
            self.min_length = float("inf") if min_length is None else float(min_length)
        if keep_empty:
            self.flags |= SELECT_KEEP_EMPTY

    def __repr__(self):
        return "SelectPred(flags=%#x, window=%r, min_area=%r, min_length=%r)" % (
            self.flags, tuple(self.window), self.min_area, self.min_length)


# property predicates (include/covt.h "Property predicates")
WHERE_MAX_CLAUSES, WHERE_MAX_VALUES, WHERE_MAX_TEXT, WHERE_MAX_IN = 8, 32, 1024, 16
(WHERE_EQ, WHERE_NE, WHERE_LT, WHERE_LE, WHERE_GT, WHERE_GE, WHERE_IN, WHERE_NOT_IN, WHERE_IS_NULL,
 WHERE_NOT_NULL) = range(10)
WHERE_BOOL, WHERE_INT, WHERE_REAL, WHERE_STRING = 1, 2, 4, 8
WHERE_NULL_MATCHES = 1
WHERE_WRITE, WHERE_AND = 0, 1
_WHERE_OPS = {"==": WHERE_EQ, "!=": WHERE_NE, "<": WHERE_LT, "<=": WHERE_LE, ">": WHERE_GT, ">=": WHERE_GE,
              "in": WHERE_IN, "not in": WHERE_NOT_IN, "is null": WHERE_IS_NULL, "not null": WHERE_NOT_NULL}


class WhereValue(C.Structure):
    """covt_where_value: one literal of a Where, a value per kind it may be read as."""
    _fields_ = [("i", C.c_int64), ("d", C.c_double), ("str_off", C.c_int32), ("str_len", C.c_int32),
                ("kinds", C.c_uint32), ("b", C.c_int32)]


class WhereClause(C.Structure):
    """covt_where_clause: op, flags, the range of its literals and of its column name."""
    _fields_ = [("op", C.c_int32), ("flags", C.c_uint32), ("first_value", C.c_int32), ("n_values", C.c_int32),
                ("name_off", C.c_int32), ("name_len", C.c_int32), ("reserved", C.c_int32 * 2)]


class WhereLiteral(C.Structure):
    """covt_where_literal: a literal as covt_where_add_clause takes it."""
    _fields_ = [("kinds", C.c_uint32), ("b", C.c_int32), ("i", C.c_int64), ("d", C.c_double), ("str", C.c_char_p),
                ("str_len", C.c_int32), ("reserved", C.c_int32)]


def _where_literal(x) -> WhereLiteral:
    """The literal of a Python value: bool -> BOOL; int -> INT, plus REAL when |x| <= 2^53; float -> REAL (NaN
    raises), plus INT when integral and inside int64; str / bytes -> STRING."""
    L = WhereLiteral()
    if isinstance(x, (bool, np.bool_)):
        L.kinds, L.b = WHERE_BOOL, int(bool(x))
    elif isinstance(x, (int, np.integer)):
        x = int(x)
        if not -(1 << 63) <= x < (1 << 63):
            raise IllegalArgumentException("integer literal %d does not fit int64" % x)
        L.kinds, L.i = WHERE_INT, x
        if abs(x) <= (1 << 53):
            L.kinds |= WHERE_REAL
            L.d = float(x)
    elif isinstance(x, (float, np.floating)):
        x = float(x)
        if x != x:
            raise IllegalArgumentException("a NaN literal compares with nothing")
        L.kinds, L.d = WHERE_REAL, x
        if x.is_integer() and -2.0 ** 63 <= x < 2.0 ** 63:
            L.kinds |= WHERE_INT
            L.i = int(x)
    elif isinstance(x, (str, bytes, bytearray)):
        raw = x.encode("utf-8") if isinstance(x, str) else bytes(x)
        L.kinds, L.str, L.str_len = WHERE_STRING, raw, len(raw)
    else:
        raise IllegalArgumentException("a literal must be a bool, int, float, str or bytes, not %r" % type(x).__name__)
    return L


class MvtOptions(C.Structure):
    """covt_mvt_options (include/covt.h "Geometry as MVT"): orient winds polygon rings as MVT 2.1 asks, shift
    divides the coordinates by 2^shift (a tile of extent E >> shift, after simplify(shift))."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("shift", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, orient: bool = False, shift: int = 0):
        super().__init__(C.sizeof(MvtOptions), MVT_ORIENT if orient else 0, int(shift), 0)


class Where(C.Structure):
    """covt_where (include/covt.h "Property predicates"): a conjunction of clauses over named property columns,
    ``Where(("class", "in", ["motorway", "trunk"]), ("rank", "<=", 3), ("name:de", "is null"))``.  A clause is
    (name, op, value[, null_matches]) with op one of "==" "!=" "<" "<=" ">" ">=" "in" "not in" "is null"
    "not null" (the last two take no value); a name is the column's, plus ':<lang>' for a localized sub-column
    (Plan.property_name).  null_matches: a feature without a value satisfies the clause."""
    _fields_ = [("size", C.c_uint32), ("n_clauses", C.c_uint32), ("n_values", C.c_uint32), ("text_len", C.c_uint32),
                ("clauses", WhereClause * WHERE_MAX_CLAUSES), ("values", WhereValue * WHERE_MAX_VALUES),
                ("text", C.c_uint8 * WHERE_MAX_TEXT)]

    def __init__(self, *clauses):
        super().__init__()
        lib().covt_where_init(C.byref(self))
        for c in clauses:
            self.add(*c)

    def add(self, name, op, value=None, null_matches: bool = False) -> "Where":
        """One more clause (covt_where_add_clause); raises IllegalArgumentException where it refuses."""
        if isinstance(op, str):
            if op not in _WHERE_OPS:
                raise IllegalArgumentException("unknown op %r" % op)
            op = _WHERE_OPS[op]
        if op in (WHERE_IS_NULL, WHERE_NOT_NULL):
            vals = [] if value is None else [value]
        elif op in (WHERE_IN, WHERE_NOT_IN) and not isinstance(value, (str, bytes, bytearray)) and np.ndim(value) == 1:
            vals = list(value)
        elif op in (WHERE_IN, WHERE_NOT_IN) and isinstance(value, (set, frozenset)):
            vals = sorted(value)
        else:
            vals = [value]
        lits = (WhereLiteral * max(len(vals), 1))(*[_where_literal(v) for v in vals])
        raw = name.encode("utf-8") if isinstance(name, str) else bytes(name)
        _raise(lib().covt_where_add_clause(C.byref(self), raw, len(raw), int(op),
                                           WHERE_NULL_MATCHES if null_matches else 0, lits, len(vals)),
               "covt_where_add_clause")
        return self

    def valid(self) -> bool:
        return bool(lib().covt_where_valid(C.byref(self)))

    def tobytes(self) -> bytes:
        return bytes(memoryview(self))

    def __repr__(self):
        return "Where(n_clauses=%d, n_values=%d, text=%r)" % (self.n_clauses, self.n_values,
                                                             bytes(self.text[:self.text_len]))


# geometry queries (include/covt.h "Geometry queries")
QUERY_INTERSECTS, QUERY_WITHIN = 0, 1
_QUERY_RELATIONS = {"intersects": QUERY_INTERSECTS, "within": QUERY_WITHIN}


class SelectQuery(C.Structure):
    """covt_select_query (include/covt.h "Geometry queries"): an exact relation of every feature with a closed,
    axis-aligned int32 window in tile pixels, decided from the coordinates.  ``window`` = (x0, y0, x1, y1);
    ``relation`` "intersects" keeps the features that share a point with the window (a polygon's interior
    counts, its holes do not), "within" those that lie wholly inside it.  ``SelectQuery.at(x, y, radius)`` is
    the point query with a tolerance: what is under this pixel."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("relation", C.c_int32), ("reserved", C.c_int32),
                ("window", C.c_int32 * 4)]

    def __init__(self, window=(0, 0, 0, 0), relation="intersects"):
        super().__init__()
        lib().covt_select_query_init(C.byref(self))
        if isinstance(relation, str):
            if relation not in _QUERY_RELATIONS:
                raise IllegalArgumentException("unknown query relation %r" % (relation,))
            relation = _QUERY_RELATIONS[relation]
        w = [int(v) for v in window]
        if len(w) != 4 or any(v < -2**31 or v > 2**31 - 1 for v in w):
            raise IllegalArgumentException("a query window is four int32: (x0, y0, x1, y1)")
        self.relation = int(relation)
        self.window = (C.c_int32 * 4)(*w)

    @classmethod
    def at(cls, x: int, y: int, radius: int = 0, relation="intersects") -> "SelectQuery":
        """The point (x, y), or with ``radius`` the square of that half-width around it (clamped to int32)."""
        lo, hi = -2**31, 2**31 - 1
        x, y, r = int(x), int(y), int(radius)
        return cls((max(x - r, lo), max(y - r, lo), min(x + r, hi), min(y + r, hi)), relation)

    def __repr__(self):
        return "SelectQuery(window=%r, relation=%d)" % (tuple(self.window), self.relation)


def where_dict_bounds():
    """(workgroup per column, wave per column): the dictionary sizes up to which the where kernel answers a
    STRING clause from a match bitmap in LDS (covt_where_dict_bound)."""
    return int(lib().covt_where_dict_bound(0)), int(lib().covt_where_dict_bound(1))


STREAM_INFO_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in StreamInfo._fields_])
assert STREAM_INFO_DTYPE.itemsize == C.sizeof(StreamInfo)
assert C.sizeof(StreamDesc) == 32

_u8p, _i32p, _i64p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
_vp, _vpp, _sz = C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t
_i32, _i64, _u64, _int = C.c_int32, C.c_int64, C.c_uint64, C.c_int


def _sig(restype, argtypes, *names):
    return {n: (restype, argtypes) for n in names}


# The binding table: every entry point include/covt.h declares -> (restype, argtypes).  lib() applies it;
# a new entry point is one row here.  (argtypes None: left unset, ctypes checks nothing.)
_SIGNATURES = {
    # DecodingUtils mirror
    **_sig(_int, [_u8p, _sz, _i32p, _i32, _i32p], "covt_decode_varint", "covt_decode_zigzag_varint",
           "covt_decode_zigzag_delta_varint", "covt_decode_zigzag_delta_varint_coordinates"),
    "covt_decode_rle": (_int, [_u8p, _sz, _i32, _i32p, _i32, _i64p]),
    "covt_decode_byte_rle": (_int, [_u8p, _sz, _i32, _i32p, _i32, _u8p]),
    **_sig(_int, [_u8p, _sz, _i32, _i32, _i32p, _i32p], "covt_decode_fastpfor_zigzag_delta",
           "covt_decode_fastpfor_delta_coordinates"),
    "covt_decode_delta_varint_morton_codes": (_int, [_u8p, _sz, _i32p, _i32, _i32, _i32p]),
    "covt_decode_fastpfor_delta_morton_codes": (_int, [_u8p, _sz, _i32, _i32, _i32p, _i32, _i32p]),
    "covt_decode_byte_rle_reencode": (_int, [_u8p, _sz, _i32, _i32p, _u8p]),
    "covt_decode_floats_le": (_int, [_u8p, _sz, _i32p, _i32, C.POINTER(C.c_float)]),
    "covt_decode_string": (_int, [_u8p, _sz, _i32p, _i32p, _i32p]),
    "covt_version": (C.c_char_p, None),
    "covt_device_count": (_int, [_i32p]),
    "covt_release_scratch": (_int, [_vp, _int]),
    "covt_scratch_blocks": (_i64, None),
    # host plan
    "covt_plan_create": (_int, [_u8p, _u64p, _u64p, _i32, _i32, _i32, _vpp]),
    "covt_plan_create_ex": (_int, [_u8p, _u64p, _u64p, _i32, _i32, _i32, C.c_uint32, _vpp]),
    "covt_plan_create_opts": (_int, [_u8p, _u64p, _u64p, _i32, _i32, _i32, _vp, _vpp]),
    **_sig(None, [_vp], "covt_plan_options_init", "covt_plan_destroy", "covt_device_plan_destroy"),
    **_sig(_i64, [_vp], "covt_plan_num_streams", "covt_plan_output_bytes", "covt_plan_num_descs",
           "covt_plan_num_geometry_columns", "covt_plan_assembly_bytes", "covt_plan_wkb_bytes", "covt_plan_bbox_bytes",
           "covt_plan_measures_bytes", "covt_plan_select_bytes", "covt_plan_simplify_bytes", "covt_plan_mvt_bytes",
           "covt_plan_num_property_columns", "covt_plan_property_bytes"),
    **_sig(_int, [_vp, _i64p, _i64p, _i64p], "covt_plan_totals", "covt_device_plan_totals"),
    **_sig(_int, [_vp, _vp], "covt_plan_streams", "covt_plan_descs", "covt_plan_geometry_columns",
           "covt_plan_geometry_descs", "covt_plan_wkb_columns", "covt_plan_wkb_descs", "covt_plan_bbox_columns",
           "covt_plan_bbox_descs", "covt_plan_measures_columns", "covt_plan_measures_descs", "covt_plan_select_columns",
           "covt_plan_select_descs", "covt_plan_simplify_columns", "covt_plan_simplify_descs",
           "covt_plan_simplified_geometry_descs", "covt_plan_mvt_columns", "covt_plan_mvt_descs",
           "covt_plan_property_columns", "covt_plan_property_descs"),
    **_sig(_int, [_vp, _i64p], "covt_plan_desc_streams", "covt_plan_family_counts", "covt_device_plan_family_counts"),
    "covt_plan_tile_status": (_int, [_vp, _i32p]),
    "covt_plan_release_device": (_int, [_vp]),
    **_sig(_int, [_vp, _u8p, _u64, _vp, _vp], "covt_plan_decode_host", "covt_plan_assemble_host", "covt_plan_wkb_host",
           "covt_plan_bbox_host", "covt_plan_measures_host", "covt_plan_properties_host"),
    "covt_plan_decode_host_multi": (_int, [_vp, _u8p, _u64, _i32, _vp, _vp]),
    "covt_plan_decode_host_shards": (_int, [_vp, _u8p, _u64, _i32, _i32p, _vp, _vp]),
    # launches over device buffers
    "covt_decode_streams_device": (_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_decode_streams_device_grouped": (_int, [_vp, _vp, _i64p, _vp, _vp, _vp]),
    "covt_decode_streams_device_grouped_mode": (_int, [_vp, _vp, _i64p, _vp, _vp, _vp, _i32]),
    "covt_assemble_geometry_device": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_materialize_properties_device": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_geometry_wkb_device": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_geometry_bbox_device": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_geometry_measures_device": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    # feature selection
    "covt_select_pred_init": (None, [_vp]),
    "covt_select_predicate_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_geometry_select_device": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "covt_plan_select_host": (_int, [_vp, _u8p, _u64, _i32, _vp, _vp, _vp, _vp]),
    # property predicates
    "covt_where_init": (None, [_vp]),
    "covt_where_add_clause": (_int, [_vp, C.c_char_p, _i32, _i32, C.c_uint32, _vp, _i32]),
    "covt_where_valid": (_int, [_vp]),
    "covt_where_bind": (_int, [_vp, _vp, _i64, _vp, _i64, _u8p, _u64, _vp]),
    "covt_plan_where_bind": (_int, [_vp, _u8p, _u64, _vp, _vp]),
    "covt_where_dict_bound": (_i32, [_i32]),
    "covt_select_where_device": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp]),
    "covt_plan_select_where_host": (_int, [_vp, _u8p, _u64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    # geometry queries
    "covt_select_query_init": (None, [_vp]),
    "covt_select_query_device": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "covt_plan_select_query_host": (_int, [_vp, _u8p, _u64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # geometry simplification
    "covt_plan_simplify_shifts": (_int, [_vp, _vp, _vp]),
    "covt_geometry_simplify_device": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "covt_plan_simplify_host": (_int, [_vp, _u8p, _u64, _i32, _vp, _vp, _vp]),
    "covt_plan_set_simplify": (_int, [_vp, _i32, _i32, _vp]),
    "covt_device_plan_simplify": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    # geometry as MVT
    "covt_mvt_options_init": (None, [_vp]),
    "covt_geometry_mvt_device": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "covt_plan_mvt_host": (_int, [_vp, _u8p, _u64, _vp, _vp, _vp]),
    "covt_device_plan_mvt": (_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    # georeferenced geometry
    "covt_geo_transform": (_int, [_i32, _i32, _i32, _i32, _i32, _vp]),
    "covt_plan_geometry_extents": (_int, [_vp, _vp]),
    "covt_plan_geo_transforms": (_int, [_vp, _i32, _vp, _vp, C.POINTER(C.c_uint32)]),
    "covt_geometry_wkb_projected_device": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, C.c_uint32, _vp]),
    "covt_geometry_bbox_projected_device": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, C.c_uint32, _vp]),
    **_sig(_int, [_vp, _u8p, _u64, _i32, _vp, _vp, _vp], "covt_plan_wkb_projected_host",
           "covt_plan_bbox_projected_host"),
    # device plan
    "covt_device_plan_create": (_int, [_vp, _u64, _vp, _vp, _i32, _i32, _i32, _vp, _vpp]),
    "covt_device_plan_create_opts": (_int, [_vp, _u64, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vpp]),
    "covt_device_plan_pool_trim": (_int, [_int, _u64]),
    **_sig(_i64, [_vp], "covt_device_plan_num_streams", "covt_device_plan_num_descs", "covt_device_plan_output_bytes",
           "covt_device_plan_num_geometry_columns", "covt_device_plan_assembly_bytes", "covt_device_plan_wkb_bytes",
           "covt_device_plan_bbox_bytes", "covt_device_plan_measures_bytes", "covt_device_plan_select_bytes",
           "covt_device_plan_simplify_bytes", "covt_device_plan_mvt_bytes", "covt_device_plan_num_property_columns", "covt_device_plan_property_bytes"),
    **_sig(_vp, [_vp], "covt_device_plan_descs_device", "covt_device_plan_streams_device",
           "covt_device_plan_tile_status_device", "covt_device_plan_order_device",
           "covt_device_plan_geometry_descs_device", "covt_device_plan_wkb_descs_device",
           "covt_device_plan_bbox_descs_device", "covt_device_plan_measures_descs_device", "covt_device_plan_select_descs_device",
           "covt_device_plan_simplify_descs_device", "covt_device_plan_simplified_geometry_descs_device",
           "covt_device_plan_mvt_descs_device",
           "covt_device_plan_property_descs_device"),
    "covt_device_plan_copy": (_int, [_vp, _vp, _vp, _i32p]),
    **_sig(_int, [_vp, _vp, _vp], "covt_device_plan_geometry_copy", "covt_device_plan_wkb_copy",
           "covt_device_plan_bbox_copy", "covt_device_plan_measures_copy", "covt_device_plan_select_copy",
           "covt_device_plan_simplify_copy", "covt_device_plan_mvt_copy", "covt_device_plan_property_copy"),
    "covt_device_plan_geometry": (_int, [_vp, _vp]),
    "covt_device_plan_decode": (_int, [_vp, _vp, _vp, _vp, _vp]),
    **_sig(_int, [_vp] * 6, "covt_device_plan_assemble", "covt_device_plan_bbox", "covt_device_plan_select"),
    **_sig(_int, [_vp] * 7, "covt_device_plan_materialize", "covt_device_plan_measures"),
    "covt_device_plan_wkb": (_int, [_vp] * 8),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def release_scratch(stream=None, all: bool = False, pinned: bool = False) -> int:
    """covt_release_scratch: free the small-batch assembly / property scratch of (current device, `stream`),
    or every block with all=True; blocks pinned by a graph capture only with pinned=True (no graph captured
    on them may replay afterwards); returns the number of blocks freed."""
    import torch

    s = stream if stream is not None else (torch.cuda.current_stream() if not all else None)
    flags = (1 if all else 0) | (RELEASE_PINNED if pinned else 0)
    return lib().covt_release_scratch(C.c_void_p(s.cuda_stream if s is not None else 0), flags)


def scratch_blocks() -> int:
    """Scratch blocks held by the small-batch paths (covt_scratch_blocks)."""
    return int(lib().covt_scratch_blocks())


def build(force: bool = False) -> str:
    """Compile libcovt.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", _HERE, "libcovt.so"]
    if force:
        subprocess.check_call(["make", "-s", "-C", _HERE, "clean"])
    subprocess.check_call(args)
    return _LIB


_lib = None


def lib() -> C.CDLL:
    """Load libcovt.so.  torch is imported first so libcovt binds to the same HIP runtime."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  -- shares its libamdhip64 with libcovt (same SONAME)
    except ImportError:
        pass
    if not os.path.exists(_LIB):
        raise ImportError("libcovt.so is not built (run __graft_entry__.build() or make -C cov-tiles_amd)")
    L = C.CDLL(_LIB)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def device_count() -> int:
    n = C.c_int32(0)
    lib().covt_device_count(C.byref(n))
    return n.value


def geo_transform(crs: int, z: int, x: int, y: int, extent: int) -> np.ndarray:
    """covt_geo_transform: the transform of tile z/x/y for a layer of `extent` pixels a side, one
    GEO_XFORM_DTYPE record (include/covt.h "Georeferenced geometry"); raises on an invalid argument."""
    out = np.zeros(1, dtype=GEO_XFORM_DTYPE)
    _raise(lib().covt_geo_transform(crs, z, x, y, extent, out.ctypes.data), "covt_geo_transform")
    return out[0]


def _zxy(tile_zxy, n_tiles: int) -> np.ndarray:
    """z, x, y of every tile as a C-contiguous int32 [n_tiles, 3] array."""
    a = np.ascontiguousarray(tile_zxy, dtype=np.int32).reshape(-1)
    if a.size != 3 * n_tiles:
        raise IllegalArgumentException("tile_zxy must hold z, x, y of each of the %d tiles" % n_tiles)
    return a


def _u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf, dtype=np.uint8)
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t))


# ---------------------------------------------------------------------------
# DecodingUtils mirror (DecodingUtils.java)
# ---------------------------------------------------------------------------
class IntWrapper:
    """me.lemire.integercompression.IntWrapper: the mutable cursor of the Java API."""

    def __init__(self, v: int = 0):
        self.value = int(v)

    def get(self) -> int:
        return self.value

    def set(self, v: int) -> None:
        self.value = int(v)

    def increment(self) -> None:
        self.value += 1

    def add(self, v: int) -> None:
        self.value += int(v)

    def __repr__(self):
        return "IntWrapper(%d)" % self.value


def _cursor(pos):
    return pos if isinstance(pos, IntWrapper) else IntWrapper(pos)


class DecodingUtils:
    """Static methods mirroring com.covt.decoder.DecodingUtils (names, argument order, semantics).
    Every call decodes on the GPU through libcovt."""

    @staticmethod
    def _varint_like(fn, src, pos, n, out_n, what):
        pos = _cursor(pos)
        a = _u8(src)
        out = np.zeros(max(out_n, 1), dtype=np.int32)
        p = C.c_int32(pos.get())
        _raise(getattr(lib(), fn)(_ptr(a, C.c_uint8), a.size, C.byref(p), int(n), _ptr(out, C.c_int32)), what)
        pos.set(p.value)
        return out[:out_n]

    @staticmethod
    def decodeVarint(src, pos: IntWrapper, numValues: int) -> np.ndarray:  # DecodingUtils.java:35
        return DecodingUtils._varint_like("covt_decode_varint", src, pos, numValues, numValues, "decodeVarint")

    @staticmethod
    def decodeZigZagVarint(src, pos: IntWrapper, numValues: int) -> np.ndarray:  # :46
        return DecodingUtils._varint_like("covt_decode_zigzag_varint", src, pos, numValues, numValues,
                                          "decodeZigZagVarint")

    @staticmethod
    def decodeZigZagDeltaVarint(src, pos: IntWrapper, numValues: int) -> np.ndarray:  # :55
        return DecodingUtils._varint_like("covt_decode_zigzag_delta_varint", src, pos, numValues, numValues,
                                          "decodeZigZagDeltaVarint")

    @staticmethod
    def decodeZigZagDeltaVarintCoordinates(src, pos: IntWrapper, numValues: int) -> np.ndarray:  # :95
        return DecodingUtils._varint_like("covt_decode_zigzag_delta_varint_coordinates", src, pos, numValues,
                                          numValues, "decodeZigZagDeltaVarintCoordinates")

    @staticmethod
    def decodeDeltaVarintMortonCodes(src, pos: IntWrapper, numVertices: int, numBits: int) -> np.ndarray:  # :394
        pos = _cursor(pos)
        a = _u8(src)
        out = np.zeros(max(2 * numVertices, 1), dtype=np.int32)
        p = C.c_int32(pos.get())
        _raise(lib().covt_decode_delta_varint_morton_codes(_ptr(a, C.c_uint8), a.size, C.byref(p), numVertices,
                                                           numBits, _ptr(out, C.c_int32)),
               "decodeDeltaVarintMortonCodes")
        pos.set(p.value)
        return out[:2 * numVertices]

    @staticmethod
    def decodeRle(buffer, numValues: int, pos: IntWrapper, signed: bool) -> np.ndarray:  # :257
        pos = _cursor(pos)
        a = _u8(buffer)
        out = np.zeros(max(numValues, 1), dtype=np.int64)
        p = C.c_int32(pos.get())
        _raise(lib().covt_decode_rle(_ptr(a, C.c_uint8), a.size, numValues, C.byref(p), int(bool(signed)),
                                     _ptr(out, C.c_int64)), "decodeRle")
        pos.set(p.value)
        return out[:numValues]

    @staticmethod
    def decodeByteRle(buffer, numValues: int, pos: IntWrapper, byteLength: Optional[int] = None) -> np.ndarray:
        """:275 (with byteLength: advance by it) and the :290 overload (without: advance by the length
        of the values' ORC re-encoding, as CovtParser.java:295 relies on for Gen D present streams)."""
        pos = _cursor(pos)
        a = _u8(buffer)
        out = np.zeros(max(numValues, 1), dtype=np.uint8)
        p = C.c_int32(pos.get())
        if byteLength is None:
            st = lib().covt_decode_byte_rle_reencode(_ptr(a, C.c_uint8), a.size, numValues, C.byref(p),
                                                     _ptr(out, C.c_uint8))
        else:
            st = lib().covt_decode_byte_rle(_ptr(a, C.c_uint8), a.size, numValues, C.byref(p), byteLength,
                                            _ptr(out, C.c_uint8))
        _raise(st, "decodeByteRle")
        pos.set(p.value)
        return out[:numValues]

    @staticmethod
    def decodeFloatsLE(encodedValues, pos: IntWrapper, numValues: int) -> np.ndarray:  # :446
        pos = _cursor(pos)
        a = _u8(encodedValues)
        out = np.zeros(max(numValues, 1), dtype=np.float32)
        p = C.c_int32(pos.get())
        _raise(lib().covt_decode_floats_le(_ptr(a, C.c_uint8), a.size, C.byref(p), numValues,
                                           out.ctypes.data_as(C.POINTER(C.c_float))), "decodeFloatsLE")
        pos.set(p.value)
        return out[:numValues]

    @staticmethod
    def decodeString(content, pos: IntWrapper, numChars: Optional[int] = None) -> str:  # :21 / :28
        pos = _cursor(pos)
        a = _u8(content)
        if numChars is not None:  # :28 -- the caller knows the length
            if pos.get() < 0 or pos.get() + numChars > a.size or numChars < 0:
                _raise(ERR_TRUNCATED, "decodeString")
            s = bytes(a[pos.get():pos.get() + numChars]).decode("utf-8", errors="replace")
            pos.set(pos.get() + numChars)
            return s
        p, off, ln = C.c_int32(pos.get()), C.c_int32(), C.c_int32()
        _raise(lib().covt_decode_string(_ptr(a, C.c_uint8), a.size, C.byref(p), C.byref(off), C.byref(ln)),
               "decodeString")
        pos.set(p.value)
        return bytes(a[off.value:off.value + ln.value]).decode("utf-8", errors="replace")

    @staticmethod
    def _fpf(fn, buf, n, byte_length, pos, out_n, extra, what):
        pos = _cursor(pos)
        a = _u8(buf)
        out = np.zeros(max(out_n, 1), dtype=np.int32)
        p = C.c_int32(pos.get())
        args = [_ptr(a, C.c_uint8), a.size, n, byte_length, C.byref(p)] + extra + [_ptr(out, C.c_int32)]
        _raise(getattr(lib(), fn)(*args), what)
        pos.set(p.value)
        return out[:out_n]

    @staticmethod
    def decodeFastPfor128ZigZagDelta(encodedValues, numValues: int, byteLength: int, pos: IntWrapper):  # :316
        return DecodingUtils._fpf("covt_decode_fastpfor_zigzag_delta", encodedValues, numValues, byteLength, pos,
                                  numValues, [], "decodeFastPfor128ZigZagDelta")

    @staticmethod
    def decodeFastPfor128DeltaCoordinates(encodedValues, numValues: int, byteLength: int, pos: IntWrapper):  # :349
        return DecodingUtils._fpf("covt_decode_fastpfor_delta_coordinates", encodedValues, numValues, byteLength,
                                  pos, numValues, [], "decodeFastPfor128DeltaCoordinates")

    @staticmethod
    def decodeFastPfor128DeltaMortonCodes(encodedValues, numVertices: int, byteLength: int, pos: IntWrapper,
                                          numBits: int):  # :411
        return DecodingUtils._fpf("covt_decode_fastpfor_delta_morton_codes", encodedValues, numVertices,
                                  byteLength, pos, 2 * numVertices, [numBits], "decodeFastPfor128DeltaMortonCodes")


# ---------------------------------------------------------------------------
# Batch path
# ---------------------------------------------------------------------------
def pack_tiles(tiles: List[bytes], align: int = 16):
    """Concatenate tiles (16-byte aligned starts) -> (uint8 blob incl. INPUT_PADDING, offsets, sizes)."""
    sizes = np.array([len(t) for t in tiles], dtype=np.uint64)
    offs = np.zeros(len(tiles), dtype=np.uint64)
    pos = 0
    for i, t in enumerate(tiles):
        offs[i] = pos
        pos += (len(t) + align - 1) // align * align
    blob = np.zeros(pos + INPUT_PADDING, dtype=np.uint8)
    for i, t in enumerate(tiles):
        blob[int(offs[i]):int(offs[i]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return blob, offs, sizes


class _Product(NamedTuple):
    """A per-column product of a plan (assembly, WKB, bounding boxes, properties) as the bindings size,
    allocate and read it back; the first four name attributes Plan and DevicePlan share."""
    count: str  # number of columns
    nbytes: str  # bytes of the product's buffer
    descs: str  # Plan only: descriptors, launch order
    records: str  # Plan only: records, tile order (their desc_index reorders the results)
    info_dtype: np.dtype
    desc_dtype: np.dtype  # (uint8: descriptors kept as bytes)
    desc_size: int
    res_dtype: np.dtype
    res_words: tuple  # a result as torch elements: (dtype name, count)
    zeroed: bool  # the buffer starts zeroed, not uninitialised
    needs_geometry: bool  # DevicePlan: sized only after geometry()
    attrs: tuple  # DeviceBatch attributes: (descriptors, buffer, results)

    def alloc(self, owner, device):
        """(buffer, results) on the device, sized by `owner` (a Plan or DevicePlan)."""
        import torch

        return ((torch.zeros if self.zeroed else torch.empty)(max(getattr(owner, self.nbytes), 16), dtype=torch.uint8,
                                                              device=device),
                torch.zeros(max(getattr(owner, self.count), 1) * self.res_words[1],
                            dtype=getattr(torch, self.res_words[0]), device=device))


_PRODUCTS = {
    "geometry": _Product("num_geometry_columns", "assembly_bytes", "gdescs", "geom", GEOM_INFO_DTYPE,
                         np.dtype(np.uint8), C.sizeof(GeomDesc), GEOM_RESULT_DTYPE, ("int32", 4), False, True,
                         ("d_gdesc", "d_asm", "d_gres")),
    "wkb": _Product("num_geometry_columns", "wkb_bytes", "wdescs", "wkb", WKB_INFO_DTYPE, WKB_DESC_DTYPE,
                    WKB_DESC_DTYPE.itemsize, WKB_RESULT_DTYPE, ("int64", 2), False, True,
                    ("d_wdesc", "d_wkb", "d_wres")),
    "bbox": _Product("num_geometry_columns", "bbox_bytes", "bdescs", "bbox", BBOX_INFO_DTYPE, BBOX_DESC_DTYPE,
                     BBOX_DESC_DTYPE.itemsize, BBOX_RESULT_DTYPE, ("int64", 5), False, True,
                     ("d_bdesc", "d_bbox", "d_bres")),
    "measures": _Product("num_geometry_columns", "measures_bytes", "mdescs", "measures", MEASURES_INFO_DTYPE,
                         MEASURES_DESC_DTYPE, MEASURES_DESC_DTYPE.itemsize, MEASURES_RESULT_DTYPE, ("int32", 2), False,
                         True, ("d_mdesc", "d_measures", "d_mres")),
    "select": _Product("num_geometry_columns", "select_bytes", "sdescs", "select", SELECT_INFO_DTYPE, SELECT_DESC_DTYPE,
                       SELECT_DESC_DTYPE.itemsize, SELECT_RESULT_DTYPE, ("int64", 2), False, True,
                       ("d_sdesc", "d_select", "d_sres")),
    "simplify": _Product("num_geometry_columns", "simplify_bytes", "spdescs", "simplify", SIMPLIFY_INFO_DTYPE,
                         SIMPLIFY_DESC_DTYPE, SIMPLIFY_DESC_DTYPE.itemsize, GEOM_RESULT_DTYPE, ("int32", 4), False, True,
                         ("d_spdesc", "d_simplify", "d_sgres")),
    "mvt": _Product("num_geometry_columns", "mvt_bytes", "mvdescs", "mvt", MVT_INFO_DTYPE, MVT_DESC_DTYPE,
                    MVT_DESC_DTYPE.itemsize, MVT_RESULT_DTYPE, ("int64", 2), False, True, ("d_mvdesc", "d_mvt", "d_mvres")),
    "property": _Product("num_property_columns", "property_bytes", "pdescs", "props", PROP_INFO_DTYPE, PROP_DESC_DTYPE,
                         PROP_DESC_DTYPE.itemsize, PROP_RESULT_DTYPE, ("int32", 2), True, False,
                         ("d_pdesc", "d_props", "d_pres")),
}


def _stream(stream, device) -> int:
    """The HIP stream handle of `stream`, or of torch's current stream on `device`."""
    import torch

    return (stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream


def _host_results(d_buf, nbytes: int, res: np.ndarray, index: np.ndarray):
    """(the first nbytes of a device buffer, launch-order results reordered by `index`) on the host."""
    return d_buf.cpu().numpy()[:nbytes], res[index] if index.size else res


class Plan:
    """Host-side container walk of a tile batch -> per-stream descriptors (covt_plan_create)."""

    def __init__(self, blob: np.ndarray, offsets, sizes, fmt: int = FORMAT_GENC, id_mode: int = ID_FORMAT,
                 flags: int = 0, options: Optional[PlanOptions] = None):
        L = lib()
        self.blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
        self.n_tiles = int(self.offsets.size)
        opts = PlanOptions() if options is None else PlanOptions(**{f: getattr(options, f) for f, _ in
                                                                   PlanOptions._fields_[1:]})
        opts.flags |= flags
        self.options = opts
        h = C.c_void_p()
        _raise(L.covt_plan_create_opts(_ptr(self.blob, C.c_uint8), _ptr(self.offsets, C.c_uint64),
                                       _ptr(self.sizes, C.c_uint64), self.n_tiles, fmt, id_mode, C.byref(opts),
                                       C.byref(h)), "covt_plan_create")
        self._h = h
        self.num_streams = int(L.covt_plan_num_streams(h))
        self.output_bytes = int(L.covt_plan_output_bytes(h))
        ib, ob, vx = C.c_int64(), C.c_int64(), C.c_int64()
        L.covt_plan_totals(h, C.byref(ib), C.byref(ob), C.byref(vx))
        self.in_bytes, self.out_bytes, self.vertices = ib.value, ob.value, vx.value
        self.streams = np.zeros(self.num_streams, dtype=STREAM_INFO_DTYPE)
        if self.num_streams:
            L.covt_plan_streams(h, self.streams.ctypes.data)
        self.num_descs = int(L.covt_plan_num_descs(h))  # >= num_streams: split chunks and their pads
        self.descs = np.zeros(self.num_descs * 32, dtype=np.uint8)
        self.desc_streams = np.zeros(self.num_descs, dtype=np.int64)
        if self.num_descs:
            L.covt_plan_descs(h, self.descs.ctypes.data)
            L.covt_plan_desc_streams(h, _ptr(self.desc_streams, C.c_int64))
        self.family_counts = np.zeros(NUM_FAMILIES, dtype=np.int64)
        L.covt_plan_family_counts(h, _ptr(self.family_counts, C.c_int64))
        self.tile_status = np.zeros(max(self.n_tiles, 1), dtype=np.int32)[:self.n_tiles]
        if self.n_tiles:
            L.covt_plan_tile_status(h, _ptr(self.tile_status, C.c_int32))
        # geometry assembly (include/covt.h "Geometry assembly")
        self.num_geometry_columns = int(L.covt_plan_num_geometry_columns(h))
        self.assembly_bytes = int(L.covt_plan_assembly_bytes(h))
        self.geom = np.zeros(self.num_geometry_columns, dtype=GEOM_INFO_DTYPE)
        self.gdescs = np.zeros(self.num_geometry_columns * C.sizeof(GeomDesc), dtype=np.uint8)
        if self.num_geometry_columns:
            L.covt_plan_geometry_columns(h, self.geom.ctypes.data)
            L.covt_plan_geometry_descs(h, self.gdescs.ctypes.data)
        # the extent of each geometry column's layer (include/covt.h "Georeferenced geometry")
        self.geometry_extents = np.zeros(self.num_geometry_columns, dtype=np.int32)
        if self.num_geometry_columns:
            L.covt_plan_geometry_extents(h, self.geometry_extents.ctypes.data)
        # geometry as WKB (include/covt.h "Geometry as WKB"): one column per geometry column
        self.wkb_bytes = int(L.covt_plan_wkb_bytes(h))
        self.wkb = np.zeros(self.num_geometry_columns, dtype=WKB_INFO_DTYPE)
        self.wdescs = np.zeros(self.num_geometry_columns, dtype=WKB_DESC_DTYPE)
        if self.num_geometry_columns:
            L.covt_plan_wkb_columns(h, self.wkb.ctypes.data)
            L.covt_plan_wkb_descs(h, self.wdescs.ctypes.data)
        # geometry bounding boxes (include/covt.h "Geometry bounding boxes"): one column per geometry column
        self.bbox_bytes = int(L.covt_plan_bbox_bytes(h))
        self.bbox = np.zeros(self.num_geometry_columns, dtype=BBOX_INFO_DTYPE)
        self.bdescs = np.zeros(self.num_geometry_columns, dtype=BBOX_DESC_DTYPE)
        if self.num_geometry_columns:
            L.covt_plan_bbox_columns(h, self.bbox.ctypes.data)
            L.covt_plan_bbox_descs(h, self.bdescs.ctypes.data)
        # geometry measures (include/covt.h "Geometry measures"): one column per geometry column
        self.measures_bytes = int(L.covt_plan_measures_bytes(h))
        self.measures = np.zeros(self.num_geometry_columns, dtype=MEASURES_INFO_DTYPE)
        self.mdescs = np.zeros(self.num_geometry_columns, dtype=MEASURES_DESC_DTYPE)
        if self.num_geometry_columns:
            L.covt_plan_measures_columns(h, self.measures.ctypes.data)
            L.covt_plan_measures_descs(h, self.mdescs.ctypes.data)
        # feature selection (include/covt.h "Feature selection"): one column per geometry column
        self.select_bytes = int(L.covt_plan_select_bytes(h))
        self.select = np.zeros(self.num_geometry_columns, dtype=SELECT_INFO_DTYPE)
        self.sdescs = np.zeros(self.num_geometry_columns, dtype=SELECT_DESC_DTYPE)
        if self.num_geometry_columns:
            L.covt_plan_select_columns(h, self.select.ctypes.data)
            L.covt_plan_select_descs(h, self.sdescs.ctypes.data)
        # geometry simplification (include/covt.h "Geometry simplification"): one column per geometry column,
        # and the geometry descriptors that name the simplified columns
        self.simplify_bytes = int(L.covt_plan_simplify_bytes(h))
        self.simplify = np.zeros(self.num_geometry_columns, dtype=SIMPLIFY_INFO_DTYPE)
        self.spdescs = np.zeros(self.num_geometry_columns, dtype=SIMPLIFY_DESC_DTYPE)
        self.sgdescs = np.zeros(self.num_geometry_columns * C.sizeof(GeomDesc), dtype=np.uint8)
        if self.num_geometry_columns:
            L.covt_plan_simplify_columns(h, self.simplify.ctypes.data)
            L.covt_plan_simplify_descs(h, self.spdescs.ctypes.data)
            L.covt_plan_simplified_geometry_descs(h, self.sgdescs.ctypes.data)
        # geometry as MVT (include/covt.h "Geometry as MVT"): one column per geometry column
        self.mvt_bytes = int(L.covt_plan_mvt_bytes(h))
        self.mvt = np.zeros(self.num_geometry_columns, dtype=MVT_INFO_DTYPE)
        self.mvdescs = np.zeros(self.num_geometry_columns, dtype=MVT_DESC_DTYPE)
        if self.num_geometry_columns:
            L.covt_plan_mvt_columns(h, self.mvt.ctypes.data)
            L.covt_plan_mvt_descs(h, self.mvdescs.ctypes.data)
        # property columns (include/covt.h "Property columns"; plans made with PLAN_PROPERTIES)
        self.num_property_columns = int(L.covt_plan_num_property_columns(h))
        self.property_bytes = int(L.covt_plan_property_bytes(h))
        self.props = np.zeros(self.num_property_columns, dtype=PROP_INFO_DTYPE)
        self.pdescs = np.zeros(self.num_property_columns, dtype=PROP_DESC_DTYPE)
        if self.num_property_columns:
            L.covt_plan_property_columns(h, self.props.ctypes.data)
            L.covt_plan_property_descs(h, self.pdescs.ctypes.data)

    @classmethod
    def from_tiles(cls, tiles: List[bytes], fmt: int = FORMAT_GENC, id_mode: int = ID_FORMAT, flags: int = 0,
                   options: Optional[PlanOptions] = None):
        blob, offs, sizes = pack_tiles(tiles)
        return cls(blob, offs, sizes, fmt, id_mode, flags, options)

    def close(self):
        if getattr(self, "_h", None):
            lib().covt_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def release_device(self):
        """Free the device buffers decode_host cached on this plan (covt_plan_release_device)."""
        _raise(lib().covt_plan_release_device(self._h), "covt_plan_release_device")

    def decode_host(self, n_gpus: int = 1, out=None, res=None, shard_devices=None):
        """H2D + decode + D2H of the whole plan (covt_plan_decode_host[_multi]).
        Returns (uint8 output buffer, results[num_streams, 2] = (status, consumed)) in plan order.
        `out` / `res` may be caller-owned buffers reused across calls (C-contiguous uint8 of at least
        output_bytes, int32 of shape (>= num_streams, 2)); fresh zeroed ones are allocated otherwise."""
        if out is None:
            out = np.zeros(max(self.output_bytes, 1), dtype=np.uint8)
        if res is None:
            res = np.zeros((max(self.num_streams, 1), 2), dtype=np.int32)
        if (out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < self.output_bytes
                or res.dtype != np.int32 or not res.flags.c_contiguous or res.ndim != 2 or res.shape[1] != 2
                or res.shape[0] < self.num_streams):
            raise ValueError("decode_host: out/res buffers have the wrong dtype, layout or size")
        if shard_devices is not None:
            devs = np.ascontiguousarray(shard_devices, dtype=np.int32)
            st = lib().covt_plan_decode_host_shards(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, devs.size,
                                                    _ptr(devs, C.c_int32), out.ctypes.data, res.ctypes.data)
        elif n_gpus > 1:
            st = lib().covt_plan_decode_host_multi(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, n_gpus,
                                                   out.ctypes.data, res.ctypes.data)
        else:
            st = lib().covt_plan_decode_host(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, out.ctypes.data,
                                             res.ctypes.data)
        _raise(st, "covt_plan_decode_host")
        return out[:self.output_bytes], res[:self.num_streams]

    def _product_host(self, kind: str, entry: str, crs=None, tile_zxy=None):
        """One whole-plan entry point: (uint8 buffer of the product, its results in tile order).  With `crs`
        the entry point's _projected_ twin, which takes the CRS and the tiles' addresses."""
        q = _PRODUCTS[kind]
        nbytes, n = getattr(self, q.nbytes), getattr(self, q.count)
        buf = np.zeros(max(nbytes, 1), dtype=np.uint8)
        res = np.zeros(max(n, 1), dtype=q.res_dtype)
        if crs is None:
            _raise(getattr(lib(), entry)(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, buf.ctypes.data,
                                         res.ctypes.data), entry)
        else:
            entry = entry.replace("_host", "_projected_host")
            zxy = _zxy(tile_zxy, self.n_tiles) if tile_zxy is not None else None
            _raise(getattr(lib(), entry)(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, crs,
                                         zxy.ctypes.data if zxy is not None else None, buf.ctypes.data,
                                         res.ctypes.data), entry)
        return buf[:nbytes], res[:n]

    def geo_transforms(self, crs: int, tile_zxy=None):
        """covt_plan_geo_transforms: (the transform table of this plan's geometry columns for `crs` in launch
        order, GEO_XFORM_DTYPE; kinds, the OR of 1 << kind over it).  tile_zxy: z, x, y of every tile."""
        table = np.zeros(self.num_geometry_columns, dtype=GEO_XFORM_DTYPE)
        kinds = C.c_uint32(0)
        zxy = _zxy(tile_zxy, self.n_tiles) if tile_zxy is not None else None
        _raise(lib().covt_plan_geo_transforms(self._h, crs, zxy.ctypes.data if zxy is not None else None,
                                              table.ctypes.data, C.byref(kinds)), "covt_plan_geo_transforms")
        return table, int(kinds.value)

    def assemble_host(self):
        """H2D + decode + geometry assembly + D2H (covt_plan_assemble_host).
        Returns (uint8 assembly buffer, results[num_geometry_columns] in tile order)."""
        return self._product_host("geometry", "covt_plan_assemble_host")

    def wkb_host(self, crs=None, tile_zxy=None):
        """H2D + decode + geometry assembly + WKB serialization + D2H (covt_plan_wkb_host; with `crs` and the
        tiles' z, x, y covt_plan_wkb_projected_host: coordinates in that CRS instead of tile pixels).
        Returns (uint8 WKB buffer, results[num_geometry_columns] in tile order); see wkb_column."""
        return self._product_host("wkb", "covt_plan_wkb_host", crs, tile_zxy)

    def wkb_column(self, buf: np.ndarray, wres: np.ndarray, c: int) -> "WkbColumn":
        """Column c (tile order) of a WKB buffer -> WkbColumn (raises on its status)."""
        w, r = self.wkb[c], wres[c]
        _raise(int(r["status"]), "WKB column %d (tile %d, layer %d)" % (c, w["tile"], w["layer"]))
        o, b = int(w["offsets_off"]), int(w["bytes_off"])
        return WkbColumn(buf[o:o + 4 * (int(w["n_features"]) + 1)].view(np.int32), buf[b:b + int(r["n_bytes"])])

    def bbox_host(self, crs=None, tile_zxy=None):
        """H2D + decode + geometry assembly + bounding boxes + D2H (covt_plan_bbox_host; with `crs` and the
        tiles' z, x, y covt_plan_bbox_projected_host: boxes in that CRS instead of tile pixels).
        Returns (uint8 bounding-box buffer, results[num_geometry_columns] in tile order); see bbox_column."""
        return self._product_host("bbox", "covt_plan_bbox_host", crs, tile_zxy)

    def bbox_column(self, buf: np.ndarray, bres: np.ndarray, c: int) -> "BboxColumn":
        """Column c (tile order) of a bounding-box buffer -> BboxColumn (raises on its status)."""
        b, r = self.bbox[c], bres[c]
        _raise(int(r["status"]), "bounding-box column %d (tile %d, layer %d)" % (c, b["tile"], b["layer"]))
        o, n = int(b["off"]), int(b["n_features"])
        a = buf[o:o + 32 * n].view(np.float64)
        return BboxColumn(a[:n], a[n:2 * n], a[2 * n:3 * n], a[3 * n:], np.array(r["extent"], dtype=np.float64),
                          int(r["n_empty"]))

    def mvt_host(self, opts: Optional["MvtOptions"] = None):
        """H2D + decode + geometry assembly (+ simplification while set_simplify is set) + MVT encoding + D2H
        (covt_plan_mvt_host).  Returns (uint8 mvt buffer, results[num_geometry_columns] in tile order); see
        mvt_column."""
        opts = opts if opts is not None else MvtOptions()
        buf = np.zeros(max(self.mvt_bytes, 1), dtype=np.uint8)
        res = np.zeros(max(self.num_geometry_columns, 1), dtype=MVT_RESULT_DTYPE)
        _raise(lib().covt_plan_mvt_host(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, C.addressof(opts),
                                        buf.ctypes.data, res.ctypes.data), "covt_plan_mvt_host")
        return buf[:self.mvt_bytes], res[:self.num_geometry_columns]

    def mvt_column(self, buf: np.ndarray, res: np.ndarray, c: int) -> "MvtColumn":
        """Column c (tile order) of an mvt buffer -> MvtColumn (raises on its status)."""
        q, r = self.mvt[c], res[c]
        _raise(int(r["status"]), "mvt column %d (tile %d, layer %d)" % (c, q["tile"], q["layer"]))
        a16 = lambda x: (x + 15) & ~15  # noqa: E731  (covt_mvt_plan.h: every member padded to 16 bytes)
        o, n = int(q["off"]), int(q["n_features"])
        oo = o + a16(n)
        ob = oo + a16(4 * (n + 1))
        return MvtColumn(buf[o:o + n], buf[oo:oo + 4 * (n + 1)].view(np.int32), buf[ob:ob + int(r["n_bytes"])],
                         int(r["n_empty"]))

    def measures_host(self):
        """H2D + decode + geometry assembly + measures + D2H (covt_plan_measures_host).
        Returns (uint8 measures buffer, results[num_geometry_columns] in tile order); see measures_column."""
        return self._product_host("measures", "covt_plan_measures_host")

    def measures_column(self, buf: np.ndarray, mres: np.ndarray, c: int) -> "MeasuresColumn":
        """Column c (tile order) of a measures buffer -> MeasuresColumn (raises on its status)."""
        m, r = self.measures[c], mres[c]
        _raise(int(r["status"]), "measures column %d (tile %d, layer %d)" % (c, m["tile"], m["layer"]))
        o, n = int(m["off"]), int(m["n_features"])
        return MeasuresColumn(buf[o:o + 8 * n].view(np.float64), buf[o + 8 * n:o + 16 * n].view(np.float64),
                              buf[o + 16 * n:o + 20 * n].view(np.int32))

    def select_host(self, pred: Optional["SelectPred"], crs=None, tile_zxy=None, where: Optional["Where"] = None,
                    query: Optional["SelectQuery"] = None):
        """H2D + decode + geometry assembly + WKB and bounding boxes (in `crs`, given the tiles' z, x, y) +
        measures if `pred` has a size cut + predicate + select + D2H (covt_plan_select_host).  With `where`
        (a plan made with PLAN_PROPERTIES) covt_plan_select_where_host: the property predicate ANDed into
        `pred`'s masks, or alone with pred=None; its per-column statuses in tile order are kept as
        ``self.where_status``.  With `query` (covt_plan_select_query_host) the exact window query, in tile
        pixels, ANDed into those masks, or alone with pred=None and where=None; its per-column statuses are kept
        as ``self.query_status``.
        Returns (uint8 select buffer, results[num_geometry_columns] in tile order); see select_column."""
        buf = np.zeros(max(self.select_bytes, 1), dtype=np.uint8)
        res = np.zeros(max(self.num_geometry_columns, 1), dtype=SELECT_RESULT_DTYPE)
        zxy = _zxy(tile_zxy, self.n_tiles) if tile_zxy is not None else None
        if query is not None:
            wst = np.zeros(max(self.num_geometry_columns, 1), dtype=np.int32)
            qst = np.zeros(max(self.num_geometry_columns, 1), dtype=np.int32)
            _raise(lib().covt_plan_select_query_host(self._h, _ptr(self.blob, C.c_uint8), self.blob.size,
                                                     CRS_TILE if crs is None else crs,
                                                     zxy.ctypes.data if zxy is not None else None,
                                                     C.byref(pred) if pred is not None else None,
                                                     C.byref(where) if where is not None else None, C.byref(query),
                                                     buf.ctypes.data, res.ctypes.data, wst.ctypes.data,
                                                     qst.ctypes.data), "covt_plan_select_query_host")
            if where is not None:
                self.where_status = wst[:self.num_geometry_columns]
            self.query_status = qst[:self.num_geometry_columns]
            return buf[:self.select_bytes], res[:self.num_geometry_columns]
        if where is None:
            _raise(lib().covt_plan_select_host(self._h, _ptr(self.blob, C.c_uint8), self.blob.size,
                                               CRS_TILE if crs is None else crs,
                                               zxy.ctypes.data if zxy is not None else None, C.byref(pred),
                                               buf.ctypes.data, res.ctypes.data), "covt_plan_select_host")
            return buf[:self.select_bytes], res[:self.num_geometry_columns]
        wst = np.zeros(max(self.num_geometry_columns, 1), dtype=np.int32)
        _raise(lib().covt_plan_select_where_host(self._h, _ptr(self.blob, C.c_uint8), self.blob.size,
                                                 CRS_TILE if crs is None else crs,
                                                 zxy.ctypes.data if zxy is not None else None,
                                                 C.byref(pred) if pred is not None else None, C.byref(where),
                                                 buf.ctypes.data, res.ctypes.data, wst.ctypes.data),
               "covt_plan_select_where_host")
        self.where_status = wst[:self.num_geometry_columns]
        return buf[:self.select_bytes], res[:self.num_geometry_columns]

    def where_bind(self, where: "Where") -> np.ndarray:
        """covt_plan_where_bind: int32 [num_geometry_columns, WHERE_MAX_CLAUSES] in launch order, entry [c, k]
        the property descriptor clause k reads in geometry column c (-1: none in that layer)."""
        out = np.full((max(self.num_geometry_columns, 1), WHERE_MAX_CLAUSES), -1, dtype=np.int32)
        _raise(lib().covt_plan_where_bind(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, C.byref(where),
                                          out.ctypes.data), "covt_plan_where_bind")
        return out[:self.num_geometry_columns]

    def select_column(self, buf: np.ndarray, sres: np.ndarray, c: int) -> "SelectedColumn":
        """Column c (tile order) of a select buffer -> SelectedColumn (raises on its status)."""
        q, r = self.select[c], sres[c]
        _raise(int(r["status"]), "select column %d (tile %d, layer %d)" % (c, q["tile"], q["layer"]))
        o, n, k = int(q["off"]), int(q["n_features"]), int(r["n_selected"])
        a16 = lambda x: (x + 15) & ~15  # noqa: E731  (covt_select_plan.h: every member padded to 16 bytes)
        sel = o + a16(n)
        offs = sel + a16(4 * n)
        data = offs + a16(4 * (n + 1))
        return SelectedColumn(buf[sel:sel + 4 * k].view(np.int32),
                              WkbColumn(buf[offs:offs + 4 * (k + 1)].view(np.int32), buf[data:data + int(r["n_bytes"])]))

    def _tile_shifts(self, shift):
        """(uniform shift, per-tile int32 array or None) of a `shift` argument: an int or one per tile."""
        if np.ndim(shift) == 0:
            return int(shift), None
        ts = np.ascontiguousarray(shift, dtype=np.int32)
        if ts.shape != (self.n_tiles,):
            raise IllegalArgumentException("shift must be an int or hold one entry per tile")
        return 0, ts

    def simplify_shifts(self, tile_shift) -> np.ndarray:
        """covt_plan_simplify_shifts: per-tile shifts -> per-column shifts in launch order (int32)."""
        _, ts = self._tile_shifts(np.asarray(tile_shift).reshape(-1))
        out = np.zeros(self.num_geometry_columns, dtype=np.int32)
        _raise(lib().covt_plan_simplify_shifts(self._h, ts.ctypes.data, out.ctypes.data), "covt_plan_simplify_shifts")
        return out

    def simplify_host(self, shift):
        """H2D + decode + geometry assembly + simplification + D2H (covt_plan_simplify_host).  shift: the grid
        is 2^shift tile pixels; an int, or one per tile.  Returns (uint8 simplify buffer, geometry
        results[num_geometry_columns] in tile order); see simplified_arrays."""
        s, ts = self._tile_shifts(shift)
        buf = np.zeros(max(self.simplify_bytes, 1), dtype=np.uint8)
        res = np.zeros(max(self.num_geometry_columns, 1), dtype=GEOM_RESULT_DTYPE)
        _raise(lib().covt_plan_simplify_host(self._h, _ptr(self.blob, C.c_uint8), self.blob.size, s,
                                             ts.ctypes.data if ts is not None else None, buf.ctypes.data,
                                             res.ctypes.data), "covt_plan_simplify_host")
        return buf[:self.simplify_bytes], res[:self.num_geometry_columns]

    def simplified_arrays(self, buf: np.ndarray, gres: np.ndarray, c: int) -> "GeoArrowGeometry":
        """Column c (tile order) of a simplify buffer -> GeoArrowGeometry (raises on its status)."""
        q, r = self.simplify[c], gres[c]
        _raise(int(r["status"]), "simplified column %d (tile %d, layer %d)" % (c, q["tile"], q["layer"]))
        a16 = lambda x: (x + 15) & ~15  # noqa: E731  (covt_simplify_plan.h: every member padded to 16 bytes)
        n = int(q["n_features"])
        geo = int(q["off"])
        part = geo + a16(4 * (n + 1))
        ring = part + a16(4 * (int(q["part_cap"]) + 1))
        xy = ring + a16(4 * (int(q["ring_cap"]) + 1))
        seg = lambda o, k: buf[o:o + 4 * k].view(np.int32)  # noqa: E731
        return GeoArrowGeometry(seg(geo, n + 1), seg(part, int(r["num_parts"]) + 1), seg(ring, int(r["num_rings"]) + 1),
                                seg(xy, 2 * int(r["num_coords"])).reshape(-1, 2))

    def set_simplify(self, shift):
        """covt_plan_set_simplify: while set (an int, or one shift per tile), wkb_host, bbox_host, measures_host
        and select_host read the simplified column; None unsets it (the default)."""
        if shift is None:
            _raise(lib().covt_plan_set_simplify(self._h, 0, 0, None), "covt_plan_set_simplify")
            return
        s, ts = self._tile_shifts(shift)
        _raise(lib().covt_plan_set_simplify(self._h, 1, s, ts.ctypes.data if ts is not None else None),
               "covt_plan_set_simplify")

    def properties_host(self):
        """H2D + decode + property materialization + D2H (covt_plan_properties_host).
        Returns (uint8 property buffer, results[num_property_columns] in tile order)."""
        return self._product_host("property", "covt_plan_properties_host")

    def property_name(self, c: int) -> str:
        """Column name of property (sub)column c, plus ':<lang>' for a localized language stream."""
        p = self.props[c]
        name = bytes(self.blob[int(p["name_off"]):int(p["name_off"]) + int(p["name_len"])]).decode("utf-8") \
            if p["name_off"] >= 0 else ""
        if p["lang"] >= 0:
            name += ":" + bytes(self.blob[int(p["lang_off"]):int(p["lang_off"]) + int(p["lang_len"])]).decode("utf-8")
        return name

    def property_column(self, buf: np.ndarray, pres: np.ndarray, c: int) -> "PropertyColumn":
        """Property (sub)column c (tile order) of a property buffer (raises on its status)."""
        p, r = self.props[c], pres[c]
        _raise(int(r["status"]), "property column %d (tile %d, layer %d)" % (c, p["tile"], p["layer"]))
        n = int(p["n_features"])
        nb = (n + 7) // 8
        t = int(p["type"])

        def seg(k, nbytes):
            o = int(p["out_off"][k])
            return buf[o:o + nbytes]

        vals = {PROP_BOOLEAN: lambda: seg(1, nb), PROP_INT64: lambda: seg(1, 8 * n).view(np.int64),
                PROP_FLOAT: lambda: seg(1, 4 * n).view(np.float32), PROP_STRING: lambda: seg(1, 4 * n).view(np.int32)}[t]()
        doff = dby = None
        if t == PROP_STRING and p["out_off"][2] >= 0:
            doff = seg(2, 4 * (int(p["n_dict"]) + 1)).view(np.int32)
            dby = seg(3, int(p["dict_bytes"]))
        return PropertyColumn(self.property_name(c), t, n, seg(0, nb), vals, doff, dby, int(r["n_valid"]))

    def geometry_arrays(self, asm: np.ndarray, gres: np.ndarray, c: int):
        """Column c (tile order) of an assembly buffer -> GeoArrowGeometry (raises on its status)."""
        g, r = self.geom[c], gres[c]
        _raise(int(r["status"]), "geometry column %d (tile %d, layer %d)" % (c, g["tile"], g["layer"]))

        def seg(k, n, dt=np.int32, w=4):
            o = int(g["out_off"][k])
            return asm[o:o + n * w].view(dt)

        return GeoArrowGeometry(seg(0, int(g["n_features"]) + 1), seg(1, int(r["num_parts"]) + 1),
                                seg(2, int(r["num_rings"]) + 1), seg(3, 2 * int(r["num_coords"])).reshape(-1, 2))

    def subset_descs(self, mask):
        """Descriptor table of the streams selected by `mask` (bool per stream, plan order), in launch
        order (still grouped by family, largest first inside a family) -> (uint8 descs, family counts,
        plan-order stream index of each selected descriptor that holds a stream's result, else -1).
        Outputs keep their slices in the full output
        buffer; results land at the subset position."""
        mask = np.asarray(mask, dtype=bool)
        if mask.shape != (self.num_streams,):
            raise ValueError("subset mask must have one entry per stream")
        keep = mask[self.desc_streams]  # every descriptor of a selected stream (split chunks + pads)
        fam = np.repeat(np.arange(NUM_FAMILIES), self.family_counts)
        primary = np.full(self.num_descs, -1, dtype=np.int64)  # the descriptor holding the stream's result
        primary[self.streams["desc_index"]] = np.arange(self.num_streams)
        descs = np.ascontiguousarray(self.descs.reshape(-1, 32)[keep]).reshape(-1)
        counts = np.bincount(fam[keep], minlength=NUM_FAMILIES).astype(np.int64)
        return descs, counts, primary[keep]

    def stream_array(self, out: np.ndarray, i: int) -> np.ndarray:
        s = self.streams[i]
        dt = {1: np.uint8, 4: np.int32, 8: np.int64}[int(s["elem_bytes"])]
        off, n = int(s["out_off"]), int(s["out_elems"])
        return out[off:off + n * int(s["elem_bytes"])].view(dt)


class DeviceBatch:
    """A plan whose tile bytes, descriptors and outputs live in HBM (torch uint8 tensors on `device`).
    ``decode()`` enqueues the single decode launch on the current torch HIP stream."""

    def __init__(self, plan: Plan, device="cuda"):
        import torch

        self.plan = plan
        self.device = torch.device(device)
        self.d_in = torch.from_numpy(plan.blob).to(self.device)
        if self.d_in.data_ptr() % 16:
            raise DeviceError("device input buffer is not 16-byte aligned")
        n = max(plan.num_descs, 1)  # one result entry per descriptor (split pads hold look-back records)
        self.d_desc = torch.from_numpy(plan.descs).to(self.device) if plan.num_descs else \
            torch.zeros(32, dtype=torch.uint8, device=self.device)
        self.d_out = torch.zeros(max(plan.output_bytes, 16), dtype=torch.uint8, device=self.device)
        self.d_res = torch.zeros(n * 2, dtype=torch.int32, device=self.device)

    def decode_graph(self):
        """The same launch replayed from a captured HIP graph on the current torch stream: the fork,
        the four family kernels on their forked streams and the join become one graph launch, so
        back-to-back decodes pay one submission instead of eleven stream operations."""
        import torch

        g = getattr(self, "_graph", None)
        if g is None:
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):  # the fork streams and events exist before the capture
                self.decode(side)
            torch.cuda.current_stream(self.device).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.decode(torch.cuda.current_stream(self.device))
            self._graph = g
        g.replay()

    def decode(self, stream=None, launch: int = 0):
        """launch: LAUNCH_AUTO (0), LAUNCH_FUSED or LAUNCH_FORKED, optionally | LAUNCH_FPF_STREAM or LAUNCH_FPF_CLASSIC
        (covt_decode_streams_device_grouped_mode)."""
        st = lib().covt_decode_streams_device_grouped_mode(self.d_in.data_ptr(), self.d_desc.data_ptr(),
                                                           _ptr(self.plan.family_counts, C.c_int64),
                                                           self.d_out.data_ptr(), self.d_res.data_ptr(),
                                                           _stream(stream, self.device), launch)
        _raise(st, "covt_decode_streams_device_grouped_mode")

    def subset(self, mask) -> "DeviceSubset":
        """A launch over only the streams selected by `mask` (Plan.subset_descs), sharing this batch's
        device input and output buffers."""
        return DeviceSubset(self, mask)

    def _buffers(self, kind: str):
        """The device descriptors, buffer and results of a product (the attributes _PRODUCTS names), made once."""
        import torch

        q = _PRODUCTS[kind]
        if getattr(self, q.attrs[1], None) is None:
            descs = getattr(self.plan, q.descs).view(np.uint8).reshape(-1)
            d_desc = torch.from_numpy(descs).to(self.device) if getattr(self.plan, q.count) else \
                torch.zeros(q.desc_size, dtype=torch.uint8, device=self.device)
            for name, t in zip(q.attrs, (d_desc,) + q.alloc(self.plan, self.device)):
                setattr(self, name, t)

    def _results(self, kind: str):
        q = _PRODUCTS[kind]
        n = getattr(self.plan, q.count)
        return _host_results(getattr(self, q.attrs[1]), getattr(self.plan, q.nbytes),
                             getattr(self, q.attrs[2]).cpu().numpy().view(q.res_dtype)[:n],
                             getattr(self.plan, q.records)["desc_index"])

    def assemble(self, stream=None):
        """Enqueue the geometry assembly (after decode() on the same stream)."""
        self._buffers("geometry")
        _raise(lib().covt_assemble_geometry_device(self.d_out.data_ptr(), self.d_res.data_ptr(),
                                                   self.d_gdesc.data_ptr(), self.plan.num_geometry_columns,
                                                   self.d_asm.data_ptr(), self.d_gres.data_ptr(),
                                                   _stream(stream, self.device)), "covt_assemble_geometry_device")

    def _xf(self, xf):
        """The device copy of a (table, kinds) pair of Plan.geo_transforms, uploaded once and kept on the
        batch (a pair with another table replaces it) -> (device pointer, kinds)."""
        import torch

        table, kinds = xf
        table = np.ascontiguousarray(table, dtype=GEO_XFORM_DTYPE)
        if table.size != self.plan.num_geometry_columns:
            raise IllegalArgumentException("the transform table must hold one entry per geometry column")
        kept = getattr(self, "_xf_host", None)
        if kept is None or kept.tobytes() != table.tobytes():
            raw = table.view(np.uint8).reshape(-1)
            self.d_xf = torch.from_numpy(raw.copy()).to(self.device) if table.size else \
                torch.zeros(GEO_XFORM_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
            self._xf_host = table.copy()
        return self.d_xf.data_ptr(), int(kinds)

    def simplify(self, shift, stream=None):
        """Enqueue the geometry simplification of every assembled column (after assemble() on the same stream):
        the grid is 2^shift tile pixels; shift an int, or one per tile."""
        import torch

        self._buffers("geometry")
        self._buffers("simplify")
        s, ts = self.plan._tile_shifts(shift)
        d_shift = None
        if ts is not None:  # (kept on the batch: the launch reads it on the stream)
            self.d_shift = d_shift = torch.from_numpy(self.plan.simplify_shifts(ts)).to(self.device)
        if getattr(self, "d_sgdesc", None) is None:
            self.d_sgdesc = torch.from_numpy(self.plan.sgdescs).to(self.device) if self.plan.num_geometry_columns else \
                torch.zeros(C.sizeof(GeomDesc), dtype=torch.uint8, device=self.device)
        _raise(lib().covt_geometry_simplify_device(
            self.d_out.data_ptr(), self.d_gdesc.data_ptr(), self.d_asm.data_ptr(), self.d_gres.data_ptr(),
            self.d_spdesc.data_ptr(), self.plan.num_geometry_columns, s,
            d_shift.data_ptr() if d_shift is not None and d_shift.numel() else None, self.d_simplify.data_ptr(),
            self.d_sgres.data_ptr(), _stream(stream, self.device)), "covt_geometry_simplify_device")

    def simplify_results(self):
        """(simplify bytes, geometry results in tile order) copied to the host (after simplify()); see
        Plan.simplified_arrays."""
        return self._results("simplify")

    def _column_source(self, simplified: bool):
        """(geometry descriptors, column buffer, geometry results) a product reads: the assembly's, or with
        `simplified` the retargeted descriptors, the simplify buffer and its results (after simplify())."""
        self._buffers("geometry")
        if not simplified:
            return self.d_gdesc.data_ptr(), self.d_asm.data_ptr(), self.d_gres.data_ptr()
        if getattr(self, "d_sgdesc", None) is None:
            raise IllegalArgumentException("simplified=True needs simplify() first")
        return self.d_sgdesc.data_ptr(), self.d_simplify.data_ptr(), self.d_sgres.data_ptr()

    def wkb(self, stream=None, xf=None, simplified: bool = False):
        """Enqueue the WKB serialization of every assembled geometry column (after assemble() on the
        same stream).  xf: the (table, kinds) pair of Plan.geo_transforms -> coordinates in its CRS.
        simplified: of the simplified column (after simplify() on the same stream)."""
        gdesc, col, gres = self._column_source(simplified)
        self._buffers("wkb")
        if xf is not None:
            d_xf, kinds = self._xf(xf)
            _raise(lib().covt_geometry_wkb_projected_device(
                self.d_out.data_ptr(), gdesc, col, gres,
                self.d_wdesc.data_ptr(), self.plan.num_geometry_columns, self.d_wkb.data_ptr(), self.d_wres.data_ptr(),
                d_xf, kinds, _stream(stream, self.device)), "covt_geometry_wkb_projected_device")
            return
        _raise(lib().covt_geometry_wkb_device(self.d_out.data_ptr(), gdesc, col,
                                              gres, self.d_wdesc.data_ptr(),
                                              self.plan.num_geometry_columns, self.d_wkb.data_ptr(),
                                              self.d_wres.data_ptr(), _stream(stream, self.device)),
               "covt_geometry_wkb_device")

    def wkb_results(self):
        """(WKB bytes, WKB results in tile order) copied to the host (after wkb())."""
        return self._results("wkb")

    def bbox(self, stream=None, xf=None, simplified: bool = False):
        """Enqueue the bounding boxes of every assembled geometry column (after assemble() on the same
        stream).  xf: the (table, kinds) pair of Plan.geo_transforms -> boxes in its CRS.
        simplified: of the simplified column (after simplify() on the same stream)."""
        gdesc, col, gres = self._column_source(simplified)
        self._buffers("bbox")
        if xf is not None:
            d_xf, kinds = self._xf(xf)
            _raise(lib().covt_geometry_bbox_projected_device(
                gdesc, col, gres, self.d_bdesc.data_ptr(),
                self.plan.num_geometry_columns, self.d_bbox.data_ptr(), self.d_bres.data_ptr(), d_xf, kinds,
                _stream(stream, self.device)), "covt_geometry_bbox_projected_device")
            return
        _raise(lib().covt_geometry_bbox_device(gdesc, col, gres,
                                               self.d_bdesc.data_ptr(), self.plan.num_geometry_columns,
                                               self.d_bbox.data_ptr(), self.d_bres.data_ptr(),
                                               _stream(stream, self.device)), "covt_geometry_bbox_device")

    def bbox_results(self):
        """(bounding-box bytes, results in tile order) copied to the host (after bbox())."""
        return self._results("bbox")

    def mvt(self, opts: Optional["MvtOptions"] = None, stream=None, simplified: bool = False):
        """Enqueue the MVT encoding of every assembled geometry column (after assemble() on the same stream).
        simplified: of the simplified column (after simplify() on the same stream)."""
        gdesc, col, gres = self._column_source(simplified)
        self._buffers("mvt")
        opts = opts if opts is not None else MvtOptions()
        _raise(lib().covt_geometry_mvt_device(self.d_out.data_ptr(), gdesc, col, gres, self.d_mvdesc.data_ptr(),
                                              self.plan.num_geometry_columns, C.addressof(opts), self.d_mvt.data_ptr(),
                                              self.d_mvres.data_ptr(), _stream(stream, self.device)),
               "covt_geometry_mvt_device")

    def mvt_results(self):
        """(mvt bytes, mvt results in tile order) copied to the host (after mvt()); see Plan.mvt_column."""
        return self._results("mvt")

    def measures(self, stream=None, simplified: bool = False):
        """Enqueue the measures (area, length, num_coords) of every assembled geometry column (after
        assemble() on the same stream).  simplified: of the simplified column (after simplify())."""
        gdesc, col, gres = self._column_source(simplified)
        self._buffers("measures")
        _raise(lib().covt_geometry_measures_device(self.d_out.data_ptr(), gdesc,
                                                   col, gres,
                                                   self.d_mdesc.data_ptr(), self.plan.num_geometry_columns,
                                                   self.d_measures.data_ptr(), self.d_mres.data_ptr(),
                                                   _stream(stream, self.device)), "covt_geometry_measures_device")

    def measures_results(self):
        """(measures bytes, results in tile order) copied to the host (after measures())."""
        return self._results("measures")

    def select_mask(self, c: int):
        """The keep mask of column c (tile order): a torch uint8 view of n_features bytes of the select buffer,
        which select_predicate() writes and a caller may write instead (any non-zero byte keeps a feature)."""
        self._buffers("select")
        q = self.plan.select[c]
        return self.d_select[int(q["off"]):int(q["off"]) + int(q["n_features"])]

    def select_predicate(self, pred: "SelectPred", stream=None):
        """Enqueue the predicate pass: every column's keep mask from its bounding boxes and, with a size cut,
        its measures (after bbox() and measures() on the same stream); the window is in the boxes' space."""
        for kind in ("bbox", "measures", "select"):
            self._buffers(kind)
        _raise(lib().covt_select_predicate_device(self.d_bdesc.data_ptr(), self.d_bbox.data_ptr(),
                                                  self.d_bres.data_ptr(), self.d_mdesc.data_ptr(),
                                                  self.d_measures.data_ptr(), self.d_mres.data_ptr(),
                                                  self.d_sdesc.data_ptr(), self.plan.num_geometry_columns,
                                                  C.byref(pred), self.d_select.data_ptr(),
                                                  _stream(stream, self.device)), "covt_select_predicate_device")

    def _where(self, where: "Where"):
        """The device copies of a Where and its bind table, uploaded once and kept on the batch (another
        predicate replaces them) -> (blob pointer, bind pointer)."""
        import torch

        raw = where.tobytes()
        if getattr(self, "_where_host", None) != raw:
            bind = self.plan.where_bind(where).reshape(-1)
            self.d_where = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(self.device)
            self.d_bind = torch.from_numpy(bind.copy()).to(self.device) if bind.size else \
                torch.zeros(WHERE_MAX_CLAUSES, dtype=torch.int32, device=self.device)
            self._where_host = raw
        return self.d_where.data_ptr(), self.d_bind.data_ptr()

    def select_where(self, where: "Where", mode: int = WHERE_WRITE, stream=None):
        """Enqueue the where pass: every column's keep mask from the property predicate (WHERE_WRITE), or ANDed
        into the masks already there (WHERE_AND), after materialize_properties() and whatever wrote the masks
        on the same stream.  The blob and its bind table are uploaded on the first call with a predicate (call
        once before capturing a graph)."""
        import torch

        self._buffers("property")
        self._buffers("select")
        d_where, d_bind = self._where(where)
        if getattr(self, "d_where_status", None) is None:
            self.d_where_status = torch.zeros(max(self.plan.num_geometry_columns, 1), dtype=torch.int32,
                                              device=self.device)
        _raise(lib().covt_select_where_device(self.d_pdesc.data_ptr(), self.d_props.data_ptr(), self.d_pres.data_ptr(),
                                              self.plan.num_property_columns, self.d_sdesc.data_ptr(),
                                              self.plan.num_geometry_columns, d_where, d_bind, int(mode),
                                              self.d_select.data_ptr(), self.d_where_status.data_ptr(),
                                              _stream(stream, self.device)), "covt_select_where_device")

    def where_status(self) -> np.ndarray:
        """The where pass's per-column statuses in tile order, copied to the host (after select_where())."""
        st = self.d_where_status.cpu().numpy()[:self.plan.num_geometry_columns]
        idx = self.plan.select["desc_index"]
        return st[idx] if idx.size else st

    def select_query(self, query: "SelectQuery", mode: int = WHERE_WRITE, stream=None, simplified: bool = False):
        """Enqueue the query pass: every column's keep mask from the exact relation of its features with the
        query's window (WHERE_WRITE), or ANDed into the masks already there (WHERE_AND), after assemble() and
        whatever wrote the masks on the same stream.  simplified: over the simplified column (after
        simplify()).  Until select() runs, the head of each slice's bytes member holds the pass's scratch."""
        import torch

        gdesc, col, gres = self._column_source(simplified)
        self._buffers("select")
        if getattr(self, "d_query_status", None) is None:
            self.d_query_status = torch.zeros(max(self.plan.num_geometry_columns, 1), dtype=torch.int32,
                                              device=self.device)
        _raise(lib().covt_select_query_device(self.d_out.data_ptr(), gdesc, col, gres, self.d_sdesc.data_ptr(),
                                              self.plan.num_geometry_columns, C.byref(query), int(mode),
                                              self.d_select.data_ptr(), self.d_query_status.data_ptr(),
                                              _stream(stream, self.device)), "covt_select_query_device")

    def query_status(self) -> np.ndarray:
        """The query pass's per-column statuses in tile order, copied to the host (after select_query())."""
        st = self.d_query_status.cpu().numpy()[:self.plan.num_geometry_columns]
        idx = self.plan.select["desc_index"]
        return st[idx] if idx.size else st

    def select(self, stream=None):
        """Enqueue the selection: every column's selection vector and compacted WKB from its keep mask (after
        wkb() and select_predicate(), or the caller's own masks, on the same stream)."""
        self._buffers("wkb")
        self._buffers("select")
        _raise(lib().covt_geometry_select_device(self.d_wdesc.data_ptr(), self.d_wkb.data_ptr(), self.d_wres.data_ptr(),
                                                 self.d_sdesc.data_ptr(), self.plan.num_geometry_columns,
                                                 self.d_select.data_ptr(), self.d_sres.data_ptr(),
                                                 _stream(stream, self.device)), "covt_geometry_select_device")

    def select_results(self):
        """(select bytes, results in tile order) copied to the host (after select()); see Plan.select_column."""
        return self._results("select")

    def materialize_properties(self, stream=None):
        """Enqueue the property-column materialization (after decode() on the same stream)."""
        self._buffers("property")
        _raise(lib().covt_materialize_properties_device(self.d_in.data_ptr(), self.d_out.data_ptr(),
                                                        self.d_res.data_ptr(), self.d_pdesc.data_ptr(),
                                                        self.plan.num_property_columns, self.d_props.data_ptr(),
                                                        self.d_pres.data_ptr(), _stream(stream, self.device)),
               "covt_materialize_properties_device")

    def property_results(self):
        """(property bytes, results in tile order) copied to the host."""
        self._buffers("property")
        return self._results("property")

    def assembly_results(self):
        """(assembly bytes, geometry results in tile order) copied to the host."""
        self._buffers("geometry")
        return self._results("geometry")

    def results(self):
        """(output bytes, results in plan order) copied to the host."""
        return _host_results(self.d_out, self.plan.output_bytes,
                             self.d_res.cpu().numpy().reshape(-1, 2)[:self.plan.num_descs],
                             self.plan.streams["desc_index"])


class DevicePlan:
    """covt_device_plan_create: the Id / Geometry plan built on the GPU from tiles already in HBM.

    `d_blob` is a uint8 torch tensor on the device holding the tiles, `offsets` / `sizes` the tiles'
    byte ranges in it (host arrays or device tensors).  The walk, prefix sums, launch-order sort and
    descriptor fill run on the current torch stream; the result has the host plan's layout exactly
    (Plan.streams / Plan.descs / Plan.family_counts with the same options, split chunks included)."""

    def __init__(self, d_blob, offsets, sizes, fmt: int = FORMAT_GENC, id_mode: int = ID_FORMAT, stream=None,
                 options: Optional[PlanOptions] = None):
        import torch

        self.device = d_blob.device
        if d_blob.dtype != torch.uint8 or not d_blob.is_contiguous() or d_blob.device.type != "cuda":
            raise IllegalArgumentException("d_blob must be a contiguous uint8 device tensor")
        self.d_in = d_blob
        as_dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64) if not torch.is_tensor(a) else a,
                                           dtype=torch.int64).to(self.device).contiguous()
        self.d_off, self.d_size = as_dev(offsets), as_dev(sizes)
        if self.d_off.numel() != self.d_size.numel():
            raise IllegalArgumentException("offsets and sizes differ in length")
        self.n_tiles = int(self.d_off.numel())
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _raise(lib().covt_device_plan_create_opts(d_blob.data_ptr(), d_blob.numel(), self.d_off.data_ptr(),
                                                      self.d_size.data_ptr(), self.n_tiles, fmt, id_mode,
                                                      C.byref(options) if options is not None else None,
                                                      _stream(stream, self.device), C.byref(h)),
                   "covt_device_plan_create")
        self._h = h
        L = lib()
        self.num_streams = L.covt_device_plan_num_streams(h)
        self.num_descs = L.covt_device_plan_num_descs(h)
        self.output_bytes = L.covt_device_plan_output_bytes(h)
        self.family_counts = np.zeros(NUM_FAMILIES, dtype=np.int64)
        L.covt_device_plan_family_counts(h, _ptr(self.family_counts, C.c_int64))
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.covt_device_plan_totals(h, C.byref(a), C.byref(b), C.byref(c))
        self.in_bytes, self.out_payload, self.vertices = a.value, b.value, c.value
        self.num_property_columns = L.covt_device_plan_num_property_columns(h)
        self.property_bytes = L.covt_device_plan_property_bytes(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().covt_device_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def host_copy(self):
        """(stream records in tile order, descriptors in launch order, tile statuses) as host arrays."""
        info = np.zeros(self.num_streams, dtype=STREAM_INFO_DTYPE)
        descs = np.zeros(self.num_descs * 32, dtype=np.uint8)
        st = np.zeros(max(self.n_tiles, 1), dtype=np.int32)
        _raise(lib().covt_device_plan_copy(self._h, info.ctypes.data, descs.ctypes.data, _ptr(st, C.c_int32)),
               "covt_device_plan_copy")
        return info, descs, st[:self.n_tiles]

    def _copy(self, kind: str, entry: str):
        """(a product's records in tile order, its descriptors in launch order) as host arrays."""
        q = _PRODUCTS[kind]
        if q.needs_geometry:
            self.geometry()
        n = getattr(self, q.count)
        info = np.zeros(n, dtype=q.info_dtype)
        descs = np.zeros(n * q.desc_size, dtype=np.uint8).view(q.desc_dtype)
        _raise(getattr(lib(), entry)(self._h, info.ctypes.data, descs.ctypes.data), entry)
        return info, descs

    def _alloc(self, kind: str):
        q = _PRODUCTS[kind]
        if q.needs_geometry:
            self.geometry()
        return q.alloc(self, self.device)

    def property_copy(self):
        """(property records in tile order, property descriptors in materialization order) as host arrays
        (plans made with PLAN_PROPERTIES in the options' flags; Plan.props / Plan.pdescs of the host plan)."""
        return self._copy("property", "covt_device_plan_property_copy")

    def alloc_properties(self):
        """(property buffer, property results) on the device, sized for this plan's property columns."""
        return self._alloc("property")

    def materialize(self, d_out, d_res, d_props, d_pres, stream=None):
        """Enqueue the property materialization over this plan's property descriptors (after decode())."""
        _raise(lib().covt_device_plan_materialize(self._h, self.d_in.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                                  d_props.data_ptr(), d_pres.data_ptr(), _stream(stream, self.device)),
               "covt_device_plan_materialize")

    def alloc(self):
        """(output buffer, result buffer) on the device, sized for this plan."""
        import torch

        return (torch.zeros(max(self.output_bytes, 16), dtype=torch.uint8, device=self.device),
                torch.zeros(max(self.num_descs, 1) * 2, dtype=torch.int32, device=self.device))

    def decode(self, d_out, d_res, stream=None):
        """Enqueue the grouped decode launch over this plan's descriptors."""
        _raise(lib().covt_device_plan_decode(self._h, self.d_in.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                             _stream(stream, self.device)), "covt_device_plan_decode")

    def geometry(self, stream=None):
        """Build the geometry-column records and descriptors on the device (once; synchronises the
        stream): Plan.geom / Plan.gdescs / Plan.assembly_bytes without the host plan."""
        import torch

        with torch.cuda.device(self.device):
            _raise(lib().covt_device_plan_geometry(self._h, _stream(stream, self.device)), "covt_device_plan_geometry")
        self.num_geometry_columns = lib().covt_device_plan_num_geometry_columns(self._h)
        self.assembly_bytes = lib().covt_device_plan_assembly_bytes(self._h)
        self.wkb_bytes = lib().covt_device_plan_wkb_bytes(self._h)
        self.bbox_bytes = lib().covt_device_plan_bbox_bytes(self._h)
        self.measures_bytes = lib().covt_device_plan_measures_bytes(self._h)
        self.select_bytes = lib().covt_device_plan_select_bytes(self._h)
        self.simplify_bytes = lib().covt_device_plan_simplify_bytes(self._h)
        self.mvt_bytes = lib().covt_device_plan_mvt_bytes(self._h)
        return self.num_geometry_columns

    def geometry_copy(self):
        """(geometry records in tile order, geometry descriptors in launch order) as host arrays."""
        return self._copy("geometry", "covt_device_plan_geometry_copy")

    def alloc_assembly(self):
        """(assembly buffer, geometry results) on the device, sized for this plan's geometry columns."""
        return self._alloc("geometry")

    def assemble(self, d_out, d_res, d_asm, d_gres, stream=None):
        """Enqueue the geometry assembly over this plan's geometry descriptors (after decode())."""
        self.geometry(stream)
        _raise(lib().covt_device_plan_assemble(self._h, d_out.data_ptr(), d_res.data_ptr(), d_asm.data_ptr(),
                                               d_gres.data_ptr(), _stream(stream, self.device)),
               "covt_device_plan_assemble")

    def wkb_copy(self):
        """(WKB records in tile order, WKB descriptors in launch order) as host arrays (Plan.wkb / Plan.wdescs)."""
        return self._copy("wkb", "covt_device_plan_wkb_copy")

    def alloc_wkb(self):
        """(WKB buffer, WKB results) on the device, sized for this plan's geometry columns."""
        return self._alloc("wkb")

    def wkb(self, d_out, d_res, d_asm, d_gres, d_wkb, d_wres, stream=None, d_xf=None, kinds: int = 0):
        """Enqueue the WKB serialization over this plan's descriptors (after assemble() on the same stream).
        d_xf: a device tensor holding one GEO_XFORM_DTYPE entry per geometry column in launch order (the
        device plan does not read extents: the table comes from a host plan or the caller), kinds its promise."""
        self.geometry(stream)
        if d_xf is not None:
            L = lib()
            _raise(L.covt_geometry_wkb_projected_device(
                d_out.data_ptr(), L.covt_device_plan_geometry_descs_device(self._h), d_asm.data_ptr(),
                d_gres.data_ptr(), L.covt_device_plan_wkb_descs_device(self._h), self.num_geometry_columns,
                d_wkb.data_ptr(), d_wres.data_ptr(), d_xf.data_ptr(), kinds, _stream(stream, self.device)),
                "covt_geometry_wkb_projected_device")
            return
        _raise(lib().covt_device_plan_wkb(self._h, d_out.data_ptr(), d_res.data_ptr(), d_asm.data_ptr(),
                                          d_gres.data_ptr(), d_wkb.data_ptr(), d_wres.data_ptr(),
                                          _stream(stream, self.device)), "covt_device_plan_wkb")

    def bbox_copy(self):
        """(bounding-box records in tile order, descriptors in launch order) as host arrays (Plan.bbox /
        Plan.bdescs)."""
        return self._copy("bbox", "covt_device_plan_bbox_copy")

    def alloc_bbox(self):
        """(bounding-box buffer, results) on the device, sized for this plan's geometry columns."""
        return self._alloc("bbox")

    def bbox(self, d_asm, d_gres, d_bbox, d_bres, stream=None, d_xf=None, kinds: int = 0):
        """Enqueue the bounding boxes over this plan's descriptors (after assemble() on the same stream).
        d_xf / kinds: as wkb()."""
        self.geometry(stream)
        if d_xf is not None:
            L = lib()
            _raise(L.covt_geometry_bbox_projected_device(
                L.covt_device_plan_geometry_descs_device(self._h), d_asm.data_ptr(), d_gres.data_ptr(),
                L.covt_device_plan_bbox_descs_device(self._h), self.num_geometry_columns, d_bbox.data_ptr(),
                d_bres.data_ptr(), d_xf.data_ptr(), kinds, _stream(stream, self.device)),
                "covt_geometry_bbox_projected_device")
            return
        _raise(lib().covt_device_plan_bbox(self._h, d_asm.data_ptr(), d_gres.data_ptr(), d_bbox.data_ptr(),
                                           d_bres.data_ptr(), _stream(stream, self.device)), "covt_device_plan_bbox")

    def measures_copy(self):
        """(measures records in tile order, descriptors in launch order) as host arrays (Plan.measures /
        Plan.mdescs)."""
        return self._copy("measures", "covt_device_plan_measures_copy")

    def alloc_measures(self):
        """(measures buffer, results) on the device, sized for this plan's geometry columns."""
        return self._alloc("measures")

    def measures(self, d_out, d_asm, d_gres, d_measures, d_mres, stream=None):
        """Enqueue the measures over this plan's descriptors (after assemble() on the same stream); d_out is
        the decode output, which holds the GeometryTypes."""
        self.geometry(stream)
        _raise(lib().covt_device_plan_measures(self._h, d_out.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(),
                                               d_measures.data_ptr(), d_mres.data_ptr(),
                                               _stream(stream, self.device)), "covt_device_plan_measures")


    def select_copy(self):
        """(select records in tile order, descriptors in launch order) as host arrays (Plan.select /
        Plan.sdescs)."""
        return self._copy("select", "covt_device_plan_select_copy")

    def alloc_select(self):
        """(select buffer, results) on the device, sized for this plan's geometry columns."""
        return self._alloc("select")

    def select(self, d_wkb, d_wres, d_select, d_sres, stream=None):
        """Enqueue the selection over this plan's descriptors (after wkb() and whatever wrote the masks into
        d_select on the same stream)."""
        self.geometry(stream)
        _raise(lib().covt_device_plan_select(self._h, d_wkb.data_ptr(), d_wres.data_ptr(), d_select.data_ptr(),
                                             d_sres.data_ptr(), _stream(stream, self.device)),
               "covt_device_plan_select")

    def where_bind(self, where: "Where", blob) -> np.ndarray:
        """covt_where_bind over this plan's record copies: int32 [num_geometry_columns, WHERE_MAX_CLAUSES] in
        launch order.  `blob`: the tiles' bytes on the host (the column names are read from them)."""
        ginfo, _ = self.geometry_copy()
        pinfo, _ = self.property_copy()
        raw = _u8(blob)
        out = np.full((max(ginfo.size, 1), WHERE_MAX_CLAUSES), -1, dtype=np.int32)
        _raise(lib().covt_where_bind(C.byref(where), ginfo.ctypes.data, ginfo.size, pinfo.ctypes.data, pinfo.size,
                                     _ptr(raw, C.c_uint8), raw.size, out.ctypes.data), "covt_where_bind")
        return out[:ginfo.size]

    def select_where(self, d_props, d_pres, d_where, d_bind, d_select, mode: int = WHERE_WRITE, d_status=None,
                     stream=None):
        """Enqueue the where pass over this plan's property and select descriptors (after materialize() and
        whatever wrote the masks on the same stream): d_where the Where's bytes and d_bind the table of
        where_bind() as device tensors, d_status an int32 tensor of num_geometry_columns entries or None."""
        self.geometry(stream)
        L = lib()
        _raise(L.covt_select_where_device(L.covt_device_plan_property_descs_device(self._h), d_props.data_ptr(),
                                          d_pres.data_ptr(), self.num_property_columns,
                                          L.covt_device_plan_select_descs_device(self._h), self.num_geometry_columns,
                                          d_where.data_ptr(), d_bind.data_ptr(), int(mode), d_select.data_ptr(),
                                          d_status.data_ptr() if d_status is not None else None,
                                          _stream(stream, self.device)), "covt_select_where_device")

    def select_query(self, d_out, d_asm, d_gres, query: "SelectQuery", d_select, mode: int = WHERE_WRITE,
                     d_status=None, stream=None):
        """Enqueue the query pass over this plan's geometry and select descriptors (after assemble() and whatever
        wrote the masks on the same stream); d_out is the decode output, which holds the GeometryTypes;
        d_status an int32 tensor of num_geometry_columns entries or None."""
        self.geometry(stream)
        L = lib()
        _raise(L.covt_select_query_device(d_out.data_ptr(), L.covt_device_plan_geometry_descs_device(self._h),
                                          d_asm.data_ptr(), d_gres.data_ptr(),
                                          L.covt_device_plan_select_descs_device(self._h), self.num_geometry_columns,
                                          C.byref(query), int(mode), d_select.data_ptr(),
                                          d_status.data_ptr() if d_status is not None else None,
                                          _stream(stream, self.device)), "covt_select_query_device")

    def simplify_copy(self):
        """(simplify records in tile order, descriptors in launch order) as host arrays (Plan.simplify /
        Plan.spdescs)."""
        return self._copy("simplify", "covt_device_plan_simplify_copy")

    def alloc_simplify(self):
        """(simplify buffer, geometry results) on the device, sized for this plan's geometry columns."""
        return self._alloc("simplify")

    def simplify(self, d_out, d_asm, d_gres, shift: int, d_simplify, d_sgres, stream=None, d_shift=None):
        """Enqueue the simplification over this plan's descriptors (after assemble() on the same stream); d_out
        is the decode output, which holds the GeometryTypes.  d_shift: an int32 device tensor with one shift per
        column in launch order, instead of `shift` for all.  The products read the result through
        simplified_geometry_descs_device()."""
        self.geometry(stream)
        _raise(lib().covt_device_plan_simplify(self._h, d_out.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(), int(shift),
                                               d_shift.data_ptr() if d_shift is not None else None,
                                               d_simplify.data_ptr(), d_sgres.data_ptr(), _stream(stream, self.device)),
               "covt_device_plan_simplify")

    def mvt_copy(self):
        """(mvt records in tile order, descriptors in launch order) as host arrays (Plan.mvt / Plan.mvdescs)."""
        return self._copy("mvt", "covt_device_plan_mvt_copy")

    def alloc_mvt(self):
        """(mvt buffer, mvt results) on the device, sized for this plan's geometry columns."""
        return self._alloc("mvt")

    def mvt(self, d_out, d_asm, d_gres, opts, d_mvt, d_mvres, stream=None, simplified: bool = False):
        """Enqueue the MVT encoding over this plan's descriptors (after assemble() on the same stream; simplified:
        after simplify(), d_asm / d_gres its buffer and results); results in launch order."""
        opts = opts if opts is not None else MvtOptions()
        _raise(lib().covt_device_plan_mvt(self._h, d_out.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(),
                                          1 if simplified else 0, C.addressof(opts), d_mvt.data_ptr(), d_mvres.data_ptr(),
                                          _stream(stream, self.device)), "covt_device_plan_mvt")

    def simplified_geometry_descs_device(self) -> int:
        """Device address of the geometry descriptors that name the simplified columns (launch order)."""
        self.geometry()
        return lib().covt_device_plan_simplified_geometry_descs_device(self._h)


class DeviceSubset:
    """One decode launch over a subset of a DeviceBatch's streams (e.g. BASELINE configs 2-4, which are
    stream selections of fixture tiles); its own descriptor table and result array on the device."""

    def __init__(self, batch: DeviceBatch, mask):
        import torch

        self.batch = batch
        descs, self.family_counts, self.stream_index = batch.plan.subset_descs(mask)
        self.num_descs = int(self.stream_index.size)
        self.num_streams = int((self.stream_index >= 0).sum())
        self.d_desc = torch.from_numpy(descs).to(batch.device) if self.num_descs else \
            torch.zeros(32, dtype=torch.uint8, device=batch.device)
        self.d_res = torch.zeros(max(self.num_descs, 1) * 2, dtype=torch.int32, device=batch.device)

    def decode(self, stream=None):
        b = self.batch
        _raise(lib().covt_decode_streams_device_grouped(b.d_in.data_ptr(), self.d_desc.data_ptr(),
                                                        _ptr(self.family_counts, C.c_int64), b.d_out.data_ptr(),
                                                        self.d_res.data_ptr(), _stream(stream, b.device)),
               "covt_decode_streams_device_grouped")

    def decode_graph(self):
        """This subset's launch replayed from a captured HIP graph on the current torch stream (as
        DeviceBatch.decode_graph): the split-record memset, the fork, every family and chunk kernel on
        its queue and the join become one graph launch."""
        import torch

        g = getattr(self, "_graph", None)
        if g is None:
            dev = self.batch.device
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):  # the fork streams and events exist before the capture
                self.decode(side)
            torch.cuda.current_stream(dev).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.decode(torch.cuda.current_stream(dev))
            self._graph = g
        g.replay()

    def results(self):
        """(full output bytes, results[k, 2] of the subset's k streams, their plan-order indices)."""
        out = self.batch.d_out.cpu().numpy()[:self.batch.plan.output_bytes]
        res = self.d_res.cpu().numpy().reshape(-1, 2)[:self.num_descs]
        prim = self.stream_index >= 0
        return out, res[prim], self.stream_index[prim]


# ---------------------------------------------------------------------------
# CovtParser mirror (Id + Geometry columns)
# ---------------------------------------------------------------------------
@dataclass
class GeometryColumn:
    """record GeometryColumn, CovtParser.java:29-36 (absent streams are None)."""
    geometryTypes: Optional[np.ndarray] = None
    geometryOffsets: Optional[np.ndarray] = None
    partOffsets: Optional[np.ndarray] = None
    ringOffsets: Optional[np.ndarray] = None
    vertexOffsets: Optional[np.ndarray] = None
    vertexBuffer: Optional[np.ndarray] = None


@dataclass
class GeoArrowGeometry:
    """One assembled geometry column (include/covt.h "Geometry assembly"): nested offsets
    feature -> parts -> rings -> coordinates, coords int32 [k, 2]; polygon rings closed."""
    geometry_offsets: np.ndarray
    part_offsets: np.ndarray
    ring_offsets: np.ndarray
    coords: np.ndarray

    def feature(self, i: int):
        """Parts of feature i as lists of rings, each an int32 [m, 2] array."""
        g, p, r = self.geometry_offsets, self.part_offsets, self.ring_offsets
        return [[self.coords[r[k]:r[k + 1]] for k in range(p[j], p[j + 1])] for j in range(g[i], g[i + 1])]


@dataclass
class WkbColumn:
    """One geometry column as an Arrow binary column of little-endian ISO WKB values (include/covt.h
    "Geometry as WKB"): int32 offsets [n + 1] into data; feature i is data[offsets[i]:offsets[i + 1]]."""
    offsets: np.ndarray
    data: np.ndarray

    def __len__(self) -> int:
        return int(self.offsets.size) - 1

    def feature(self, i: int) -> bytes:
        if not 0 <= i < len(self):
            raise IndexError(i)
        return bytes(self.data[int(self.offsets[i]):int(self.offsets[i + 1])])


@dataclass
class MvtColumn:
    """One geometry column as MVT geometry (include/covt.h "Geometry as MVT"): per feature its GeomType (types,
    uint8: 1 point, 2 line, 3 polygon) and the payload of Feature.geometry, an Arrow binary column: int32 offsets
    [n + 1] into data; feature i is data[offsets[i]:offsets[i + 1]], empty for a feature without a coordinate."""
    types: np.ndarray
    offsets: np.ndarray
    data: np.ndarray
    n_empty: int = 0

    def __len__(self) -> int:
        return int(self.offsets.size) - 1

    def feature(self, i: int) -> bytes:
        if not 0 <= i < len(self):
            raise IndexError(i)
        return bytes(self.data[int(self.offsets[i]):int(self.offsets[i + 1])])


@dataclass
class BboxColumn:
    """One geometry column's bounding boxes (include/covt.h "Geometry bounding boxes"), the four arrays of
    a GeoParquet bbox covering column: float64 views of n values each, NaN in all four for a feature
    without a coordinate; extent = (xmin, ymin, xmax, ymax) of the column, n_empty its NaN rows."""
    xmin: np.ndarray
    ymin: np.ndarray
    xmax: np.ndarray
    ymax: np.ndarray
    extent: np.ndarray
    n_empty: int = 0

    def __len__(self) -> int:
        return int(self.xmin.size)

    def as_struct(self) -> np.ndarray:
        """(n, 4) float64: one (xmin, ymin, xmax, ymax) row per feature."""
        return np.stack([self.xmin, self.ymin, self.xmax, self.ymax], axis=1)


@dataclass
class MeasuresColumn:
    """One geometry column's measures (include/covt.h "Geometry measures"), in tile pixels: per feature its
    area (float64, shell minus holes; +0.0 unless a polygon type), its length (float64, line length or
    polygon perimeter; +0.0 for point types) and num_coords (int32, the points of its WKB value)."""
    area: np.ndarray
    length: np.ndarray
    num_coords: np.ndarray

    def __len__(self) -> int:
        return int(self.area.size)


@dataclass
class SelectedColumn:
    """The kept features of one geometry column (include/covt.h "Feature selection"): index, the int32 feature
    numbers in increasing order, and wkb, their WKB values as a column of their own.  The ids, boxes, measures and
    property values of the kept features are array[index]."""
    index: np.ndarray
    wkb: WkbColumn

    def __len__(self) -> int:
        return int(self.index.size)


@dataclass
class PropertyColumn:
    """One materialized property (sub)column (include/covt.h "Property columns"): Arrow-style validity
    bitmap (LSB first) + values at feature positions (BOOLEAN: bitmap; INT64: int64; FLOAT: float32;
    STRING: int32 dictionary index) + dictionary offsets / UTF-8 bytes."""
    name: str
    type: int
    n_features: int
    validity: np.ndarray
    values: np.ndarray
    dict_offsets: Optional[np.ndarray]
    dict_bytes: Optional[np.ndarray]
    n_valid: int

    def valid(self, i: int) -> bool:
        return bool((int(self.validity[i >> 3]) >> (i & 7)) & 1)

    def value(self, i: int):
        """CovtParser's Optional for feature i: None (empty) or the value."""
        if not self.valid(i):
            return None
        if self.type == PROP_BOOLEAN:
            return bool((int(self.values[i >> 3]) >> (i & 7)) & 1)
        if self.type == PROP_INT64:
            return int(self.values[i])
        if self.type == PROP_FLOAT:
            return float(self.values[i])
        k = int(self.values[i])
        return bytes(self.dict_bytes[self.dict_offsets[k]:self.dict_offsets[k + 1]]).decode("utf-8")

    def to_list(self):
        """The List<Optional> of decodePropertyColumn (CovtParser.java:276-354)."""
        return [self.value(i) for i in range(self.n_features)]


@dataclass
class LayerColumns:
    layer: int
    ids: Optional[np.ndarray]
    geometry: GeometryColumn
    num_bits: int = 0
    column_type: int = 0
    properties: Optional[dict] = None
    wkb: Optional[WkbColumn] = None  # the layer's geometries, one WKB value per feature
    bbox: Optional[BboxColumn] = None  # their bounding boxes, the bbox covering column beside wkb
    crs: int = CRS_TILE  # the CRS of wkb and bbox (geometry.vertexBuffer stays in tile pixels)
    measures: Optional["MeasuresColumn"] = None  # their area, length and num_coords, in tile pixels whatever the crs
    selected: Optional["SelectedColumn"] = None  # decode_covt(select=...): the features the predicate keeps
    simplified: Optional["GeoArrowGeometry"] = None  # decode_covt(simplify=shift): the simplified column
    mvt: Optional["MvtColumn"] = None  # decode_covt(mvt=MvtOptions): the geometries as MVT command streams


_GEOM_FIELD = {GEOMETRY_TYPES: "geometryTypes", GEOMETRY_OFFSETS: "geometryOffsets", PART_OFFSETS: "partOffsets",
               RING_OFFSETS: "ringOffsets", VERTEX_OFFSETS: "vertexOffsets", VERTEX_BUFFER: "vertexBuffer"}


def split_layers(plan: Plan, out: np.ndarray, res: np.ndarray, tile: int = 0) -> List[LayerColumns]:
    layers = {}
    for i in np.nonzero(plan.streams["tile"] == tile)[0]:
        s = plan.streams[i]
        _raise(int(res[i][0]), "stream %d (layer %d, type %d)" % (i, s["layer"], s["stream_type"]))
        if int(s["column_kind"]) == 2:  # property streams: see Plan.property_column
            continue
        lc = layers.setdefault(int(s["layer"]), LayerColumns(int(s["layer"]), None, GeometryColumn()))
        arr = plan.stream_array(out, int(i))
        if int(s["column_kind"]) == 0:
            lc.ids = arr
        else:
            setattr(lc.geometry, _GEOM_FIELD[int(s["stream_type"])], arr)
            lc.num_bits = int(s["num_bits"])
            lc.column_type = int(s["column_type"])
    return [layers[k] for k in sorted(layers)]


class CovtParser:
    @staticmethod
    def decode_covt(covt_buffer: bytes, fmt: int = FORMAT_GENC, id_mode: int = ID_FORMAT,
                    properties: bool = False, tile_id=None, crs: int = CRS_TILE,
                    select: Optional[SelectPred] = None, simplify: Optional[int] = None,
                    where: Optional["Where"] = None, mvt: Optional["MvtOptions"] = None,
                    query: Optional["SelectQuery"] = None) -> List[LayerColumns]:
        """CovtParser.decodeCovt (CovtParser.java:53-133) decoded on the GPU: Id + Geometry columns, and with
        ``properties`` every property column as a PropertyColumn (LayerColumns.properties, by name).
        ``tile_id`` = (z, x, y) and ``crs`` give every layer's wkb / bbox in that CRS (LayerColumns.crs).
        ``select``, a SelectPred whose window is in that CRS, gives every layer the features it keeps
        (LayerColumns.selected: their numbers and their WKB values; the other columns are array[selected.index]).
        ``simplify``, a shift, gives every layer's wkb, bbox, measures and selected from the column simplified to
        the grid of 2^shift tile pixels, and that column as LayerColumns.simplified; None: no simplification.
        ``where``, a Where, keeps in LayerColumns.selected only the features whose properties satisfy it (with
        ``select`` both must hold); it implies the property plan, and a layer without a named column sees that
        clause's values as absent.
        ``mvt``, an MvtOptions, gives every layer's geometries as MVT command streams (LayerColumns.mvt), from the
        simplified column when ``simplify`` is given; mvt_layer_bytes and mvt_tile_bytes wrap them into a tile.
        ``query``, a SelectQuery (tile pixels, whatever ``crs``), keeps in LayerColumns.selected only the features
        in that exact relation with its window (with ``select`` and ``where`` all must hold), of the simplified
        column when ``simplify`` is given."""
        if crs != CRS_TILE and tile_id is None:
            raise IllegalArgumentException("a CRS other than CRS_TILE needs the tile's (z, x, y)")
        geo = (crs, [tile_id]) if crs != CRS_TILE else (None, None)
        plan = Plan.from_tiles([covt_buffer], fmt, id_mode, PLAN_PROPERTIES if properties or where is not None else 0)
        _raise(int(plan.tile_status[0]), "decodeLayerMetadata")
        out, res = plan.decode_host()
        layers = split_layers(plan, out, res, 0)
        for lc in layers:
            lc.crs = crs
        if plan.num_geometry_columns:
            by_layer = {lc.layer: lc for lc in layers}
            if simplify is not None:
                plan.set_simplify(int(simplify))  # (the host products below read the simplified column)
                sbuf, sgres = plan.simplify_host(int(simplify))
                for c in range(plan.num_geometry_columns):
                    lc = by_layer.get(int(plan.simplify["layer"][c]))
                    if lc is not None and int(sgres["status"][c]) == OK:  # (a failed column keeps simplified = None)
                        lc.simplified = plan.simplified_arrays(sbuf, sgres, c)
            wbuf, wres = plan.wkb_host(*geo)
            for c in range(plan.num_geometry_columns):
                lc = by_layer.get(int(plan.wkb["layer"][c]))
                if lc is not None and int(wres["status"][c]) == OK:  # (a failed column keeps wkb = None)
                    lc.wkb = plan.wkb_column(wbuf, wres, c)
            bbuf, bres = plan.bbox_host(*geo)
            for c in range(plan.num_geometry_columns):
                lc = by_layer.get(int(plan.bbox["layer"][c]))
                if lc is not None and int(bres["status"][c]) == OK:  # (a failed column keeps bbox = None)
                    lc.bbox = plan.bbox_column(bbuf, bres, c)
            mbuf, mres = plan.measures_host()
            for c in range(plan.num_geometry_columns):
                lc = by_layer.get(int(plan.measures["layer"][c]))
                if lc is not None and int(mres["status"][c]) == OK:  # (a failed column keeps measures = None)
                    lc.measures = plan.measures_column(mbuf, mres, c)
            if mvt is not None:
                vbuf, vres = plan.mvt_host(mvt)
                for c in range(plan.num_geometry_columns):
                    lc = by_layer.get(int(plan.mvt["layer"][c]))
                    if lc is not None and int(vres["status"][c]) == OK:  # (a failed column keeps mvt = None)
                        lc.mvt = plan.mvt_column(vbuf, vres, c)
            if select is not None or where is not None or query is not None:
                sbuf, sres = plan.select_host(select, *geo, where=where, query=query)
                for c in range(plan.num_geometry_columns):
                    lc = by_layer.get(int(plan.select["layer"][c]))
                    if lc is not None and int(sres["status"][c]) == OK:  # (a failed column keeps selected = None)
                        lc.selected = plan.select_column(sbuf, sres, c)
        if properties and plan.num_property_columns:
            buf, pres = plan.properties_host()
            by_layer = {lc.layer: lc for lc in layers}
            for c in range(plan.num_property_columns):
                L = int(plan.props["layer"][c])
                lc = by_layer.setdefault(L, LayerColumns(L, None, GeometryColumn()))
                if lc.properties is None:
                    lc.properties = {}
                col = plan.property_column(buf, pres, c)
                lc.properties[col.name] = col
            layers = [by_layer[k] for k in sorted(by_layer)]
        return layers


# ---- MVT tile writer (host side, the framing of vector_tile.proto 2.1 around the device's command streams) ----
def _pb_varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _pb_bytes(field: int, payload: bytes) -> bytes:
    return _pb_varint(field << 3 | 2) + _pb_varint(len(payload)) + payload


def _mvt_value(ptype: int, v) -> bytes:
    """A Tile.Value message: STRING string_value, FLOAT float_value, INT64 uint_value (>= 0) or sint_value,
    BOOLEAN bool_value."""
    if ptype == PROP_STRING:
        return _pb_bytes(1, v.encode("utf-8"))
    if ptype == PROP_FLOAT:
        return b"\x15" + struct.pack("<f", v)
    if ptype == PROP_INT64:
        return b"\x28" + _pb_varint(v) if v >= 0 else b"\x30" + _pb_varint(((v << 1) ^ (v >> 63)) & 0xFFFFFFFFFFFFFFFF)
    return b"\x38" + (b"\x01" if v else b"\x00")


def mvt_layer_bytes(name: str, extent: int, column: "MvtColumn", ids=None, properties=None, index=None) -> bytes:
    """One complete Tile.layers entry (the field-3 record) of an MVT 2.1 tile around an MvtColumn: version 2,
    name, features, keys, values, extent.  A feature carries its id (when ``ids`` is given), its packed tags
    (when it has any), its type and its geometry; features with an empty value are left out.  ``index`` (for
    example LayerColumns.selected.index) restricts and orders the features written.  ``properties``: a dict
    of PropertyColumns (LayerColumns.properties) or a sequence of them, one key per (sub)column in that order;
    a feature gets a tag where the validity bit is set.  Values are deduplicated by kind and exact value
    (floats by bit pattern) in first-use order."""
    props = list(properties.values()) if isinstance(properties, dict) else list(properties or ())
    values: List[bytes] = []
    value_index: dict = {}
    feats = bytearray()
    for i in (range(len(column)) if index is None else (int(k) for k in index)):
        geom = column.feature(i)
        if not geom:
            continue
        f = bytearray()
        if ids is not None:
            f += b"\x08" + _pb_varint(int(ids[i]) & 0xFFFFFFFFFFFFFFFF)
        tags = bytearray()
        for k, pc in enumerate(props):
            v = pc.value(i)
            if v is None:
                continue
            enc = _mvt_value(pc.type, v)
            j = value_index.get(enc)
            if j is None:
                j = value_index[enc] = len(values)
                values.append(enc)
            tags += _pb_varint(k) + _pb_varint(j)
        if tags:
            f += _pb_bytes(2, bytes(tags))
        f += b"\x18" + _pb_varint(int(column.types[i])) + _pb_bytes(4, geom)
        feats += _pb_bytes(2, bytes(f))
    layer = (b"\x78\x02" + _pb_bytes(1, name.encode("utf-8")) + bytes(feats)
             + b"".join(_pb_bytes(3, pc.name.encode("utf-8")) for pc in props)
             + b"".join(_pb_bytes(4, v) for v in values) + b"\x28" + _pb_varint(int(extent)))
    return _pb_bytes(3, layer)


def mvt_tile_bytes(layers) -> bytes:
    """A complete MVT tile: the concatenation of mvt_layer_bytes records."""
    return b"".join(layers)


def version() -> str:
    return lib().covt_version().decode()


# the files whose sha256 (in this order) the Makefile compiles into covt_version() as "src:<16 hex>"
_BUILD_SOURCES = (  # the Makefile's SRC, then its HDR, one to one
    ("csrc/covt_decode.hip", "csrc/covt_assemble.hip", "csrc/covt_props.hip", "csrc/covt_plan_device.hip",
     "csrc/covt_wkb.hip", "csrc/covt_bbox.hip", "csrc/covt_measures.hip", "csrc/covt_select.hip",
     "csrc/covt_simplify.hip", "csrc/covt_where.hip", "csrc/covt_mvt.hip", "csrc/covt_query.hip", "csrc/covt_host.cpp")
    + ("../include/covt.h", "csrc/covt_internal.h", "csrc/covt_wave.h", "csrc/covt_segscan.h", "csrc/covt_walk.h",
       "csrc/covt_props_plan.h",
       "csrc/covt_scratch.h", "csrc/covt_coop.h", "csrc/covt_wkb_plan.h", "csrc/covt_bbox_plan.h",
       "csrc/covt_measures_plan.h", "csrc/covt_select_plan.h", "csrc/covt_simplify_plan.h", "csrc/covt_geo_plan.h", "csrc/covt_arena.h", "csrc/covt_split_plan.h",
       "csrc/covt_container.h", "csrc/covt_where_plan.h", "csrc/covt_mvt_plan.h", "csrc/covt_products.h",
       "csrc/covt_query_plan.h"))


def source_build_id() -> str:
    """sha256 prefix of the library sources as they are in this tree (the Makefile's BUILD_ID)."""
    import hashlib

    h = hashlib.sha256()
    for f in _BUILD_SOURCES:
        with open(os.path.join(_HERE, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def library_build_id() -> str:
    """The build id compiled into the loaded libcovt.so (covt_version)."""
    v = version()
    return v.rsplit("src:", 1)[1] if "src:" in v else "unknown"

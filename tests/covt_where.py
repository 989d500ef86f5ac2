"""Reference property predicates (include/covt.h "Property predicates"): what the where pass of covt_where.hip is
held to, byte for byte.  where_ref is written straight from the definition in numpy and plain Python (a
dictionary entry's verdict is Python's bytes ==); the ctypes structs mirror the blob so the tests build
predicates without the product's helpers."""
import ctypes as C

import numpy as np

MAX_CLAUSES, MAX_VALUES, MAX_TEXT, MAX_IN = 8, 32, 1024, 16
EQ, NE, LT, LE, GT, GE, IN, NOT_IN, IS_NULL, NOT_NULL = range(10)
BOOL, INT, REAL, STRING = 1, 2, 4, 8
NULL_MATCHES = 1
WRITE, AND = 0, 1
T_BOOLEAN, T_INT64, T_FLOAT, T_STRING = 0, 1, 2, 3  # COVT_PROP_*
OK, INVALID_ARG = 0, -6


class Value(C.Structure):  # covt_where_value
    _fields_ = [("i", C.c_int64), ("d", C.c_double), ("str_off", C.c_int32), ("str_len", C.c_int32),
                ("kinds", C.c_uint32), ("b", C.c_int32)]


class Clause(C.Structure):  # covt_where_clause
    _fields_ = [("op", C.c_int32), ("flags", C.c_uint32), ("first_value", C.c_int32), ("n_values", C.c_int32),
                ("name_off", C.c_int32), ("name_len", C.c_int32), ("reserved", C.c_int32 * 2)]


class Blob(C.Structure):  # covt_where
    _fields_ = [("size", C.c_uint32), ("n_clauses", C.c_uint32), ("n_values", C.c_uint32), ("text_len", C.c_uint32),
                ("clauses", Clause * MAX_CLAUSES), ("values", Value * MAX_VALUES), ("text", C.c_uint8 * MAX_TEXT)]


class Literal(C.Structure):  # covt_where_literal
    _fields_ = [("kinds", C.c_uint32), ("b", C.c_int32), ("i", C.c_int64), ("d", C.c_double), ("str", C.c_char_p),
                ("str_len", C.c_int32), ("reserved", C.c_int32)]


def lit(x=None, *, kinds=None, b=0, i=0, d=0.0, s=b""):
    """A literal as a dict {kinds, b, i, d, s}: from a Python value by the binding's rule (bool -> BOOL; int ->
    INT, plus REAL when |x| <= 2^53; float -> REAL, plus INT when integral and inside int64; str / bytes ->
    STRING), or field by field with `kinds` given."""
    if kinds is not None:
        return {"kinds": kinds, "b": b, "i": i, "d": d, "s": bytes(s)}
    if isinstance(x, bool):
        return {"kinds": BOOL, "b": int(x), "i": 0, "d": 0.0, "s": b""}
    if isinstance(x, int):
        real = abs(x) <= 2 ** 53
        return {"kinds": INT | (REAL if real else 0), "b": 0, "i": x, "d": float(x) if real else 0.0, "s": b""}
    if isinstance(x, float):
        whole = x == x and abs(x) != float("inf") and x == int(x) and -2.0 ** 63 <= x < 2.0 ** 63
        return {"kinds": REAL | (INT if whole else 0), "b": 0, "i": int(x) if whole else 0, "d": x, "s": b""}
    raw = x.encode("utf-8") if isinstance(x, str) else bytes(x)
    return {"kinds": STRING, "b": 0, "i": 0, "d": 0.0, "s": raw}


def make_blob(clauses):
    """The blob of clauses [(name, op, flags, [literal dicts])], laid out as covt_where_add_clause lays it out:
    per clause its name, then its string literals, appended to the text."""
    w = Blob()
    w.size = C.sizeof(Blob)
    text = b""
    for name, op, flags, lits in clauses:
        name = name.encode("utf-8") if isinstance(name, str) else bytes(name)
        c = w.clauses[w.n_clauses]
        c.op, c.flags, c.first_value, c.n_values = op, flags, w.n_values, len(lits)
        c.name_off, c.name_len = len(text), len(name)
        text += name
        for L in lits:
            v = w.values[w.n_values]
            v.kinds, v.b, v.i, v.d = L["kinds"], L["b"], L["i"], L["d"]
            if L["kinds"] & STRING:
                v.str_off, v.str_len = len(text), len(L["s"])
                text += L["s"]
            w.n_values += 1
        w.n_clauses += 1
    assert len(text) <= MAX_TEXT
    w.text_len = len(text)
    C.memmove(w.text, text, len(text))
    return w


def bits(bitmap, n):
    """The first n bits of an LSB-first bitmap as a bool array."""
    return np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little")[:n].astype(bool)


def pack(flags):
    """An LSB-first bitmap of a bool array."""
    return np.packbits(np.asarray(flags, bool), bitorder="little")


def dict_matches(col, lits):
    """bool per dictionary entry: the entry equals one of the STRING literals.  Entry e is
    dict_bytes[dict_offsets[e] .. dict_offsets[e + 1]) with the offsets clamped to [0, dict_bytes]."""
    nd = max(int(col.get("n_dict", 0)), 0)
    out = np.zeros(nd, bool)
    if not nd:
        return out
    raw = bytes(np.asarray(col["dict_bytes"], np.uint8))
    offs = np.clip(np.asarray(col["dict_offsets"], np.int64), 0, len(raw))
    want = {L["s"] for L in lits if L["kinds"] & STRING}
    for e in range(nd):
        o, end = int(offs[e]), int(offs[e + 1])
        out[e] = raw[o:max(end, o)] in want
    return out


def clause_truth(col, n, op, flags, lits):
    """bool[n]: the truth of one clause over a property column (None: the clause is unbound)."""
    absent = True if op == IS_NULL else False if op == NOT_NULL else bool(flags & NULL_MATCHES)
    if col is None:
        return np.full(n, absent)
    valid = bits(col["validity"], n)
    eq, lt, gt = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    t = col["type"]
    with np.errstate(invalid="ignore"):
        if t == T_BOOLEAN:
            v = bits(col["values"], n)
            for L in lits:
                if L["kinds"] & BOOL:
                    eq |= v == (L["b"] != 0)
        elif t == T_INT64:
            v = np.asarray(col["values"], np.int64)[:n]
            for j, L in enumerate(lits):
                if L["kinds"] & INT:
                    eq |= v == np.int64(L["i"])
                    if j == 0:
                        lt, gt = v < np.int64(L["i"]), v > np.int64(L["i"])
        elif t == T_FLOAT:
            v = np.asarray(col["values"], np.float32)[:n].astype(np.float64)  # (exact)
            for j, L in enumerate(lits):
                if L["kinds"] & REAL:
                    eq |= v == np.float64(L["d"])
                    if j == 0:
                        lt, gt = v < np.float64(L["d"]), v > np.float64(L["d"])
        elif t == T_STRING:
            idx = np.asarray(col["values"], np.int32)[:n].astype(np.int64)
            m = dict_matches(col, lits)
            inside = (idx >= 0) & (idx < m.size)
            eq = inside & (m[np.where(inside, idx, 0)] if m.size else False)
    present = {EQ: eq, IN: eq, NE: ~eq, NOT_IN: ~eq, LT: lt, LE: lt | eq, GT: gt, GE: gt | eq,
               IS_NULL: np.zeros(n, bool), NOT_NULL: np.ones(n, bool)}[op]
    return np.where(valid, present, absent)


def where_ref(columns, n_features, clauses, bind_row, mask_in, mode):
    """(mask uint8[n_features], status) of one geometry column.  columns: the property columns by descriptor
    index, dicts {type, n_features, status, validity, values[, n_dict, dict_offsets, dict_bytes]}; clauses:
    [(op, flags, [literal dicts])]; bind_row[k]: clause k's column, -1 unbound; mask_in: the incoming mask
    (read in AND mode)."""
    n = int(n_features)
    mask_in = np.asarray(mask_in, np.uint8)
    for k in range(len(clauses)):  # the column rule: the lowest clause with a cause
        b = int(bind_row[k])
        if b < -1 or b >= len(columns):
            return np.zeros(n, np.uint8), INVALID_ARG
        if b >= 0 and int(columns[b]["status"]) != OK:
            return np.zeros(n, np.uint8), int(columns[b]["status"])
        if b >= 0 and int(columns[b]["n_features"]) != n:
            return np.zeros(n, np.uint8), INVALID_ARG
    keep = np.ones(n, bool)
    for k, (op, flags, lits) in enumerate(clauses):
        b = int(bind_row[k])
        keep &= clause_truth(columns[b] if b >= 0 else None, n, op, flags, lits)
    if mode == AND:
        keep &= mask_in[:n] != 0
    return keep.astype(np.uint8), OK

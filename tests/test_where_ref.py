"""CPU: the where pass's reference (tests/covt_where.py) against answers written out by hand, and the rules of
covt_where_plan.h in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import numpy as np
import pytest

import covt_where as W
from conftest import ROOT

OPS = [W.EQ, W.NE, W.LT, W.LE, W.GT, W.GE, W.IN, W.NOT_IN, W.IS_NULL, W.NOT_NULL]


def _col(t, values, valid, **kw):
    n = len(valid)
    vals = W.pack(values) if t == W.T_BOOLEAN else np.asarray(
        values, {W.T_INT64: np.int64, W.T_FLOAT: np.float32, W.T_STRING: np.int32}[t])
    return dict(type=t, n_features=n, status=0, validity=W.pack(valid), values=vals, **kw)


def _dict(entries):
    raw = b"".join(entries)
    offs = np.cumsum([0] + [len(e) for e in entries]).astype(np.int32)
    return dict(n_dict=len(entries), dict_offsets=offs, dict_bytes=np.frombuffer(raw, np.uint8))


# a column of each type: the value below the literal, equal to it, above it, then an absent slot;
# present truth per op as (below, equal, above)
ORDERED = {W.EQ: (0, 1, 0), W.NE: (1, 0, 1), W.LT: (1, 0, 0), W.LE: (1, 1, 0), W.GT: (0, 0, 1), W.GE: (0, 1, 1),
           W.IN: (0, 1, 0), W.NOT_IN: (1, 0, 1), W.IS_NULL: (0, 0, 0), W.NOT_NULL: (1, 1, 1)}
# types without an order: (different, equal, different)
UNORDERED = {**ORDERED, W.LT: (0, 0, 0), W.LE: (0, 1, 0), W.GT: (0, 0, 0), W.GE: (0, 1, 0)}
VALID = [1, 1, 1, 0]
COLUMNS = {
    W.T_BOOLEAN: (_col(W.T_BOOLEAN, [0, 1, 0, 1], VALID), W.lit(True), UNORDERED),
    W.T_INT64: (_col(W.T_INT64, [4, 5, 6, 5], VALID), W.lit(5), ORDERED),
    W.T_FLOAT: (_col(W.T_FLOAT, [0.25, 0.5, 0.75, 0.5], VALID), W.lit(0.5), ORDERED),
    W.T_STRING: (_col(W.T_STRING, [0, 1, 2, 1], VALID, **_dict([b"a", b"b", b"c"])), W.lit("b"), UNORDERED),
}


@pytest.mark.parametrize("null_matches", [0, W.NULL_MATCHES])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("t", sorted(COLUMNS))
def test_known_answers(t, op, null_matches):
    """Every op on every column type: present values below / at / above the literal, an absent value, an
    unbound clause, with and without NULL_MATCHES."""
    col, literal, table = COLUMNS[t]
    lits = [] if op in (W.IS_NULL, W.NOT_NULL) else [literal]
    absent = 1 if op == W.IS_NULL else 0 if op == W.NOT_NULL else int(bool(null_matches))
    want = list(table[op]) + [absent]
    ones = np.ones(4, np.uint8)
    mask, st = W.where_ref([col], 4, [(op, null_matches, lits)], [0], ones, W.WRITE)
    assert st == 0 and mask.dtype == np.uint8 and mask.tolist() == want
    mask, st = W.where_ref([col], 4, [(op, null_matches, lits)], [-1], ones, W.WRITE)  # unbound: all absent
    assert st == 0 and mask.tolist() == [absent] * 4
    # a literal of another kind: eq and the orders are undefined (false), NE and NOT_IN their negation
    other = W.lit("x") if t != W.T_STRING else W.lit(5)
    if lits:
        neg = 1 if op in (W.NE, W.NOT_IN) else 0
        mask, _ = W.where_ref([col], 4, [(op, null_matches, [other])], [0], ones, W.WRITE)
        assert mask.tolist() == [neg] * 3 + [absent]


def test_conjunction_modes_and_column_rule():
    a = _col(W.T_INT64, [1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 0, 1])
    s = _col(W.T_STRING, [0, 1, 0, 3, -1, 1], [1, 1, 1, 1, 1, 0], **_dict([b"x", b"", b"x"]))
    clauses = [(W.GE, 0, [W.lit(2)]), (W.IN, W.NULL_MATCHES, [W.lit("x"), W.lit("")])]
    incoming = np.array([1, 0, 0x80, 0xFF, 1, 2], np.uint8)
    m, st = W.where_ref([a, s], 6, clauses, [0, 1], incoming, W.WRITE)
    #                 f: 0 (1 < 2)  1  2  3 (index 3 outside)  4 (a absent)  5 (s absent: matches)
    assert st == 0 and m.tolist() == [0, 1, 1, 0, 0, 1]
    m, st = W.where_ref([a, s], 6, clauses, [0, 1], incoming, W.AND)
    assert st == 0 and m.tolist() == [0, 0, 1, 0, 0, 1]
    assert W.where_ref([a, s], 6, [], [], incoming, W.WRITE)[0].tolist() == [1] * 6  # no clause: true
    assert W.where_ref([a, s], 6, [], [], incoming, W.AND)[0].tolist() == [1, 0, 1, 1, 1, 1]
    # a duplicate entry: index 2 is "x" as index 0 is
    m, _ = W.where_ref([a, s], 6, [(W.EQ, 0, [W.lit("x")])], [1], incoming, W.WRITE)
    assert m.tolist() == [1, 0, 1, 0, 0, 0]
    # the column rule: a failed column, a feature count that differs, a bind entry out of range; the lowest clause wins
    bad = dict(a, status=-2)
    short = dict(a, n_features=5)
    for cols, bind, want in (([bad, s], [0, 1], -2), ([short, s], [0, 1], -6), ([a, s], [0, 2], -6),
                             ([a, s], [-2, 1], -6), ([short, dict(s, status=-3)], [0, 1], -6),
                             ([short, dict(s, status=-3)], [1, 0], -3)):
        m, st = W.where_ref(cols, 6, clauses, bind, incoming, W.AND)
        assert st == want and m.tolist() == [0] * 6
    # garbage dictionary offsets are read clamped to the dictionary's bytes
    g = dict(s, dict_offsets=np.array([-5, 1, 0, 99], np.int32))  # entries "x", "" (inverted), "xx"
    m, _ = W.where_ref([g], 6, [(W.EQ, 0, [W.lit("x")])], [0], incoming, W.WRITE)
    assert m.tolist() == [1, 0, 1, 0, 0, 0]
    # float: widened exactly; NaN equals nothing and is ordered with nothing
    f = _col(W.T_FLOAT, [0.1, np.nan, -0.0, np.inf], [1, 1, 1, 1])
    for op, lit_, want in ((W.EQ, 0.1, [0, 0, 0, 0]), (W.GT, 0.1, [1, 0, 0, 1]), (W.NE, 0.1, [1, 1, 1, 1]),
                           (W.EQ, 0.0, [0, 0, 1, 0]), (W.LE, float("inf"), [1, 0, 1, 1]), (W.GE, 0.0, [1, 0, 1, 1])):
        assert W.where_ref([f], 4, [(op, 0, [W.lit(lit_)])], [0], np.ones(4, np.uint8), W.WRITE)[0].tolist() == want


def test_literal_kinds_and_blob_layout():
    assert W.lit(True)["kinds"] == W.BOOL and W.lit(3)["kinds"] == W.INT | W.REAL
    assert W.lit(2 ** 53 + 1)["kinds"] == W.INT and W.lit(-2 ** 53)["kinds"] == W.INT | W.REAL
    assert W.lit(100.0)["kinds"] == W.REAL | W.INT and W.lit(100.0)["i"] == 100
    assert W.lit(0.5)["kinds"] == W.REAL and W.lit(float("inf"))["kinds"] == W.REAL and W.lit(2.0 ** 63)["kinds"] == W.REAL
    assert W.lit("é")["s"] == b"\xc3\xa9" and W.lit(b"\x00")["kinds"] == W.STRING
    import ctypes as C

    assert (C.sizeof(W.Value), C.sizeof(W.Clause), C.sizeof(W.Blob), C.sizeof(W.Literal)) == (32, 32, 2320, 40)
    w = W.make_blob([("class", W.IN, 0, [W.lit("motorway"), W.lit("trunk")]), ("rank", W.LE, 1, [W.lit(3)])])
    assert (w.size, w.n_clauses, w.n_values, w.text_len) == (2320, 2, 3, 22)
    assert bytes(w.text[:22]) == b"classmotorwaytrunkrank"
    assert (w.clauses[1].name_off, w.clauses[1].name_len, w.clauses[1].first_value, w.clauses[1].flags) == (18, 4, 2, 1)
    assert (w.values[1].str_off, w.values[1].str_len) == (13, 5) and w.values[2].d == 3.0


def test_plan_rules_under_sanitizers(tmp_path):
    """covt_where_plan.h (validation, the single-value comparisons, the bind rule) in a stand-alone program built
    with AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU."""
    exe = str(tmp_path / "where_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "where_plan", "where_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout.split()
    assert p.returncode == 0 and out[:1] == ["ok"] and int(out[1]) > 1000, (p.stdout, p.stderr[-2000:])

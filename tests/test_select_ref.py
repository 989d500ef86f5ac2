"""CPU: the reference selection and predicate of tests/covt_select.py (the definition the GPU passes of
covt_select.hip are held to, include/covt.h "Feature selection"), and the layout rule of covt_select_plan.h.

1. known answers for select_ref: keep all / none / some, zero-length values, non-zero mask bytes other than 1;
2. known answers for predicate_ref: closed window edges on all four sides, an inverted window, empty features
   with and without KEEP_EMPTY, the size cut with +-0.0 and minima of 0, both flags at once;
3. the layout rule and the predicate's argument rule in a stand-alone program under AddressSanitizer + UBSan.
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np

import covt_select as S
from conftest import ROOT

NAN = float("nan")


def _pred(flags=0, window=(0, 0, 0, 0), min_area=0.0, min_length=0.0):
    return SimpleNamespace(flags=flags, window=window, min_area=min_area, min_length=min_length)


def test_select_ref_known_answers():
    offs = np.array([0, 3, 3, 8, 9, 9], np.int32)  # lengths 3, 0, 5, 1, 0
    data = np.arange(9, dtype=np.uint8) + 100
    sel, o, b = S.select_ref(offs, data, [1, 1, 1, 1, 1])
    assert sel.tolist() == [0, 1, 2, 3, 4] and o.tolist() == offs.tolist() and b.tobytes() == data.tobytes()
    sel, o, b = S.select_ref(offs, data, [0, 0, 0, 0, 0])
    assert sel.size == 0 and o.tolist() == [0] and b.size == 0
    sel, o, b = S.select_ref(offs, data, [0, 0x80, 0xFF, 0, 2])  # any non-zero byte keeps
    assert sel.tolist() == [1, 2, 4] and o.tolist() == [0, 0, 5, 5] and b.tolist() == [103, 104, 105, 106, 107]
    sel, o, b = S.select_ref(offs, data, [1, 0, 0, 1, 0])
    assert sel.tolist() == [0, 3] and o.tolist() == [0, 3, 4] and b.tolist() == [100, 101, 102, 108]
    assert sel.dtype == o.dtype == np.int32 and b.dtype == np.uint8
    sel, o, b = S.select_ref([0], [], [])
    assert sel.size == 0 and o.tolist() == [0] and b.size == 0


def test_member_offsets():
    assert S.member_offsets(0) == (0, 0, 0, 16) and S.member_offsets(1) == (0, 16, 32, 48)
    assert S.member_offsets(16) == (0, 16, 80, 160) and S.member_offsets(17) == (0, 32, 112, 192)


def test_predicate_ref_known_answers():
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    # boxes against the window [10, 30] x [20, 40]: touching each side, one unit off each side, inside, empty
    xmin = f8([30, 0, 12, 12, 31, 0, 12, 12, 15, NAN])
    xmax = f8([50, 10, 14, 14, 50, 9, 14, 14, 16, NAN])
    ymin = f8([25, 25, 40, 0, 25, 25, 41, 0, 25, NAN])
    ymax = f8([26, 26, 60, 20, 26, 26, 60, 19, 26, NAN])
    z = np.zeros(10)
    win = _pred(S.WINDOW, (10, 20, 30, 40))
    assert S.predicate_ref(xmin, ymin, xmax, ymax, z, z, win).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1, 0]
    win.flags |= S.KEEP_EMPTY
    assert S.predicate_ref(xmin, ymin, xmax, ymax, z, z, win).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1, 1]
    assert S.predicate_ref(xmin, ymin, xmax, ymax, z, z, _pred()).tolist() == [1] * 9 + [0]
    assert S.predicate_ref(xmin, ymin, xmax, ymax, z, z, _pred(S.KEEP_EMPTY)).tolist() == [1] * 10
    # inverted in x, in y: nothing but (with KEEP_EMPTY) the empty feature
    for w in ((30, 20, 10, 40), (10, 40, 30, 20)):
        assert S.predicate_ref(xmin, ymin, xmax, ymax, z, z, _pred(S.WINDOW, w)).tolist() == [0] * 10
        assert S.predicate_ref(xmin, ymin, xmax, ymax, z, z, _pred(S.WINDOW | S.KEEP_EMPTY, w)).tolist() == [0] * 9 + [1]
        # ... also of a box that spans both ends of the inverted interval
        assert S.predicate_ref(f8([0]), f8([0]), f8([100]), f8([100]), z[:1], z[:1], _pred(S.WINDOW, w)).tolist() == [0]
    # a point window on a corner of a box
    assert S.predicate_ref(f8([5]), f8([6]), f8([7]), f8([8]), z[:1], z[:1], _pred(S.WINDOW, (7, 8, 7, 8))).tolist() == [1]
    # the size cut
    area = f8([4.0, 3.9, 3.9, 0.0, -0.0, 0.0, -96.0, 1e300])
    length = f8([0.0, 8.0, 7.9, 0.0, 0.0, 0.1, 7.0, 0.0])
    b = np.zeros(8)
    size = _pred(S.MIN_SIZE, min_area=4.0, min_length=8.0)
    assert S.predicate_ref(b, b, b, b, area, length, size).tolist() == [1, 1, 0, 1, 1, 0, 0, 1]
    assert S.predicate_ref(b, b, b, b, area, length, _pred(S.MIN_SIZE)).tolist() == [1, 1, 1, 1, 1, 1, 1, 1]  # minima 0
    assert S.predicate_ref(b, b, b, b, area, length, _pred(S.MIN_SIZE, min_area=-0.0, min_length=np.inf)).tolist() == \
        [1, 1, 1, 1, 1, 1, 0, 1]
    # both: W && S, and the empty rule before either
    both = _pred(S.WINDOW | S.MIN_SIZE, (0, 0, 0, 0), 4.0, 8.0)
    assert S.predicate_ref(b, b, b, b, area, length, both).tolist() == [1, 1, 0, 1, 1, 0, 0, 1]
    both.window = (1, 1, 2, 2)
    assert S.predicate_ref(b, b, b, b, area, length, both).tolist() == [0] * 8
    nanbox = np.full(8, NAN)
    both.flags |= S.KEEP_EMPTY
    assert S.predicate_ref(nanbox, nanbox, nanbox, nanbox, area, length, both).tolist() == [1] * 8
    assert S.predicate_ref(b, b, b, b, area, length, both).dtype == np.uint8


def test_layout_rule_under_sanitizers(tmp_path):
    """The host-side layout code (covt_select_plan.h) in a stand-alone program built with AddressSanitizer and
    UndefinedBehaviorSanitizer, on the CPU."""
    exe = str(tmp_path / "select_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "select_layout", "select_layout_check.cc")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["ok", "200000"], (p.stdout, p.stderr[-2000:])

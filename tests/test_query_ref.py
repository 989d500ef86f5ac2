"""CPU: the two references of the query pass (tests/covt_query.py; include/covt.h "Geometry queries") against
known answers and against each other, and the shared rules of covt_query_plan.h in a stand-alone program under
the sanitizers against a table the definition's reference writes."""
import os
import subprocess

import numpy as np
import pytest

import covt_query as Q
from conftest import ROOT


@pytest.mark.parametrize("case", Q.KNOWN, ids=[k[0] for k in Q.KNOWN])
def test_known_answers(case):
    """Both relations of every known case, from both references, alone and in one column with the others of its
    window."""
    name, w, feature, inter, within = case
    col = Q.assemble([feature])
    for ref in (Q.query_ref, Q.query_clip_ref):
        i, n = ref(*col, w)
        assert (int(i[0]), int(n[0])) == (inter, within), (name, ref.__name__)
    same = [k for k in Q.KNOWN if k[1] == w]
    col = Q.assemble([k[2] for k in same])
    for ref in (Q.query_ref, Q.query_clip_ref):
        i, n = ref(*col, w)
        assert i.tolist() == [k[3] for k in same] and n.tolist() == [k[4] for k in same], ref.__name__


def test_within_implies_intersects_and_empty_features_get_neither():
    rng = np.random.default_rng(7)
    feats = [Q.valid_feature(rng) for _ in range(2000)]
    col = Q.assemble(feats)
    for _ in range(20):
        w = Q.random_window(rng)
        i, n = Q.query_ref(*col, w)
        assert not (n & ~i).any()
        empty = np.array([not any(r for p in f[1] for r in p) for f in feats])
        assert not i[empty].any() and not n[empty].any()
        if w[0] > w[2] or w[1] > w[3]:
            assert not i.any() and not n.any()


def test_references_agree_on_random_valid_features():
    """A few thousand valid features with coordinates in +-12 against small windows: touching cases, points on
    edges and windows inside holes are frequent; both relations must agree feature for feature."""
    rng = np.random.default_rng(11)
    hits = np.zeros(2, dtype=np.int64)
    total = 0
    for _ in range(1500):
        feats = [Q.valid_feature(rng) for _ in range(4)]
        col = Q.assemble(feats)
        w = Q.random_window(rng)
        a, b = Q.query_ref(*col, w), Q.query_clip_ref(*col, w)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), (feats, w)
        hits += (int(a[0].sum()), int(a[1].sum()))
        total += 4
    assert total == 6000 and 500 < hits[0] < total - 500 and hits[1] > 20  # (neither answer is rare)


def test_numpy_reference_is_the_definition():
    """query_ref_numpy (what the fixture tiles are held to) gives query_ref's answers: on the known cases, on
    random valid features against small windows and on coordinates up to its bound of 2^30."""
    rng = np.random.default_rng(15)
    for w in sorted({k[1] for k in Q.KNOWN}):
        col = Q.assemble([k[2] for k in Q.KNOWN if k[1] == w])
        a, b = Q.query_ref(*col, w), Q.query_ref_numpy(*col, w)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), w
    for _ in range(60):
        col = Q.assemble([Q.valid_feature(rng) for _ in range(50)])
        w = Q.random_window(rng)
        a, b = Q.query_ref(*col, w), Q.query_ref_numpy(*col, w)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), w
    big = (-(1 << 30), -(1 << 30) + 1, -1, 0, 1, (1 << 30) - 1, 1 << 30)
    for _ in range(100):
        pt = lambda: (int(rng.choice(big)), int(rng.choice(big)))  # noqa: E731
        feats = [Q.line([pt() for _ in range(int(rng.integers(0, 5)))]) for _ in range(6)]
        feats += [Q.polygon([(lambda r: r + r[:1])([pt() for _ in range(3)])]) for _ in range(6)]
        col = Q.assemble(feats)
        w = tuple(int(rng.choice(big)) for _ in range(4))
        a, b = Q.query_ref(*col, w), Q.query_ref_numpy(*col, w)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), (feats, w)
    assert Q.query_ref_numpy(*Q.assemble([]), Q.W10)[0].size == 0


def _extreme_features(rng, k):
    pt = lambda: (int(rng.choice(Q.EXTREMES)), int(rng.choice(Q.EXTREMES)))  # noqa: E731
    feats = []
    for _ in range(k):
        t = int(rng.integers(0, 4))
        if t == 0:
            feats.append(Q.point(*pt()))
        elif t == 1:
            feats.append(Q.line([pt() for _ in range(int(rng.integers(2, 5)))]))
        elif t == 2:
            feats.append(Q.multipoint([pt() for _ in range(int(rng.integers(1, 4)))]))
        else:  # one ring: the part rule and even-odd are the same rule
            r = [pt() for _ in range(int(rng.integers(3, 5)))]
            feats.append(Q.polygon([r + r[:1]]))
    return feats


def test_references_agree_on_extreme_coordinates():
    """Coordinates and window corners from {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX}:
    33-bit differences and 66-bit products on every route."""
    rng = np.random.default_rng(12)
    for _ in range(400):
        feats = _extreme_features(rng, 5)
        col = Q.assemble(feats)
        w = tuple(int(rng.choice(Q.EXTREMES)) for _ in range(4))
        a, b = Q.query_ref(*col, w), Q.query_clip_ref(*col, w)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), (feats, w)


def test_source_column_and_assemble_agree_with_the_oracle(oracle):
    """The hand-made columns of the GPU tests: the oracle's assembly of source_column() is assemble()."""
    import covt_asm as A

    rng = np.random.default_rng(13)
    feats = [k[2] for k in Q.KNOWN] + [Q.valid_feature(rng) for _ in range(200)]
    src = Q.source_column(feats)
    o = oracle.assemble_geometry(src["types"], src["go"], src["po"], src["ro"], src["vo"], src["vb"], True, A.caps(src))
    want = Q.assemble(feats)
    assert o[0] == 0
    for got, w in zip(o[1:], want[1:]):
        assert np.asarray(got).reshape(-1).tolist() == np.asarray(w).reshape(-1).tolist()


def _table():
    """The check program's input: segments (small, touching, extreme), one-coordinate rings, query_valid and the
    per-feature rule, answered by the definition's reference."""
    rng = np.random.default_rng(14)
    rows = []

    def seg(a, b, w):
        e = int(Q.q_meets(w, a, b)) | int(not Q.q_in(w, a) or not Q.q_in(w, b)) << 1 | int(Q.q_cross(w, a, b)) << 2
        rows.append("S %d %d %d %d %d %d %d %d %d %d %d %d" % (*a, *b, *w, Q.q_in(w, a), Q.q_meets(w, a, b),
                                                            Q.q_cross(w, a, b), e))
        rows.append("P %d %d %d %d %d %d %d" % (*a, *w, Q.ring_bits(w, [a])))

    for _ in range(6000):
        p = rng.integers(-12, 13, size=4)
        seg((int(p[0]), int(p[1])), (int(p[2]), int(p[3])), Q.random_window(rng))
    for _ in range(6000):
        p = [int(v) for v in rng.choice(Q.EXTREMES, 8)]
        seg((p[0], p[1]), (p[2], p[3]), tuple(p[4:]))
    for _ in range(3000):  # anywhere in int32, against windows anywhere: the wide signs with every bit in play
        p = [int(v) for v in rng.integers(Q.LO, Q.HI + 1, size=8)]
        seg((p[0], p[1]), (p[2], p[3]), (min(p[4], p[6]), min(p[5], p[7]), max(p[4], p[6]), max(p[5], p[7])))
    for k in Q.KNOWN:
        for part in k[2][1]:
            for r in part:
                for a, b in zip(r, r[1:]):
                    seg(a, b, k[1])
    for size in (0, 31, 32, 33):
        for flags in (0, 1, 0x80000000):
            for rel in (-1, 0, 1, 2):
                for reserved in (0, 1, -1):
                    rows.append("V %d %d %d %d %d" % (size, flags, rel, reserved,
                                                     size == 32 and flags == 0 and rel in (0, 1) and reserved == 0))
    for v in range(8):
        for t in range(7):
            for has in (0, 1):
                inter = has and ((v & 1) or (t in (2, 5) and (v & 4)))
                rows.append("F %d %d %d 0 %d" % (v, t, has, bool(inter)))
                rows.append("F %d %d %d 1 %d" % (v, t, has, bool(has and not v & 2)))
    return rows


def test_plan_rules_under_sanitizers(tmp_path):
    """covt_query_plan.h (query_valid, in / meets / cross, the edge term, the join, the per-feature rule) in a
    stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU: a 64-bit
    overflow in a wide sign would stop it."""
    exe = str(tmp_path / "query_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "query_plan", "query_check.cc")])
    rows = _table()
    p = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=120)
    out = p.stdout.split()
    assert p.returncode == 0 and out[:1] == ["ok"], (p.stdout[-2000:], p.stderr[-2000:])
    n_seg = sum(r[0] == "S" for r in rows)
    assert n_seg > 15000 and int(out[1]) == 512 + 6 * n_seg + (len(rows) - n_seg)

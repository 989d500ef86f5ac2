"""GPU: the mvt pass (covt_mvt.hip, include/covt.h "Geometry as MVT") against the reference of tests/covt_mvt.py,
byte for byte (types, offsets, bytes[0, n_bytes), n_empty, n_bytes), through the C-ABI: covt_geometry_mvt_device on
hand-made assembled columns (offsets, coordinates and types written here, no decode), covt_plan_mvt_host on the
fixture tiles, the host tile writer read back by the tests' MVT readers and the oracle's decoder, the DeviceBatch
/ DevicePlan paths, a HIP-graph replay and decode_covt.  Buffers start as a fill pattern; every byte the
definition leaves unwritten (the gaps between slices, the capacity past n_bytes, the slices of failed columns)
must still hold it -- the scratch of a column that ran excepted -- and the input buffers must be unchanged.

The kernels' step sizes the boundary cases are built around: the rings pass (orientation) works in chunks of 128
coordinates, 4 waves a workgroup, up to 64 workgroups per column while 8192 / n_columns allows (4096 columns: 2,
4097: 1); the count and write passes work in chunks of 1024 coordinates (8 rows of 128), a wave each, and mark the
rings that start in a row 64 at a step; a feature of 64 rings or more is finished by its whole wave; the scan takes
1024 chunks per step (256 in a batch of more than 4096 columns).  The carry from one scan step to the next is
reached only in the wave's form (the ring of 300,001 coordinates: 293 chunks, in the batch of 4097); the workgroup's
form shares that code, and a column of more than 1024 chunks (a million coordinates) is larger than a test here
should be.
"""
import json
import os

import numpy as np
import pytest

import covt_asm as A
import covt_geom as G
import covt_mvt as MV
import covt_props as P
import covt_simplify as S
from conftest import GOLDEN, tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
ROW, CHUNK = 128, 1024
LO, HI = -(1 << 31), (1 << 31) - 1
GDESC = np.dtype([("in_off", np.int64, 6), ("in_len", np.int32, 6), ("in_res", np.int32, 6), ("out_off", np.int64, 6),
                  ("part_cap", np.int32), ("ring_cap", np.int32), ("coord_cap", np.int32), ("flags", np.int32)])


def _a16(x):
    return (x + 15) & ~15


def _members(n, rc, cc):
    """Offsets of type, offsets, bytes, the scratch and the slice's end; the byte capacity."""
    cap = 10 * cc + 7 * rc + 5 * n
    offs = _a16(n)
    data = offs + _a16(4 * (n + 1))
    scratch = data + _a16(cap)
    return 0, offs, data, scratch, scratch + _a16(16 * rc) + _a16(4 * rc) + _a16(4 * ((cc + CHUNK - 1) // CHUNK + 1)), cap


# ---- hand-made assembled columns ----------------------------------------------------------------------------
def _column(features):
    """features: [(type, parts)], parts: [rings], ring: [(x, y)] -> an assembled column."""
    types, geo, part, ring, xy = [], [0], [0], [0], []
    for t, parts in features:
        types.append(t)
        for rings in parts:
            for r in rings:
                xy += [v for pt in r for v in pt]
                ring.append(ring[-1] + len(r))
            part.append(part[-1] + len(rings))
        geo.append(geo[-1] + len(parts))
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return {"types": np.asarray(types, np.uint8), "geo": i32(geo), "part": i32(part), "ring": i32(ring),
            "xy": i32(xy).reshape(-1, 2)}


def _walk(rng, k, step=300, lim=1 << 14):
    """k points of a random walk: deltas of one and two varint bytes."""
    if k == 0:
        return []
    p = rng.integers(-lim, lim, size=2) + np.cumsum(rng.integers(-step, step + 1, size=(k, 2)), axis=0)
    return [(int(x), int(y)) for x, y in p]


def _closed(rng, k, step=300):
    p = _walk(rng, max(k - 1, 1), step)
    return p + p[:1] if k > 1 else p


def _box(x0, y0, w, h, cw=False):
    b = [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h), (x0, y0)]
    return b[::-1] if cw else b


def _pack(covt, cols, pad=(3, 5, 7)):
    """The decode buffer (types only), the assembly buffer, the geometry descriptors and results, and the mvt
    descriptors by the plan's layout rule with a 16-byte gap after every slice."""
    nc = len(cols)
    gd = np.zeros(nc, GDESC)
    gres = np.zeros(nc, covt.GEOM_RESULT_DTYPE)
    md = np.zeros(nc, covt.MVT_DESC_DTYPE)
    dec_off = asm_off = m_off = 0
    lay = []
    for ci, col in enumerate(cols):
        n, P_, R, V = col["types"].size, col["part"].size - 1, col["ring"].size - 1, col["xy"].shape[0]
        pc, rc, cc = P_ + pad[0], R + pad[1], V + pad[2]
        gd[ci]["in_off"][:] = -1
        gd[ci]["in_res"][:] = -1
        gd[ci]["in_off"][0], gd[ci]["in_len"][0] = dec_off, n
        o = [asm_off, 0, 0, 0]
        o[1] = o[0] + _a16(4 * (n + 1))
        o[2] = o[1] + _a16(4 * (pc + 1))
        o[3] = o[2] + _a16(4 * (rc + 1))
        gd[ci]["out_off"][:4] = o
        gd[ci]["part_cap"], gd[ci]["ring_cap"], gd[ci]["coord_cap"] = pc, rc, cc
        gd[ci]["flags"] = col.get("gflags", 0)
        gres[ci] = (col.get("status", 0), P_, R, V)
        m = _members(n, rc, cc)
        md[ci]["off"] = m_off + col.get("md_off", 0)
        md[ci]["n_features"] = n + col.get("md_n", 0)
        md[ci]["ring_cap"], md[ci]["coord_cap"] = rc + col.get("md_rc", 0), cc + col.get("md_cc", 0)
        md[ci]["byte_cap"] = m[5] + col.get("md_cap", 0)
        md[ci]["flags"] = col.get("mflags", 0)
        lay.append((dec_off, o, m_off, (n, rc, cc)))
        dec_off += _a16(n)
        asm_off = o[3] + _a16(8 * cc)
        m_off += m[4] + 16
    dec = np.full(max(dec_off, 16), FILL, np.uint8)
    asm = np.full(max(asm_off, 16), FILL, np.uint8)
    for col, (d_off, o, _, _) in zip(cols, lay):
        dec[d_off:d_off + col["types"].size] = col["types"]
        for k, name in enumerate(("geo", "part", "ring", "xy")):
            a = np.ascontiguousarray(col[name]).view(np.uint8).reshape(-1)
            asm[o[k]:o[k] + a.size] = a
    return dec, asm, gd, gres, md, max(m_off, 16), lay


def _opts(covt, orient, shift):
    return covt.MvtOptions(orient=orient, shift=shift)


def _run(covt, cols, orient=False, shift=0, expect=0, opts=None):
    """covt_geometry_mvt_device over hand-made columns -> (mvt buffer, results, layout)."""
    import ctypes as C

    import torch

    dec, asm, gd, gres, md, m_bytes, lay = _pack(covt, cols)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_dec, d_asm, d_gd, d_gres, d_md = up(dec), up(asm), up(gd), up(gres), up(md)
    d_out = torch.full((m_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_res = torch.full((16 * len(cols),), FILL, dtype=torch.uint8, device=dev)
    opts = opts if opts is not None else _opts(covt, orient, shift)
    st = covt.lib().covt_geometry_mvt_device(
        d_dec.data_ptr(), d_gd.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(), d_md.data_ptr(), len(cols),
        C.addressof(opts), d_out.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert st == expect
    # the inputs are unchanged
    assert d_dec.cpu().numpy().tobytes() == dec.tobytes() and d_asm.cpu().numpy().tobytes() == asm.tobytes()
    assert d_gd.cpu().numpy().tobytes() == gd.tobytes() and d_gres.cpu().numpy().tobytes() == gres.tobytes()
    assert d_md.cpu().numpy().tobytes() == md.tobytes()
    return d_out.cpu().numpy(), d_res.cpu().numpy().view(covt.MVT_RESULT_DTYPE), lay


def _reference(col, orient, shift, cache):
    key = (id(col), orient, shift)
    if key not in cache:
        cache[key] = MV.mvt_ref(col["types"], col["geo"], col["part"], col["ring"], col["xy"], orient, shift)
    return cache[key]


def _same(got_t, got_o, got_b, want, what):
    gt, offs, data = want
    assert got_t.tobytes() == gt.tobytes(), what
    if got_o.tobytes() != offs.tobytes():
        bad = int(np.nonzero(got_o != offs)[0][0])
        raise AssertionError("%s: offsets differ first at feature %d: got %r, want %r" % (what, bad, got_o[bad:bad + 3], offs[bad:bad + 3]))
    if got_b.tobytes() != data.tobytes():
        bad = int(np.nonzero(got_b != data)[0][0])
        f = int(np.searchsorted(offs, bad, side="right")) - 1
        raise AssertionError("%s: bytes differ first at %d (feature %d, its byte %d): got %r, want %r"
                             % (what, bad, f, bad - int(offs[f]), got_b[bad:bad + 8], data[bad:bad + 8]))


def _check(covt, cols, buf, res, lay, orient=False, shift=0, status=None, cache=None):
    """Every column equals the reference byte for byte; every byte the definition leaves unwritten holds FILL
    (the scratch of a column that ran: contents unspecified)."""
    cache = {} if cache is None else cache
    untouched = np.ones(buf.size, dtype=bool)
    for ci, col in enumerate(cols):
        want_st = status[ci] if status else 0
        assert int(res["status"][ci]) == want_st, (ci, res[ci], want_st)
        if want_st:
            assert res[ci].tolist() == (want_st, 0, 0), (ci, res[ci])
            continue
        want = _reference(col, orient, shift, cache)
        _, _, o, (n, rc, cc) = lay[ci]
        m = _members(n, rc, cc)
        nb = int(want[2].size)
        assert res[ci].tolist() == (0, int((np.diff(want[1]) == 0).sum()), nb), (ci, res[ci], nb)
        _same(buf[o:o + n], buf[o + m[1]:o + m[1] + 4 * (n + 1)].view(np.int32), buf[o + m[2]:o + m[2] + nb], want,
              "column %d (orient %d, shift %d)" % (ci, orient, shift))
        untouched[o:o + n] = False
        untouched[o + m[1]:o + m[1] + 4 * (n + 1)] = False
        untouched[o + m[2]:o + m[2] + nb] = False
        untouched[o + m[3]:o + m[4]] = False
    assert (buf[untouched] == FILL).all(), np.nonzero(untouched & (buf != FILL))[0][:8]


def _tiny():
    return _column([(1, [[[(0, 0), (40, 40)]]])])


def _all_ways(covt, cols, shifts=(0,), big_batch=True):
    """Orientation off and on; the columns with up to 64 workgroups each, and in a batch of 4097 (one workgroup, a
    wave's scan)."""
    cache = {}
    for shift in shifts:
        for orient in (False, True):
            buf, res, lay = _run(covt, cols, orient, shift)
            _check(covt, cols, buf, res, lay, orient, shift, cache=cache)
    if big_batch:
        padded = cols + [_tiny()] * (4097 - len(cols))
        buf, res, lay = _run(covt, padded, True, shifts[0])
        _check(covt, padded, buf, res, lay, True, shifts[0], cache=cache)


# ---- step boundaries ----------------------------------------------------------------------------------------
def test_rings_around_chunk_and_row_boundaries_of_every_type(covt, gpu_available):
    """Rings of every type that start and end 0, 1 and 2 items around the boundaries of the 128-item rows and the
    1024-item chunks (a closed polygon ring's last position is no item: its ClosePath rides on the item before);
    polygon rings wound both ways, so reversed rings straddle the boundaries."""
    rng = np.random.default_rng(81)
    cols = []
    for edge in (ROW, CHUNK, 2 * CHUNK):
        for d in (-2, -1, 0, 1, 2):
            k = edge + d
            cols.append(_column([(1, [[_walk(rng, k)]]), (1, [[_walk(rng, 9)]]), (4, [[_walk(rng, k - 9)], [_walk(rng, 700)]]),
                                 (1, [[_walk(rng, 4 * CHUNK + 7 - k)]])]))
            ring = _closed(rng, k)
            cols.append(_column([(2, [[ring, ring[::-1], _closed(rng, 7)]]), (2, [[_closed(rng, 2 * CHUNK - k - 7)[::-1]]]),
                                 (5, [[_closed(rng, 30)], [_closed(rng, 5)[::-1]] * 2])]))
            cols.append(_column([(3, [[[pt]] for pt in _walk(rng, k)]), (0, [[_walk(rng, 1)]]), (3, [[_walk(rng, k)]]),
                                 (3, [[[pt]] for pt in _walk(rng, 130)])]))
    _all_ways(covt, cols)


def test_small_rings_empty_rings_and_the_cursor_across_chunks(covt, gpu_available):
    """Rings of 0 .. 5 coordinates of every type between longer ones; empty rings between non-empty ones of one
    feature, placed so that the cursor's predecessor lies in the chunk before; more than 64 empty rings in a row."""
    rng = np.random.default_rng(82)
    small = []
    for t in range(6):
        for k in range(6):
            ring = _closed(rng, k) if t in (2, 5) else _walk(rng, k)
            small.append((t, [[ring]] if t < 3 else [[ring], [ring[::-1]]]))
            small.append((1, [[_walk(rng, 50)]]))
    cols = [_column(small), _column(small[::-1])]
    for lead in (CHUNK - 2, CHUNK - 1, CHUNK, ROW - 1, ROW):
        cols.append(_column([(4, [[_walk(rng, lead)], [[]], [[]], [_walk(rng, 40)], [[]] * 70, [_walk(rng, 3)]]),
                             (5, [[_closed(rng, lead), [], _closed(rng, 6)[::-1]], [[], []], [_closed(rng, 9)]]),
                             (3, [[_walk(rng, lead)], [[]], [_walk(rng, 2)]])]))
    cols.append(_column([(1, [[_walk(rng, 50)]]), (4, [[[]]] * 200), (1, [[_walk(rng, 50)]]), (5, [[[], []]] * 70),
                         (1, [[_walk(rng, 9)]]), (4, [[[]]] * 64), (2, [[_closed(rng, 9)]])]))
    _all_ways(covt, cols)


def test_shell_with_70_holes_mixed_windings(covt, gpu_available):
    """A part of 1 shell and 70 holes wound both ways (wider than the thread-per-feature path), shells wound both
    ways, and a multipolygon of 200 parts: the first ring of every part is found by the wave's search."""
    holes = [_box(100 + 40 * (i % 10), 100 + 40 * (i // 10), 20 + i % 3, 18, cw=bool(i % 3)) for i in range(70)]
    many = [[_box(0, 0, 640, 640, cw=bool(i & 1))] + holes[:i % 5] for i in range(200)]
    col = _column([(2, [[_box(0, 0, 640, 640)] + holes]), (2, [[_box(0, 0, 640, 640, cw=True)] + holes]), (5, many),
                   (5, [[_box(0, 0, 640, 640, cw=True)] + holes, [_box(0, 0, 700, 700)] + holes[::-1]])])
    p = MV.ring_plan(col["types"], col["geo"], col["part"], col["ring"], col["xy"], True, 0)
    assert 100 < int(p["rev"].sum()) < p["R"] - 100
    _all_ways(covt, [col])


def test_one_ring_of_300000_coordinates_and_100000_points(covt, gpu_available):
    """One ring alone, stored against its role (reversed with orientation on) and as its role asks; a MULTIPOINT of
    100,000 single-point parts (100,000 rings walked by one wave) and one of 100,000 points in one ring."""
    rng = np.random.default_rng(83)
    k = 300001
    ang = np.linspace(0.0, 2.0 * np.pi, k - 1, endpoint=False)
    p = np.stack([np.cos(ang), np.sin(ang)], axis=1) * 1.0e6 + rng.integers(-40, 41, size=(k - 1, 2))
    ccw = np.concatenate([p, p[:1]]).astype(np.int32)
    one = lambda t, xy: {"types": np.array([t], np.uint8), "geo": np.array([0, 1], np.int32),  # noqa: E731
                         "part": np.array([0, 1], np.int32), "ring": np.array([0, xy.shape[0]], np.int32), "xy": xy}
    pts = rng.integers(-50000, 50000, size=(100000, 2)).astype(np.int32)
    multi = {"types": np.array([3], np.uint8), "geo": np.array([0, 100000], np.int32),
             "part": np.arange(100001, dtype=np.int32), "ring": np.arange(100001, dtype=np.int32), "xy": pts}
    cols = [one(2, ccw), one(2, np.ascontiguousarray(ccw[::-1])), one(1, ccw), multi, one(3, pts)]
    rp = [MV.ring_plan(c["types"], c["geo"], c["part"], c["ring"], c["xy"], True, 0) for c in cols[:2]]
    assert not rp[0]["rev"][0] and rp[1]["rev"][0]
    cache = {}
    for orient in (False, True):
        buf, res, lay = _run(covt, cols, orient, 0)
        _check(covt, cols, buf, res, lay, orient, 0, cache=cache)
    padded = cols[1:2] + [_tiny()] * 4096
    buf, res, lay = _run(covt, padded, True, 0)
    _check(covt, padded, buf, res, lay, True, 0, cache=cache)


# the worked examples of the MVT 2.1 specification (section 4.3.5), the winding and the wrap-around of the issue:
# (type, parts, orientation, the value byte for byte) -- literal bytes, not the reference's
_SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]
_SHELL = [(11, 11), (20, 11), (20, 20), (11, 20), (11, 11)]
_HOLE = [(13, 13), (13, 17), (17, 17), (17, 13), (13, 13)]
_LINE = [(2, 2), (2, 10), (10, 10)]
_CW = [(0, 0), (0, 10), (10, 10), (10, 0), (0, 0)]
_SPEC_MULTIPOLYGON = [9, 0, 0, 26, 20, 0, 0, 20, 19, 0, 15, 9, 22, 2, 26, 18, 0, 0, 18, 17, 0, 15, 9, 4, 13, 26, 0, 8, 8, 0,
                      0, 7, 15]
KNOWN = [(0, [[[(25, 17)]]], None, [9, 50, 34]),
         (3, [[[(5, 7)]], [[(3, 2)]]], None, [17, 10, 14, 3, 9]),
         (1, [[_LINE]], None, [9, 4, 4, 18, 0, 16, 16, 0]),
         (4, [[_LINE], [[(1, 1), (3, 5)]]], None, [9, 4, 4, 18, 0, 16, 16, 0, 9, 17, 17, 10, 4, 8]),
         (2, [[[(3, 6), (8, 12), (20, 34), (3, 6)]]], None, [9, 6, 12, 18, 10, 12, 24, 44, 15]),
         (5, [[_SQUARE], [_SHELL, _HOLE]], None, _SPEC_MULTIPOLYGON),
         (2, [[_CW]], False, [9, 0, 0, 26, 0, 20, 20, 0, 0, 19, 15]),
         (2, [[_CW]], True, [9, 0, 0, 26, 20, 0, 0, 20, 19, 0, 15]),
         (1, [[[(LO, HI), (HI, LO)]]], None, [0x09, 0xFF, 0xFF, 0xFF, 0xFF, 0x0F, 0xFE, 0xFF, 0xFF, 0xFF, 0x0F, 0x0A, 0x01, 0x02])]


def test_known_answers_on_the_device(covt, gpu_available):
    """The kernel against the literal bytes of the specification's examples (orientation off and on: they are wound
    as the specification asks), of the issue's winding example and of its wrap-around example, each example a
    column of its own and all of them features of one column."""
    for orient in (False, True):
        known = [k for k in KNOWN if k[2] in (None, orient)]
        cols = [_column([(t, parts)]) for t, parts, _, _ in known] + [_column([(t, parts) for t, parts, _, _ in known])]
        buf, res, lay = _run(covt, cols, orient, 0)
        assert (res["status"] == 0).all()
        values = []
        for ci, col in enumerate(cols):
            o, (n, rc, cc) = lay[ci][2], lay[ci][3]
            m = _members(n, rc, cc)
            offs = buf[o + m[1]:o + m[1] + 4 * (n + 1)].view(np.int32)
            values.append([buf[o + m[2] + offs[i]:o + m[2] + offs[i + 1]].tolist() for i in range(n)])
            assert buf[o:o + n].tolist() == [int(t) % 3 + 1 for t in col["types"]]
        want = [k[3] for k in known]
        assert [v[0] for v in values[:-1]] == want and values[-1] == want, orient


@pytest.mark.parametrize("shift", [0, 1, 30])
def test_int32_extremes(covt, gpu_available, shift):
    vals = [HI, HI - 1, LO, LO + 1, -1, 0, 1, 1 << 30, -(1 << 30), (1 << 30) - 1]
    pts = [(a, b) for a in vals for b in vals]
    col = _column([(1, [[pts]]), (3, [[pts[:40]]]), (2, [[[(LO, LO), (HI, LO), (HI, HI), (LO, HI), (LO, LO)]]]),
                   (2, [[[(LO, LO), (LO, HI), (HI, HI), (HI, LO), (LO, LO)]]]), (1, [[[(LO, HI), (HI, LO)]]]),
                   (0, [[[(LO, LO)]]]), (0, [[[(HI, HI)]]])])
    _all_ways(covt, [col], shifts=(shift,), big_batch=False)
    if shift == 0:
        gt, offs, data = MV.mvt_ref(col["types"], col["geo"], col["part"], col["ring"], col["xy"], False, 0)
        assert MV.feature_value(offs, data, 4).hex() == "09ffffffff0ffeffffff0f0a0102"


def test_batches_of_4096_and_4097_columns_give_the_same_bytes(covt, gpu_available):
    rng = np.random.default_rng(84)
    base = [_column([(1, [[_walk(rng, int(k))]]) for k in rng.integers(0, 40, size=30)]),
            _column([(2, [[_closed(rng, int(k)), _closed(rng, 6)[::-1]]]) for k in rng.integers(1, 300, size=12)]),
            _column([(3, [[[pt]] for pt in _walk(rng, 70)]), (0, [[_walk(rng, 1)]])]), _column([(1, [[_walk(rng, 2500)]])])]
    cache = {}
    slices = {}
    for nc in (4096, 4097):
        cols = (base * (nc // len(base) + 1))[:nc]
        buf, res, lay = _run(covt, cols, True, 0)
        _check(covt, cols, buf, res, lay, True, 0, cache=cache)
        for ci in range(len(base)):
            _, _, o, caps = lay[ci]
            m = _members(*caps)
            nb = int(res["n_bytes"][ci])
            slices.setdefault(ci, []).append(buf[o:o + m[2] + nb].tobytes())
    assert all(a == b for a, b in slices.values())


def test_columns_with_no_features_no_rings_or_nothing_emitted(covt, gpu_available):
    rng = np.random.default_rng(85)
    none = _column([])
    no_coords = _column([(1, [[[]]]), (2, [[[], []]]), (5, []), (3, []), (4, [[[]], [[]]])])
    no_rings = _column([(1, []), (2, []), (3, [])])
    mixed = _column([(3, []), (1, [[_walk(rng, 5)]]), (2, [[[]]]), (2, [[_closed(rng, 5)]]), (5, [])])
    _all_ways(covt, [none, no_coords, no_rings, mixed])
    buf, res, lay = _run(covt, [none, no_coords, no_rings, mixed])
    assert res["n_empty"].tolist() == [0, 5, 3, 3] and res["n_bytes"].tolist()[:3] == [0, 0, 0]


def test_status_paths(covt, gpu_available):
    rng = np.random.default_rng(86)
    ok = _column([(2, [[_closed(rng, 30)]]), (1, [[_walk(rng, 90)]])] * 10)
    I = covt.ERR_INVALID_ARG
    cols = [ok, dict(ok, status=covt.ERR_TRUNCATED), dict(ok, gflags=0x80000000 - (1 << 32)), dict(ok, md_rc=1),
            dict(ok, mflags=covt.MVT_TOO_LARGE), dict(ok, md_off=8), dict(ok, md_n=1), dict(ok, md_cc=-1), dict(ok, md_cap=16),
            ok]
    status = [0, covt.ERR_TRUNCATED, I, I, I, I, I, I, I, 0]
    buf, res, lay = _run(covt, cols, True, 0)
    _check(covt, cols, buf, res, lay, True, 0, status=status)
    for ci, st in enumerate(status):  # a failed column's slice, its scratch included, is untouched
        if st:
            o = lay[ci][2]
            assert (buf[o:o + _members(*lay[ci][3])[4] + 16] == FILL).all(), ci
    # options the call refuses: nothing written
    for bad in (covt.MvtOptions(shift=31), covt.MvtOptions(shift=-1)):
        buf, res, lay = _run(covt, [ok, ok], expect=I, opts=bad)
        assert (buf == FILL).all() and (res.view(np.uint8) == FILL).all()
    bad = covt.MvtOptions()
    bad.flags = 2
    buf, res, lay = _run(covt, [ok], expect=I, opts=bad)
    assert (buf == FILL).all()
    bad = covt.MvtOptions()
    bad.size = 12
    buf, res, lay = _run(covt, [ok], expect=I, opts=bad)
    assert (buf == FILL).all()


# ---- fixture tiles ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(covt, oracle, gpu_available):
    """Every fixture tile in one plan, its assembly (the reference's input) and the types of every column."""
    paths = tile_paths()
    tiles = [open(p, "rb").read() for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    asm, gres = plan.assemble_host()
    types, cache = [], {}
    for c in range(plan.num_geometry_columns):
        t, L = int(plan.geom["tile"][c]), int(plan.geom["layer"][c])
        if t not in cache:
            cache[t] = A.oracle_tile_columns(oracle, tiles[t])
        types.append(cache[t][L].get("types"))  # (None: a source stream failed to decode)
    return {"paths": paths, "plan": plan, "asm": asm, "gres": gres, "types": types, "simplified": {}}


@pytest.mark.parametrize("orient", [False, True])
@pytest.mark.parametrize("simplify", [None, 4])
def test_fixture_tiles(covt, fixtures, orient, simplify):
    """covt_plan_mvt_host on every fixture tile against the reference applied to assemble_host's output; with
    set_simplify(4) and shift 4 against the reference applied to the reference's simplified column."""
    plan, asm, gres, types = fixtures["plan"], fixtures["asm"], fixtures["gres"], fixtures["types"]
    shift = simplify or 0
    if simplify is not None:
        plan.set_simplify(simplify)
    try:
        buf, res = plan.mvt_host(covt.MvtOptions(orient=orient, shift=shift))
    finally:
        plan.set_simplify(None)
    n_ok = n_bytes = n_coords = 0
    for c in range(plan.num_geometry_columns):
        if int(gres["status"][c]):
            assert res[c].tolist() == (int(gres["status"][c]), 0, 0)
            continue
        g = plan.geometry_arrays(asm, gres, c)
        ring, xy = g.ring_offsets, g.coords
        if simplify is not None:
            if c not in fixtures["simplified"]:
                fixtures["simplified"][c] = S.simplify_ref(types[c], g.geometry_offsets, g.part_offsets, ring, xy, simplify)
            ring, xy = fixtures["simplified"][c]
        want = MV.mvt_ref(types[c], g.geometry_offsets, g.part_offsets, ring, xy, orient, shift)
        got = plan.mvt_column(buf, res, c)
        what = "%s layer %d" % (tile_key(fixtures["paths"][int(plan.geom["tile"][c])]), int(plan.geom["layer"][c]))
        assert (int(res["n_empty"][c]), int(res["n_bytes"][c])) == (int((np.diff(want[1]) == 0).sum()), want[2].size), what
        _same(got.types, got.offsets, got.data, want, what)
        assert got.n_empty == int(res["n_empty"][c])
        n_ok += 1
        n_bytes += want[2].size
        n_coords += int(xy.shape[0])
    # (a coordinate takes 2 to 10 bytes of parameters; as WKB it takes 16)
    assert n_ok >= 700 and 2 * n_coords <= n_bytes <= 10 * n_coords


def test_twelve_omt_tiles_as_mvt_read_back(covt, oracle, gpu_available):
    """On the 12 smallest OMT tiles of mvt_digests.json: the GPU's values wrapped by mvt_layer_bytes and read by
    covt_geom.mvt_layers reproduce the digests of the MVT originals; the tags written from the decoded property
    columns read back through covt_props.mvt_properties equal PropertyColumn.to_list() (absent where None); the
    oracle's MVT decoder accepts the tile, its feature and vertex totals the columns'."""
    dig = json.load(open(os.path.join(GOLDEN, "mvt_digests.json")))
    names = sorted(dig, key=lambda n: os.path.getsize(os.path.join(GOLDEN, "tiles", "omt", n + ".covt")))[:12]
    pinned = tagged = 0
    for name in names:
        tile = open(os.path.join(GOLDEN, "tiles", "omt", name + ".covt"), "rb").read()
        layers = covt.CovtParser.decode_covt(tile, properties=True, mvt=covt.MvtOptions(orient=True))
        recs, n_feat, n_vert = [], 0, 0
        for lc in layers:
            rec = dig[name].get(str(lc.layer))
            if rec is None or lc.mvt is None:
                continue
            recs.append(covt.mvt_layer_bytes(rec["name"], 4096, lc.mvt, ids=lc.ids, properties=lc.properties))
            got = G.mvt_layers(recs[-1])[rec["name"]]["features"]
            assert len(got) == len(lc.mvt) - lc.mvt.n_empty
            if rec["oracle_geom_match"]:
                assert G.layer_digest([(cls, parts) for _, cls, parts in got]) == rec["geom"], (name, lc.layer)
                pinned += 1
            n_feat += len(got)
            n_vert += sum(len(p) for _, _, parts in got for p in parts)
            if lc.properties:  # (the writer leaves the features with an empty value out: so does the comparison)
                tags = P.mvt_properties(recs[-1])[rec["name"]]
                written = np.flatnonzero(np.diff(lc.mvt.offsets) > 0)
                for key, pc in lc.properties.items():
                    values = pc.to_list()
                    assert [t.get(key) for t in tags] == [values[i] for i in written], (name, lc.layer, key)
                    tagged += 1
        data = covt.mvt_tile_bytes(recs)
        st, nf, nv = oracle.mvt_decode(data, with_props=True)[:3]
        assert (st, nf, nv) == (0, n_feat, n_vert), name
    assert pinned >= 60 and tagged >= 100


# ---- DeviceBatch / DevicePlan, graph replay, decode_covt ----------------------------------------------------
def _batch(covt, n_tiles):
    tiles = [open(p, "rb").read() for p in tile_paths(("omt",))[:n_tiles]]
    plan = covt.Plan.from_tiles(tiles)
    return plan, covt.DeviceBatch(plan, "cuda:0")


def _columns_equal(plan, res, x, y):
    """The written members of every column in two mvt buffers hold the same bytes."""
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(res["status"][c]):
            continue
        a, b = plan.mvt_column(x, res, c), plan.mvt_column(y, res, c)
        assert a.types.tobytes() == b.types.tobytes() and a.offsets.tobytes() == b.offsets.tobytes(), c
        assert a.data.tobytes() == b.data.tobytes(), c
        n_ok += 1
    return n_ok


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_device_paths_match_host_path(covt, gpu_available, n_tiles):
    import torch

    plan, b = _batch(covt, n_tiles)
    opts = covt.MvtOptions(orient=True, shift=4)
    plain_h, pres_h = plan.mvt_host(covt.MvtOptions(orient=True))
    plan.set_simplify(4)
    try:
        simp_h, sres_h = plan.mvt_host(opts)
    finally:
        plan.set_simplify(None)
    assert (pres_h["status"] == 0).any() and int(pres_h["n_bytes"].sum()) > int(sres_h["n_bytes"].sum()) > 0
    b.decode()
    b.assemble()
    b.mvt(covt.MvtOptions(orient=True))
    torch.cuda.synchronize()
    buf_d, res_d = b.mvt_results()
    buf_d = buf_d.copy()
    assert res_d.tobytes() == pres_h.tobytes() and _columns_equal(plan, pres_h, plain_h, buf_d) > 0
    with pytest.raises(covt.IllegalArgumentException):
        b.mvt(opts, simplified=True)  # (needs simplify() first)
    b.simplify(4)
    b.mvt(opts, simplified=True)
    torch.cuda.synchronize()
    buf_d, res_d = b.mvt_results()
    assert res_d.tobytes() == sres_h.tobytes() and _columns_equal(plan, sres_h, simp_h, buf_d) > 0
    # the device plan: the same records and descriptors, the same bytes
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    mi, mdd = dp.mvt_copy()
    assert mi.tobytes() == plan.mvt.tobytes() and mdd.tobytes() == plan.mvdescs.tobytes()
    assert dp.mvt_bytes == plan.mvt_bytes
    n_g = plan.num_geometry_columns
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_sim, d_sgres = dp.alloc_simplify()
    d_mvt, d_mvres = dp.alloc_mvt()
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.mvt(d_out, d_asm, d_gres, covt.MvtOptions(orient=True), d_mvt, d_mvres)
    torch.cuda.synchronize()
    res_p = d_mvres.cpu().numpy().view(covt.MVT_RESULT_DTYPE)[:n_g][plan.mvt["desc_index"]]
    assert res_p.tobytes() == pres_h.tobytes()
    assert _columns_equal(plan, pres_h, plain_h, d_mvt.cpu().numpy()[:plan.mvt_bytes]) > 0
    dp.simplify(d_out, d_asm, d_gres, 4, d_sim, d_sgres)
    dp.mvt(d_out, d_sim, d_sgres, opts, d_mvt, d_mvres, simplified=True)
    torch.cuda.synchronize()
    res_p = d_mvres.cpu().numpy().view(covt.MVT_RESULT_DTYPE)[:n_g][plan.mvt["desc_index"]]
    assert res_p.tobytes() == sres_h.tobytes()
    assert _columns_equal(plan, sres_h, simp_h, d_mvt.cpu().numpy()[:plan.mvt_bytes]) > 0


@pytest.mark.parametrize("n_tiles", [1, 12])
def test_assemble_simplify_mvt_replay_in_a_hip_graph(covt, gpu_available, n_tiles):
    """assemble + simplify + mvt of the simplified column captured in one HIP graph and replayed twice into
    poisoned buffers: the bytes of the eager run each time (no atomics, every element written once; the
    assembly's scratch needs the warm-up launch on the capture stream before the capture)."""
    import torch

    plan, b = _batch(covt, n_tiles)
    s = torch.cuda.Stream(b.device)
    opts = covt.MvtOptions(orient=True, shift=4)

    def launch():
        b.assemble(s)
        b.simplify(4, s)
        b.mvt(opts, s, simplified=True)

    with torch.cuda.stream(s):
        b.decode(s)
        launch()
    torch.cuda.synchronize()
    buf_e, res_e = b.mvt_results()
    buf_e = buf_e.copy()
    assert (res_e["status"] == 0).any() and int(res_e["n_bytes"].sum()) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for _ in range(2):
        b.d_simplify.fill_(FILL)
        b.d_sgres.fill_(0x5A5A5A5A)
        b.d_asm.fill_(FILL)
        b.d_mvt.fill_(FILL)
        b.d_mvres.fill_(0x5A5A5A5A5A5A5A5A)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        buf, res = b.mvt_results()
        assert res.tobytes() == res_e.tobytes()
        assert _columns_equal(plan, res_e, buf_e, buf) == int((res_e["status"] == 0).sum())
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


@pytest.mark.parametrize("n_tiles", [1, 3])
def test_decode_covt_mvt(covt, gpu_available, decodable_tiles, n_tiles):
    """decode_covt(mvt=...): every layer's mvt column is the reference over its plain geometry, or with simplify
    over the reference's simplified column; without the argument mvt is None."""
    for ti, (_, tile) in enumerate(decodable_tiles[:n_tiles]):
        plain = covt.CovtParser.decode_covt(tile, mvt=covt.MvtOptions(orient=True))
        simp = covt.CovtParser.decode_covt(tile, simplify=4, mvt=covt.MvtOptions(orient=True, shift=4))
        if ti == 0:
            assert all(lc.mvt is None for lc in covt.CovtParser.decode_covt(tile))
        plan = covt.Plan.from_tiles([tile])
        asm, gres = plan.assemble_host()
        by_layer = {int(plan.geom["layer"][c]): c for c in range(plan.num_geometry_columns)}
        n_ok = 0
        for lp, ls in zip(plain, simp):
            if lp.wkb is None:
                continue
            g = plan.geometry_arrays(asm, gres, by_layer[lp.layer])
            types = np.asarray(lp.geometry.geometryTypes, np.uint8)
            _same(lp.mvt.types, lp.mvt.offsets, lp.mvt.data,
                  MV.mvt_ref(types, g.geometry_offsets, g.part_offsets, g.ring_offsets, g.coords, True, 0), lp.layer)
            ring, xy = S.simplify_ref(types, g.geometry_offsets, g.part_offsets, g.ring_offsets, g.coords, 4)
            assert ls.simplified.coords.tobytes() == xy.tobytes()
            _same(ls.mvt.types, ls.mvt.offsets, ls.mvt.data,
                  MV.mvt_ref(types, g.geometry_offsets, g.part_offsets, ring, xy, True, 4), ls.layer)
            n_ok += 1
        assert n_ok > 0
        plan.close()

"""GPU: the measures pass (covt_measures.hip, include/covt.h "Geometry measures") against the references of
tests/covt_measures.py over the CPU oracle's assembly, through the C-ABI: covt_geometry_measures_device on
synthetic and hand-made columns, covt_plan_measures_host on the fixture tiles (also held against the GPU's
own WKB), the DeviceBatch / DevicePlan paths, decode_covt, a HIP-graph replay and the JNI shim.  Area and
num_coords are compared as bytes, length within the header's bound (m_f + 4) * 2^-52 of the exactly rounded
sum; bytes outside the written arrays must still hold the fill pattern (the per-ring scratch excepted).

The kernel's step sizes the boundary cases are built around: a wave chunk of 128 coordinates, ring and
feature steps of 64 lanes, a workgroup of 4 waves (512 coordinates when every wave has one chunk), up to 64
workgroups per column while 8192 / n_columns allows, a feature of 64 rings or parts or more finished by its
whole wave, and a ring that has 2048 coordinates or more left past its owner's run finished by the whole
workgroup (fewer: by the owning wave).
"""
import numpy as np
import pytest

import covt_asm as A
import covt_measures as M
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
CHUNK, WAVES, LANES, NARROW, WIDE = 128, 4, 64, 64, 2048
LO, HI = -(1 << 31), (1 << 31) - 1


def _a16(x):
    return (x + 15) & ~15


def _rows_bytes(n):
    return 16 * n + _a16(4 * n)


def _measures_layout(covt, cols, mflags=None):
    """Measures descriptors (the plan's layout rule) for pack_columns' columns -> (desc array, bytes)."""
    d = np.zeros(len(cols), dtype=covt.MEASURES_DESC_DTYPE)
    off = 0
    for ci, col in enumerate(cols):
        n, rcap = col["types"].size, (col.get("caps") or A.caps(col))[1]
        d[ci]["off"] = off
        d[ci]["n_features"] = n
        d[ci]["ring_cap"] = rcap
        d[ci]["flags"] = mflags[ci] if mflags else 0
        off = _a16(off + _rows_bytes(n) + 16 * rcap) + 16  # (a gap after every slice: it must stay untouched)
    return d, max(off, 16)


def _run(covt, cols, flags_extra=None, in_res=None, dres=None, mflags=None):
    """covt_assemble_geometry_device + covt_geometry_measures_device over synthetic columns."""
    import torch

    dec, desc, asm_bytes, lay = A.pack_columns(covt, cols, flags_extra, in_res)
    md, m_bytes = _measures_layout(covt, cols, mflags)
    dev = torch.device("cuda:0")
    d_dec = torch.from_numpy(dec).to(dev)
    d_desc = torch.from_numpy(desc).to(dev)
    d_mdesc = torch.from_numpy(md.view(np.uint8).reshape(-1)).to(dev)
    d_asm = torch.full((asm_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_m = torch.full((m_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_gres = torch.zeros(4 * len(cols), dtype=torch.int32, device=dev)
    d_mres = torch.full((8 * len(cols),), FILL, dtype=torch.uint8, device=dev)
    d_res = torch.from_numpy(np.zeros(2, np.int32) if dres is None else np.asarray(dres, np.int32)).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    L = covt.lib()
    assert L.covt_assemble_geometry_device(d_dec.data_ptr(), d_res.data_ptr(), d_desc.data_ptr(), len(cols),
                                           d_asm.data_ptr(), d_gres.data_ptr(), s) == 0
    assert L.covt_geometry_measures_device(d_dec.data_ptr(), d_desc.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(),
                                           d_mdesc.data_ptr(), len(cols), d_m.data_ptr(), d_mres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    return (d_m.cpu().numpy(), d_mres.cpu().numpy().view(covt.MEASURES_RESULT_DTYPE),
            d_gres.cpu().numpy().view(covt.GEOM_RESULT_DTYPE), md)


def _reference(oracle, col, cache=None):
    """(status, reference measures, segment counts) over the oracle's assembly (cached per column object):
    measures_plain for small columns, measures_numpy(fsum=True) -- the same bytes -- for the others."""
    if cache is not None and id(col) in cache:
        return cache[id(col)]
    o = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"], col["vb"], col["closed"],
                                 col.get("caps") or A.caps(col))
    if o[0]:
        ref = (o[0], None, None)
    else:
        small = o[4].shape[0] < 20000
        fn = M.measures_plain if small else (lambda *a: M.measures_numpy(*a, fsum=True))
        ref = (0, fn(col["types"], *o[1:]), M.segments(*o[1:4]))
    if cache is not None:
        cache[id(col)] = ref
    return ref


def _compare(got, ref, m, what):
    area, length, count = got
    for name, g, w in (("area", area, ref[0]), ("num_coords", count, ref[2])):
        if g.tobytes() != np.asarray(w, g.dtype).tobytes():
            bad = np.nonzero(g.view(np.uint8).reshape(g.size, -1) != w.view(np.uint8).reshape(g.size, -1))[0]
            raise AssertionError("%s %s: rows differ, first %d: %r, want %r" % (what, name, int(bad[0]), g[bad[0]], w[bad[0]]))
    err, bound = np.abs(length - ref[1]), M.length_bound(ref[1], m)
    if (err > bound).any() or np.signbit(length).any():
        bad = np.nonzero((err > bound) | np.signbit(length))[0]
        raise AssertionError("%s length: %d of %d rows out of bound, first %d: %r, want %r (m %d)"
                             % (what, bad.size, length.size, int(bad[0]), length[bad[0]], ref[1][bad[0]], int(m[bad[0]])))


def _column_arrays(buf, o, n):
    return (buf[o:o + 8 * n].view(np.float64), buf[o + 8 * n:o + 16 * n].view(np.float64),
            buf[o + 16 * n:o + 20 * n].view(np.int32))


def _check(oracle, cols, buf, mres, md, cache=None):
    """Every column equals the reference; every byte outside the written arrays and the scratch holds FILL."""
    untouched = np.ones(buf.size, dtype=bool)
    for ci, col in enumerate(cols):
        st, ref, m = _reference(oracle, col, cache)
        assert int(mres["status"][ci]) == st and int(mres["reserved"][ci]) == 0, (ci, int(mres["status"][ci]), st)
        if st:
            continue
        o, n, rcap = int(md["off"][ci]), col["types"].size, int(md["ring_cap"][ci])
        _compare(_column_arrays(buf, o, n), ref, m, "column %d" % ci)
        untouched[o:o + 20 * n] = False
        untouched[o + _rows_bytes(n):o + _rows_bytes(n) + 16 * rcap] = False  # (scratch: contents unspecified)
    assert (buf[untouched] == FILL).all()


def _pad_to_one_workgroup(rng, cols):
    """The same columns in a batch of 4097: one workgroup per column."""
    tiny = A.synth_column(rng, 1, False, False)
    return cols + [tiny] * (4097 - len(cols))


# ---- hand-made columns (source streams of the assembly; closed: rings carry their closing vertex) ----------
def _i32(a):
    return np.asarray(a, dtype=np.int32)


def _flat(rings):
    return _i32([v for r in rings for pt in r for v in pt]).reshape(-1)


def _lines(rings):
    """A LINESTRING column: one feature per ring (a list of (x, y))."""
    return {"types": np.full(len(rings), 1, np.uint8), "go": _i32([]), "po": _i32([len(r) for r in rings]),
            "ro": _i32([]), "vo": None, "vb": _flat(rings), "closed": False}


def _multilines(features):
    """A MULTILINESTRING column: features as lists of rings."""
    rings = [r for f in features for r in f]
    return {"types": np.full(len(features), 4, np.uint8), "go": _i32([len(f) for f in features]),
            "po": _i32([len(r) for r in rings]), "ro": _i32([]), "vo": None, "vb": _flat(rings), "closed": False}


def _polygons(features):
    """A POLYGON column: features as lists of closed rings (shell first)."""
    rings = [r for f in features for r in f]
    return {"types": np.full(len(features), 2, np.uint8), "go": _i32([]), "po": _i32([len(f) for f in features]),
            "ro": _i32([len(r) for r in rings]), "vo": None, "vb": _flat(rings), "closed": True}


def _multipolygons(features):
    """A MULTIPOLYGON column: features as lists of parts as lists of closed rings."""
    parts = [p for f in features for p in f]
    rings = [r for p in parts for r in p]
    return {"types": np.full(len(features), 5, np.uint8), "go": _i32([len(f) for f in features]),
            "po": _i32([len(p) for p in parts]), "ro": _i32([len(r) for r in rings]), "vo": None, "vb": _flat(rings),
            "closed": True}


def _points(xy, multi=None):
    xy = _i32(xy).reshape(-1)
    if multi is None:
        return {"types": np.zeros(xy.size // 2, np.uint8), "go": _i32([]), "po": _i32([]), "ro": _i32([]), "vo": None,
                "vb": xy, "closed": False}
    return {"types": np.full(len(multi), 3, np.uint8), "go": _i32(multi), "po": _i32([]), "ro": _i32([]), "vo": None,
            "vb": xy, "closed": False}


def _box(x0, y0, w, h, cw=False):
    r = [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h), (x0, y0)]
    return r[::-1] if cw else r


def _path(rng, k, lim=1 << 20):
    return [tuple(int(v) for v in p) for p in rng.integers(-lim, lim, size=(k, 2))]


def _closed(rng, k, lim=1 << 20):
    p = _path(rng, max(k - 1, 1), lim)
    return p + p[:1] if k > 1 else p


def _one(covt, col):
    """The three arrays of a single hand-made column."""
    buf, mres, gres, md = _run(covt, [col])
    assert int(gres["status"][0]) == 0 and int(mres["status"][0]) == 0
    return _column_arrays(buf, int(md["off"][0]), col["types"].size)


# ---- synthetic columns ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_synthetic_columns(covt, oracle, gpu_available, seed):
    rng = np.random.default_rng(300 + seed)
    cols = []
    for i in range(32):
        big = i % 8 == 7  # up to 300 parts per feature, 40 rings per polygon, 3000 vertices per ring
        n = int(rng.choice([1, 2, 5])) if big else [0, 1, 5, 63, 64, 65, 200, 1000][(i + seed) % 8]
        cols.append(A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2), big=big))
    for t in range(6):  # one-type columns: runs of empty parts and rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 1500, bool(t & 1), bool(seed & 1), probs=probs))
    assert all(max(A.caps(c)) <= covt.GEOM_MAX_CAP for c in cols)
    buf, mres, gres, md = _run(covt, cols)
    assert (gres["status"] == 0).all() and (mres["status"] == 0).all()
    cache = {}
    _check(oracle, cols, buf, mres, md, cache)
    if seed == 1:  # the same columns, one workgroup each
        cols = _pad_to_one_workgroup(rng, cols)
        buf, mres, gres, md = _run(covt, cols)
        _check(oracle, cols, buf, mres, md, cache)


# ---- step boundaries --------------------------------------------------------------------------------------
def _boundary_columns(rng):
    cols = []
    for s in (LANES, CHUNK, 2 * CHUNK, CHUNK * WAVES):  # ring lengths around every coordinate step
        for k in (s - 1, s, s + 1):
            cols.append(_lines([_path(rng, k) for _ in range(9)]))
            cols.append(_polygons([[_closed(rng, k), _closed(rng, 5)] for _ in range(5)]))
    for s in (NARROW, 2 * NARROW, 64 * WAVES):  # rings / parts per feature around the features pass's steps
        for k in (s - 1, s, s + 1):
            cols.append(_polygons([[_closed(rng, 4)], [_closed(rng, int(rng.integers(1, 7))) for _ in range(k)],
                                   [_closed(rng, 6)] * 2]))
            cols.append(_multilines([[_path(rng, 3)], [_path(rng, int(rng.integers(0, 5))) for _ in range(k)]]))
            cols.append(_multipolygons([[[_closed(rng, 5)] * 2 for _ in range(k)], [[_closed(rng, 4)]]]))
    for s in (LANES, 64 * WAVES):  # as many features as a wave / a workgroup takes per step
        for k in (s - 1, s, s + 1):
            cols.append(A.synth_column(rng, k, False, True, probs=[0, 0.3, 0.4, 0, 0, 0.3]))
    return cols


def test_step_boundaries(covt, oracle, gpu_available):
    """Ring lengths, rings and parts per feature and feature counts one below, at and one above every step
    size of the kernels, with up to 64 workgroups per column and with one."""
    rng = np.random.default_rng(25)
    cols = _boundary_columns(rng)
    cols.append(A.synth_column(rng, 20000, False, False, probs=[0.1, 0.4, 0.4, 0, 0.05, 0.05]))  # > 64 * 4 chunks
    buf, mres, gres, md = _run(covt, cols)
    assert (gres["status"] == 0).all() and (mres["status"] == 0).all()
    assert int(gres["num_coords"][-1]) > 64 * WAVES * CHUNK
    cache = {}
    _check(oracle, cols, buf, mres, md, cache)
    cols = _pad_to_one_workgroup(rng, cols)
    buf, mres, gres, md = _run(covt, cols)
    _check(oracle, cols, buf, mres, md, cache)


def test_long_ring_carried_sums_and_many_holes(covt, oracle, gpu_available):
    """A ring of 40,001 coordinates (with 64 workgroups a workgroup's run is about 630 of them, with one it is
    cut into four) whose only vertices off one line are its first and last: a triangle over a base cut into
    39,998 collinear segments, so every partial sum a wave carries or hands on is a large number that only
    the whole ring cancels to the triangle's area.  And one polygon of 5,000 holes."""
    rng = np.random.default_rng(26)
    n = 39999
    base = [(1000 + 3 * i, 7 + 2 * i) for i in range(n)]  # on the line 2 x - 3 y = 1979
    apex = (-5000, 90000)
    tri = [apex] + base + [apex]
    shell = _box(-10, -10, 1000, 1000)
    holes = [_box(10 * (i % 90) + 1, 10 * (i // 90) + 1, 3 + i % 5, 2 + i % 7, cw=bool(i & 1)) for i in range(5000)]
    cols = [_polygons([[_closed(rng, 7)], [tri], [_closed(rng, 5)]]), _polygons([[_closed(rng, 4)], [shell] + holes]),
            _lines([_path(rng, 3), tri, _path(rng, 2)])]
    want_tri = abs(sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(tri, tri[1:]))) * 0.5
    want_holes = 1000 * 1000 - sum((3 + i % 5) * (2 + i % 7) for i in range(5000))
    cache = {}
    for batch in (cols, _pad_to_one_workgroup(rng, cols)):
        buf, mres, gres, md = _run(covt, batch)
        assert (mres["status"][:3] == 0).all()
        _check(oracle, batch, buf, mres, md, cache)
        assert _column_arrays(buf, int(md["off"][0]), 3)[0][1] == want_tri
        assert _column_arrays(buf, int(md["off"][1]), 2)[0][1] == float(want_holes)
        assert _column_arrays(buf, int(md["off"][2]), 3)[0].tobytes() == bytes(24)  # a LINESTRING: +0.0


def test_ring_past_its_owners_run(covt, oracle, gpu_available):
    """A column of 40 chunks in a batch of one workgroup per column gives wave 0 the run [0, 1280): its second
    ring starts at coordinate 10 and ends 2047, 2048 or 2049 coordinates past the run (the wave finishes it /
    the workgroup does), as a line and as a polygon ring followed by a hole; the same columns cut by 64
    workgroups."""
    rng = np.random.default_rng(30)
    total = 40 * CHUNK
    cols = []
    for r in (WIDE - 1, WIDE, WIDE + 1):
        second = 10 * CHUNK - 10 + r
        rest = total - 10 - second
        lengths = [10, second] + [7] * (rest // 7) + ([rest % 7] if rest % 7 else [])
        cols.append(_lines([_path(rng, k) for k in lengths]))
        cols.append(_polygons([[_closed(rng, 10)], [_closed(rng, second), _closed(rng, 9)]] +
                              [[_closed(rng, 7)] for _ in range((rest - 9) // 7)]))
    cache = {}
    for batch in (_pad_to_one_workgroup(rng, cols), cols):
        buf, mres, gres, md = _run(covt, batch)
        assert (gres["status"] == 0).all() and (mres["status"] == 0).all()
        assert int(gres["num_coords"][0]) == total
        _check(oracle, batch, buf, mres, md, cache)


# ---- sign and type gates ----------------------------------------------------------------------------------
def test_known_answers_signs_and_type_gates(covt, oracle, gpu_available):
    shell, hole = _box(0, 0, 10, 10), _box(4, 4, 2, 2, cw=True)
    area, length, count = _one(covt, _polygons([[_box(0, 0, 1, 1)], [_box(0, 0, 1, 1, cw=True)], [shell, hole],
                                                [shell, hole[::-1]], [shell[::-1], hole], [hole, shell]]))
    assert area.tolist() == [1.0, 1.0, 96.0, 96.0, 96.0, -96.0]  # (a hole larger than its shell: negative)
    assert length.tolist() == [4.0, 4.0, 48.0, 48.0, 48.0, 48.0] and count.tolist() == [5, 5, 10, 10, 10, 10]
    tri = [(0, 0), (4, 0), (0, 3), (0, 0)]
    area, length, count = _one(covt, _multipolygons([[[tri], [_box(10, 10, 4, 4), _box(11, 11, 1, 1, cw=True)]],
                                                     [[[(9, 9)], []], [], [_box(0, 0, 1, 1, cw=True)]], []]))
    assert area.tolist() == [21.0, 1.0, 0.0] and length.tolist() == [32.0, 4.0, 0.0] and count.tolist() == [14, 6, 0]
    # lines: a 3-4-5 segment, closed paths (no area), an empty and a 1-vertex line
    area, length, count = _one(covt, _lines([[(0, 0), (3, 4)], shell, hole, [], [(5, 5)]]))
    assert area.tobytes() == bytes(40) and length.tolist() == [5.0, 40.0, 8.0, 0.0, 0.0]
    assert count.tolist() == [2, 5, 5, 0, 1]
    area, length, count = _one(covt, _multilines([[[(0, 0), (3, 4)], [(0, 0), (0, 5), (12, 5)]], [shell, shell], []]))
    assert area.tobytes() == bytes(24) and length.tolist() == [22.0, 80.0, 0.0] and count.tolist() == [5, 10, 0]
    # points: both values +0.0 bit for bit
    rng = np.random.default_rng(27)
    xy = rng.integers(LO, HI, size=(300, 2), dtype=np.int64)
    for col, want in ((_points(xy), [1] * 300), (_points(xy, [0, 1, 64, 200, 0, 35]), [0, 1, 64, 200, 0, 35])):
        area, length, count = _one(covt, col)
        assert area.tobytes() == bytes(8 * len(want)) and length.tobytes() == bytes(8 * len(want))
        assert count.tolist() == want
    # the corners at +-(2^31 - 1): the wraparound value of the definition
    area, length, count = _one(covt, _polygons([[_box(-HI, -HI, 2 * HI, 2 * HI)]]))
    assert area.tolist() == [17179869180.0] and length.tolist() == [8.0 * HI]


def test_extreme_coordinates_across_chunk_edges(covt, oracle, gpu_available):
    """Rings of INT32_MIN / INT32_MAX coordinates, of lengths that put their edges across every chunk edge:
    the area equals the mod-2^64 reference bit for bit, and segment lengths near 2^32 * sqrt(2) stay finite
    and inside the bound."""
    rng = np.random.default_rng(28)
    corner = np.array([LO, HI, LO + 1, HI - 1, 0, -1, 1], dtype=np.int64)

    def ring(k):
        p = [tuple(int(v) for v in corner[rng.integers(0, corner.size, 2)]) for _ in range(k - 1)]
        return p + p[:1]

    cols = [_polygons([[ring(int(rng.integers(2, 100))) for _ in range(int(rng.integers(1, 4)))] for _ in range(300)]),
            _polygons([[ring(CHUNK - 1), ring(CHUNK + 1)], [ring(3 * CHUNK)], [ring(700), ring(2), ring(700)]]),
            _lines([[(LO, LO), (HI, HI)], [(LO, HI), (HI, LO), (LO, HI)]] + [ring(int(rng.integers(2, 300))) for _ in range(40)])]
    cache = {}
    for batch in (cols, _pad_to_one_workgroup(rng, cols)):
        buf, mres, gres, md = _run(covt, batch)
        assert (gres["status"] == 0).all() and (mres["status"] == 0).all()
        _check(oracle, batch, buf, mres, md, cache)
        length = _column_arrays(buf, int(md["off"][2]), 42)[1]
        diag = float(HI - LO) * 2.0 ** 0.5
        assert np.isfinite(length).all() and abs(length[0] - diag) <= 4 * 2.0 ** -52 * diag
        assert abs(length[1] - 2 * diag) <= 6 * 2.0 ** -52 * 2 * diag
    assert (np.abs(_reference(oracle, cols[0], cache)[1][0]) > 2.0 ** 60).any()  # (areas far outside the true range)


# ---- statuses ---------------------------------------------------------------------------------------------
def test_status_paths(covt, oracle, gpu_available):
    rng = np.random.default_rng(29)
    ok = A.synth_column(rng, 50, False, False)
    cols = [ok, ok, ok, ok, ok]
    #        0: fine   1: source stream failed   2: COVT_GEOM_TOO_LARGE   3: COVT_MEASURES_TOO_LARGE   4: fine
    buf, mres, gres, md = _run(covt, cols, flags_extra=[0, 0, 0x80000000, 0, 0],
                               in_res=[[-1] * 6, [0, -1, -1, -1, -1, 1], [-1] * 6, [-1] * 6, [-1] * 6],
                               dres=[0, 5, covt.ERR_TRUNCATED, 7], mflags=[0, 0, 0, covt.MEASURES_TOO_LARGE, 0])
    assert gres["status"].tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_INVALID_ARG, 0, 0]
    assert mres["status"].tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_INVALID_ARG, covt.ERR_INVALID_ARG, 0]
    assert (mres["reserved"] == 0).all()
    rcap = A.caps(ok)[1]
    for ci in (1, 2, 3):  # failed columns: the slice, its scratch included, untouched
        o = int(md["off"][ci])
        assert (buf[o:o + _rows_bytes(50) + 16 * rcap + 16] == FILL).all(), ci
    st, ref, m = _reference(oracle, ok)
    for ci in (0, 4):
        _compare(_column_arrays(buf, int(md["off"][ci]), 50), ref, m, "column %d" % ci)


# ---- fixture tiles ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_measures(covt, gpu_available):
    """Plan.measures_host() over every fixture tile, once for the tests below."""
    paths = tile_paths()
    tiles = [open(p, "rb").read() for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    buf, mres = plan.measures_host()
    return paths, tiles, plan, buf, mres


def test_fixture_tiles_measures(covt, oracle, fixture_measures):
    paths, tiles, plan, buf, mres = fixture_measures
    b = plan.measures
    n_ok = 0
    cache = {}
    for c in range(plan.num_geometry_columns):
        t, L = int(b["tile"][c]), int(b["layer"][c])
        if t not in cache:
            cache[t] = A.oracle_tile_columns(oracle, tiles[t])
        oc = cache[t][L]
        st = int(mres["status"][c])
        if oc["asm"] is None:  # a source stream failed to decode (SURVEY Q4 tiles)
            assert st != 0
            continue
        assert st == oc["asm"][0] == 0, (tile_key(paths[t]), L, st)
        col = plan.measures_column(buf, mres, c)
        assert len(col) == oc["types"].size
        ref = M.measures_numpy(oc["types"], *oc["asm"][1:], fsum=True)
        _compare((col.area, col.length, col.num_coords), ref, M.segments(*oc["asm"][1:4]), "%s layer %d" % (tile_key(paths[t]), L))
        n_ok += 1
    assert n_ok >= 700


def test_fixture_tiles_measures_equal_those_of_gpu_wkb(covt, fixture_measures):
    """Two products agree: every row is the area, length and point count of the WKB value the WKB pass wrote
    for the feature."""
    paths, tiles, plan, buf, mres = fixture_measures
    wbuf, wres = plan.wkb_host()
    assert np.array_equal(mres["status"] == 0, wres["status"] == 0)
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(mres["status"][c]):
            continue
        w = plan.wkb_column(wbuf, wres, c)
        col = plan.measures_column(buf, mres, c)
        *ref, m = M.wkb_measures(w.offsets, w.data, with_segments=True, parse=False)
        _compare((col.area, col.length, col.num_coords), ref, m, "column %d" % c)
        n_ok += 1
    assert n_ok >= 700


# ---- DeviceBatch / DevicePlan -----------------------------------------------------------------------------
def _same_rows(plan, mres, x, y):
    """The columns' three arrays in two measures buffers hold the same bytes (scratch and gaps aside)."""
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(mres["status"][c]) == 0:
            o, n = int(plan.measures["off"][c]), int(plan.measures["n_features"][c])
            assert x[o:o + 20 * n].tobytes() == y[o:o + 20 * n].tobytes(), c
            n_ok += 1
    return n_ok


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_device_paths_match_host_path(covt, gpu_available, n_tiles):
    import torch

    tiles = [open(p, "rb").read() for p in tile_paths(("omt",))[:n_tiles]]
    plan = covt.Plan.from_tiles(tiles)
    buf_h, mres_h = plan.measures_host()
    assert (mres_h["status"] == 0).any()
    b = covt.DeviceBatch(plan, "cuda:0")
    b.decode()
    b.assemble()
    b.measures()
    torch.cuda.synchronize()
    buf_d, mres_d = b.measures_results()
    assert mres_h.tobytes() == mres_d.tobytes()
    assert _same_rows(plan, mres_h, buf_h, buf_d) > 0
    # the device plan: the same records and descriptors, the same bytes
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    mi, mdd = dp.measures_copy()
    assert mi.tobytes() == plan.measures.tobytes() and mdd.tobytes() == plan.mdescs.tobytes()
    assert dp.measures_bytes == plan.measures_bytes
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_m, d_mres = dp.alloc_measures()
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.measures(d_out, d_asm, d_gres, d_m, d_mres)
    torch.cuda.synchronize()
    mres_p = d_mres.cpu().numpy().view(covt.MEASURES_RESULT_DTYPE)[:plan.num_geometry_columns][plan.measures["desc_index"]]
    assert mres_h.tobytes() == mres_p.tobytes()
    assert _same_rows(plan, mres_h, buf_h, d_m.cpu().numpy()[:plan.measures_bytes]) > 0


def test_decode_covt_yields_measures_per_layer(covt, oracle, gpu_available, decodable_tiles):
    """CovtParser.decode_covt gives every layer its measures beside its WKB column."""
    tile = decodable_tiles[0][1]
    layers = covt.CovtParser.decode_covt(tile)
    cols = A.oracle_tile_columns(oracle, tile)
    assert layers and all(lc.measures is not None for lc in layers if lc.geometry.geometryTypes is not None)
    for lc in layers:
        oc = cols[lc.layer]
        assert len(lc.measures) == len(lc.wkb) == oc["types"].size
        assert lc.measures.length.size == lc.measures.num_coords.size == len(lc.wkb)
        assert int(lc.measures.num_coords.sum()) == oc["asm"][4].shape[0]
        ref = M.measures_plain(oc["types"], *oc["asm"][1:])
        _compare((lc.measures.area, lc.measures.length, lc.measures.num_coords), ref, M.segments(*oc["asm"][1:4]),
                 "layer %d" % lc.layer)


def test_decode_assemble_measures_replay_in_a_hip_graph(covt, gpu_available, decodable_tiles):
    """decode + assemble + measures of a small batch captured in one HIP graph and replayed twice into poisoned
    buffers: the bytes of the eager run each time, length included (no float atomics, every element written
    once; the assembly's scratch needs the warm-up launch on the capture stream before the capture)."""
    import torch

    tiles = [t for _, t in decodable_tiles]
    plan = covt.Plan.from_tiles(tiles)
    dev = torch.device("cuda:0")
    b = covt.DeviceBatch(plan, dev)
    s = torch.cuda.Stream(dev)

    def launch():
        b.decode(s)
        b.assemble(s)
        b.measures(s)

    with torch.cuda.stream(s):
        launch()  # fork streams, events and the assembly scratch exist before the capture
    torch.cuda.synchronize()
    buf_e, mres_e = b.measures_results()
    buf_e = buf_e.copy()
    assert (mres_e["status"] == 0).all()
    buf_h, mres_h = plan.measures_host()
    assert mres_h.tobytes() == mres_e.tobytes()
    assert _same_rows(plan, mres_e, buf_e, buf_h) == plan.num_geometry_columns  # (another entry point, the same kernels)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for _ in range(2):
        b.d_measures.fill_(FILL)
        b.d_mres.fill_(0x5A5A5A5A)
        b.d_asm.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        buf, mres = b.measures_results()
        assert mres.tobytes() == mres_e.tobytes()
        assert _same_rows(plan, mres_e, buf_e, buf) == plan.num_geometry_columns
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


# ---- GpuCovtBatch.measuresBytes / measuresColumns / geometryMeasures through the JNI shim and a fake VM ----
@pytest.fixture(scope="module")
def measures_shim(covt):
    """tests/jni_measures/jni_measures_test: the shim compiled against the stand-in tests/jni/jni.h with the
    compiler line of tests/jni/Makefile."""
    import os
    import subprocess

    from conftest import ROOT

    covt.lib()
    src = os.path.join(ROOT, "tests", "jni_measures", "jni_measures_test.cc")
    exe = src[:-3]
    lib_dir = os.path.join(ROOT, "cov-tiles_amd")
    deps = [src, os.path.join(ROOT, "tests", "jni", "jni.h"), os.path.join(lib_dir, "jni", "covt_jni.cc"),
            os.path.join(ROOT, "include", "covt.h"), os.path.join(lib_dir, "libcovt.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall",
                               "-I" + os.path.join(ROOT, "tests", "jni"), "-I" + os.path.join(ROOT, "include"),
                               "-o", exe, src, os.path.join(lib_dir, "jni", "covt_jni.cc"), "-L" + lib_dir, "-lcovt",
                               "-Wl,-rpath,$ORIGIN/../../cov-tiles_amd", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def _shim_run(exe, case):
    import subprocess

    p = subprocess.run([exe], input=case + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    (out,) = p.stdout.splitlines()
    return out.split()


def _jni_case(mode):
    import os

    from conftest import ROOT

    tile = open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()
    return [tile], "%s %d | %s" % (mode, len(tile), tile.hex())


def test_geometry_measures_through_jni(measures_shim, covt, gpu_available):
    """geometryMeasures into a direct buffer: the status rows, the MEASURES_FIELDS rows and the arrays equal
    Plan.measures_host()'s."""
    tiles, case = _jni_case("measures")
    kind, nb, cols_hex, res_hex, out_hex = _shim_run(measures_shim, case)
    plan = covt.Plan.from_tiles(tiles)
    buf, mres = plan.measures_host()
    assert kind == "ok" and int(nb) == plan.measures_bytes
    rows = np.frombuffer(bytes.fromhex(cols_hex), "<i8").reshape(-1, 5)
    b = plan.measures
    want = np.stack([b[f].astype(np.int64) for f in ("tile", "layer", "n_features", "desc_index", "off")], axis=1)
    assert np.array_equal(rows, want)
    res = np.frombuffer(bytes.fromhex(res_hex), "<i8").reshape(-1, 1)
    assert np.array_equal(res[:, 0], mres["status"]) and (mres["status"] == 0).all()
    jout = np.frombuffer(bytes.fromhex(out_hex), np.uint8)
    assert _same_rows(plan, mres, buf, jout) >= 5


@pytest.mark.parametrize("mode", ["short", "heap"])
def test_geometry_measures_jni_rejects_bad_buffers(measures_shim, gpu_available, mode):
    """A buffer one byte short of measuresBytes(), or one that is not direct: IllegalArgumentException."""
    _, case = _jni_case(mode)
    assert _shim_run(measures_shim, case) == ["exc", "java/lang/IllegalArgumentException"]

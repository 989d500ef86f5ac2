"""GPU: the simplify pass (covt_simplify.hip, include/covt.h "Geometry simplification") against the reference of
tests/covt_simplify.py, byte for byte, through the C-ABI: covt_geometry_simplify_device on hand-made assembled
columns (offsets, coordinates and types written here, no decode), covt_plan_simplify_host and the downstream
passes on the fixture tiles, the DeviceBatch / DevicePlan paths, a HIP-graph replay and decode_covt.  Buffers
start as a fill pattern; every byte the definition leaves unwritten (the gaps between slices, the capacity past
the counts, the slices of failed columns) must still hold it -- the scratch of a column that ran excepted --
and the input buffers must be unchanged.

The kernels' step sizes the boundary cases are built around: the rings pass works in chunks of 128 coordinates
(a wave's row of 64 lanes x 2), 4 waves a workgroup, up to 64 workgroups per column while 8192 / n_columns allows
(4096 columns: 2, 4097: 1), a ring with 2048 coordinates or more left past its owner's run is finished by the
whole workgroup; the count and write passes work in chunks of 1024 coordinates (8 rows of 128), a wave each, and
mark the rings that start in a row 64 at a step; a feature of 64 parts or rings or more is finished by its whole
wave; the scan takes 1024 rings (256 in a batch of
more than 4096 columns) per step.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_bbox as B
import covt_measures as M
import covt_select as SEL
import covt_simplify as S
import covt_wkb as W
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
ROW, CHUNK, WAVES, NARROW, WIDE = 128, 1024, 4, 64, 2048
FIXTURE_SHIFT = 4  # (tests/test_simplify_ref.py: the fixtures are not vacuous at this shift)
LO, HI = -(1 << 31), (1 << 31) - 1
GDESC = np.dtype([("in_off", np.int64, 6), ("in_len", np.int32, 6), ("in_res", np.int32, 6), ("out_off", np.int64, 6),
                  ("part_cap", np.int32), ("ring_cap", np.int32), ("coord_cap", np.int32), ("flags", np.int32)])


def _a16(x):
    return (x + 15) & ~15


def _members(n, pc, rc, cc):
    """Offsets of geometry_offsets, part_offsets, ring_offsets, coords, the scratch and the slice's end."""
    part = _a16(4 * (n + 1))
    ring = part + _a16(4 * (pc + 1))
    xy = ring + _a16(4 * (rc + 1))
    scratch = xy + _a16(8 * cc)
    return 0, part, ring, xy, scratch, scratch + _a16(4 * rc) + _a16(4 * ((cc + CHUNK - 1) // CHUNK + 1))


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


def _walk(rng, k, step=6, lim=1 << 14):
    """k points of a random walk with small steps: neighbours often share a grid cell."""
    if k == 0:
        return []
    p = rng.integers(-lim, lim, size=2) + np.cumsum(rng.integers(-step, step + 1, size=(k, 2)), axis=0)
    return [(int(x), int(y)) for x, y in p]


def _closed(rng, k, step=6):
    p = _walk(rng, max(k - 1, 1), step)
    return p + p[:1] if k > 1 else p


def _box(x0, y0, w, h):
    return [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h), (x0, y0)]


def _lines(rings):
    return _column([(1, [[r]]) for r in rings])


def _pack(covt, cols, pad=(3, 5, 7)):
    """The decode buffer (types only), the assembly buffer, the geometry descriptors and results, and the
    simplify descriptors by the plan's layout rule with a 16-byte gap after every slice."""
    nc = len(cols)
    gd = np.zeros(nc, GDESC)
    gres = np.zeros(nc, covt.GEOM_RESULT_DTYPE)
    sd = np.zeros(nc, covt.SIMPLIFY_DESC_DTYPE)
    dec_off = asm_off = s_off = 0
    lay = []
    for ci, col in enumerate(cols):
        n, P, R, V = col["types"].size, col["part"].size - 1, col["ring"].size - 1, col["xy"].shape[0]
        pc, rc, cc = col.get("caps") or (P + pad[0], R + pad[1], V + pad[2])
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
        gres[ci] = (col.get("status", 0), P, R, V)
        sd[ci]["off"] = s_off + col.get("sd_off", 0)
        sd[ci]["n_features"] = n + col.get("sd_n", 0)
        sd[ci]["part_cap"], sd[ci]["ring_cap"], sd[ci]["coord_cap"] = pc, rc + col.get("sd_rc", 0), cc
        sd[ci]["flags"] = col.get("sflags", 0)
        lay.append((dec_off, o, s_off, (n, pc, rc, cc)))
        dec_off += _a16(n)
        asm_off = o[3] + _a16(8 * cc)
        s_off += _members(n, pc, rc, cc)[5] + 16
    dec = np.full(max(dec_off, 16), FILL, np.uint8)
    asm = np.full(max(asm_off, 16), FILL, np.uint8)
    for col, (d_off, o, _, _) in zip(cols, lay):
        dec[d_off:d_off + col["types"].size] = col["types"]
        for k, name in enumerate(("geo", "part", "ring", "xy")):
            a = np.ascontiguousarray(col[name]).view(np.uint8).reshape(-1)
            asm[o[k]:o[k] + a.size] = a
    return dec, asm, gd, gres, sd, max(s_off, 16), lay


def _run(covt, cols, shift=0, shifts=None, expect=0):
    """covt_geometry_simplify_device over hand-made columns -> (simplify buffer, results, layout)."""
    import torch

    dec, asm, gd, gres, sd, s_bytes, lay = _pack(covt, cols)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_dec, d_asm, d_gd, d_gres, d_sd = up(dec), up(asm), up(gd), up(gres), up(sd)
    d_shift = torch.from_numpy(np.asarray(shifts, np.int32)).to(dev) if shifts is not None else None
    d_out = torch.full((s_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_res = torch.full((16 * len(cols),), FILL, dtype=torch.uint8, device=dev)
    st = covt.lib().covt_geometry_simplify_device(
        d_dec.data_ptr(), d_gd.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(), d_sd.data_ptr(), len(cols), shift,
        d_shift.data_ptr() if d_shift is not None else None, d_out.data_ptr(), d_res.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert st == expect
    # the inputs are unchanged
    assert d_dec.cpu().numpy().tobytes() == dec.tobytes() and d_asm.cpu().numpy().tobytes() == asm.tobytes()
    assert d_gd.cpu().numpy().tobytes() == gd.tobytes() and d_gres.cpu().numpy().tobytes() == gres.tobytes()
    assert d_sd.cpu().numpy().tobytes() == sd.tobytes()
    return d_out.cpu().numpy(), d_res.cpu().numpy().view(covt.GEOM_RESULT_DTYPE), lay


def _reference(col, s, cache):
    key = (id(col), s)
    if key not in cache:
        cache[key] = S.simplify_ref(col["types"], col["geo"], col["part"], col["ring"], col["xy"], s)
    return cache[key]


def _check(covt, cols, buf, res, lay, shift=0, shifts=None, status=None, cache=None):
    """Every column equals the reference byte for byte; every byte the definition leaves unwritten holds FILL
    (the scratch of a column that ran: contents unspecified)."""
    cache = {} if cache is None else cache
    untouched = np.ones(buf.size, dtype=bool)
    for ci, col in enumerate(cols):
        want_st = status[ci] if status else 0
        assert int(res["status"][ci]) == want_st, (ci, res[ci], want_st)
        if want_st:
            assert res[ci].tolist() == (want_st, 0, 0, 0), (ci, res[ci])
            continue
        s = int(shifts[ci]) if shifts is not None else shift
        ring, xy = _reference(col, s, cache)
        _, _, o, (n, pc, rc, cc) = lay[ci]
        m = _members(n, pc, rc, cc)
        P, R = col["part"].size - 1, col["ring"].size - 1
        assert res[ci].tolist() == (0, P, R, xy.shape[0]), (ci, res[ci], xy.shape[0])
        for k, want in ((0, col["geo"]), (1, col["part"]), (2, ring), (3, xy)):
            w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
            got = buf[o + m[k]:o + m[k] + w.size]
            if got.tobytes() != w.tobytes():
                bad = int(np.nonzero(got != w)[0][0]) // 4
                raise AssertionError("column %d member %d: first difference at int32 %d: got %r, want %r (shift %d)"
                                     % (ci, k, bad, got.view(np.int32)[bad:bad + 4], w.view(np.int32)[bad:bad + 4], s))
            untouched[o + m[k]:o + m[k] + w.size] = False
        untouched[o + m[4]:o + m[5]] = False
    assert (buf[untouched] == FILL).all(), np.nonzero(untouched & (buf != FILL))[0][:8]


def _tiny():
    return _column([(1, [[[(0, 0), (40, 40)]]])])


def _both_batches(covt, cols, shift):
    """The columns with up to 64 workgroups each, and in a batch of 4097 (one workgroup, a wave's scan)."""
    cache = {}
    buf, res, lay = _run(covt, cols, shift)
    _check(covt, cols, buf, res, lay, shift, cache=cache)
    tiny = _tiny()
    padded = cols + [tiny] * (4097 - len(cols))
    buf, res, lay = _run(covt, padded, shift)
    _check(covt, padded, buf, res, lay, shift, cache=cache)


# ---- step boundaries ----------------------------------------------------------------------------------------
def test_rings_around_chunk_boundaries_and_small_rings_of_every_type(covt, gpu_available):
    """Rings that end one before, at and one after the boundaries of the 128- and the 1024-coordinate chunks;
    rings of 0 .. 5 coordinates of every type between longer ones."""
    rng = np.random.default_rng(71)
    cols = []
    for edge in (ROW, 2 * ROW, CHUNK, 2 * CHUNK, WAVES * ROW):
        for d in (-1, 0, 1):
            k = edge + d
            cols.append(_lines([_walk(rng, k), _walk(rng, 9), _walk(rng, k - 9), _walk(rng, 5 * CHUNK - 2 * k + 5)]))
            cols.append(_column([(2, [[_closed(rng, k), _closed(rng, 7)]]), (2, [[_closed(rng, 2 * CHUNK - k - 7)]]),
                                 (5, [[_closed(rng, 30)], [_closed(rng, 5)] * 2])]))
    small = []
    for t in range(6):
        for k in range(6):
            ring = _closed(rng, k, step=40) if t in (2, 5) else _walk(rng, k, step=40)
            small.append((t, [[ring]] if t < 3 else [[ring], [ring[::-1]]]))
            small.append((1, [[_walk(rng, 50)]]))
    cols.append(_column(small))
    cols.append(_column(small[::-1]))
    for shift in (0, 3):
        _both_batches(covt, cols, shift)


def test_equal_runs_across_chunk_and_run_boundaries(covt, gpu_available):
    """Runs of equal coordinates that span a 128-row, a 1024-chunk and a wave-run boundary (40 rows over the 4
    waves of one workgroup: runs end at 1280, 2560, 3840), inside one ring and across two rings (the second
    ring's first coordinate is kept although it equals its predecessor)."""
    rng = np.random.default_rng(72)
    total = 40 * ROW
    pts = _walk(rng, total, step=30)
    for a, b in ((120, 140), (1000, 1100), (1270, 1290), (2559, 2562), (3800, 3900), (5100, 5119)):
        for i in range(a, b):
            pts[i] = pts[a]
    one = _lines([pts])
    # the same coordinates cut into rings inside the runs and at the boundaries
    cuts = [0, 130, 1024, 1025, 1280, 2560, 2561, 3840, 3850, total]
    two = _lines([pts[a:b] for a, b in zip(cuts, cuts[1:])])
    poly = _column([(2, [[pts[:1279] + pts[:1], pts[1279:2600] + pts[1279:1280]]]), (4, [[pts[2600:2601] * 300], [pts[2900:]]])])
    for shift in (0, 2):
        _both_batches(covt, [one, two, poly], shift)


def test_shell_with_70_holes_collapses(covt, gpu_available):
    """A part of 1 shell and 70 holes whose shell collapses (wider than the narrow path of the features pass),
    beside the same part with a standing shell, and a multipolygon of 200 parts of both kinds."""
    holes = [_box(100 + 40 * (i % 10), 100 + 40 * (i // 10), 20 + i % 3, 18) for i in range(70)]
    gone, stands = _box(3, 3, 2, 2), _box(0, 0, 640, 640)
    many = [[gone if i % 3 == 0 else stands] + holes[:i % 5] for i in range(200)]
    col = _column([(2, [[gone] + holes]), (2, [[stands] + holes]), (5, many), (5, [[gone] + holes, [stands] + holes])])
    cache = {}
    buf, res, lay = _run(covt, [col], 4)
    _check(covt, [col], buf, res, lay, 4, cache=cache)
    ring, _ = _reference(col, 4, cache)
    k = np.diff(ring)
    assert (k[:71] == 0).all() and (k[71:142] == 5).all()  # the first feature is empty, the second stands whole
    _both_batches(covt, [col], 4)


def test_one_ring_of_300000_coordinates(covt, gpu_available):
    """One ring alone: 64 workgroups cut it into runs; in a batch of 4097 wave 0 owns it and hands 225,000
    coordinates to its workgroup."""
    rng = np.random.default_rng(73)
    k = 300001
    p = np.cumsum(rng.integers(-3, 4, size=(k - 1, 2)), axis=0)
    pts = np.concatenate([p, p[:1]]).astype(np.int32)
    col = {"types": np.array([2], np.uint8), "geo": np.array([0, 1], np.int32), "part": np.array([0, 1], np.int32),
           "ring": np.array([0, k], np.int32), "xy": pts}
    line = dict(col, types=np.array([1], np.uint8))
    cache = {}
    for shift in (0, 2):
        buf, res, lay = _run(covt, [col, line], shift)
        _check(covt, [col, line], buf, res, lay, shift, cache=cache)
        assert 1000 < int(res["num_coords"][0]) < k
    padded = [col] + [_tiny()] * 4096
    buf, res, lay = _run(covt, padded, 2)
    _check(covt, padded, buf, res, lay, 2, cache=cache)


def test_batches_of_4096_and_4097_columns_give_the_same_bytes(covt, gpu_available):
    rng = np.random.default_rng(74)
    base = [_lines([_walk(rng, int(k)) for k in rng.integers(0, 40, size=30)]),
            _column([(2, [[_closed(rng, int(k), step=20), _closed(rng, 6)]]) for k in rng.integers(1, 300, size=12)]),
            _column([(3, [[[pt]] for pt in _walk(rng, 70)]), (0, [[_walk(rng, 1)]])]), _lines([_walk(rng, 2500)])]
    cache = {}
    slices = {}
    for nc in (4096, 4097):
        cols = (base * (nc // len(base) + 1))[:nc]
        buf, res, lay = _run(covt, cols, 3)
        _check(covt, cols, buf, res, lay, 3, cache=cache)
        for ci in range(len(base)):
            _, _, o, caps = lay[ci]
            slices.setdefault(ci, []).append(buf[o:o + _members(*caps)[4]].tobytes())  # (up to the scratch)
    assert all(a == b for a, b in slices.values())


def test_empty_columns_everything_collapsing_nothing_changing(covt, gpu_available):
    rng = np.random.default_rng(75)
    none = _column([])
    no_coords = _column([(1, [[[]]]), (2, [[[], []]]), (5, []), (3, []), (4, [[[]], [[]]])])
    grid = _column([(2, [[_box(16 * i, 32 * i, 160, 320), _box(16 * i + 16, 32 * i + 16, 32, 32)]]) for i in range(300)] +
                   [(1, [[[(16 * i, -16 * i) for i in range(700)]]]), (0, [[[(48, 64)]]])])
    small = _column([(1, [[_walk(rng, 50, lim=100)]]), (2, [[_closed(rng, 2000, step=2)[:-1] + [(0, 0)]]]),
                     (4, [[_walk(rng, 5, lim=100)]] * 90), (0, [[[(7, 7)]]]), (3, [[[(1, 1)]], [[(2, 2)]]])])
    # runs of more than 64 empty rings inside one row of 128 coordinates (the marks take 64 rings a step)
    gaps = _column([(1, [[_walk(rng, 50)]]), (4, [[[]]] * 200), (1, [[_walk(rng, 50)]]), (5, [[[], []]] * 70),
                    (1, [[_walk(rng, 9)]]), (4, [[[]]] * 64), (2, [[_closed(rng, 9, step=40)]])])
    cache = {}
    cols = [none, no_coords, grid, small, gaps]
    for shift, which in ((4, 2), (30, 3)):
        buf, res, lay = _run(covt, cols, shift)
        _check(covt, cols, buf, res, lay, shift, cache=cache)
        ring, xy = _reference(cols[which], shift, cache)
        if which == 2:  # on the grid already: nothing changes
            assert ring.tobytes() == grid["ring"].tobytes() and xy.tobytes() == grid["xy"].tobytes()
        else:  # everything snaps to (0, 0): only the three points are left
            assert int(ring[-1]) == 3 and not xy.any()
    _both_batches(covt, cols, 4)


def test_per_column_shifts_against_uniform(covt, gpu_available):
    rng = np.random.default_rng(76)
    base = [_lines([_walk(rng, 700, step=50)]), _column([(2, [[_closed(rng, 40, step=60), _closed(rng, 9, step=9)]])] * 20),
            _column([(5, [[_closed(rng, 12, step=300)]] * 70)])]
    shifts = [0, 1, 4, 7, 12, 30]
    cols = [base[i % 3] for i in range(3 * len(shifts))]
    per = [shifts[i // 3] for i in range(len(cols))]
    cache = {}
    buf, res, lay = _run(covt, cols, 9, shifts=per)  # (the uniform shift is not read)
    _check(covt, cols, buf, res, lay, shifts=per, cache=cache)
    for s in shifts:
        ubuf, ures, ulay = _run(covt, base, s)
        _check(covt, base, ubuf, ures, ulay, s, cache=cache)
        for k in range(3):
            ci = 3 * shifts.index(s) + k
            caps = lay[ci][3]
            end = _members(*caps)[4]
            assert buf[lay[ci][2]:lay[ci][2] + end].tobytes() == ubuf[ulay[k][2]:ulay[k][2] + end].tobytes(), (s, k)
            assert res[ci].tobytes() == ures[k].tobytes()


@pytest.mark.parametrize("s", [1, 4, 30])
def test_int32_extremes(covt, gpu_available, s):
    h = 1 << (s - 1)
    vals = [HI, HI - h, LO, -1, HI - 1, LO + 1, LO + h, h, h - 1, -h, -h - 1, 0]
    pts = [(a, b) for a in vals for b in vals]
    col = _column([(1, [[pts]]), (3, [[pts[:40]]]), (2, [[[(LO, LO), (HI, LO), (HI, HI), (LO, HI), (LO, LO)]]]),
                   (1, [[[(HI, HI), (HI - h, HI - h)]]])])
    cache = {}
    buf, res, lay = _run(covt, [col], s)
    _check(covt, [col], buf, res, lay, s, cache=cache)
    ring, xy = _reference(col, s, cache)
    m = (HI >> s) << s
    assert int(xy.max()) == m and int(xy.min()) == LO and int(np.diff(ring)[3]) == 0  # the last line snaps to one point


def test_status_paths(covt, gpu_available):
    rng = np.random.default_rng(77)
    ok = _column([(2, [[_closed(rng, 30, step=40)]]), (1, [[_walk(rng, 90, step=40)]])] * 10)
    I = covt.ERR_INVALID_ARG
    cols = [ok, dict(ok, status=covt.ERR_TRUNCATED), dict(ok, gflags=0x80000000 - (1 << 32)), dict(ok, sd_rc=1),
            dict(ok, sflags=covt.SIMPLIFY_TOO_LARGE), dict(ok, sd_off=8), dict(ok, sd_n=1), ok, ok, ok]
    status = [0, covt.ERR_TRUNCATED, I, I, I, I, I, I, I, 0]
    per = [3, 3, 3, 3, 3, 3, 3, 31, -1, 30]
    buf, res, lay = _run(covt, cols, 0, shifts=per)
    _check(covt, cols, buf, res, lay, shifts=per, status=status)
    for ci, st in enumerate(status):  # a failed column's slice, its scratch included, is untouched
        if st:
            o = lay[ci][2]
            assert (buf[o:o + _members(*lay[ci][3])[5] + 16] == FILL).all(), ci
    # a uniform shift outside the range: the call itself, nothing written
    for bad in (31, -1):
        buf, res, lay = _run(covt, [ok, ok], bad, expect=I)
        assert (buf == FILL).all() and (res.view(np.uint8) == FILL).all()


# ---- fixture tiles: the pass and everything downstream ------------------------------------------------------
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
    wkb0 = plan.wkb_host()
    return {"paths": paths, "plan": plan, "asm": asm, "gres": gres, "types": types, "wkb0": wkb0}


@pytest.mark.parametrize("shift", [0, FIXTURE_SHIFT, 12])
def test_fixture_tiles_simplify_and_downstream(covt, fixtures, shift):
    """covt_plan_simplify_host on every fixture tile against the reference applied to assemble_host's output, and
    with set_simplify the WKB, bounding-box, measures and select passes on the simplified column against their
    own references fed with the reference's simplified column.  At 12 a 4096-extent layer collapses entirely.
    Unsetting restores the plain WKB bytes."""
    plan, asm, gres, types = fixtures["plan"], fixtures["asm"], fixtures["gres"], fixtures["types"]
    sbuf, sres = plan.simplify_host(shift)
    assert np.array_equal(sres["status"], gres["status"])
    plan.set_simplify(shift)
    try:
        wbuf, wres = plan.wkb_host()
        bbuf, bres = plan.bbox_host()
        mbuf, mres = plan.measures_host()
        pred = covt.SelectPred(window=(0.0, 0.0, 3000.0, 3000.0), min_area=64.0, min_length=32.0)
        lbuf, lres = plan.select_host(pred)
    finally:
        plan.set_simplify(None)
    n_ok = removed = emptied = 0
    for c in range(plan.num_geometry_columns):
        if int(gres["status"][c]):
            assert sres[c].tolist() == (int(gres["status"][c]), 0, 0, 0)
            continue
        g = plan.geometry_arrays(asm, gres, c)
        ring, xy = S.simplify_ref(types[c], g.geometry_offsets, g.part_offsets, g.ring_offsets, g.coords, shift)
        got = plan.simplified_arrays(sbuf, sres, c)
        what = (tile_key(fixtures["paths"][int(plan.geom["tile"][c])]), int(plan.geom["layer"][c]), shift)
        assert sres[c].tolist() == (0, int(gres["num_parts"][c]), int(gres["num_rings"][c]), xy.shape[0]), what
        assert got.geometry_offsets.tobytes() == g.geometry_offsets.tobytes(), what
        assert got.part_offsets.tobytes() == g.part_offsets.tobytes(), what
        assert got.ring_offsets.tobytes() == ring.tobytes() and got.coords.tobytes() == xy.tobytes(), what
        col = (types[c], g.geometry_offsets, g.part_offsets, ring, xy)
        offs, data = W.write_numpy(*col)
        w = plan.wkb_column(wbuf, wres, c)
        assert w.offsets.tobytes() == np.asarray(offs, np.int32).tobytes() and w.data.tobytes() == data.tobytes(), what
        b = plan.bbox_column(bbuf, bres, c)
        assert B.same((b.xmin, b.ymin, b.xmax, b.ymax, b.extent, b.n_empty), B.bbox_numpy(*col[1:])), what
        m = plan.measures_column(mbuf, mres, c)
        ref = M.measures_numpy(*col, fsum=True)
        assert m.area.tobytes() == ref[0].tobytes() and m.num_coords.tobytes() == ref[2].tobytes(), what
        assert (np.abs(m.length - ref[1]) <= M.length_bound(ref[1], M.segments(*col[1:4]))).all(), what
        mask = SEL.predicate_ref(b.xmin, b.ymin, b.xmax, b.ymax, m.area, m.length, pred)
        sel, soffs, sdata = SEL.select_ref(w.offsets, w.data, mask)
        k = plan.select_column(lbuf, lres, c)
        assert k.index.tobytes() == sel.tobytes() and k.wkb.offsets.tobytes() == soffs.tobytes(), what
        assert k.wkb.data.tobytes() == sdata.tobytes(), what
        n_ok += 1
        removed += int(gres["num_coords"][c]) - xy.shape[0]
        emptied += int(xy.shape[0] == 0 and int(gres["num_coords"][c]) > 0)
    assert n_ok >= 700
    if shift:
        assert removed > 0
    if shift == 12:
        assert emptied > 0
    wbuf0, wres0 = fixtures["wkb0"]
    again, ares = plan.wkb_host()  # unset: today's bytes
    assert ares.tobytes() == wres0.tobytes()
    for c in range(plan.num_geometry_columns):
        if int(wres0["status"][c]) == 0:
            x, y = plan.wkb_column(wbuf0, wres0, c), plan.wkb_column(again, ares, c)
            assert x.offsets.tobytes() == y.offsets.tobytes() and x.data.tobytes() == y.data.tobytes(), c


def test_projected_wkb_of_the_simplified_column(covt, fixtures):
    """CRS84 once: the projected WKB pass on the simplified column (set_simplify, per-tile shifts) against the
    reference writer over the reference's simplified column, held as tests/test_gpu_geo.py holds the plain
    column: offsets and every non-coordinate byte equal, the coordinates apply(xf, simplified coordinates)."""
    import covt_geo as G
    from test_gpu_geo import _check_wkb_column

    plan, asm, gres, types = fixtures["plan"], fixtures["asm"], fixtures["gres"], fixtures["types"]
    zxy = [list(G.zxy_of_key(tile_key(p))) for p in fixtures["paths"]]
    per_tile = [FIXTURE_SHIFT if t % 2 else 6 for t in range(plan.n_tiles)]
    plan.set_simplify(per_tile)
    try:
        wbuf, wres = plan.wkb_host(covt.CRS_CRS84, zxy)
    finally:
        plan.set_simplify(None)
    sbuf, sres = plan.simplify_host(per_tile)
    table, _ = plan.geo_transforms(covt.CRS_CRS84, zxy)
    n_ok = 0
    for c in range(0, plan.num_geometry_columns, 5):
        if int(wres["status"][c]):
            continue
        g = plan.geometry_arrays(asm, gres, c)
        s = per_tile[int(plan.geom["tile"][c])]
        ring, xy = S.simplify_ref(types[c], g.geometry_offsets, g.part_offsets, g.ring_offsets, g.coords, s)
        got = plan.simplified_arrays(sbuf, sres, c)
        assert got.ring_offsets.tobytes() == ring.tobytes() and got.coords.tobytes() == xy.tobytes(), c
        offs, data = W.write_numpy(types[c], g.geometry_offsets, g.part_offsets, ring, xy)
        w = plan.wkb_column(wbuf, wres, c)
        _check_wkb_column(np.asarray(offs, np.int32), data, w.offsets, w.data, table[int(plan.geom["desc_index"][c])], xy,
                          "column %d" % c)
        n_ok += 1
    assert n_ok >= 100


# ---- DeviceBatch / DevicePlan, graph replay, decode_covt ----------------------------------------------------
def _batch(covt, n_tiles):
    tiles = [open(p, "rb").read() for p in tile_paths(("omt",))[:n_tiles]]
    plan = covt.Plan.from_tiles(tiles)
    return plan, covt.DeviceBatch(plan, "cuda:0")


def _columns_equal(plan, sres, x, y):
    """The written members of every column in two simplify buffers hold the same bytes."""
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(sres["status"][c]):
            continue
        q = plan.simplify[c]
        o = int(q["off"])
        m = _members(int(q["n_features"]), int(q["part_cap"]), int(q["ring_cap"]), int(q["coord_cap"]))
        for k, nb in ((0, 4 * (int(q["n_features"]) + 1)), (1, 4 * (int(sres["num_parts"][c]) + 1)),
                      (2, 4 * (int(sres["num_rings"][c]) + 1)), (3, 8 * int(sres["num_coords"][c]))):
            assert x[o + m[k]:o + m[k] + nb].tobytes() == y[o + m[k]:o + m[k] + nb].tobytes(), (c, k)
        n_ok += 1
    return n_ok


def _wkb_equal(plan, wres, x, y):
    for c in range(plan.num_geometry_columns):
        if int(wres["status"][c]) == 0:
            a, b = plan.wkb_column(x, wres, c), plan.wkb_column(y, wres, c)
            assert a.offsets.tobytes() == b.offsets.tobytes() and a.data.tobytes() == b.data.tobytes(), c


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_device_paths_match_host_path(covt, gpu_available, n_tiles):
    import torch

    plan, b = _batch(covt, n_tiles)
    per_tile = [(2 + 3 * t) % 9 for t in range(n_tiles)]
    for shift in (FIXTURE_SHIFT, per_tile):
        buf_h, sres_h = plan.simplify_host(shift)
        plan.set_simplify(shift)
        try:
            wkb_h, wres_h = plan.wkb_host()
            bb_h, bres_h = plan.bbox_host()
            ms_h, mres_h = plan.measures_host()
        finally:
            plan.set_simplify(None)
        assert (sres_h["status"] == 0).any() and int(sres_h["num_coords"].sum()) > 0
        for step in (b.decode, b.assemble):
            step()
        b.simplify(shift)
        b.wkb(simplified=True)
        b.bbox(simplified=True)
        b.measures(simplified=True)
        torch.cuda.synchronize()
        buf_d, sres_d = b.simplify_results()
        assert sres_h.tobytes() == sres_d.tobytes()
        assert _columns_equal(plan, sres_h, buf_h, buf_d) > 0
        wkb_d, wres_d = b.wkb_results()
        assert wres_d.tobytes() == wres_h.tobytes()
        _wkb_equal(plan, wres_h, wkb_h, wkb_d)
        bb_d, bres_d = b.bbox_results()
        ms_d, mres_d = b.measures_results()
        assert bres_d.tobytes() == bres_h.tobytes() and mres_d.tobytes() == mres_h.tobytes()
        for c in range(plan.num_geometry_columns):
            if int(bres_h["status"][c]) == 0:
                o, n = int(plan.bbox["off"][c]), int(plan.bbox["n_features"][c])
                assert bb_d[o:o + 32 * n].tobytes() == bb_h[o:o + 32 * n].tobytes(), c
                o = int(plan.measures["off"][c])
                assert ms_d[o:o + 20 * n].tobytes() == ms_h[o:o + 20 * n].tobytes(), c
    # the plain products are what they were
    b.wkb()
    torch.cuda.synchronize()
    wkb_p, wres_p = b.wkb_results()
    wkb_0, wres_0 = plan.wkb_host()
    assert wres_p.tobytes() == wres_0.tobytes()
    _wkb_equal(plan, wres_0, wkb_0, wkb_p)
    # the device plan: the same records and descriptors, the same bytes
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    si, sdd = dp.simplify_copy()
    assert si.tobytes() == plan.simplify.tobytes() and sdd.tobytes() == plan.spdescs.tobytes()
    assert dp.simplify_bytes == plan.simplify_bytes
    n_g = plan.num_geometry_columns
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_sim, d_sgres = dp.alloc_simplify()
    d_wkb, d_wres = dp.alloc_wkb()
    d_sim.fill_(FILL)
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.simplify(d_out, d_asm, d_gres, FIXTURE_SHIFT, d_sim, d_sgres)
    L = covt.lib()
    assert L.covt_geometry_wkb_device(d_out.data_ptr(), dp.simplified_geometry_descs_device(), d_sim.data_ptr(),
                                      d_sgres.data_ptr(), L.covt_device_plan_wkb_descs_device(dp._h), n_g,
                                      d_wkb.data_ptr(), d_wres.data_ptr(),
                                      torch.cuda.current_stream(b.device).cuda_stream) == 0
    torch.cuda.synchronize()
    buf_h, sres_h = plan.simplify_host(FIXTURE_SHIFT)
    sres_p = d_sgres.cpu().numpy().view(covt.GEOM_RESULT_DTYPE)[:n_g][plan.simplify["desc_index"]]
    assert sres_p.tobytes() == sres_h.tobytes()
    assert _columns_equal(plan, sres_h, buf_h, d_sim.cpu().numpy()[:plan.simplify_bytes]) > 0
    plan.set_simplify(FIXTURE_SHIFT)
    try:
        wkb_h, wres_h = plan.wkb_host()
    finally:
        plan.set_simplify(None)
    wres_p = d_wres.cpu().numpy().view(covt.WKB_RESULT_DTYPE)[:n_g][plan.wkb["desc_index"]]
    assert wres_p.tobytes() == wres_h.tobytes()
    _wkb_equal(plan, wres_h, wkb_h, d_wkb.cpu().numpy()[:plan.wkb_bytes])


@pytest.mark.parametrize("n_tiles", [1, 12])
def test_assemble_simplify_wkb_replay_in_a_hip_graph(covt, gpu_available, n_tiles):
    """assemble + simplify + WKB of the simplified column captured in one HIP graph and replayed twice into
    poisoned buffers: the bytes of the eager run each time (no atomics, every element written once; the
    assembly's scratch needs the warm-up launch on the capture stream before the capture)."""
    import torch

    plan, b = _batch(covt, n_tiles)
    s = torch.cuda.Stream(b.device)

    def launch():
        b.assemble(s)
        b.simplify(FIXTURE_SHIFT, s)
        b.wkb(s, simplified=True)

    with torch.cuda.stream(s):
        b.decode(s)
        launch()
    torch.cuda.synchronize()
    buf_e, sres_e = b.simplify_results()
    wkb_e, wres_e = b.wkb_results()
    buf_e, wkb_e = buf_e.copy(), wkb_e.copy()
    assert (sres_e["status"] == 0).any() and int(sres_e["num_coords"].sum()) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for _ in range(2):
        b.d_simplify.fill_(FILL)
        b.d_sgres.fill_(0x5A5A5A5A)
        b.d_asm.fill_(FILL)
        b.d_wkb.fill_(FILL)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        buf, sres = b.simplify_results()
        wkb, wres = b.wkb_results()
        assert sres.tobytes() == sres_e.tobytes() and wres.tobytes() == wres_e.tobytes()
        assert _columns_equal(plan, sres_e, buf_e, buf) == int((sres_e["status"] == 0).sum())
        _wkb_equal(plan, wres_e, wkb_e, wkb)
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_decode_covt_simplify(covt, gpu_available, decodable_tiles, n_tiles):
    """decode_covt(simplify=4): every layer's simplified column is the reference over its plain geometry, and its
    wkb, bbox and measures are those of the simplified column; without the argument simplified is None."""
    removed = 0
    for ti, (_, tile) in enumerate(decodable_tiles[:n_tiles]):
        layers = covt.CovtParser.decode_covt(tile, simplify=FIXTURE_SHIFT)
        plan = covt.Plan.from_tiles([tile])
        asm, gres = plan.assemble_host()
        plain = covt.CovtParser.decode_covt(tile) if ti == 0 else None
        if plain is not None:
            assert len(plain) == len(layers) and all(lc.simplified is None for lc in plain)
        by_layer = {int(plan.geom["layer"][c]): c for c in range(plan.num_geometry_columns)}
        for lc in layers:
            if lc.wkb is None:
                continue
            c = by_layer[lc.layer]
            g = plan.geometry_arrays(asm, gres, c)
            types = np.asarray(lc.geometry.geometryTypes, np.uint8)
            ring, xy = S.simplify_ref(types, g.geometry_offsets, g.part_offsets, g.ring_offsets, g.coords, FIXTURE_SHIFT)
            assert lc.simplified.ring_offsets.tobytes() == ring.tobytes() and lc.simplified.coords.tobytes() == xy.tobytes()
            col = (types, g.geometry_offsets, g.part_offsets, ring, xy)
            offs, data = W.write_numpy(*col)
            assert lc.wkb.offsets.tobytes() == np.asarray(offs, np.int32).tobytes() and lc.wkb.data.tobytes() == data.tobytes()
            b = lc.bbox
            assert B.same((b.xmin, b.ymin, b.xmax, b.ymax, b.extent, b.n_empty), B.bbox_numpy(*col[1:]))
            assert lc.measures.num_coords.tobytes() == M.measures_numpy(*col)[2].tobytes()
            removed += g.coords.shape[0] - xy.shape[0]
        plan.close()
    assert removed > 0

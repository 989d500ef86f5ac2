"""GPU: the query pass (covt_query.hip, include/covt.h "Geometry queries") against query_ref of
tests/covt_query.py over the CPU oracle's assembly, byte for byte, and on valid inputs against query_clip_ref
too: covt_select_query_device on hand-made and synthetic columns, Plan.select_host(..., query=) on the fixture
tiles, the DeviceBatch / DevicePlan paths, a HIP-graph replay and decode_covt(query=).  Every select buffer
starts as a fill pattern with the incoming masks (0 / 1 / 0x80 / 0xFF at random) written in; after each call the
inputs are unchanged and every byte outside the mask members and the first ring_cap bytes of each `bytes`
member (the pass's scratch) still holds the fill.

The kernel's step sizes the cases sit around: a row of 128 coordinates, a workgroup of 4 waves, up to 64
workgroups per column while 8192 / n_columns allows (a batch of 4,097 columns gives each one workgroup, so a
column of 40 rows gives wave 0 the run [0, 1280)), a ring with 2,048 coordinates or more left past its owner's
run finished by the whole workgroup, a feature of 64 rings or more finished by its whole wave.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_query as Q
import covt_select as S
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
CHUNK, WIDE = 128, 2048
W10 = Q.W10
MODES = ((0, 0), (0, 1), (1, 0), (1, 1))  # (relation, mode): INTERSECTS / WITHIN x WRITE / AND


# ---- the harness ------------------------------------------------------------------------------------------
def _select_layout(covt, cols):
    """Select descriptors (the plan's layout rule, byte_cap the WKB capacity) for pack_columns' columns, a gap
    of 16 bytes after every slice -> (desc array, bytes)."""
    d = np.zeros(len(cols), dtype=covt.SELECT_DESC_DTYPE)
    off = 0
    for ci, col in enumerate(cols):
        n = col["types"].size
        pcap, rcap, ccap = col.get("caps") or A.caps(col)
        d[ci]["off"], d[ci]["n_features"] = off, n
        d[ci]["byte_cap"] = 9 * (n + pcap) + 4 * rcap + 16 * ccap
        off = S.a16(off + S.member_offsets(n)[3] + int(d[ci]["byte_cap"])) + 16
    return d, max(off, 16)


class _Run:
    """covt_assemble_geometry_device once, then covt_select_query_device per query over fresh select buffers."""

    def __init__(self, covt, cols, flags_extra=None, in_res=None, dres=None, tweak=None, seed=1):
        import torch

        self.covt, self.cols = covt, cols
        dec, desc, asm_bytes, _ = A.pack_columns(covt, cols, flags_extra, in_res)
        self.sd, sel_bytes = _select_layout(covt, cols)
        self.rcap = [(c.get("caps") or A.caps(c))[1] for c in cols]
        if tweak:
            tweak(self.sd)
        rng = np.random.default_rng(seed)
        self.base = np.full(sel_bytes, FILL, np.uint8)
        self.mask_in = []
        for ci in range(len(cols)):
            o, n = int(self.sd["off"][ci]), int(self.sd["n_features"][ci])
            m = rng.choice(np.array([0, 1, 0x80, 0xFF], np.uint8), max(n, 0))
            self.base[o:o + n] = m
            self.mask_in.append(m)
        dev = torch.device("cuda:0")
        self.d_dec = torch.from_numpy(dec).to(dev)
        self.d_desc = torch.from_numpy(desc).to(dev)
        self.d_sdesc = torch.from_numpy(self.sd.view(np.uint8).reshape(-1).copy()).to(dev)
        self.d_asm = torch.full((asm_bytes,), FILL, dtype=torch.uint8, device=dev)
        self.d_gres = torch.zeros(4 * len(cols), dtype=torch.int32, device=dev)
        d_res = torch.from_numpy(np.zeros(2, np.int32) if dres is None else np.asarray(dres, np.int32)).to(dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.dev = dev
        L = covt.lib()
        assert L.covt_assemble_geometry_device(self.d_dec.data_ptr(), d_res.data_ptr(), self.d_desc.data_ptr(), len(cols),
                                               self.d_asm.data_ptr(), self.d_gres.data_ptr(), self.stream) == 0
        torch.cuda.synchronize()
        self.inputs = [t.cpu().numpy().copy() for t in (self.d_dec, self.d_desc, self.d_sdesc, self.d_asm, self.d_gres)]
        self.gres = self.inputs[4].view(covt.GEOM_RESULT_DTYPE)

    def query(self, window, relation, mode, with_status=True):
        """-> (the select buffer after the call, the statuses or None)"""
        import torch

        covt = self.covt
        q = covt.SelectQuery(window, relation)
        d_sel = torch.from_numpy(self.base).to(self.dev)
        d_st = torch.full((max(len(self.cols), 1),), 77, dtype=torch.int32, device=self.dev)
        assert covt.lib().covt_select_query_device(
            self.d_dec.data_ptr(), self.d_desc.data_ptr(), self.d_asm.data_ptr(), self.d_gres.data_ptr(),
            self.d_sdesc.data_ptr(), len(self.cols), C_byref(q), mode, d_sel.data_ptr(),
            d_st.data_ptr() if with_status else None, self.stream) == 0
        torch.cuda.synchronize()
        for t, before in zip((self.d_dec, self.d_desc, self.d_sdesc, self.d_asm, self.d_gres), self.inputs):
            assert t.cpu().numpy().tobytes() == before.tobytes()  # the inputs are unchanged
        return d_sel.cpu().numpy(), d_st.cpu().numpy()[:len(self.cols)] if with_status else None


def C_byref(x):
    import ctypes

    return ctypes.byref(x)


def _reference(oracle, col, window, cache, valid):
    """(INTERSECTS, WITHIN) of query_ref over the oracle's assembly of the column, cached per column object and
    window; a column built valid is held against query_clip_ref first."""
    key = (id(col), tuple(window))
    if key not in cache:
        akey = (id(col), "asm")
        if akey not in cache:  # (the entry holds the column, so its id stays its own while the cache lives)
            cache[akey] = (col, oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"],
                                                         col["vb"], col["closed"], col.get("caps") or A.caps(col)))
        o = cache[akey][1]
        assert o[0] == 0
        ref = Q.query_ref(col["types"], *o[1:], window)
        if valid:
            clip = Q.query_clip_ref(col["types"], *o[1:], window)
            assert ref[0].tolist() == clip[0].tolist() and ref[1].tolist() == clip[1].tolist()
        cache[key] = ref
    return cache[key]


def _check_untouched(run, buf, failed=()):
    """Every byte outside the mask members and the scratch (a failed column: its whole slice but the mask)
    equals what the buffer held before the call."""
    same = np.ones(buf.size, dtype=bool)
    for ci in range(len(run.cols)):
        o, n = int(run.sd["off"][ci]), int(run.sd["n_features"][ci])
        same[o:o + max(n, 0)] = False
        if ci not in failed:
            b = o + S.member_offsets(n)[3]
            same[b:b + run.rcap[ci]] = False
    assert (buf[same] == run.base[same]).all()


def _verify(covt, oracle, cols, windows, cache, valid=False, seed=1):
    """Every (relation, mode) of every window over the batch, every column against the reference.  Returns the
    WRITE-mode masks: {(window, relation): [mask per column]}."""
    run = _Run(covt, cols, seed=seed)
    assert (run.gres["status"] == 0).all()
    out = {}
    for w in windows:
        for relation, mode in MODES:
            buf, st = run.query(w, relation, mode)
            assert (st == 0).all()
            _check_untouched(run, buf)
            masks = []
            for ci, col in enumerate(cols):
                o, n = int(run.sd["off"][ci]), col["types"].size
                want = _reference(oracle, col, w, cache, valid)[relation]
                if mode == 1:
                    want = want & (run.mask_in[ci] != 0)
                got = buf[o:o + n]
                assert got.tobytes() == want.astype(np.uint8).tobytes(), \
                    (ci, w, relation, mode, np.nonzero(got != want)[0][:8].tolist())
                masks.append(got.copy())
            if mode == 0:
                out[(tuple(w), relation)] = masks
    return out


def _pad_to_one_workgroup(cols):
    """The same columns in a batch of 4,097: one workgroup per column."""
    tiny = Q.source_column([Q.point(3, 3), Q.line([(20, 20), (30, 30)])])
    return cols + [tiny] * (4097 - len(cols))


# ---- paths that are out of the window, or in it, but for chosen coordinates -----------------------------------
def _far(k, i0=0):
    """k coordinates far from W10 whose edges stay far from it."""
    return [(1000 + (i0 + i) % 50, 1000 + ((i0 + i) * 7) % 50) for i in range(k)]


def _inside(k):
    """k coordinates inside W10."""
    return [(i % 11, (i * 3) % 11) for i in range(k)]


def _ring_variants(k):
    """Lines of k coordinates whose answers hang on one coordinate or edge: far; far but the last coordinate
    (the last edge is the only hit); far but the first; inside; inside but the last; inside but the first."""
    out = [_far(k)]
    if k >= 1:
        out += [_far(k - 1) + [(5, 5)], [(5, 5)] + _far(k - 1), _inside(k), _inside(k - 1) + [(50, 50)],
                [(50, 50)] + _inside(k - 1)]
    return out


def _column_with_ring(before, ring, total=None):
    """A LINESTRING column: a filler line of `before` far coordinates, the ring, then far lines of 7 up to
    `total` coordinates."""
    lines = ([_far(before)] if before else []) + [ring]
    if total is not None:
        rest = total - before - len(ring)
        lines += [_far(7, 3)] * (rest // 7) + ([_far(rest % 7)] if rest % 7 else [])
    return Q.source_column([Q.line(l) for l in lines])


# ---- known answers ------------------------------------------------------------------------------------------
def test_known_answers_as_columns(covt, oracle, gpu_available):
    cache = {}
    for w in sorted({k[1] for k in Q.KNOWN}):
        same = [k for k in Q.KNOWN if k[1] == w]
        col = Q.source_column([k[2] for k in same])
        masks = _verify(covt, oracle, [col], [w], cache, valid=True)
        assert masks[(w, 0)][0].tolist() == [k[3] for k in same]
        assert masks[(w, 1)][0].tolist() == [k[4] for k in same]


def test_feature_counts(covt, oracle, gpu_available):
    """0, 1, 63, 64, 65 and 4,097 valid features of every type, coordinates in +-12 so that touching is
    frequent, against a box, a point and an inverted window."""
    rng = np.random.default_rng(41)
    cols = [Q.source_column([Q.valid_feature(rng) for _ in range(n)]) for n in (0, 1, 63, 64, 65, 4097)]
    masks = _verify(covt, oracle, cols, [(-3, -2, 4, 5), (2, 2, 2, 2), (4, 4, -4, -4)], {}, valid=True)
    big = masks[((-3, -2, 4, 5), 0)][5]
    assert 400 < int(big.sum()) < 3700 and int(masks[((-3, -2, 4, 5), 1)][5].sum()) > 10
    assert not masks[((4, 4, -4, -4), 0)][5].any()


def test_synthetic_columns(covt, oracle, gpu_available):
    """The synthetic column builder: every geometry type, empty parts and rings, shared vertices, coordinates
    over the whole int32 range, against windows of that size."""
    rng = np.random.default_rng(42)
    cols = [A.synth_column(rng, [0, 1, 5, 63, 64, 65, 200, 300][i % 8], ice=bool(i & 1), closed=bool(i & 2))
            for i in range(16)]
    q = 1 << 30
    masks = _verify(covt, oracle, cols, [(-q, -q, q, q), (-(1 << 31), 0, (1 << 31) - 1, (1 << 31) - 1)], {})
    assert 0 < sum(int(m.sum()) for m in masks[((-q, -q, q, q), 0)]) < sum(c["types"].size for c in cols)


# ---- step boundaries ----------------------------------------------------------------------------------------
def test_rings_ending_around_row_edges(covt, oracle, gpu_available):
    """Rings that end exactly at, one before and one after a row edge (128 coordinates), starting at the row's
    first coordinate or inside it, whose answers hang on their first or last coordinate; with up to 64
    workgroups per column and with one."""
    cols = []
    for end in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        for before in (0, 5):
            for ring in _ring_variants(end - before):
                cols.append(_column_with_ring(before, ring, total=end + 20))
    cache = {}
    _verify(covt, oracle, cols, [W10], cache)
    _verify(covt, oracle, _pad_to_one_workgroup(cols), [W10], cache)


def test_rings_ending_around_a_waves_run_edge(covt, oracle, gpu_available):
    """A column of 40 rows in a batch of one workgroup per column gives wave 0 the run [0, 1280): its second
    ring starts at coordinate 10 and ends one before, at and one after the run's edge (the wave finishes it),
    or 2,047, 2,048 and 2,049 coordinates past it (the wave / the whole workgroup does: a ring longer than
    2,048 whose only hit is its last edge); the same columns cut by 64 workgroups."""
    total = 40 * CHUNK
    cols = []
    for d in (-1, 0, 1):
        for ring in _ring_variants(10 * CHUNK - 10 + d):
            cols.append(_column_with_ring(10, ring, total))
    for r in (WIDE - 1, WIDE, WIDE + 1):
        k = 10 * CHUNK - 10 + r
        for ring in (_far(k - 1) + [(5, 5)], _inside(k - 1) + [(50, 50)], _inside(k)):
            cols.append(_column_with_ring(10, ring, total))
    cache = {}
    for batch in (_pad_to_one_workgroup(cols), cols):
        masks = _verify(covt, oracle, batch, [W10], cache)
        for ci in range(18, 27, 3):  # the long rings: hit by the last edge alone, out by the last coordinate alone
            assert masks[(W10, 0)][ci][1] == 1 and masks[(W10, 1)][ci + 1][1] == 0 and masks[(W10, 1)][ci + 2][1] == 1


def _flip_ring(crossings):
    """A closed ring of (crossings + 2) * 128 coordinates around Q = (0, 0): each of its first `crossings` rows
    crosses the ray from Q once, far to the right, then a row runs back below the ray to x < 0 and the last one
    climbs there (no crossing of the ray) and runs back above it to the start.  No edge comes near (0, 0, 1, 1)."""
    pts, side, x = [], 1, 100
    for _ in range(crossings):
        for i in range(CHUNK):
            if i == 64:
                side = -side
            pts.append((x, 5 * side))
            x += 1
    pts += [(x - 7 * (i + 1), 5 * side) for i in range(CHUNK)]
    x0 = pts[-1][0]
    pts += [(x0 + 2 * i, 5) for i in range(CHUNK - 1)] + [pts[0]]
    assert len(pts) == (crossings + 2) * CHUNK and x0 < -10
    return pts


def test_crossing_parity_carried_over_rows(covt, oracle, gpu_available):
    """A polygon ring carried over seven and eight rows whose crossing parity flips in every row: the window
    (0, 0, 1, 1) lies inside the one (five crossings) and outside the other (six, and the return below the ray
    crosses it once more at the left... of Q, so not at all), no edge touching it."""
    first = _far(CHUNK - 1) + [_far(1)[0]]  # a closed far ring of one row: the long ring starts at a row edge
    cols = [Q.source_column([Q.polygon([first]), Q.polygon([_flip_ring(k)]), Q.line(_flip_ring(k))]) for k in (5, 6, 1, 2)]
    cache = {}
    w = (0, 0, 1, 1)
    for batch in (cols, _pad_to_one_workgroup(cols)):
        masks = _verify(covt, oracle, batch, [w], cache)
        assert [masks[(w, 0)][ci].tolist() for ci in range(4)] == [[0, 1, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]]


def test_features_of_many_rings(covt, oracle, gpu_available):
    """Features of 63, 64 and 65 rings whose only touching ring (or only ring with a coordinate outside) is the
    last; 64 and 65 nested rings around the window (even-odd: outside, inside); a multipoint of 200 points with
    only the last one inside, and one with only the last one outside."""
    feats = []
    for k in (63, 64, 65, 130):
        feats.append(Q.multiline([_far(3, i) for i in range(k - 1)] + [[(50, 5), (5, 5)]]))
        feats.append(Q.multiline([_far(3, i) for i in range(k)]))
        feats.append(Q.multiline([_inside(3) for _ in range(k - 1)] + [[(5, 5), (5, 11)]]))
        feats.append(Q.multiline([_inside(3) for _ in range(k)]))
        feats.append(Q.polygon([Q.box(-5 - i, -5 - i, 20 + 2 * i, 20 + 2 * i, cw=bool(i & 1)) for i in range(k)]))
        feats.append(Q.multipolygon([[Q.box(-5 - i, -5 - i, 20 + 2 * i, 20 + 2 * i)] for i in range(k)]))
    feats.append(Q.multipoint(_far(199) + [(5, 5)]))
    feats.append(Q.multipoint(_inside(199) + [(11, 5)]))
    feats.append(Q.multipoint(_inside(200)))
    feats.append(Q.multipoint(_far(200)))
    col = Q.source_column(feats)
    want_i = [1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0] + [1, 1, 1, 0]
    want_w = [0, 0, 0, 1, 0, 0] * 4 + [0, 0, 1, 0]
    cache = {}
    for batch in ([col], _pad_to_one_workgroup([col])):
        masks = _verify(covt, oracle, batch, [W10], cache)
        assert masks[(W10, 0)][0].tolist() == want_i and masks[(W10, 1)][0].tolist() == want_w


def test_empty_rings_and_parts_between_others(covt, oracle, gpu_available):
    big, hole = Q.box(-5, -5, 20, 20), Q.box(-2, -2, 14, 14, cw=True)
    feats = [Q.multiline([[], _far(3), [], [(50, 5), (5, 5)], []]), Q.multiline([[], [], _far(2), []]),
             Q.multiline([[], _inside(4), [], _inside(2)]), Q.multipolygon([[], [big], []]),
             Q.multipolygon([[], [big, [], hole], [], [Q.box(100, 100, 5, 5)]]), Q.polygon([[], big, []]),
             Q.polygon([big, [], hole, []]), Q.multipolygon([[], []]), Q.multipoint([]), Q.line([]),
             Q.multipolygon([[[]], [Q.box(1, 1, 2, 2), []]])]
    col = Q.source_column(feats)
    masks = _verify(covt, oracle, [col] * 3, [W10], {})
    assert masks[(W10, 0)][0].tolist() == [1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1]
    assert masks[(W10, 1)][0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]


def test_one_column_alone_and_among_200(covt, oracle, gpu_available):
    """The same column with 64 workgroups to itself and with 40 among 200 columns: identical masks."""
    rng = np.random.default_rng(43)
    col = Q.source_column([Q.valid_feature(rng, lim=40) for _ in range(1500)])
    others = [A.synth_column(rng, int(rng.integers(0, 40)), bool(i & 1), bool(i & 2)) for i in range(199)]
    cache = {}
    windows = [(-9, -9, 12, 7), (3, -4, 3, -4)]
    alone = _verify(covt, oracle, [col], windows, cache, valid=True)
    among = _verify(covt, oracle, others[:77] + [col] + others[77:], windows, cache)
    for key in alone:
        assert alone[key][0].tobytes() == among[key][77].tobytes()
    assert 100 < int(alone[(windows[0], 0)][0].sum()) < 1400


def test_extreme_coordinates_across_row_edges(covt, oracle, gpu_available):
    """Rings of INT32_MIN / INT32_MAX coordinates of lengths that put their edges across the row edges, against
    windows with corners from the same set: 33-bit differences and 66-bit products on the device."""
    rng = np.random.default_rng(44)
    pt = lambda: (int(rng.choice(Q.EXTREMES)), int(rng.choice(Q.EXTREMES)))  # noqa: E731

    def ring(k):
        p = [pt() for _ in range(k - 1)]
        return p + p[:1]

    feats = [Q.polygon([ring(int(rng.integers(4, 40)))]) for _ in range(60)]
    feats += [Q.line([pt() for _ in range(k)]) for k in (CHUNK - 1, CHUNK + 1, 2, 3 * CHUNK, 2)]
    feats += [Q.polygon([ring(k)]) for k in (CHUNK, CHUNK + 1, 300)] + [Q.point(*pt()) for _ in range(40)]
    feats += [Q.line([(Q.LO, Q.LO), (Q.HI, Q.HI)]), Q.line([(Q.LO, Q.HI), (Q.HI, Q.LO)]),
              Q.polygon([Q.box(Q.LO, Q.LO, Q.HI - Q.LO, Q.HI - Q.LO)])]
    col = Q.source_column(feats)
    windows = [tuple(int(rng.choice(Q.EXTREMES)) for _ in range(4)) for _ in range(5)]
    windows += [(Q.LO, Q.LO, Q.HI, Q.HI), (Q.HI, Q.HI, Q.HI, Q.HI), (Q.LO, Q.LO, Q.LO, Q.LO), (-1, -1, 1, 1), (0, 0, 0, 0)]
    cache = {}
    masks = _verify(covt, oracle, [col], windows, cache, valid=True)  # (one ring each: both references apply)
    _verify(covt, oracle, _pad_to_one_workgroup([col]), windows[:3], cache)
    assert masks[((Q.LO, Q.LO, Q.HI, Q.HI), 1)][0].all() and masks[((0, 0, 0, 0), 0)][0][-3:].tolist() == [1, 0, 1]  # (x + y = -1 misses it)


# ---- statuses -----------------------------------------------------------------------------------------------
def test_status_paths(covt, oracle, gpu_available):
    """A failed assembly (a source stream's status; COVT_GEOM_TOO_LARGE), a select descriptor flagged too large,
    misaligned, planned for another feature count, or with byte_cap < ring_cap: a zero mask in both modes, the
    status in d_status, and the rest of the slice, the scratch included, untouched; d_status may be null."""
    rng = np.random.default_rng(45)
    ok = Q.source_column([Q.valid_feature(rng) for _ in range(50)])
    cols = [ok] * 8
    rcap = A.caps(ok)[1]

    def tweak(sd):
        sd["flags"][3] = covt.SELECT_TOO_LARGE
        sd["off"][4] += 8
        sd["n_features"][5] -= 1
        sd["byte_cap"][6] = rcap - 1

    run = _Run(covt, cols, flags_extra=[0, 0, 0x80000000, 0, 0, 0, 0, 0],
               in_res=[[-1] * 6, [0, -1, -1, -1, -1, 1]] + [[-1] * 6] * 6, dres=[0, 5, covt.ERR_TRUNCATED, 7], tweak=tweak)
    I = covt.ERR_INVALID_ARG
    assert run.gres["status"].tolist() == [0, covt.ERR_TRUNCATED, I, 0, 0, 0, 0, 0]
    cache = {}
    w = (-3, -2, 4, 5)
    for relation, mode in MODES:
        for with_status in (True, False):
            buf, st = run.query(w, relation, mode, with_status)
            if with_status:
                assert st.tolist() == [0, covt.ERR_TRUNCATED, I, I, I, I, I, 0]
            _check_untouched(run, buf, failed=range(1, 7))
            for ci in range(8):
                o, n = int(run.sd["off"][ci]), int(run.sd["n_features"][ci])
                if 1 <= ci <= 6:
                    assert not buf[o:o + n].any(), ci
                    continue
                want = _reference(oracle, ok, w, cache, True)[relation]
                if mode == 1:
                    want = want & (run.mask_in[ci] != 0)
                assert buf[o:o + n].tobytes() == want.astype(np.uint8).tobytes(), ci


# ---- fixture tiles ------------------------------------------------------------------------------------------
class _Tiles:
    """Every fixture tile in one plan (made with properties, for the combined case), the oracle's assembly of
    every column and the plan's own WKB and boxes, computed once."""

    def __init__(self, covt, oracle):
        from test_gpu_where import _Fixtures

        self.fx = _Fixtures(covt)
        self.plan = self.fx.plan
        self.paths = tile_paths()
        tiles = [open(p, "rb").read() for p in self.paths]
        by_tile = {}
        self.cols = []
        for c in range(self.plan.num_geometry_columns):
            t, L = int(self.plan.geom["tile"][c]), int(self.plan.geom["layer"][c])
            if t not in by_tile:
                by_tile[t] = A.oracle_tile_columns(oracle, tiles[t])
            self.cols.append(by_tile[t][L])
        self._ref = {}

    def ref(self, c, window):
        """query_ref over the oracle's assembly of column c (None: a source stream failed to decode)."""
        key = (c, tuple(window))
        if key not in self._ref:
            oc = self.cols[c]
            self._ref[key] = None if oc["asm"] is None or oc["asm"][0] else \
                Q.query_ref_numpy(oc["types"], *oc["asm"][1:], window)
        return self._ref[key]


@pytest.fixture(scope="module")
def tiles(covt, oracle, gpu_available):
    return _Tiles(covt, oracle)


WINDOWS = {"window": (0, 0, 2048, 2048), "point": (2040, 2040, 2056, 2056), "inverted": (2048, 2048, 0, 0)}


@pytest.mark.parametrize("name", list(WINDOWS))
@pytest.mark.parametrize("relation", ["intersects", "within"])
def test_fixture_tiles_select_query_host(covt, tiles, name, relation):
    """Plan.select_host(None, query=...) on every fixture tile: the mask is query_ref over the oracle's
    assembly, n_selected its count; against the plan's own boxes WITHIN is "the box lies inside W" and
    INTERSECTS implies "the box meets W"."""
    plan = tiles.plan
    w = WINDOWS[name]
    q = covt.SelectQuery(w, relation) if name != "point" else covt.SelectQuery.at(2048, 2048, 8, relation)
    assert tuple(q.window) == w
    (wbuf, wres), (bbuf, bres) = tiles.fx.products(covt.CRS_TILE)
    sbuf, sres = plan.select_host(None, query=q)
    assert np.array_equal(sres["status"], wres["status"])
    n_ok = kept = total = 0
    for c in range(plan.num_geometry_columns):
        ref = tiles.ref(c, w)
        if ref is None:
            assert int(sres["status"][c]) != 0 and int(plan.query_status[c]) != 0
            continue
        assert int(sres["status"][c]) == 0 and int(plan.query_status[c]) == 0, c
        o, n = int(plan.select["off"][c]), int(plan.select["n_features"][c])
        want = ref[0 if relation == "intersects" else 1]
        mask = sbuf[o:o + n]
        assert mask.tobytes() == want.tobytes(), (tile_key(tiles.paths[int(plan.geom["tile"][c])]), c,
                                                  np.nonzero(mask != want)[0][:5].tolist())
        assert int(sres["n_selected"][c]) == int(want.sum())
        b = plan.bbox_column(bbuf, bres, c)
        with np.errstate(invalid="ignore"):
            inside = (b.xmin >= w[0]) & (b.xmax <= w[2]) & (b.ymin >= w[1]) & (b.ymax <= w[3])
            meets = (b.xmin <= w[2]) & (b.xmax >= w[0]) & (b.ymin <= w[3]) & (b.ymax >= w[1])
        if relation == "within":
            assert np.array_equal(mask != 0, inside), c
        else:
            assert not (mask != 0)[~meets].any(), c
        n_ok += 1
        kept += int(want.sum())
        total += n
    assert n_ok >= 700
    assert kept == 0 if name == "inverted" else 0 < kept < total


def test_fixture_tiles_query_finer_than_the_boxes(covt, tiles):
    """What the pass is for: over the fixture tiles some feature's box meets the window while the feature does
    not, so the exact mask is a strict subset of the box prefilter's."""
    plan = tiles.plan
    w = WINDOWS["point"]
    (_, _), (bbuf, bres) = tiles.fx.products(covt.CRS_TILE)
    finer = 0
    for c in range(plan.num_geometry_columns):
        ref = tiles.ref(c, w)
        if ref is None:
            continue
        b = plan.bbox_column(bbuf, bres, c)
        with np.errstate(invalid="ignore"):
            meets = (b.xmin <= w[2]) & (b.xmax >= w[0]) & (b.ymin <= w[3]) & (b.ymax >= w[1])
        finer += int((meets & (ref[0] == 0)).sum())
    assert finer > 0


def test_query_of_the_simplified_column(covt, oracle, gpu_available):
    """With set_simplify(4) the query reads the simplified column: the mask is query_ref over the arrays
    simplify_host returns."""
    paths = tile_paths(("omt",))[:12]
    tile_bytes = [open(p, "rb").read() for p in paths]
    plan = covt.Plan.from_tiles(tile_bytes)
    plan.set_simplify(4)
    zbuf, zres = plan.simplify_host(4)
    w = (512, 512, 3000, 2500)
    n_ok = differs = 0
    plain = covt.Plan.from_tiles(tile_bytes)
    pbuf, pres = plain.select_host(None, query=covt.SelectQuery(w))
    for relation in ("intersects", "within"):
        sbuf, sres = plan.select_host(None, query=covt.SelectQuery(w, relation))
        for c in range(plan.num_geometry_columns):
            if int(zres["status"][c]):
                assert int(sres["status"][c]) != 0
                continue
            t, L = int(plan.geom["tile"][c]), int(plan.geom["layer"][c])
            types = A.oracle_tile_columns(oracle, tile_bytes[t])[L]["types"] if relation == "intersects" else None
            if types is None:
                continue
            g = plan.simplified_arrays(zbuf, zres, c)
            ref = Q.query_ref_numpy(types, g.geometry_offsets, g.part_offsets, g.ring_offsets, g.coords, w)
            o, n = int(plan.select["off"][c]), int(plan.select["n_features"][c])
            assert sbuf[o:o + n].tobytes() == ref[0].tobytes(), c
            differs += int((sbuf[o:o + n] != pbuf[o:o + n]).sum())
            n_ok += 1
    assert n_ok >= 50 and differs > 0  # (and the simplified column is another column)


def test_query_with_a_predicate_and_a_where(covt, tiles):
    """select_host(pred, where=, query=): the kept set is the AND of the three references, and sel / offsets /
    bytes are select_ref over the plan's own WKB column."""
    from test_gpu_where import PREDICATES  # noqa: F401  (the names where_masks knows)

    plan, fx = tiles.plan, tiles.fx
    (wbuf, wres), (bbuf, bres) = fx.products(covt.CRS_TILE)
    mbuf, mres = fx.measures
    pred = covt.SelectPred(window=(0.0, 0.0, 3072.0, 3072.0), min_area=4.0, min_length=8.0)
    where, wref = fx.where_masks("class_ne")
    w = (600, 600, 3000, 2800)
    sbuf, sres = plan.select_host(pred, where=where, query=covt.SelectQuery(w))
    n_ok = kept = dropped_by_query = 0
    for c in range(plan.num_geometry_columns):
        ref = tiles.ref(c, w)
        if int(sres["status"][c]):
            continue
        assert ref is not None and int(plan.query_status[c]) == 0
        o, n = int(plan.select["off"][c]), int(plan.select["n_features"][c])
        assert int(plan.where_status[c]) == wref[c][1]
        both = wref[c][0].copy()
        if int(bres["status"][c]) == 0 and int(mres["status"][c]) == 0:
            b, m = plan.bbox_column(bbuf, bres, c), plan.measures_column(mbuf, mres, c)
            both &= S.predicate_ref(b.xmin, b.ymin, b.xmax, b.ymax, m.area, m.length, pred)
        else:
            both[:] = 0
        want = both & ref[0]
        mask = sbuf[o:o + n]
        assert mask.tobytes() == want.tobytes(), c
        wk = plan.wkb_column(wbuf, wres, c)
        sel, offs, data = S.select_ref(wk.offsets, wk.data, mask)
        col = plan.select_column(sbuf, sres, c)
        assert col.index.tobytes() == sel.tobytes() and col.wkb.offsets.tobytes() == offs.tobytes()
        assert col.wkb.data.tobytes() == data.tobytes()
        n_ok += 1
        kept += int(want.sum())
        dropped_by_query += int((both & ~ref[0] & 1).sum())
    assert n_ok >= 700 and kept > 0 and dropped_by_query > 0


# ---- DeviceBatch / DevicePlan, graph replay, decode_covt ----------------------------------------------------
def _columns_equal(plan, sres, x, y):
    """The written members of every column in two select buffers hold the same bytes."""
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(sres["status"][c]):
            continue
        o, n, k = int(plan.select["off"][c]), int(plan.select["n_features"][c]), int(sres["n_selected"][c])
        m_mask, m_sel, m_off, m_bytes = S.member_offsets(n)
        for a, b in ((0, n), (m_sel, m_sel + 4 * k), (m_off, m_off + 4 * (k + 1)),
                     (m_bytes, m_bytes + int(sres["n_bytes"][c]))):
            assert x[o + a:o + b].tobytes() == y[o + a:o + b].tobytes(), (c, a)
        n_ok += 1
    return n_ok


QUERY = (700, 300, 3300, 2900)


@pytest.mark.parametrize("n_tiles", [1, 12])
def test_device_paths_match_host_path(covt, gpu_available, n_tiles):
    """DeviceBatch: decode -> assemble -> wkb -> select_query -> select equals the host path, alone (WRITE) and
    after select_predicate (AND); the same through DevicePlan."""
    import torch

    tile_bytes = [open(p, "rb").read() for p in tile_paths(("omt",))[:n_tiles]]
    plan = covt.Plan.from_tiles(tile_bytes)
    q = covt.SelectQuery(QUERY)
    buf_h, sres_h = plan.select_host(None, query=q)
    qst_h = plan.query_status.copy()
    assert (sres_h["status"] == 0).any() and 0 < int(sres_h["n_selected"].sum()) < int(plan.select["n_features"].sum())
    b = covt.DeviceBatch(plan, "cuda:0")
    for step in (b.decode, b.assemble, b.wkb):
        step()
    b.select_query(q)
    b.select()
    torch.cuda.synchronize()
    buf_d, sres_d = b.select_results()
    assert sres_h.tobytes() == sres_d.tobytes() and np.array_equal(b.query_status(), qst_h)
    assert _columns_equal(plan, sres_h, buf_h, buf_d) > 0
    # AND mode after the geometric predicate
    pred = covt.SelectPred(window=(0.0, 0.0, 3072.0, 3072.0), min_area=4.0, min_length=8.0)
    buf_a, sres_a = plan.select_host(pred, query=covt.SelectQuery(QUERY, "within"))
    b.bbox()
    b.measures()
    b.select_predicate(pred)
    b.select_query(covt.SelectQuery(QUERY, "within"), covt.WHERE_AND)
    b.select()
    torch.cuda.synchronize()
    buf_d, sres_d = b.select_results()
    assert sres_a.tobytes() == sres_d.tobytes() and _columns_equal(plan, sres_a, buf_a, buf_d) > 0
    # the device plan
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_wkb, d_wres = dp.alloc_wkb()
    d_sel, d_sres = dp.alloc_select()
    d_sel.fill_(FILL)
    d_st = torch.full((max(plan.num_geometry_columns, 1),), 77, dtype=torch.int32, device=b.device)
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.wkb(d_out, d_res, d_asm, d_gres, d_wkb, d_wres)
    dp.select_query(d_out, d_asm, d_gres, q, d_sel, covt.WHERE_WRITE, d_st)
    dp.select(d_wkb, d_wres, d_sel, d_sres)
    torch.cuda.synchronize()
    sres_p = d_sres.cpu().numpy().view(covt.SELECT_RESULT_DTYPE)[:plan.num_geometry_columns][plan.select["desc_index"]]
    assert sres_p.tobytes() == sres_h.tobytes()
    assert _columns_equal(plan, sres_h, buf_h, d_sel.cpu().numpy()[:plan.select_bytes]) > 0
    assert np.array_equal(d_st.cpu().numpy()[:plan.num_geometry_columns][plan.select["desc_index"]], qst_h)


def test_query_and_select_replay_in_a_hip_graph(covt, gpu_available):
    """query + select captured in one HIP graph and replayed twice on its capture stream into poisoned
    buffers: the bytes of the eager run each time (no atomics, every byte written once, nothing allocated)."""
    import torch

    plan = covt.Plan.from_tiles([open(p, "rb").read() for p in tile_paths(("omt",))[:12]])
    b = covt.DeviceBatch(plan, "cuda:0")
    q = covt.SelectQuery(QUERY)
    s = torch.cuda.Stream(b.device)
    with torch.cuda.stream(s):
        for step in (b.decode, b.assemble, b.wkb):
            step(s)
        b.select_query(q, covt.WHERE_WRITE, s)
        b.select(s)
    torch.cuda.synchronize()
    buf_e, sres_e = b.select_results()
    buf_e, sres_e, qst_e = buf_e.copy(), sres_e.copy(), b.query_status().copy()
    assert (sres_e["status"] == 0).any() and int(sres_e["n_selected"].sum()) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.select_query(q, covt.WHERE_WRITE, s)
        b.select(s)
    for _ in range(2):
        b.d_select.fill_(FILL)
        b.d_sres.fill_(0x5A5A5A5A5A5A5A5A)
        b.d_query_status.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        buf, sres = b.select_results()
        assert sres.tobytes() == sres_e.tobytes() and np.array_equal(b.query_status(), qst_e)
        assert _columns_equal(plan, sres_e, buf_e, buf) == int((sres_e["status"] == 0).sum())
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_decode_covt_query(covt, oracle, gpu_available, decodable_tiles, n_tiles):
    """decode_covt(query=...): every layer's selected features are exactly those of query_ref over the oracle's
    assembly, and their WKB values those of the layer's WKB column."""
    q = covt.SelectQuery.at(2048, 2048, 600)
    w = tuple(q.window)
    kept = total = 0
    for key, tile in [kt for kt in decodable_tiles if kt[0].startswith("omt/")][:n_tiles]:
        cols = A.oracle_tile_columns(oracle, tile)
        for lc in covt.CovtParser.decode_covt(tile, query=q):
            if lc.wkb is None:
                assert lc.selected is None
                continue
            oc = cols[lc.layer]
            ref = Q.query_ref_numpy(oc["types"], *oc["asm"][1:], w)[0]
            assert lc.selected.index.tolist() == np.nonzero(ref)[0].tolist(), (key, lc.layer)
            sel, offs, data = S.select_ref(lc.wkb.offsets, lc.wkb.data, ref)
            assert lc.selected.wkb.offsets.tobytes() == offs.tobytes() and lc.selected.wkb.data.tobytes() == data.tobytes()
            kept += int(ref.sum())
            total += ref.size
    assert 0 < kept < total

"""GPU: the select passes (covt_select.hip, include/covt.h "Feature selection") against the references of
tests/covt_select.py, byte for byte: covt_geometry_select_device on synthetic binary columns (hand-made
wkb_offsets, bytes, WKB results and masks; no decode or assembly), covt_select_predicate_device on synthetic
bounding-box and measures buffers, covt_plan_select_host on every fixture tile, the DeviceBatch / DevicePlan
paths, a HIP-graph replay and decode_covt(select=...).  Every buffer starts as a fill pattern, and every byte
the definition leaves unwritten (the masks, sel and offsets past n_selected, bytes past n_bytes, the 16-byte
gaps between slices, failed columns' slices) must still hold it.

The kernels' step sizes the cases sit around: the copy cuts a column's output bytes into chunks of 1024 (64
lanes x 16 bytes) and stages the offsets of 256 values per LDS window; the scan takes a workgroup of 16 waves
per column in steps of 4096 features for batches of at most 4096 columns (a wave per column in steps of 256
beyond); the copy runs min(64, 8192 / n_columns) workgroups of 4 waves per column: 64 for a column alone, 2 at
4096 columns, and from 4097 columns on one workgroup, where each column also gets one wave for its scan.
"""
import numpy as np
import pytest

import covt_geo as G
import covt_select as S
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
CHUNK, WINDOW, COOP_STEP, SMALL = 1024, 256, 4096, 4096
SD = np.dtype([("off", np.int64), ("byte_cap", np.int64), ("n_features", np.int32), ("flags", np.int32)])


# ---- synthetic binary columns -----------------------------------------------------------------------------
def _column(lengths, mask, rng):
    """A binary column of the given value lengths with pseudo-random bytes, and its keep mask."""
    lengths = np.asarray(lengths, np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    data = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    data[data == FILL] = FILL ^ 0xFF  # (a copied byte never looks unwritten)
    mask = np.asarray(mask, np.uint8)
    assert mask.size == lengths.size
    return {"offs": offs, "data": data, "mask": mask}


def _masks(n, rng):
    """(name, mask) over n features: keep all, none, alternate, the first only, the last only, random with
    non-zero bytes other than 1."""
    alt = (np.arange(n) & 1).astype(np.uint8)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[:1] = 0x80
    last[n - 1:] = 0xFF
    rnd = rng.choice(np.array([0, 0, 1, 0x80, 0xFF, 2], np.uint8), n)
    return [("all", np.ones(n, np.uint8)), ("none", np.zeros(n, np.uint8)), ("alternate", alt), ("first", first),
            ("last", last), ("random", rnd)]


def _run(covt, cols, wstatus=None, wflags=None, sflags=None, s_n=None, s_cap=None):
    """covt_geometry_select_device over synthetic columns -> (select buffer, results, select descriptors).
    The WKB buffer and the select buffer are laid out here with a 16-byte gap after every slice."""
    import torch

    nc = len(cols)
    wd = np.zeros(nc, covt.WKB_DESC_DTYPE)
    wr = np.zeros(nc, covt.WKB_RESULT_DTYPE)
    sd = np.zeros(nc, covt.SELECT_DESC_DTYPE)
    assert covt.SELECT_DESC_DTYPE == SD
    woff = soff = 0
    for ci, col in enumerate(cols):
        n, nb = col["mask"].size, int(col["offs"][-1])
        cap = nb + (ci % 3) * 7  # (capacities above the byte count, as a plan's are)
        wd[ci] = (woff, S.a16(woff + 4 * (n + 1)), cap, n, wflags[ci] if wflags else 0)
        woff = S.a16(int(wd[ci]["bytes_off"]) + cap) + 16
        wr[ci] = (wstatus[ci] if wstatus else 0, 0, nb)
        sd[ci] = (soff, cap if s_cap is None or s_cap[ci] is None else s_cap[ci],
                  n if s_n is None or s_n[ci] is None else s_n[ci], sflags[ci] if sflags else 0)
        soff = S.a16(soff + S.member_offsets(n)[3] + cap) + 16
    wkb = np.full(max(woff, 16), FILL, np.uint8)
    sel = np.full(max(soff, 16), FILL, np.uint8)
    for ci, col in enumerate(cols):
        n, nb = col["mask"].size, int(col["offs"][-1])
        o, b = int(wd[ci]["offsets_off"]), int(wd[ci]["bytes_off"])
        wkb[o:o + 4 * (n + 1)] = col["offs"].view(np.uint8)
        wkb[b:b + nb] = col["data"]
        sel[int(sd[ci]["off"]):int(sd[ci]["off"]) + n] = col["mask"]
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    d_wd, d_wr, d_sd, d_wkb, d_sel = up(wd), up(wr), up(sd), up(wkb), up(sel)
    d_sres = torch.full((16 * nc,), FILL, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    assert covt.lib().covt_geometry_select_device(d_wd.data_ptr(), d_wkb.data_ptr(), d_wr.data_ptr(), d_sd.data_ptr(),
                                                  nc, d_sel.data_ptr(), d_sres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert d_wkb.cpu().numpy().tobytes() == wkb.tobytes()  # (the input is read only)
    return d_sel.cpu().numpy(), d_sres.cpu().numpy().view(covt.SELECT_RESULT_DTYPE), sd


def _check(cols, buf, sres, sd, failed=()):
    """Every column equals select_ref byte for byte; every byte the definition leaves alone holds FILL (the
    masks hold what the caller wrote)."""
    untouched = np.ones(buf.size, bool)
    for ci, col in enumerate(cols):
        o, n = int(sd["off"][ci]), col["mask"].size
        m_mask, m_sel, m_off, m_bytes = S.member_offsets(n)
        assert buf[o:o + n].tobytes() == col["mask"].tobytes(), ci
        untouched[o:o + n] = False
        if ci in failed:
            continue
        sel, offs, data = S.select_ref(col["offs"], col["data"], col["mask"])
        k = sel.size
        r = sres[ci]
        assert (int(r["status"]), int(r["n_selected"]), int(r["n_bytes"])) == (0, k, data.size), (ci, r)
        assert buf[o + m_sel:o + m_sel + 4 * k].tobytes() == sel.tobytes(), "column %d: sel" % ci
        assert buf[o + m_off:o + m_off + 4 * (k + 1)].tobytes() == offs.tobytes(), "column %d: offsets" % ci
        got = buf[o + m_bytes:o + m_bytes + data.size]
        if got.tobytes() != data.tobytes():
            bad = np.nonzero(got != data)[0]
            raise AssertionError("column %d: %d of %d bytes differ, first at %d (value %d): %d, want %d" % (
                ci, bad.size, data.size, int(bad[0]), int(np.searchsorted(offs, bad[0], "right")) - 1,
                int(got[bad[0]]), int(data[bad[0]])))
        untouched[o + m_sel:o + m_sel + 4 * k] = False
        untouched[o + m_off:o + m_off + 4 * (k + 1)] = False
        untouched[o + m_bytes:o + m_bytes + data.size] = False
    assert (buf[untouched] == FILL).all(), np.nonzero(untouched & (buf != FILL))[0][:8]


def _pad_batch(cols, n_total, rng):
    """The same columns among enough tiny ones to make a batch of n_total."""
    tiny = _column([21, 0, 5], [1, 0, 1], rng)
    return cols + [tiny] * (n_total - len(cols))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097])
def test_feature_counts_and_masks(covt, gpu_available, n):
    """Feature counts around the wave, the scan's cooperative step and its wave-per-column step, every mask
    shape; values of mixed small lengths (zero-length ones among them)."""
    rng = np.random.default_rng(100 + n)
    lengths = rng.choice([0, 1, 9, 15, 16, 17, 21, 31, 32, 33], n)
    cols = [_column(lengths, m, rng) for _, m in _masks(n, rng)]
    buf, sres, sd = _run(covt, cols)
    _check(cols, buf, sres, sd)
    keep_all = cols[0]
    o = int(sd["off"][0]) + S.member_offsets(n)[3]
    assert buf[o:o + keep_all["data"].size].tobytes() == keep_all["data"].tobytes()  # keep all: the input bytes


@pytest.mark.parametrize("length", [0, 1, 9, 15, 16, 17, 21, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1])
def test_value_lengths(covt, gpu_available, length):
    """Columns of one value length (below, at and above the 16-byte vector and the chunk), every mask shape."""
    rng = np.random.default_rng(200 + length)
    n = 300 if length < 100 else 9
    cols = [_column([length] * n, m, rng) for _, m in _masks(n, rng)]
    cols.append(_column([length, 3, length, 0, length], [1, 0, 1, 1, 1], rng))
    buf, sres, sd = _run(covt, cols)
    _check(cols, buf, sres, sd)


def test_every_source_and_destination_residue(covt, gpu_available):
    """A dropped first value of p bytes shifts every source address by p against the 16-byte destination
    vectors, and a kept prefix of q bytes every destination: p, q in 0 .. 15 with values of 100 bytes (vectors
    inside one value: the unaligned load) and of 21 (vectors put together from pieces)."""
    rng = np.random.default_rng(7)
    cols = []
    for p in range(16):
        for body in (100, 21):
            cols.append(_column([p] + [body] * 40, [0] + [1] * 40, rng))
            cols.append(_column([p, (p * 7) % 16] + [body] * 40, [0, 1] + [1] * 40, rng))
    buf, sres, sd = _run(covt, cols)
    _check(cols, buf, sres, sd)


def test_one_value_over_many_waves_and_workgroups(covt, gpu_available):
    """One value of about 300 KB between small ones: alone its 301 chunks go to the waves of 64 workgroups; the
    same column in a batch of 4096 gets two workgroups, in a batch of 4097 one workgroup and a one-wave scan.
    The bytes are the same each time."""
    rng = np.random.default_rng(8)
    big = 300 * 1024 + 5
    col = _column([21, 7, big, 21, 0, 33], [1, 0, 1, 1, 1, 1], rng)
    dropped = _column([21, big, 40], [1, 0, 1], rng)
    outs = []
    for total in (2, SMALL, SMALL + 1):
        cols = _pad_batch([col, dropped], total, rng)
        buf, sres, sd = _run(covt, cols)
        _check(cols, buf, sres, sd)
        o = int(sd["off"][0])
        outs.append(buf[o:o + S.member_offsets(6)[3] + int(sres["n_bytes"][0])].tobytes())
    assert outs[0] == outs[1] == outs[2] and int(sres["n_bytes"][0]) == big + 21 + 21 + 33


def test_runs_longer_than_the_window(covt, gpu_available):
    """A run of dropped features longer than the LDS window between two kept ones; runs of kept zero-length
    values longer than the window (they share an offset: a byte's owner is the last of them), at the column's
    start, inside a chunk and at its end; more values than a window holds inside one chunk (1-byte values)."""
    rng = np.random.default_rng(9)
    run = WINDOW + 44
    cols = [
        _column([50] + [21] * run + [50], [1] + [0] * run + [1], rng),
        _column([50] + [0] * run + [50], [1] * (run + 2), rng),
        _column([0] * run + [50] + [0] * run, [1] * (2 * run + 1), rng),
        _column([0] * (3 * run) + [5], [1] * (3 * run + 1), rng),
        _column([0] * 10, [1] * 10, rng),  # kept values, no bytes at all
        _column([1] * (3 * CHUNK), [1] * (3 * CHUNK), rng),
        _column([1, 0, 0, 2] * (2 * CHUNK), [1] * (8 * CHUNK), rng),
        _column(rng.choice([0, 0, 0, 1, 40], 5000), rng.integers(0, 2, 5000), rng),
    ]
    buf, sres, sd = _run(covt, cols)
    _check(cols, buf, sres, sd)
    many = _pad_batch(cols, SMALL + 1, rng)
    buf, sres, sd = _run(covt, many)
    _check(many, buf, sres, sd)


def test_many_columns_one_wave_each(covt, gpu_available):
    """4097 columns (a wave per column in the scan, one workgroup per column in the copy) of 0 .. 700 features."""
    rng = np.random.default_rng(10)
    cols = []
    for i in range(SMALL + 1):
        n = int(rng.choice([0, 1, 3, 64, 255, 256, 257, 700])) if i % 16 == 0 else int(rng.integers(0, 6))
        cols.append(_column(rng.choice([0, 5, 21, 37, 200], n), rng.integers(0, 2, n) * rng.choice([1, 0x80], n), rng))
    buf, sres, sd = _run(covt, cols)
    _check(cols, buf, sres, sd)


def test_status_paths(covt, gpu_available):
    """A WKB status that is not OK, either TOO_LARGE flag, a mismatched n_features or byte_cap: that status or
    COVT_ERR_INVALID_ARG, n_selected 0, n_bytes 0 and the slice untouched, between columns that succeed."""
    rng = np.random.default_rng(11)
    mk = lambda: _column([21] * 50 + [300], [1] * 51, rng)  # noqa: E731
    cols = [mk() for _ in range(8)]
    I = covt.ERR_INVALID_ARG
    buf, sres, sd = _run(covt, cols,
                         wstatus=[0, covt.ERR_TRUNCATED, 0, 0, 0, 0, covt.ERR_COUNT_MISMATCH, 0],
                         wflags=[0, 0, covt.WKB_TOO_LARGE, 0, 0, 0, 0, 0],
                         sflags=[0, 0, 0, covt.SELECT_TOO_LARGE, 0, 0, 0, 0],
                         s_n=[None, None, None, None, 50, None, None, None],
                         s_cap=[None, None, None, None, None, 1 << 20, None, None])
    assert sres["status"].tolist() == [0, covt.ERR_TRUNCATED, I, I, I, I, covt.ERR_COUNT_MISMATCH, 0]
    failed = (1, 2, 3, 4, 5, 6)
    for ci in failed:
        assert int(sres["n_selected"][ci]) == 0 and int(sres["n_bytes"][ci]) == 0
    _check(cols, buf, sres, sd, failed)


# ---- the predicate ----------------------------------------------------------------------------------------
def _run_predicate(covt, boxes, measures, pred, bstatus=None, mstatus=None):
    """covt_select_predicate_device over synthetic bounding-box and measures buffers -> the masks."""
    import torch

    nc = len(boxes)
    bd = np.zeros(nc, covt.BBOX_DESC_DTYPE)
    md = np.zeros(nc, covt.MEASURES_DESC_DTYPE)
    sd = np.zeros(nc, covt.SELECT_DESC_DTYPE)
    br = np.zeros(nc, covt.BBOX_RESULT_DTYPE)
    mr = np.zeros(nc, covt.MEASURES_RESULT_DTYPE)
    boff = moff = soff = 0
    for ci, box in enumerate(boxes):
        n = box[0].size
        bd[ci] = (boff, n, 0)
        md[ci] = (moff, n, 0, 0, 0)
        sd[ci] = (soff, 64, n, 0)
        br[ci]["status"] = bstatus[ci] if bstatus else 0
        mr[ci]["status"] = mstatus[ci] if mstatus else 0
        boff = S.a16(boff + 32 * n) + 16
        moff = S.a16(moff + 16 * n + S.a16(4 * n)) + 16
        soff = S.a16(soff + S.member_offsets(n)[3] + 64) + 16
    bbuf, mbuf = np.full(max(boff, 16), FILL, np.uint8), np.full(max(moff, 16), FILL, np.uint8)
    for ci, (box, ms) in enumerate(zip(boxes, measures)):
        n = box[0].size
        for k in range(4):
            o = int(bd[ci]["off"]) + 8 * n * k
            bbuf[o:o + 8 * n] = box[k].view(np.uint8)
        for k in range(2):
            o = int(md[ci]["off"]) + 8 * n * k
            mbuf[o:o + 8 * n] = ms[k].view(np.uint8)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    t = [up(a) for a in (bd, bbuf, br, md, mbuf, mr, sd)]
    d_sel = torch.full((max(soff, 16),), FILL, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    import ctypes as C
    assert covt.lib().covt_select_predicate_device(*[x.data_ptr() for x in t], nc, C.byref(pred), d_sel.data_ptr(), s) == 0
    torch.cuda.synchronize()
    buf = d_sel.cpu().numpy()
    untouched = np.ones(buf.size, bool)
    masks = []
    for ci, box in enumerate(boxes):
        o, n = int(sd[ci]["off"]), box[0].size
        masks.append(buf[o:o + n].copy())
        untouched[o:o + n] = False
    assert (buf[untouched] == FILL).all()  # nothing but the masks is written
    return masks


def _synthetic_boxes(rng, n, window):
    """n boxes around `window`, with rows touching each of its four edges, one step outside each, NaN rows, and
    measures with +-0.0, values at and next to the minima 4.0 / 8.0."""
    x0, y0, x1, y1 = window
    xmin = rng.uniform(x0 - 30, x1 + 10, n)
    ymin = rng.uniform(y0 - 30, y1 + 10, n)
    xmax = xmin + rng.uniform(0, 25, n)
    ymax = ymin + rng.uniform(0, 25, n)
    for i, (a, b, c, d) in enumerate([(x1, y0, x1 + 5, y1), (x0 - 5, y0, x0, y1), (x0, y1, x1, y1 + 5),
                                      (x0, y0 - 5, x1, y0), (np.nextafter(x1, np.inf), y0, x1 + 5, y1),
                                      (x0 - 5, y0, np.nextafter(x0, -np.inf), y1), (x0, np.nextafter(y1, np.inf), x1, y1 + 5),
                                      (x0, y0 - 5, x1, np.nextafter(y0, -np.inf)), (x0 - 99, y0 - 99, x1 + 99, y1 + 99)]):
        if i < n:
            xmin[i], ymin[i], xmax[i], ymax[i] = a, b, c, d
    empty = rng.random(n) < 0.1
    for a in (xmin, ymin, xmax, ymax):
        a[empty] = np.nan
    area = rng.choice([0.0, -0.0, 3.9999, 4.0, 4.0001, 100.0, -96.0], n)
    length = rng.choice([0.0, -0.0, 7.9999, 8.0, 8.0001, 0.5], n)
    return (xmin, ymin, xmax, ymax), (area, length)


def test_predicate_on_synthetic_buffers(covt, gpu_available):
    rng = np.random.default_rng(12)
    window = (10.0, 20.0, 30.0, 40.0)
    sizes = [0, 1, 9, 63, 64, 65, 300, 5000, 20000]  # (one workgroup pass holds 64 x 256 features)
    data = [_synthetic_boxes(rng, n, window) for n in sizes]
    boxes, measures = [d[0] for d in data], [d[1] for d in data]
    P = covt.SelectPred
    preds = [P(), P(keep_empty=True), P(window=window), P(window=window, keep_empty=True),
             P(window=(30.0, 20.0, 10.0, 40.0)), P(window=(10.0, 40.0, 30.0, 20.0), keep_empty=True),  # inverted
             P(min_area=4.0, min_length=8.0), P(min_area=0.0, min_length=0.0), P(min_area=-0.0),
             P(window=window, min_area=4.0, min_length=8.0, keep_empty=True), P(window=(30.0, 40.0, 30.0, 40.0))]
    kept = 0
    for pi, pred in enumerate(preds):
        masks = _run_predicate(covt, boxes, measures, pred)
        for ci in range(len(sizes)):
            want = S.predicate_ref(*boxes[ci], *measures[ci], pred)
            assert masks[ci].tobytes() == want.tobytes(), (pi, ci, np.nonzero(masks[ci] != want)[0][:5])
            kept += int(want.sum())
            if pi in (4, 5):  # an inverted window: nothing but (asked for) the empty features
                assert (want == (np.isnan(boxes[ci][0]) if pi == 5 else 0)).all()
    assert kept > 10000
    # a failed bounding-box column, and with a size cut a failed measures column: an all-zero mask
    st_b = [0, 0, 0, 0, covt.ERR_TRUNCATED, 0, 0, covt.ERR_INVALID_ARG, 0]
    st_m = [0, 0, 0, 0, 0, covt.ERR_COUNT_MISMATCH, 0, 0, 0]
    for pred, dead in ((P(keep_empty=True), (4, 7)), (P(min_area=0.0, keep_empty=True), (4, 5, 7))):
        masks = _run_predicate(covt, boxes, measures, pred, st_b, st_m)
        for ci in range(len(sizes)):
            want = S.predicate_ref(*boxes[ci], *measures[ci], pred)
            assert masks[ci].tobytes() == (bytes(sizes[ci]) if ci in dead else want.tobytes()), ci
    # many columns: a wave per column
    small = [_synthetic_boxes(rng, int(rng.integers(0, 200)), window) for _ in range(50)]
    boxes = [small[i % 50][0] for i in range(SMALL + 1)]
    measures = [small[i % 50][1] for i in range(SMALL + 1)]
    pred = P(window=window, min_area=4.0, min_length=8.0, keep_empty=True)
    masks = _run_predicate(covt, boxes, measures, pred)
    for ci in range(SMALL + 1):
        assert masks[ci].tobytes() == S.predicate_ref(*boxes[ci], *measures[ci], pred).tobytes(), ci


# ---- fixture tiles ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_products(covt, gpu_available):
    """Every fixture tile in one plan, its WKB columns, boxes and measures in tile pixels and in CRS84 (the
    references' inputs), computed once for the tests below."""
    paths = tile_paths()
    plan = covt.Plan.from_tiles([open(p, "rb").read() for p in paths])
    zxy = [list(G.zxy_of_key(tile_key(p))) for p in paths]
    out = {"plan": plan, "zxy": zxy, "measures": plan.measures_host()}
    for crs in (covt.CRS_TILE, covt.CRS_CRS84):
        out[crs] = (plan.wkb_host(crs, zxy), plan.bbox_host(crs, zxy))
    return out


@pytest.mark.parametrize("crs_name", ["CRS_TILE", "CRS_CRS84"])
def test_fixture_tiles_select_host(covt, fixture_products, crs_name):
    """covt_plan_select_host on every fixture tile: the mask equals predicate_ref over the plan's own boxes and
    measures, sel / offsets / bytes equal select_ref over its own WKB column, and SelectedColumn.wkb.feature(j)
    is the plain column's feature(index[j])."""
    crs = getattr(covt, crs_name)
    plan, zxy = fixture_products["plan"], fixture_products["zxy"]
    (wbuf, wres), (bbuf, bres) = fixture_products[crs]
    mbuf, mres = fixture_products["measures"]
    # a quarter of each tile in pixels; a band of longitudes and latitudes in degrees
    window = (0.0, 0.0, 2048.0, 2048.0) if crs == covt.CRS_TILE else (-20.0, -10.0, 60.0, 50.0)
    preds = [covt.SelectPred(window=window, min_area=4.0, min_length=8.0), covt.SelectPred(window=window, keep_empty=True)]
    for pi, pred in enumerate(preds):
        sbuf, sres = plan.select_host(pred, crs, zxy)
        assert np.array_equal(sres["status"], wres["status"])
        n_ok = n_kept = n_dropped = 0
        for c in range(plan.num_geometry_columns):
            if int(sres["status"][c]):
                assert int(sres["n_selected"][c]) == 0 and int(sres["n_bytes"][c]) == 0
                continue
            w = plan.wkb_column(wbuf, wres, c)
            n, o = len(w), int(plan.select["off"][c])
            box_ok = int(bres["status"][c]) == 0 and (pi or int(mres["status"][c]) == 0)
            if box_ok:
                b, m = plan.bbox_column(bbuf, bres, c), plan.measures_column(mbuf, mres, c)
                want = S.predicate_ref(b.xmin, b.ymin, b.xmax, b.ymax, m.area, m.length, pred)
            else:
                want = np.zeros(n, np.uint8)
            mask = sbuf[o:o + n]
            assert mask.tobytes() == want.tobytes(), (c, np.nonzero(mask != want)[0][:5])
            sel, offs, data = S.select_ref(w.offsets, w.data, mask)
            col = plan.select_column(sbuf, sres, c)
            assert (int(sres["n_selected"][c]), int(sres["n_bytes"][c])) == (sel.size, data.size), c
            assert col.index.tobytes() == sel.tobytes() and col.wkb.offsets.tobytes() == offs.tobytes(), c
            assert col.wkb.data.tobytes() == data.tobytes(), c
            for j in range(0, len(col), max(1, len(col) // 7)):
                assert col.wkb.feature(j) == w.feature(int(col.index[j])), (c, j)
            n_ok += 1
            n_kept += sel.size
            n_dropped += n - sel.size
        assert n_ok >= 700 and n_kept > 0 and n_dropped > 0, (n_ok, n_kept, n_dropped)


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


def _batch(covt, n_tiles):
    tiles = [open(p, "rb").read() for p in tile_paths(("omt",))[:n_tiles]]
    plan = covt.Plan.from_tiles(tiles)
    b = covt.DeviceBatch(plan, "cuda:0")
    return plan, b


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_device_paths_match_host_path(covt, gpu_available, n_tiles):
    import torch

    plan, b = _batch(covt, n_tiles)
    pred = covt.SelectPred(window=(0.0, 0.0, 2048.0, 2048.0), min_area=4.0, min_length=8.0)
    buf_h, sres_h = plan.select_host(pred)
    assert (sres_h["status"] == 0).any() and int(sres_h["n_selected"].sum()) > 0
    for step in (b.decode, b.assemble, b.wkb, b.bbox, b.measures):
        step()
    b.select_predicate(pred)
    b.select()
    torch.cuda.synchronize()
    buf_d, sres_d = b.select_results()
    assert sres_h.tobytes() == sres_d.tobytes()
    assert _columns_equal(plan, sres_h, buf_h, buf_d) > 0
    # a caller-written mask: keep every third feature of every column
    wbuf, wres = b.wkb_results()
    for c in range(plan.num_geometry_columns):
        m = b.select_mask(c)
        assert m.dtype == torch.uint8 and m.numel() == int(plan.select["n_features"][c])
        m.copy_(torch.from_numpy(((np.arange(m.numel()) % 3 == 0) * 0x80).astype(np.uint8)))
    b.select()
    torch.cuda.synchronize()
    buf_m, sres_m = b.select_results()
    for c in range(plan.num_geometry_columns):
        if int(wres["status"][c]):
            continue
        w = plan.wkb_column(wbuf, wres, c)
        sel, offs, data = S.select_ref(w.offsets, w.data, np.arange(len(w)) % 3 == 0)
        col = plan.select_column(buf_m, sres_m, c)
        assert col.index.tobytes() == sel.tobytes() and col.wkb.offsets.tobytes() == offs.tobytes()
        assert col.wkb.data.tobytes() == data.tobytes()
    # the device plan: the same records and descriptors, the same bytes from the batch's masks
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    si, sdd = dp.select_copy()
    assert si.tobytes() == plan.select.tobytes() and sdd.tobytes() == plan.sdescs.tobytes()
    assert dp.select_bytes == plan.select_bytes
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_wkb, d_wres = dp.alloc_wkb()
    d_sel, d_sres = dp.alloc_select()
    d_sel.fill_(FILL)
    d_sel[:plan.select_bytes].copy_(b.d_select[:plan.select_bytes])  # (the masks; the rest is rewritten)
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.wkb(d_out, d_res, d_asm, d_gres, d_wkb, d_wres)
    dp.select(d_wkb, d_wres, d_sel, d_sres)
    torch.cuda.synchronize()
    sres_p = d_sres.cpu().numpy().view(covt.SELECT_RESULT_DTYPE)[:plan.num_geometry_columns][plan.select["desc_index"]]
    assert sres_p.tobytes() == sres_m.tobytes()
    assert _columns_equal(plan, sres_m, buf_m, d_sel.cpu().numpy()[:plan.select_bytes]) > 0


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_predicate_and_select_replay_in_a_hip_graph(covt, gpu_available, n_tiles):
    """predicate + select captured in one HIP graph (no scratch: nothing to warm up but the code objects) and
    replayed twice on its capture stream into poisoned buffers: the bytes of the eager run each time."""
    import torch

    plan, b = _batch(covt, n_tiles)
    pred = covt.SelectPred(window=(1024.0, 1024.0, 3072.0, 3072.0), min_length=8.0, keep_empty=True)
    s = torch.cuda.Stream(b.device)
    with torch.cuda.stream(s):
        for step in (b.decode, b.assemble, b.wkb, b.bbox, b.measures):
            step(s)
        b.select_predicate(pred, s)
        b.select(s)
    torch.cuda.synchronize()
    buf_e, sres_e = b.select_results()
    buf_e, sres_e = buf_e.copy(), sres_e.copy()
    assert (sres_e["status"] == 0).any() and int(sres_e["n_selected"].sum()) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.select_predicate(pred, s)
        b.select(s)
    for _ in range(2):
        b.d_select.fill_(FILL)
        b.d_sres.fill_(0x5A5A5A5A5A5A5A5A)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        buf, sres = b.select_results()
        assert sres.tobytes() == sres_e.tobytes()
        assert _columns_equal(plan, sres_e, buf_e, buf) == int((sres_e["status"] == 0).sum())
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_decode_covt_select(covt, gpu_available, decodable_tiles, n_tiles):
    """decode_covt(select=...) gives every layer the kept features: index and their WKB values, consistent with
    the layer's own wkb, bbox and measures; without the argument selected is None."""
    pred = covt.SelectPred(window=(0.0, 0.0, 2048.0, 4096.0), min_area=16.0, min_length=32.0)
    kept = total = 0
    for ti, (_, tile) in enumerate(decodable_tiles[:n_tiles]):
        layers = covt.CovtParser.decode_covt(tile, select=pred)
        if ti == 0:  # without the argument: the same layers, selected None
            plain = covt.CovtParser.decode_covt(tile)
            assert plain and len(plain) == len(layers) and all(lc.selected is None for lc in plain)
            assert all(a.wkb.data.tobytes() == b.wkb.data.tobytes() for a, b in zip(layers, plain) if a.wkb is not None)
        for lc in layers:
            if lc.wkb is None:
                assert lc.selected is None
                continue
            want = S.predicate_ref(lc.bbox.xmin, lc.bbox.ymin, lc.bbox.xmax, lc.bbox.ymax, lc.measures.area,
                                   lc.measures.length, pred)
            sel, offs, data = S.select_ref(lc.wkb.offsets, lc.wkb.data, want)
            assert lc.selected.index.tobytes() == sel.tobytes() and lc.selected.wkb.offsets.tobytes() == offs.tobytes()
            assert lc.selected.wkb.data.tobytes() == data.tobytes()
            for j in range(len(lc.selected)):
                assert lc.selected.wkb.feature(j) == lc.wkb.feature(int(lc.selected.index[j]))
            if lc.ids is not None and lc.ids.size == len(lc.wkb):
                assert lc.ids[lc.selected.index].size == len(lc.selected)
            kept += len(lc.selected)
            total += len(lc.wkb)
    assert 0 < kept < total

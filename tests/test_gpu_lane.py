"""The lane-per-stream RLE decoder (covt_decode.hip decode_lane_kernel and the lane segment of
decode_fused_kernel: LaneBytes, Pack16, lane_rle_int, lane_rle_byte) against the oracle
(RunLengthIntegerReader / RunLengthByteReader, DecodingUtils.java:257-313) and against the wave-per-stream
decoder, on streams built to break it.  The plan turns lanes on only from 65,536 eligible streams, so every
other synthetic test reaches the wave decoders alone.

* descriptor level (tests/covt_lane.py): hand-built descriptors with COVT_DESC_LANE through the grouped
  launch, fused (128 streams per workgroup) and forked (256), every stream checked against the oracle
  (status, values, consumed) and the same descriptors through the wave kernel: identical result rows,
  failures included (consumed is 0 for a failed stream on every path, include/covt.h).  Output slots of
  exactly align16(n * elem) bytes, packed back to back in shuffled order in a buffer pre-filled with 0x5A:
  bytes [n * elem, align16) of a slot are unspecified (the last packet is written whole), a failed stream
  may touch only its own slot, every byte outside the slots keeps 0x5A.
* the corpus proves on the CPU (no GPU mark) that it reaches what it aims at.
* plan level: adversarial Gen D RLE tiles and synthetic property layers planned with lane_min_streams=0,
  row for row equal to the same tiles planned without lanes."""
import ctypes as C

import numpy as np
import pytest

import covt_lane as CL
from test_gpu_split import DESC

GUARD = 256  # bytes of 0x5A before the first and after the last output slot
_CACHE = {}


def _corpus(covt, oracle):
    """(corpus, the oracle's (status, values, consumed) per row), built once and never changed."""
    if "corpus" not in _CACHE:
        c = CL.build_corpus(covt)
        _CACHE["corpus"] = (c, [CL.expected(c, oracle, r) for r in c.rows])
    return _CACHE["corpus"]


# ---------------------------------------------------------------------------------------------------------
# the corpus proves its own coverage (CPU)
# ---------------------------------------------------------------------------------------------------------
def test_corpus_covers_the_lane_code(covt, oracle):
    c, exp = _corpus(covt, oracle)
    rows = c.rows
    assert len(rows) > 3000
    ok = np.array([e[0] == 0 for e in exp])
    st = np.array([e[0] for e in exp])
    run_slots, lit_starts, straddles = set(), set(), set()
    for r, e in zip(rows, exp):
        w = CL.window_walk(c, r)
        if r["expect"] is None:  # the model walks a stream to its end exactly where the oracle decodes it
            bad_type = e[0] == covt.ERR_BAD_HEADER
            assert (w is not None) == (e[0] == 0 or bad_type), (r, e[0])
        if e[0] != 0 or w is None:
            continue
        assert w["consumed"] == e[2], r
        per = 16 // c.elem[r["op"]]
        assert all(0 <= s < per for s in w["runs"])
        run_slots |= {(r["op"], s) for s in w["runs"]}
        lit_starts |= {(r["op"], o, a) for o, a, cnt in w["lits"] if cnt >= 8}
        straddles |= {(kind, min(edge, 2)) for kind, edge in w["straddles"]}
    # every (op, packet slot) a run can start in
    for op in c.int_ops + c.byte_ops:
        for s in range(16 // c.elem[op]):
            assert (op, s) in run_slots, (op, s)
    # byte literal groups of >= 8 bytes: every output offset mod 16 x input address mod 4, both byte ops
    for op in c.byte_ops:
        for o in range(16):
            for a in range(4):
                assert (op, o, a) in lit_starts, (op, o, a)
    # each kind of field across the first window edge and across a later one
    for kind in ("varint", "run", "bytelit"):
        assert (kind, 1) in straddles and (kind, 2) in straddles, (kind, sorted(straddles))
    fail = 1.0 - ok.mean()
    assert 0.20 <= fail <= 0.60, fail
    assert (st == covt.ERR_TRUNCATED).any() and (st == covt.ERR_BAD_HEADER).any()
    long_ok = sum(1 for r, e in zip(rows, exp) if e[0] == 0 and e[2] > CL.WINDOW)
    assert long_ok >= 0.30 * ok.sum(), (long_ok, int(ok.sum()))
    fams = {}
    for r, e in zip(rows, exp):
        if r["fam"] >= 0:
            fams.setdefault(r["fam"], set()).add(e[0] == 0)
    assert len(fams) >= 12 and all(v == {True, False} for v in fams.values())
    # the surplus rules: literals past num_values are read (integers) or skipped unchecked (bytes)
    sur = [(r, e) for r, e in zip(rows, exp) if r["group"] == "surplus"]
    whole = [(r, e) for r, e in sur if r["note"] == "complete"]
    assert len(whole) > 40 and all(e[0] == 0 and e[2] == r["avail"] for r, e in whole)
    assert any(e[0] == covt.ERR_TRUNCATED for r, e in sur if r["op"] in c.int_ops)
    for note, want in (("bad_surplus", 0), ("bad_run_unread", 0), ("bad_last_taken", covt.ERR_BAD_HEADER),
                       ("bad_run_first", covt.ERR_BAD_HEADER)):
        hit = [e[0] for r, e in sur if r["note"] == note and r["op"] == covt.OP_BYTE_RLE_U8]
        assert hit and all(s == want for s in hit), (note, hit)
    assert {r["group"] for r in rows} == {g for g, _ in CL.GROUPS}


# ---------------------------------------------------------------------------------------------------------
# descriptor level (GPU)
# ---------------------------------------------------------------------------------------------------------
def _layout(c, idx, rng, shuffle=True):
    """Descriptors of rows `idx` in launch order and their output slots: exactly align16(n * elem) bytes each,
    back to back in an order of their own after GUARD bytes.  -> (DESC array, row index per descriptor,
    slot offsets, slot sizes, buffer bytes)."""
    idx = np.asarray(idx)
    order = rng.permutation(idx) if shuffle else idx
    size = np.array([CL.align16(max(c.rows[i]["n"], 0) * c.elem.get(c.rows[i]["op"], 4)) for i in order], dtype=np.int64)
    pos = rng.permutation(order.size)
    off = np.zeros(order.size, dtype=np.int64)
    off[pos] = GUARD + np.concatenate(([0], np.cumsum(size[pos])[:-1]))
    d = np.zeros(order.size, dtype=DESC)
    for k, i in enumerate(order):
        r = c.rows[i]
        d[k] = (r["in_off"], off[k], r["avail"], r["n"], r["op"], 0, 0, r["avail"])
    return d, order, off, size, GUARD + int(size.sum()) + GUARD


def _device_input(covt, c):
    import torch

    if "d_in" not in _CACHE:
        dev = torch.device("cuda")
        d_in = torch.full((len(c.blob) + covt.INPUT_PADDING + 16,), CL.FILL, dtype=torch.uint8, device=dev)
        d_in[:len(c.blob)] = torch.frombuffer(bytearray(c.blob), dtype=torch.uint8).to(dev)
        assert d_in.data_ptr() % 16 == 0  # the corpus places streams by address residue
        _CACHE["d_in"] = d_in
    return _CACHE["d_in"]


def _launch(covt, d_in, d, family, flags, total, launch):
    import torch

    d = d.copy()
    d["flags"] = flags
    counts = np.zeros(covt.NUM_FAMILIES, dtype=np.int64)
    counts[family] = d.size
    dev = d_in.device
    d_desc = torch.from_numpy(d.view(np.uint8)).to(dev)
    d_out = torch.full((total,), 0x5A, dtype=torch.uint8, device=dev)
    d_res = torch.full((d.size * 2,), 0x33, dtype=torch.int32, device=dev)
    st = covt.lib().covt_decode_streams_device_grouped_mode(
        d_in.data_ptr(), d_desc.data_ptr(), counts.ctypes.data_as(C.POINTER(C.c_int64)), d_out.data_ptr(),
        d_res.data_ptr(), torch.cuda.current_stream().cuda_stream, launch)
    assert st == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_res.cpu().numpy().reshape(-1, 2)


def _check(c, exp, order, off, size, out, res, what):
    """Every descriptor against the oracle; -> (descriptors checked, streams whose values were compared)."""
    bad = []
    n_checked = n_values = 0
    free = np.ones(out.size, dtype=bool)
    for k, i in enumerate(order):
        r, (st, vals, cons) = c.rows[i], exp[i]
        free[off[k]:off[k] + size[k]] = False
        tag = (what, r["group"], int(i), r["op"], r["n"], r["avail"], r["in_off"] & 15)
        if int(res[k, 0]) != st:
            bad.append(("status", tag, int(res[k, 0]), st))
        elif int(res[k, 1]) != cons:
            bad.append(("consumed", tag, int(res[k, 1]), cons))
        elif st == 0 and vals is not None:
            got = out[off[k]:off[k] + vals.nbytes]
            if got.tobytes() != vals.tobytes():
                first = int(np.nonzero(got != np.frombuffer(vals.tobytes(), np.uint8))[0][0])
                bad.append(("values", tag, "first differing output byte %d" % first))
        if st == 0:
            n_values += 1
        n_checked += 1
    assert not bad, (len(bad), bad[:8])
    stray = np.nonzero(free & (out != 0x5A))[0]
    assert stray.size == 0, (what, "bytes outside every slot were written", stray[:8].tolist())
    return n_checked, n_values


def _run_both_paths(covt, c, exp, idx, launch, rng, shuffle=True):
    d_in = _device_input(covt, c)
    d, order, off, size, total = _layout(c, idx, rng, shuffle)
    out_l, res_l = _launch(covt, d_in, d, covt.FAMILY_LANE, covt.DESC_LANE, total, launch)
    n_ok = sum(1 for i in order if exp[i][0] == 0)
    assert _check(c, exp, order, off, size, out_l, res_l, "lane") == (order.size, n_ok)
    # the same descriptors, one wave per stream (a varint op flagged for a lane has no wave counterpart)
    keep = np.array([not c.rows[i]["lane_only"] for i in order])
    out_w, res_w = _launch(covt, d_in, d[keep], covt.FAMILY_RLE, 0, total, launch)
    assert _check(c, exp, order[keep], off[keep], size[keep], out_w, res_w, "wave") == (int(keep.sum()), sum(
        1 for i in order[keep] if exp[i][0] == 0))
    assert np.array_equal(res_l[keep], res_w)  # identical (status, consumed) rows, failures included
    for k in np.nonzero(keep)[0]:
        i = order[k]
        if exp[i][0] == 0:
            nb = exp[i][1].nbytes
            assert np.array_equal(out_l[off[k]:off[k] + nb], out_w[off[k]:off[k] + nb]), int(i)
    return order.size


@pytest.mark.gpu
@pytest.mark.parametrize("launch", [1, 2], ids=["fused", "forked"])  # COVT_LAUNCH_FUSED / _FORKED
def test_lane_corpus_against_oracle_and_wave_kernel(covt, oracle, gpu_available, launch):
    c, exp = _corpus(covt, oracle)
    assert launch in (covt.LAUNCH_FUSED, covt.LAUNCH_FORKED)
    n = _run_both_paths(covt, c, exp, np.arange(len(c.rows)), launch, np.random.default_rng(launch))
    assert n == len(c.rows)  # one launch per path holds the whole corpus: no descriptor is skipped


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_lane_grid_shapes(covt, oracle, gpu_available, count):
    """Descriptor counts around the 64-lane wave, the fused workgroup (128) and the forked one (256); every wave
    mixes the five ops, and 4,000-byte streams sit beside 3-byte ones."""
    c, exp = _corpus(covt, oracle)
    rows = c.rows
    long_rows = [i for i, r in enumerate(rows) if r["group"] == "lengths" and r["avail"] >= 4000]
    tiny_rows = [i for i, r in enumerate(rows) if r["group"] == "lengths" and r["avail"] == 3]
    assert len(long_rows) >= 5 and len(tiny_rows) == 5
    rng = np.random.default_rng(5)
    rest = rng.permutation([i for i, r in enumerate(rows) if r["group"] in ("runs", "literals", "surplus", "window")])
    idx = []
    for k in range(5):
        idx += [tiny_rows[k], long_rows[k], tiny_rows[(k + 1) % 5]] + rest[20 * k:20 * k + 20].tolist()
    idx += rest[100:400].tolist()
    assert len({rows[i]["op"] for i in idx[:64]}) == 5
    for launch in (covt.LAUNCH_FUSED, covt.LAUNCH_FORKED):
        assert _run_both_paths(covt, c, exp, idx[:count], launch, rng, shuffle=False) == count


# ---------------------------------------------------------------------------------------------------------
# plan level (GPU)
# ---------------------------------------------------------------------------------------------------------
def _small_tile(rng, bad_types):
    """test_gpu_rle_adversarial._tile with topology streams short enough for a lane."""
    from oracle import gend as W
    from test_gpu_rle_adversarial import _counts

    layers = []
    for L in range(int(rng.integers(1, 4))):
        n = int(rng.choice([1, 3, 64, 257, 1000, 5000]))
        types = rng.integers(0, 6, size=n).astype(np.uint8)
        if n > 8:
            types[: n // 3] = types[0]  # byte runs
        if bad_types and n > 1:
            types[int(rng.integers(0, n))] = 6 + int(rng.integers(0, 200))
        go, po, ro = (_counts(rng, int(rng.choice([1, 2, 5, 40, 300]))) for _ in range(3))
        xy = rng.integers(0, 4096, size=(64, 2))
        g = W.geometry_column(types, geometry_offsets=go, part_offsets=po, ring_offsets=ro, vertices=xy,
                              column_type=W.CT_PLAIN, allow_fpf_topology=False, allow_fpf_vertex=False)
        layers.append(W.layer("L%d" % L, 4096, n, [W.id_column(np.arange(n, dtype=np.uint64)), g], layer_id=L))
    return W.tile(layers)


def _lane_descs(covt, plan):
    d = plan.descs.view(DESC)
    return d[(d["flags"] & covt.DESC_LANE) != 0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["format", "java"])
def test_plan_adversarial_rle_tiles_in_lanes(covt, oracle, gpu_available, mode):
    import torch

    from test_gpu_gend import _check_streams

    rng = np.random.default_rng(70 + mode)
    tiles = [_small_tile(rng, bad_types=(i % 5 == 4)) for i in range(24)]
    off = covt.Plan.from_tiles(tiles, covt.FORMAT_GEND, mode, options=covt.PlanOptions(lane_min_streams=0,
                                                                                      lane_max_bytes=-1))
    assert (off.tile_status == 0).all() and off.family_counts[covt.FAMILY_LANE] == 0
    ref_res = off.decode_host()[1]
    wide = dict(lane_min_streams=0, lane_max_bytes=4096, lane_max_values=32767)
    for k, opts in enumerate((covt.PlanOptions(lane_min_streams=0), covt.PlanOptions(**wide))):
        plan = covt.Plan.from_tiles(tiles, covt.FORMAT_GEND, mode, options=opts)
        assert (plan.tile_status == 0).all()
        assert plan.family_counts[covt.FAMILY_LANE] > 0
        lanes = _lane_descs(covt, plan)
        assert lanes.size == plan.family_counts[covt.FAMILY_LANE]
        if k == 1:
            assert (lanes["avail"] > 128).any()
        out, res = plan.decode_host()
        assert _check_streams(covt, oracle, plan, out, res, tiles, mode) >= 100
        gt = plan.streams["op"] == covt.OP_BYTE_RLE_U8
        assert (res[gt, 0] == covt.ERR_BAD_HEADER).any() and (res[gt, 0] == 0).any()
        assert np.array_equal(res, ref_res), k  # row for row what the wave decoders report
        db = covt.DeviceBatch(plan, "cuda")
        for launch in (covt.LAUNCH_FUSED, covt.LAUNCH_FORKED):
            db.d_out.fill_(0x5A)
            db.d_res.fill_(0x33)
            db.decode(launch=launch)
            torch.cuda.synchronize()
            dout, dres = db.results()
            assert np.array_equal(dres, ref_res), (k, launch)
            assert _check_streams(covt, oracle, plan, dout, dres, tiles, mode) >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["format", "java"])
def test_plan_synthetic_gend_properties_in_lanes(covt, oracle, gpu_available, mode):
    import torch

    from oracle import gend as W
    from test_gpu_gend import _check_props, _check_streams, _synthetic_layer

    rng = np.random.default_rng(2024)
    tiles = [W.tile([_synthetic_layer(rng, L) for L in range(int(rng.integers(1, 5)))]) for _ in range(24)]
    got = []
    for lane_max_bytes in (0, -1):  # 0: the plan's own limits (512 bytes, 512 values with properties); -1: no lanes
        opts = covt.PlanOptions(lane_min_streams=0)
        if lane_max_bytes < 0:
            opts.lane_max_bytes = lane_max_bytes
        plan = covt.Plan.from_tiles(tiles, covt.FORMAT_GEND, mode, covt.PLAN_PROPERTIES, options=opts)
        assert (plan.tile_status == 0).all()
        assert (plan.family_counts[covt.FAMILY_LANE] > 0) == (lane_max_bytes >= 0)
        out, res = plan.decode_host()
        _check_streams(covt, oracle, plan, out, res, tiles, mode)
        buf, pres = plan.properties_host()
        assert _check_props(covt, oracle, plan, buf, pres, tiles, mode) > 50
        # the device path on zeroed buffers: every byte of the property buffer is then defined, padding included
        # (properties_host copies its device buffer back whole, and that buffer starts uninitialised)
        db = covt.DeviceBatch(plan, "cuda")
        db.decode()
        db.materialize_properties()
        torch.cuda.synchronize()
        dbuf, dpres = db.property_results()
        assert dpres.tobytes() == pres.tobytes()
        cols = []
        for k in range(plan.num_property_columns):
            if pres["status"][k] == 0:
                col = plan.property_column(buf, pres, k)
                cols.append(b"|".join(np.ascontiguousarray(x).tobytes() for x in
                                      (col.validity, col.values, col.dict_offsets, col.dict_bytes) if x is not None))
            else:
                cols.append(None)
        got.append((res, pres, cols, dbuf.copy(), plan.props.copy(), _lane_descs(covt, plan)))
    (res, pres, cols, dbuf, props, lanes), (res0, pres0, cols0, dbuf0, props0, _) = got
    assert (lanes["avail"] > 128).any() or (lanes["num_values"] > 256).any()  # the raised property limits in use
    assert np.array_equal(res, res0)
    assert props.tobytes() == props0.tobytes()  # the same buffer layout
    assert pres.tobytes() == pres0.tobytes() and cols == cols0  # every column's bytes
    assert np.array_equal(dbuf, dbuf0)  # and the whole buffer

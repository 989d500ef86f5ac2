"""GPU: the bounding-box pass (covt_bbox.hip, include/covt.h "Geometry bounding boxes") against the
references of tests/covt_bbox.py over the CPU oracle's assembly, byte for byte (the four arrays, the
extent, n_empty), through the C-ABI: covt_geometry_bbox_device on synthetic and hand-made columns,
covt_plan_bbox_host on the fixture tiles (also held against the bounds of the GPU's own WKB), the
DeviceBatch / DevicePlan paths, and a HIP-graph replay.

The kernel's step sizes the boundary cases are built around: a wave chunk of 256 coordinates, feature
steps of 64 lanes, a 512-entry window of feature starts (restaged when fewer than 320 lie ahead), a
workgroup of 4 waves, up to 64 workgroups per column while 8192 / n_columns allows, and a feature that
has 2048 coordinates or more left past its owner's run finished by the whole workgroup.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_bbox as B
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
CHUNK, WAVES, WIN, WIDE = 256, 4, 512, 2048
LO, HI = -(1 << 31), (1 << 31) - 1


def _a16(x):
    return (x + 15) & ~15


def _bbox_layout(covt, cols, bflags=None):
    """Bounding-box descriptors (the plan's layout rule) for pack_columns' columns -> (desc array, bytes)."""
    d = np.zeros(len(cols), dtype=covt.BBOX_DESC_DTYPE)
    off = 0
    for ci, col in enumerate(cols):
        n = col["types"].size
        d[ci]["off"] = off
        d[ci]["n_features"] = n
        d[ci]["flags"] = bflags[ci] if bflags else 0
        off = _a16(off + 32 * n) + 16  # (a gap after every slice: it must stay untouched)
    return d, max(off, 16)


def _run(covt, cols, flags_extra=None, in_res=None, dres=None, bflags=None):
    """covt_assemble_geometry_device + covt_geometry_bbox_device over synthetic columns."""
    import torch

    dec, desc, asm_bytes, lay = A.pack_columns(covt, cols, flags_extra, in_res)
    bd, bbox_bytes = _bbox_layout(covt, cols, bflags)
    dev = torch.device("cuda:0")
    d_dec = torch.from_numpy(dec).to(dev)
    d_desc = torch.from_numpy(desc).to(dev)
    d_bdesc = torch.from_numpy(bd.view(np.uint8).reshape(-1)).to(dev)
    d_asm = torch.full((asm_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_bbox = torch.full((bbox_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_gres = torch.zeros(4 * len(cols), dtype=torch.int32, device=dev)
    d_bres = torch.full((40 * len(cols),), FILL, dtype=torch.uint8, device=dev)
    d_res = torch.from_numpy(np.zeros(2, np.int32) if dres is None else np.asarray(dres, np.int32)).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    L = covt.lib()
    assert L.covt_assemble_geometry_device(d_dec.data_ptr(), d_res.data_ptr(), d_desc.data_ptr(), len(cols),
                                           d_asm.data_ptr(), d_gres.data_ptr(), s) == 0
    assert L.covt_geometry_bbox_device(d_desc.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(), d_bdesc.data_ptr(),
                                       len(cols), d_bbox.data_ptr(), d_bres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    return (d_bbox.cpu().numpy(), d_bres.cpu().numpy().view(covt.BBOX_RESULT_DTYPE),
            d_gres.cpu().numpy().view(covt.GEOM_RESULT_DTYPE), bd)


def _reference(oracle, col, cache=None, plain=True):
    """(status, reference result) over the oracle's assembly (cached per column object)."""
    if cache is not None and id(col) in cache:
        return cache[id(col)]
    o = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"], col["vb"], col["closed"],
                                 col.get("caps") or A.caps(col))
    ref = (o[0], None) if o[0] else (0, (B.bbox_plain if plain else B.bbox_numpy)(*o[1:]))
    if cache is not None:
        cache[id(col)] = ref
    return ref


NAN4 = np.full(4, np.nan).tobytes()


def _check(oracle, cols, buf, bres, bd, cache=None, plain=True):
    """Every column equals the reference as bytes; every byte outside the written slices still holds FILL."""
    written = np.zeros(buf.size, dtype=bool)
    for ci, col in enumerate(cols):
        st, ref = _reference(oracle, col, cache, plain)
        assert int(bres["status"][ci]) == st, (ci, int(bres["status"][ci]), st)
        if st:
            assert int(bres["n_empty"][ci]) == 0 and bres["extent"][ci].tobytes() == NAN4, ci
            continue
        o, n = int(bd["off"][ci]), col["types"].size
        got = buf[o:o + 32 * n].view(np.float64)
        for k, name in enumerate(("xmin", "ymin", "xmax", "ymax")):
            g, w = got[k * n:(k + 1) * n], ref[k]
            if g.tobytes() != w.tobytes():
                bad = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0]
                raise AssertionError("column %d %s: %d of %d rows differ, first %d: %r, want %r"
                                     % (ci, name, bad.size, n, int(bad[0]), g[bad[0]], w[bad[0]]))
        assert bres["extent"][ci].tobytes() == ref[4].tobytes(), (ci, bres["extent"][ci], ref[4])
        assert int(bres["n_empty"][ci]) == ref[5], (ci, int(bres["n_empty"][ci]), ref[5])
        written[o:o + 32 * n] = True
    assert (buf[~written] == FILL).all()


def _lines(lengths, xy):
    """A LINESTRING column: feature f has lengths[f] vertices, xy the (sum, 2) int32 coordinates."""
    xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
    assert xy.shape[0] == sum(lengths)
    return {"types": np.full(len(lengths), 1, np.uint8), "go": np.zeros(0, np.int32), "po": np.asarray(lengths, np.int32),
            "ro": np.zeros(0, np.int32), "vo": None, "vb": xy.reshape(-1), "closed": False}


def _rand_xy(rng, n, lim=1 << 20):
    return rng.integers(-lim, lim, size=(n, 2), dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_synthetic_columns(covt, oracle, gpu_available, seed):
    rng = np.random.default_rng(200 + seed)
    cols = []
    for i in range(32):
        big = i % 8 == 7  # up to 300 parts per feature, 40 rings per polygon, 3000 vertices per ring
        n = int(rng.choice([1, 2, 5])) if big else [0, 1, 5, 63, 64, 65, 200, 1000, 5000][(i + seed) % 9]
        cols.append(A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2), big=big))
    for t in range(6):  # one-type columns: runs of empty parts and rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 1500, bool(t & 1), bool(seed & 1), probs=probs))
    assert all(max(A.caps(c)) <= covt.GEOM_MAX_CAP for c in cols)
    buf, bres, gres, bd = _run(covt, cols)
    assert (gres["status"] == 0).all() and (bres["status"] == 0).all()
    _check(oracle, cols, buf, bres, bd, plain=False)  # (bbox_numpy: the big features; == bbox_plain on the CPU)
    small = [c for c in cols if c["types"].size <= 1000 and c["vb"].size < 40000]
    assert len(small) >= 20
    buf, bres, gres, bd = _run(covt, small)
    _check(oracle, small, buf, bres, bd)


def _boundary_columns(rng):
    cols = []
    steps = (64, WIN - 320, CHUNK, WIN, CHUNK * WAVES, WIDE)  # feature step, restage, chunk, window, workgroup, wide
    for s in steps:
        for n in (s - 1, s, s + 1):
            cols.append(A.synth_column(rng, n, False, False, probs=[1, 0, 0, 0, 0, 0]))  # as many coordinates as features
            cols.append(A.synth_column(rng, n, True, False, probs=[0, 1, 0, 0, 0, 0]))   # chunks inside features
    return cols


def test_step_and_chunk_boundaries(covt, oracle, gpu_available):
    """POINT and LINESTRING columns one below, at and one above every step size of the kernel, and a column
    whose 64 workgroups each take several coordinate chunks."""
    rng = np.random.default_rng(15)
    cols = _boundary_columns(rng)
    cols.append(A.synth_column(rng, 70000, False, False, probs=[0.1, 0.5, 0.4, 0, 0, 0]))  # > 64 * 4 chunks, twice
    buf, bres, gres, bd = _run(covt, cols)
    assert (bres["status"] == 0).all()
    assert int(gres["num_coords"][-1]) > 2 * 64 * WAVES * CHUNK
    cache = {}
    _check(oracle, cols, buf, bres, bd, cache=cache)
    # all of them again, one workgroup per column
    tiny = A.synth_column(rng, 1, False, False)
    cols = cols + [tiny] * (4097 - len(cols))
    buf, bres, gres, bd = _run(covt, cols)
    _check(oracle, cols, buf, bres, bd, cache=cache)


def _long_feature_columns(rng):
    """Features that run on past their owner's run.  A column of 40 chunks in a batch of one workgroup per
    column gives wave 0 the run [0, 2560): its second feature starts at coordinate 10 and ends 2047, 2048 or
    2049 coordinates past the run (the wave finishes it / the workgroup does).  One feature of 300000
    coordinates is longer than three runs of a workgroup however the column is cut, with its minimum in its
    first coordinate and its maximum in its last, and the other way round.  A feature whose extreme is the
    last coordinate of a chunk, and one with it in the first coordinate of the next."""
    cols = []
    total = 40 * CHUNK
    for r in (WIDE - 1, WIDE, WIDE + 1):
        second = 10 * CHUNK - 10 + r
        rest = total - 10 - second
        lengths = [10, second] + [7] * (rest // 7) + ([rest % 7] if rest % 7 else [])
        xy = _rand_xy(rng, total)
        xy[10 + second - 1] = (HI, LO)  # the last coordinate the owner takes
        cols.append(_lines(lengths, xy))
    for swap in (False, True):
        n = 300000
        xy = _rand_xy(rng, 5 + n + 3)
        first, last = (LO, LO), (HI, HI)
        xy[5], xy[5 + n - 1] = (last, first) if swap else (first, last)
        cols.append(_lines([5, n, 3], xy))
    for at in (CHUNK - 1, CHUNK, 3 * CHUNK - 1, 3 * CHUNK):
        xy = _rand_xy(rng, 1000)
        xy[at] = (HI, LO)
        cols.append(_lines([200, 700, 100] if at < 2 * CHUNK else [100, 150, 650, 100], xy))
    return cols


def test_long_features_and_chunk_edges(covt, oracle, gpu_available):
    rng = np.random.default_rng(16)
    cols = _long_feature_columns(rng)
    cache = {}
    buf, bres, gres, bd = _run(covt, cols)  # up to 64 workgroups per column
    assert (bres["status"] == 0).all()
    _check(oracle, cols, buf, bres, bd, cache=cache)
    assert bres["extent"][3].tolist() == [LO, LO, HI, HI]
    tiny = A.synth_column(rng, 1, False, False)
    cols = cols + [tiny] * (4097 - len(cols))  # one workgroup per column: 4 waves, 10 chunks each
    buf, bres, gres, bd = _run(covt, cols)
    _check(oracle, cols, buf, bres, bd, cache=cache)


RUNS = [0, 1, 63, 64, 65, 127, 128, 129, 1000]


def _multipoints(rng, counts):
    """A MULTIPOINT column: feature f has counts[f] points (0: an empty feature)."""
    k = int(sum(counts))
    return {"types": np.full(len(counts), 3, np.uint8), "go": np.asarray(counts, np.int32), "po": np.zeros(0, np.int32),
            "ro": np.zeros(0, np.int32), "vo": None,
            "vb": rng.integers(-(1 << 31), 1 << 31, size=2 * k, dtype=np.int64).astype(np.int32), "closed": False}


def test_runs_of_empty_features(covt, oracle, gpu_available):
    """Runs of empty features at the start, in the middle and at the end of a column, of lengths either side
    of the 64-feature step and far past the window; a column of nothing but empty features."""
    rng = np.random.default_rng(19)
    cols = [_multipoints(rng, [0] * run + [1] * 300 + [0] * run + [2] * 300 + [0] * run) for run in RUNS]
    cols.append(_multipoints(rng, [0] * 700))
    cache = {}
    buf, bres, gres, bd = _run(covt, cols)
    assert (gres["status"] == 0).all() and (bres["status"] == 0).all()
    _check(oracle, cols, buf, bres, bd, cache=cache)
    assert bres["n_empty"].tolist() == [3 * r for r in RUNS] + [700]
    assert bres["extent"][-1].tobytes() == NAN4 and int(gres["num_coords"][-1]) == 0
    tiny = A.synth_column(rng, 1, False, False)
    cols = cols + [tiny] * (4097 - len(cols))  # the same columns, one workgroup each
    buf, bres, gres, bd = _run(covt, cols)
    _check(oracle, cols, buf, bres, bd, cache=cache)


@pytest.mark.parametrize("n_cols", [128, 129, 4096, 4097])
def test_batch_size_switch(covt, oracle, gpu_available, n_cols):
    """Workgroups per column = 8192 / n_columns, between 1 and 64: 64 up to 128 columns, one from 4097 on.
    The same columns either side of both ends."""
    rng = np.random.default_rng(17)
    head = [A.synth_column(rng, 700, True, False), A.synth_column(rng, 257, False, True),
            A.synth_column(rng, 3, False, False, big=True)]
    tiny = [A.synth_column(rng, k, False, False) for k in (0, 1, 3)]
    cols = head + [tiny[i % 3] for i in range(n_cols - len(head))]
    buf, bres, gres, bd = _run(covt, cols)
    assert (bres["status"] == 0).all()
    _check(oracle, cols, buf, bres, bd, cache={}, plain=False)


def test_status_paths(covt, oracle, gpu_available):
    rng = np.random.default_rng(18)
    ok = A.synth_column(rng, 50, False, False)
    cols = [ok, ok, ok, ok, ok]
    #        0: fine   1: source stream failed   2: COVT_GEOM_TOO_LARGE   3: COVT_BBOX_TOO_LARGE   4: fine
    buf, bres, gres, bd = _run(covt, cols, flags_extra=[0, 0, 0x80000000, 0, 0],
                               in_res=[[-1] * 6, [0, -1, -1, -1, -1, 1], [-1] * 6, [-1] * 6, [-1] * 6],
                               dres=[0, 5, covt.ERR_TRUNCATED, 7], bflags=[0, 0, 0, covt.BBOX_TOO_LARGE, 0])
    assert gres["status"].tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_INVALID_ARG, 0, 0]
    assert bres["status"].tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_INVALID_ARG, covt.ERR_INVALID_ARG, 0]
    for ci in (1, 2, 3):  # failed columns: n_empty 0, extent NaN, slice untouched
        o = int(bd["off"][ci])
        assert int(bres["n_empty"][ci]) == 0 and bres["extent"][ci].tobytes() == NAN4, ci
        assert (buf[o:o + 32 * 50 + 16] == FILL).all(), ci
    st, ref = _reference(oracle, ok)
    for ci in (0, 4):  # the good ones are exact
        o = int(bd["off"][ci])
        assert buf[o:o + 32 * 50].tobytes() == b"".join(a.tobytes() for a in ref[:4]), ci
        assert bres["extent"][ci].tobytes() == ref[4].tobytes() and int(bres["n_empty"][ci]) == ref[5]


@pytest.fixture(scope="module")
def fixture_bbox(covt, gpu_available):
    """Plan.bbox_host() and Plan.wkb_host() over every fixture tile, once for the tests below."""
    paths = tile_paths()
    tiles = [open(p, "rb").read() for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    buf, bres = plan.bbox_host()
    return paths, tiles, plan, buf, bres


def test_fixture_tiles_bbox_bitexact(covt, oracle, fixture_bbox):
    paths, tiles, plan, buf, bres = fixture_bbox
    b = plan.bbox
    n_ok = 0
    cache = {}
    for c in range(plan.num_geometry_columns):
        t, L = int(b["tile"][c]), int(b["layer"][c])
        if t not in cache:
            cache[t] = A.oracle_tile_columns(oracle, tiles[t])
        oc = cache[t][L]
        st = int(bres["status"][c])
        if oc["asm"] is None:  # a source stream failed to decode (SURVEY Q4 tiles)
            assert st != 0 and int(bres["n_empty"][c]) == 0 and bres["extent"][c].tobytes() == NAN4
            continue
        assert st == oc["asm"][0] == 0, (tile_key(paths[t]), L, st)
        ref = B.bbox_plain(*oc["asm"][1:])
        col = plan.bbox_column(buf, bres, c)
        assert len(col) == oc["types"].size
        got = (col.xmin, col.ymin, col.xmax, col.ymax, col.extent, col.n_empty)
        assert B.same(got, ref), (tile_key(paths[t]), L)
        n_ok += 1
    assert n_ok >= 700


def test_fixture_tiles_bbox_equals_bounds_of_gpu_wkb(covt, fixture_bbox):
    """Two products agree: every box is the bounds of the WKB value the WKB pass wrote for the feature."""
    paths, tiles, plan, buf, bres = fixture_bbox
    wbuf, wres = plan.wkb_host()
    assert np.array_equal(bres["status"] == 0, wres["status"] == 0)
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(bres["status"][c]):
            continue
        w = plan.wkb_column(wbuf, wres, c)
        col = plan.bbox_column(buf, bres, c)
        got = (col.xmin, col.ymin, col.xmax, col.ymax, col.extent, col.n_empty)
        assert B.same(got, B.wkb_column_bounds(w.offsets, w.data)), c
        n_ok += 1
    assert n_ok >= 700


def _same_slices(plan, bres, x, y):
    """The columns' slices of two bounding-box buffers hold the same bytes (the gaps are alignment only)."""
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(bres["status"][c]) == 0:
            o, n = int(plan.bbox["off"][c]), int(plan.bbox["n_features"][c])
            assert x[o:o + 32 * n].tobytes() == y[o:o + 32 * n].tobytes(), c
            n_ok += 1
    return n_ok


def test_device_paths_match_host_path(covt, gpu_available):
    import torch

    tiles = [open(p, "rb").read() for p in tile_paths(("omt",))[:30]]
    plan = covt.Plan.from_tiles(tiles)
    buf_h, bres_h = plan.bbox_host()
    assert (bres_h["status"] == 0).any()
    b = covt.DeviceBatch(plan, "cuda:0")
    b.decode()
    b.assemble()
    b.bbox()
    torch.cuda.synchronize()
    buf_d, bres_d = b.bbox_results()
    assert bres_h.tobytes() == bres_d.tobytes()
    assert _same_slices(plan, bres_h, buf_h, buf_d) > 0
    # the device plan: the same records and descriptors, the same bytes
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    bi, bdd = dp.bbox_copy()
    assert bi.tobytes() == plan.bbox.tobytes() and bdd.tobytes() == plan.bdescs.tobytes()
    assert dp.bbox_bytes == plan.bbox_bytes
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_bbox, d_bres = dp.alloc_bbox()
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.bbox(d_asm, d_gres, d_bbox, d_bres)
    torch.cuda.synchronize()
    bres_p = d_bres.cpu().numpy().view(covt.BBOX_RESULT_DTYPE)[:plan.num_geometry_columns][plan.bbox["desc_index"]]
    assert bres_h.tobytes() == bres_p.tobytes()
    _same_slices(plan, bres_h, buf_h, d_bbox.cpu().numpy()[:plan.bbox_bytes])


def test_decode_covt_yields_bbox_per_layer(covt, oracle, gpu_available, decodable_tiles):
    """CovtParser.decode_covt gives every layer its bounding boxes beside its WKB column."""
    tile = decodable_tiles[0][1]
    layers = covt.CovtParser.decode_covt(tile)
    cols = A.oracle_tile_columns(oracle, tile)
    assert layers and all(lc.bbox is not None for lc in layers if lc.geometry.geometryTypes is not None)
    for lc in layers:
        oc = cols[lc.layer]
        assert len(lc.bbox) == len(lc.wkb) == oc["types"].size
        got = (lc.bbox.xmin, lc.bbox.ymin, lc.bbox.xmax, lc.bbox.ymax, lc.bbox.extent, lc.bbox.n_empty)
        assert B.same(got, B.bbox_plain(*oc["asm"][1:])), lc.layer
        assert B.same(got, B.wkb_column_bounds(lc.wkb.offsets, lc.wkb.data)), lc.layer
        assert lc.bbox.as_struct().shape == (len(lc.bbox), 4)


def test_decode_assemble_bbox_replay_in_a_hip_graph(covt, gpu_available, decodable_tiles):
    """decode + assemble + bbox of a small batch captured in one HIP graph and replayed three times into
    poisoned buffers: the bytes of the eager run each time (the pass holds no scratch and writes every
    double once; the assembly's scratch needs the warm-up launch on the capture stream before the capture)."""
    import torch

    tiles = [t for _, t in decodable_tiles]  # (the batch of test_gpu_parity.py::test_graph_replay_equals_launch)
    plan = covt.Plan.from_tiles(tiles)
    buf_h, bres_h = plan.bbox_host()
    assert (bres_h["status"] == 0).all()
    dev = torch.device("cuda:0")
    b = covt.DeviceBatch(plan, dev)
    s = torch.cuda.Stream(dev)

    def launch():
        b.decode(s)
        b.assemble(s)
        b.bbox(s)

    with torch.cuda.stream(s):
        launch()  # fork streams, events and the assembly scratch exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for _ in range(3):
        b.d_bbox.fill_(FILL)
        b.d_bres.fill_(0x5A5A5A5A5A5A5A5A)
        b.d_asm.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        buf, bres = b.bbox_results()
        assert bres.tobytes() == bres_h.tobytes()
        assert _same_slices(plan, bres_h, buf_h, buf) == plan.num_geometry_columns
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


# ---- GpuCovtBatch.bboxBytes / bboxColumns / geometryBbox through the JNI shim and a fake VM --------------
@pytest.fixture(scope="module")
def bbox_shim(covt):
    """tests/jni_bbox/jni_bbox_test: the shim compiled against the stand-in tests/jni/jni.h with the
    compiler line of tests/jni/Makefile."""
    import os
    import subprocess

    from conftest import ROOT

    covt.lib()
    src = os.path.join(ROOT, "tests", "jni_bbox", "jni_bbox_test.cc")
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


JNI_KEYS = ["omt/5_16_20", "omt/14_8298_10748", "bing/4-8-5"]


def _jni_case(mode):
    import os

    from conftest import ROOT

    tiles = [open(os.path.join(ROOT, "tests", "golden", "tiles", k + ".covt"), "rb").read() for k in JNI_KEYS]
    return tiles, mode + " " + " ".join(str(len(t)) for t in tiles) + " | " + b"".join(tiles).hex()


def test_geometry_bbox_through_jni(bbox_shim, covt, gpu_available):
    """geometryBbox into a direct buffer: the (status, n_empty, extent bits) rows, the BBOX_FIELDS rows and
    the buffer equal Plan.bbox_host()'s."""
    tiles, case = _jni_case("bbox")
    kind, nb, cols_hex, res_hex, out_hex = _shim_run(bbox_shim, case)
    plan = covt.Plan.from_tiles(tiles)
    buf, bres = plan.bbox_host()
    assert kind == "ok" and int(nb) == plan.bbox_bytes
    rows = np.frombuffer(bytes.fromhex(cols_hex), "<i8").reshape(-1, 5)
    b = plan.bbox
    want = np.stack([b[f].astype(np.int64) for f in ("tile", "layer", "n_features", "desc_index", "off")], axis=1)
    assert np.array_equal(rows, want)
    res = np.frombuffer(bytes.fromhex(res_hex), "<i8").reshape(-1, 6)
    assert np.array_equal(res[:, 0], bres["status"]) and np.array_equal(res[:, 1], bres["n_empty"])
    assert res[:, 2:].tobytes() == np.ascontiguousarray(bres["extent"]).tobytes()  # (the doubles' bits)
    jout = np.frombuffer(bytes.fromhex(out_hex), np.uint8)
    assert _same_slices(plan, bres, buf, jout) >= 10


@pytest.mark.parametrize("mode", ["short", "heap"])
def test_geometry_bbox_jni_rejects_bad_buffers(bbox_shim, gpu_available, mode):
    """A buffer one byte short of bboxBytes(), or one that is not direct: IllegalArgumentException."""
    _, case = _jni_case(mode)
    assert _shim_run(bbox_shim, case) == ["exc", "java/lang/IllegalArgumentException"]

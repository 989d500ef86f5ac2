"""GPU: the WKB serialization (covt_wkb.hip, include/covt.h "Geometry as WKB") against the reference
writers of tests/covt_wkb.py over the CPU oracle's assembly, byte for byte (offsets, bytes, results),
through the C-ABI: covt_geometry_wkb_device on synthetic columns, covt_plan_wkb_host on the fixture
tiles, the DeviceBatch / DevicePlan paths, and a HIP-graph replay.
"""
import numpy as np
import pytest

import covt_asm as A
import covt_wkb as W
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A


def _a16(x):
    return (x + 15) & ~15


def _cap(col):
    pcap, rcap, ccap = col.get("caps") or A.caps(col)
    return 9 * (col["types"].size + pcap) + 4 * rcap + 16 * ccap


def _wkb_layout(covt, cols, cap_delta=None, wflags=None):
    """WKB descriptors (the plan's layout rule) for pack_columns' columns -> (desc array, buffer bytes)."""
    d = np.zeros(len(cols), dtype=covt.WKB_DESC_DTYPE)
    off = 0
    for ci, col in enumerate(cols):
        n = col["types"].size
        d[ci]["offsets_off"] = off
        off = _a16(off + 4 * (n + 1))
        d[ci]["bytes_off"] = off
        d[ci]["byte_cap"] = _cap(col) + (cap_delta[ci] if cap_delta else 0)
        off = _a16(off + _cap(col))
        d[ci]["n_features"] = n
        d[ci]["flags"] = wflags[ci] if wflags else 0
    return d, max(off, 16)


def _run(covt, cols, flags_extra=None, in_res=None, dres=None, cap_delta=None, wflags=None):
    """covt_assemble_geometry_device + covt_geometry_wkb_device over synthetic columns."""
    import torch

    dec, desc, asm_bytes, lay = A.pack_columns(covt, cols, flags_extra, in_res)
    wd, wkb_bytes = _wkb_layout(covt, cols, cap_delta, wflags)
    dev = torch.device("cuda:0")
    d_dec = torch.from_numpy(dec).to(dev)
    d_desc = torch.from_numpy(desc).to(dev)
    d_wdesc = torch.from_numpy(wd.view(np.uint8).reshape(-1)).to(dev)
    d_asm = torch.full((asm_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_wkb = torch.full((wkb_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_gres = torch.zeros(4 * len(cols), dtype=torch.int32, device=dev)
    d_wres = torch.full((2 * len(cols),), -1, dtype=torch.int64, device=dev)
    d_res = torch.from_numpy(np.zeros(2, np.int32) if dres is None else np.asarray(dres, np.int32)).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    L = covt.lib()
    assert L.covt_assemble_geometry_device(d_dec.data_ptr(), d_res.data_ptr(), d_desc.data_ptr(), len(cols),
                                           d_asm.data_ptr(), d_gres.data_ptr(), s) == 0
    assert L.covt_geometry_wkb_device(d_dec.data_ptr(), d_desc.data_ptr(), d_asm.data_ptr(), d_gres.data_ptr(),
                                      d_wdesc.data_ptr(), len(cols), d_wkb.data_ptr(), d_wres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    return (d_wkb.cpu().numpy(), d_wres.cpu().numpy().view(covt.WKB_RESULT_DTYPE),
            d_gres.cpu().numpy().view(covt.GEOM_RESULT_DTYPE), wd)


def _reference(oracle, col, cache=None):
    """(status, offsets, bytes) of the plain writer over the oracle's assembly (cached per column object)."""
    if cache is not None and id(col) in cache:
        return cache[id(col)]
    o = oracle.assemble_geometry(col["types"], col["go"], col["po"], col["ro"], col["vo"], col["vb"], col["closed"],
                                 col.get("caps") or A.caps(col))
    ref = (o[0], None, None) if o[0] else (0,) + W.write_plain(col["types"], *o[1:])
    if cache is not None:
        cache[id(col)] = ref
    return ref


def _check(oracle, cols, buf, wres, wd, cache=None):
    """Every column equals the reference; every byte outside the written ranges still holds FILL."""
    written = np.zeros(buf.size, dtype=bool)
    for ci, col in enumerate(cols):
        st, offs, data = _reference(oracle, col, cache)
        assert int(wres["status"][ci]) == st, (ci, int(wres["status"][ci]), st)
        if st:
            assert int(wres["n_bytes"][ci]) == 0, ci
            continue
        oo, bo, n = int(wd["offsets_off"][ci]), int(wd["bytes_off"][ci]), col["types"].size
        assert int(wres["n_bytes"][ci]) == len(data) == int(offs[-1]), (ci, int(wres["n_bytes"][ci]), len(data))
        assert np.array_equal(buf[oo:oo + 4 * (n + 1)].view(np.int32), offs), ci
        got = buf[bo:bo + len(data)]
        if got.tobytes() != data:
            bad = np.nonzero(got != np.frombuffer(data, np.uint8))[0]
            raise AssertionError("column %d: %d bytes differ, first at %d" % (ci, bad.size, int(bad[0])))
        written[oo:oo + 4 * (n + 1)] = True
        written[bo:bo + len(data)] = True
    assert (buf[~written] == FILL).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_synthetic_columns(covt, oracle, gpu_available, seed):
    rng = np.random.default_rng(100 + seed)
    cols = []
    for i in range(32):
        big = i % 8 == 7  # up to 300 parts per feature, 40 rings per polygon, 3000 vertices per ring
        n = int(rng.choice([1, 2, 5])) if big else [0, 1, 5, 63, 64, 65, 200, 1000, 5000][(i + seed) % 9]
        cols.append(A.synth_column(rng, n, ice=bool(i & 1), closed=bool(i & 2), big=big))
    for t in range(6):  # one-type columns: runs of empty parts and rings, 1-vertex rings
        probs = [0.0] * 6
        probs[t] = 1.0
        cols.append(A.synth_column(rng, 1500, bool(t & 1), bool(seed & 1), probs=probs))
    assert all(max(A.caps(c)) <= covt.GEOM_MAX_CAP and _cap(c) < 1 << 31 for c in cols)
    buf, wres, gres, wd = _run(covt, cols)
    assert (gres["status"] == 0).all() and (wres["status"] == 0).all() and (wres["reserved"] == 0).all()
    _check(oracle, cols, buf, wres, wd)


def test_step_and_chunk_boundaries(covt, oracle, gpu_available):
    """Columns just under, at and just over the sizes at which the kernels take another step: the write
    chunk of 256 items and the wave scan's 256-feature step, the cooperative scan's 4096-feature step
    (POINT columns: as many coordinates as features; LINESTRING columns: coordinate chunks inside
    features), and a column whose 64 workgroups each take several coordinate chunks."""
    rng = np.random.default_rng(5)
    cols = []
    for n in (255, 256, 257, 4095, 4096, 4097):
        cols.append(A.synth_column(rng, n, False, False, probs=[1, 0, 0, 0, 0, 0]))
        cols.append(A.synth_column(rng, n, True, False, probs=[0, 1, 0, 0, 0, 0]))
    cols.append(A.synth_column(rng, 70000, False, False, probs=[0.1, 0.5, 0.4, 0, 0, 0]))  # > 64 * 4 chunks
    buf, wres, gres, wd = _run(covt, cols)
    assert (wres["status"] == 0).all()
    assert int(gres["num_coords"][-1]) > 2 * 64 * 4 * 256
    _check(oracle, cols, buf, wres, wd)


RUNS = [0, 1, 126, 127, 128, 129, 130, 382, 383, 384, 385, 386, 1000]


def _empty_run_columns(rng):
    """Columns whose offsets hold long runs of empty segments at one level each -- empty MULTIPOINT
    features, MULTIPOLYGON parts without rings, polygon rings without vertices -- with 300 one-item
    segments between the runs.  The write kernel stages 384 offsets of a level per 256-item chunk and
    searches global memory when a chunk's segments pass that window: run lengths either side of 128
    (window less chunk) and of 384, and far past both."""
    def vb(n):
        return rng.integers(-(1 << 31), 1 << 31, size=2 * n, dtype=np.int64).astype(np.int32)

    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    pat = []
    for run in RUNS:
        pat += [1] * 300 + [0] * run
    pat += [1] * 5
    k = len(pat)
    # features level: MULTIPOINTs of one point or none
    a = {"types": np.full(k, 3, np.uint8), "go": i32(pat), "po": i32([]), "ro": i32([]), "vo": None,
         "vb": vb(sum(pat)), "closed": False}
    # parts level: MULTIPOLYGONs of 60 parts, a part one triangle ring or no ring
    nf = (k + 59) // 60
    parts = pat + [1] * (nf * 60 - k)
    b = {"types": np.full(nf, 5, np.uint8), "go": i32([60] * nf), "po": i32(parts), "ro": i32([3] * sum(parts)),
         "vo": None, "vb": vb(3 * sum(parts)), "closed": False}
    # rings level: POLYGONs of 45 rings, a ring two vertices (closed: three) or none
    nf = (k + 44) // 45
    rings = pat + [1] * (nf * 45 - k)
    c = {"types": np.full(nf, 2, np.uint8), "go": i32([]), "po": i32([45] * nf), "ro": i32([2 * x for x in rings]),
         "vo": None, "vb": vb(2 * sum(rings)), "closed": False}
    return [a, b, c]


def test_long_runs_of_empty_segments(covt, oracle, gpu_available):
    rng = np.random.default_rng(9)
    cols = _empty_run_columns(rng)
    buf, wres, gres, wd = _run(covt, cols)
    assert (gres["status"] == 0).all() and (wres["status"] == 0).all()
    assert int(gres["num_parts"][1]) - int(gres["num_rings"][1]) == sum(RUNS)  # the empty parts are there
    _check(oracle, cols, buf, wres, wd)
    # the same columns in a large batch (one workgroup per column, each wave a longer run of chunks)
    tiny = A.synth_column(rng, 1, False, False)
    cols = cols + [tiny] * 4094
    buf, wres, gres, wd = _run(covt, cols)
    assert (wres["status"] == 0).all()
    _check(oracle, cols, buf, wres, wd, cache={})


@pytest.mark.parametrize("n_cols", [4096, 4097])
def test_batch_size_threshold(covt, oracle, gpu_available, n_cols):
    """At most 4096 columns: a workgroup per column scans, several workgroups write; more: a wave per
    column scans and one workgroup writes.  The same columns either side of the threshold."""
    rng = np.random.default_rng(6)
    head = [A.synth_column(rng, 700, True, False), A.synth_column(rng, 257, False, True),
            A.synth_column(rng, 3, False, False, big=True)]
    tiny = [A.synth_column(rng, k, False, False) for k in (0, 1, 3)]
    cols = head + [tiny[i % 3] for i in range(n_cols - len(head))]
    buf, wres, gres, wd = _run(covt, cols)
    assert (wres["status"] == 0).all()
    _check(oracle, cols, buf, wres, wd, cache={})


def test_status_paths(covt, oracle, gpu_available):
    rng = np.random.default_rng(7)
    ok = A.synth_column(rng, 50, False, False)
    poly = A.synth_column(rng, 300, True, False, probs=[0, 0, 0.5, 0, 0, 0.5])
    cols = [ok, ok, ok, ok, poly, ok, ok]
    #        0: fine   1: source stream failed   2: COVT_GEOM_TOO_LARGE   3: COVT_WKB_TOO_LARGE
    #        4: byte_cap one byte short (total known after the scan)   5: fine   6: byte_cap over INT32_MAX
    st, offs, data = _reference(oracle, poly)
    short = len(data) - 1 - _cap(poly)
    buf, wres, gres, wd = _run(covt, cols, flags_extra=[0, 0, 0x80000000, 0, 0, 0, 0],
                               in_res=[[-1] * 6, [0, -1, -1, -1, -1, 1], [-1] * 6, [-1] * 6, [-1] * 6, [-1] * 6,
                                       [-1] * 6],
                               dres=[0, 5, covt.ERR_TRUNCATED, 7], cap_delta=[0, 0, 0, 0, short, 0, 1 << 31],
                               wflags=[0, 0, 0, covt.WKB_TOO_LARGE, 0, 0, 0])
    assert gres["status"].tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_INVALID_ARG, 0, 0, 0, 0]
    assert wres["status"].tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_INVALID_ARG, covt.ERR_INVALID_ARG,
                                       covt.ERR_COUNT_MISMATCH, 0, covt.ERR_INVALID_ARG]
    assert wres["n_bytes"].tolist()[1:5] == [0, 0, 0, 0] and int(wres["n_bytes"][6]) == 0
    # failed columns: slices untouched (the short one: its offsets may be written, never its bytes)
    for ci in (1, 2, 3, 6):
        oo, n = int(wd["offsets_off"][ci]), cols[ci]["types"].size
        assert (buf[oo:oo + 4 * (n + 1)] == FILL).all(), ci
    for ci in (1, 2, 3, 4, 6):
        bo = int(wd["bytes_off"][ci])
        assert (buf[bo:bo + _a16(_cap(cols[ci]))] == FILL).all(), ci
    # the good ones are exact, and one more byte of capacity is enough
    for ci in (0, 5):
        oo, bo = int(wd["offsets_off"][ci]), int(wd["bytes_off"][ci])
        _, o2, d2 = _reference(oracle, ok)
        assert np.array_equal(buf[oo:oo + 4 * 51].view(np.int32), o2) and buf[bo:bo + len(d2)].tobytes() == d2
    buf, wres, gres, wd = _run(covt, [poly], cap_delta=[short + 1])
    assert wres["status"].tolist() == [0] and int(wres["n_bytes"][0]) == len(data) == int(wd["byte_cap"][0])
    bo = int(wd["bytes_off"][0])
    assert buf[bo:bo + len(data)].tobytes() == data and (buf[bo + len(data):] == FILL).all()


@pytest.fixture(scope="module")
def fixture_wkb(covt, gpu_available):
    """Plan.wkb_host() over every fixture tile, once for the tests below."""
    paths = tile_paths()
    tiles = [open(p, "rb").read() for p in paths]
    plan = covt.Plan.from_tiles(tiles)
    buf, wres = plan.wkb_host()
    return paths, tiles, plan, buf, wres


def test_fixture_tiles_wkb_bitexact(covt, oracle, fixture_wkb):
    paths, tiles, plan, buf, wres = fixture_wkb
    w = plan.wkb
    n_ok = 0
    cache = {}
    for c in range(plan.num_geometry_columns):
        t, L = int(w["tile"][c]), int(w["layer"][c])
        if t not in cache:
            cache[t] = A.oracle_tile_columns(oracle, tiles[t])
        oc = cache[t][L]
        st = int(wres["status"][c])
        if oc["asm"] is None:  # a source stream failed to decode (SURVEY Q4 tiles)
            assert st != 0 and int(wres["n_bytes"][c]) == 0, (tile_key(paths[t]), L)
            continue
        assert st == oc["asm"][0] == 0, (tile_key(paths[t]), L, st)
        offs, data = W.write_numpy(oc["types"], *oc["asm"][1:])
        col = plan.wkb_column(buf, wres, c)
        assert len(col) == oc["types"].size and int(wres["n_bytes"][c]) == data.size
        assert np.array_equal(col.offsets, offs), (tile_key(paths[t]), L)
        assert np.array_equal(col.data, data), (tile_key(paths[t]), L)
        n_ok += 1
    assert n_ok >= 700


def test_fixture_tiles_parse_back(covt, oracle, fixture_wkb):
    """The README claim: the WKB values of a layer parse back into exactly the oracle's geometry."""
    paths, tiles, plan, buf, wres = fixture_wkb
    w = plan.wkb
    picks = [paths.index(tile_paths((s,))[0]) for s in ("omt", "bing", "amazon")]
    n = 0
    for c in range(plan.num_geometry_columns):
        t = int(w["tile"][c])
        if t not in picks or int(wres["status"][c]) != 0:
            continue
        oc = A.oracle_tile_columns(oracle, tiles[t])[int(w["layer"][c])]
        col = plan.wkb_column(buf, wres, c)
        feats = [W.parse(col.feature(i), unclose=True) for i in range(len(col))]
        assert feats == A.to_features(oc["types"], *oc["asm"][1:]), (tile_key(paths[t]), int(w["layer"][c]))
        n += 1
    assert n >= 3


def test_device_paths_match_host_path(covt, gpu_available):
    import torch

    tiles = [open(p, "rb").read() for p in tile_paths(("omt",))[:30]]
    plan = covt.Plan.from_tiles(tiles)
    buf_h, wres_h = plan.wkb_host()
    assert (wres_h["status"] == 0).any()
    b = covt.DeviceBatch(plan, "cuda:0")
    b.decode()
    b.assemble()
    b.wkb()
    torch.cuda.synchronize()
    buf_d, wres_d = b.wkb_results()
    assert np.array_equal(wres_h, wres_d)

    def same(buf, wres):
        for c in range(plan.num_geometry_columns):
            if int(wres_h["status"][c]):
                continue
            x, y = plan.wkb_column(buf_h, wres_h, c), plan.wkb_column(buf, wres, c)
            assert np.array_equal(x.offsets, y.offsets) and np.array_equal(x.data, y.data), c

    same(buf_d, wres_d)
    # the device plan: the same records and descriptors, the same bytes
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64))
    wi, wdd = dp.wkb_copy()
    assert wi.tobytes() == plan.wkb.tobytes() and wdd.tobytes() == plan.wdescs.tobytes()
    assert dp.wkb_bytes == plan.wkb_bytes
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_wkb, d_wres = dp.alloc_wkb()
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.wkb(d_out, d_res, d_asm, d_gres, d_wkb, d_wres)
    torch.cuda.synchronize()
    wres_p = d_wres.cpu().numpy().view(covt.WKB_RESULT_DTYPE)[:plan.num_geometry_columns][plan.wkb["desc_index"]]
    assert np.array_equal(wres_h, wres_p)
    same(d_wkb.cpu().numpy()[:plan.wkb_bytes], wres_p)


def test_decode_covt_yields_wkb_per_layer(covt, oracle, gpu_available, decodable_tiles):
    """The README example: CovtParser.decode_covt gives every layer its WKB column, and the parser turns it
    back into the oracle's geometry."""
    tile = decodable_tiles[0][1]
    layers = covt.CovtParser.decode_covt(tile)
    cols = A.oracle_tile_columns(oracle, tile)
    assert layers and all(lc.wkb is not None for lc in layers if lc.geometry.geometryTypes is not None)
    for lc in layers:
        oc = cols[lc.layer]
        assert len(lc.wkb) == oc["types"].size
        feats = W.parse_column(lc.wkb.offsets, lc.wkb.data, unclose=True)
        assert feats == A.to_features(oc["types"], *oc["asm"][1:]), lc.layer


def test_decode_assemble_wkb_replay_in_a_hip_graph(covt, gpu_available, decodable_tiles):
    """decode + assemble + wkb of a small batch captured in one HIP graph and replayed twice into poisoned
    buffers: the bytes of the eager run each time (the WKB pass holds no scratch; the assembly's needs the
    warm-up launch on the capture stream before the capture)."""
    import torch

    tiles = [t for _, t in decodable_tiles]  # (the batch of test_gpu_parity.py::test_graph_replay_equals_launch)
    plan = covt.Plan.from_tiles(tiles)
    assert plan.num_geometry_columns <= 4096  # a small batch: cooperative scans, several workgroups per column
    buf_h, wres_h = plan.wkb_host()
    assert (wres_h["status"] == 0).all()
    dev = torch.device("cuda:0")
    b = covt.DeviceBatch(plan, dev)
    s = torch.cuda.Stream(dev)

    def launch():
        b.decode(s)
        b.assemble(s)
        b.wkb(s)

    with torch.cuda.stream(s):
        launch()  # fork streams, events and the assembly scratch exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for _ in range(2):
        b.d_wkb.fill_(FILL)
        b.d_wres.zero_()
        b.d_asm.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        buf, wres = b.wkb_results()
        assert np.array_equal(wres, wres_h)
        for c in range(plan.num_geometry_columns):
            if int(wres_h["status"][c]) == 0:
                x, y = plan.wkb_column(buf_h, wres_h, c), plan.wkb_column(buf, wres, c)
                assert np.array_equal(x.offsets, y.offsets) and np.array_equal(x.data, y.data), c
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


# ---- GpuCovtBatch.wkbBytes / wkbColumns / geometryWkb through the JNI shim and a fake VM -----------------
@pytest.fixture(scope="module")
def wkb_shim(covt):
    """tests/jni_wkb/jni_wkb_test: the shim compiled against the stand-in tests/jni/jni.h with the
    compiler line of tests/jni/Makefile."""
    import os
    import subprocess

    from conftest import ROOT

    covt.lib()
    src = os.path.join(ROOT, "tests", "jni_wkb", "jni_wkb_test.cc")
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


def test_geometry_wkb_through_jni(wkb_shim, covt, gpu_available):
    """geometryWkb into a direct buffer: the (status, n_bytes) rows, the WKB_FIELDS rows and every
    column's offsets and bytes equal Plan.wkb_host()'s."""
    tiles, case = _jni_case("wkb")
    kind, nb, cols_hex, res_hex, out_hex = _shim_run(wkb_shim, case)
    plan = covt.Plan.from_tiles(tiles)
    buf, wres = plan.wkb_host()
    assert kind == "ok" and int(nb) == plan.wkb_bytes
    rows = np.frombuffer(bytes.fromhex(cols_hex), "<i8").reshape(-1, 7)
    w = plan.wkb
    want = np.stack([w[f].astype(np.int64) for f in ("tile", "layer", "n_features", "desc_index", "offsets_off",
                                                     "bytes_off", "byte_cap")], axis=1)
    assert np.array_equal(rows, want)
    res = np.frombuffer(bytes.fromhex(res_hex), "<i8").reshape(-1, 2)
    assert np.array_equal(res[:, 0], wres["status"]) and np.array_equal(res[:, 1], wres["n_bytes"])
    jout = np.frombuffer(bytes.fromhex(out_hex), np.uint8)
    n_ok = 0
    for c in range(plan.num_geometry_columns):
        if int(wres["status"][c]):
            continue
        x = plan.wkb_column(buf, wres, c)
        y = plan.wkb_column(jout, wres, c)
        assert np.array_equal(x.offsets, y.offsets) and np.array_equal(x.data, y.data), c
        n_ok += 1
    assert n_ok >= 10


@pytest.mark.parametrize("mode", ["short", "heap"])
def test_geometry_wkb_jni_rejects_bad_buffers(wkb_shim, gpu_available, mode):
    """A buffer one byte short of wkbBytes(), or one that is not direct: IllegalArgumentException."""
    _, case = _jni_case(mode)
    assert _shim_run(wkb_shim, case) == ["exc", "java/lang/IllegalArgumentException"]

"""The container grammars of cov-tiles_amd/csrc/covt_container.h -- the one walk_genc and the one walk_gend
that the host plan and the device plan's serial walkers (wave layout, lane layout, property walk) instantiate
-- compiled by g++ without HIP and run on the CPU against the oracle.

tests/container_walk/container_walk_check.cc is built with AddressSanitizer and UndefinedBehaviorSanitizer
(a stand-alone program, as tests/test_split_plan.py::test_split_contract_under_sanitizers).  It serves every
tile from a heap copy of exactly the tile's size, returns poison for bytes past the end, walks every tile
with two poison patterns, 32- and 64-bit cursors, visitors taking streams, properties or both, and a table
that keeps or re-reads the geometry streams, and aborts unless all of them give the same records."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import covt_gend_rt as RT
from conftest import GOLDEN, ROOT, tile_key, tile_paths

STREAM_FIELDS = ("layer", "column_kind", "stream_type", "encoding", "column_type", "num_values", "byte_length",
                 "num_bits", "offset")


def malformed_corpus(decodable_tiles):
    """test_gpu_device_plan.py::test_malformed_tiles' corpus (Gen C) over 60 base tiles: 184 tiles."""
    rng = np.random.default_rng(11)
    tiles = [b"", b"\x01", b"\x01\x05garbage", bytes(rng.integers(0, 256, 500).astype(np.uint8))]
    for _, t in decodable_tiles[:60]:
        tiles.append(t[:int(rng.integers(1, len(t)))])
        b = bytearray(t)
        for _ in range(3):  # flips in the first 256 bytes: mostly metadata
            b[int(rng.integers(0, min(256, len(b))))] ^= 1 << int(rng.integers(0, 8))
        tiles.append(bytes(b))
        tiles.append(t)
    return tiles


def _prop_row(p):
    return ([p.layer, p.column, p.type, p.column_type, p.n_features, p.lang, p.name_len, p.lang_len, p.name_off,
             p.lang_off] + list(p.s_off) + list(p.s_nv) + list(p.s_bl) + list(p.s_enc))


@pytest.fixture(scope="module")
def walked(tmp_path_factory, decodable_tiles):
    """Every tile of this module through the check program, once: {group: [(tile, status, layers, streams,
    props)]} with the records as lists of ints."""
    d = tmp_path_factory.mktemp("container_walk")
    exe = str(d / "container_walk_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cov-tiles_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "container_walk", "container_walk_check.cc")])
    groups = {
        "genc": [(0, open(p, "rb").read()) for p in tile_paths()],
        "gend_named": [(1, RT.genc_to_gend(t, optimized=False)[0]) for _, t in decodable_tiles[::3]],
        "gend_optimized": [(1, RT.genc_to_gend(t, optimized=True)[0]) for _, t in decodable_tiles[::3]],
        "malformed": [(0, t) for t in malformed_corpus(decodable_tiles)],
    }
    flat = [x for g in groups.values() for x in g]
    path = str(d / "tiles.bin")
    with open(path, "wb") as f:
        for fmt, t in flat:
            f.write(struct.pack("<iq", fmt, len(t)))
            f.write(t)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
    lines = p.stdout.splitlines()
    assert lines[-1].split()[:2] == ["ok", str(len(flat))], lines[-1]
    res, cur = [], None
    for ln in lines[:-1]:
        w = ln.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "t":
            cur = {"status": v[1], "n": v[2:5], "l": [], "s": [], "p": []}
            res.append(cur)
        else:
            cur[w[0]].append(v)
    assert len(res) == len(flat) and all(r["n"] == [len(r["s"]), len(r["p"]), len(r["l"])] for r in res)
    out, k = {}, 0
    for name, g in groups.items():
        out[name] = [(t, res[k + i]) for i, (_, t) in enumerate(g)]
        k += len(g)
    return out


def _oracle_rows(ss):
    return [[getattr(s, f) for f in STREAM_FIELDS] for s in ss]


def _assert_layers(oracle_streams, r):
    """every layer's extent and feature count as the oracle's streams of that layer state them"""
    for s in oracle_streams:
        assert r["l"][s.layer] == [s.extent, s.num_features]


def test_genc_streams_equal_golden_records(walked, golden_streams):
    """All 129 fixtures: the status and every stream's nine fields as tests/golden/oracle_streams.json has them."""
    n = 0
    for path, (t, r) in zip(tile_paths(), walked["genc"]):
        rec = golden_streams["tiles"][tile_key(path)]
        assert r["status"] == rec["walk_status"] == 0, path
        assert r["s"] == [row[:9] for row in rec["streams"]], path
        n += len(r["s"])
    assert len(walked["genc"]) == 129 and n == 6464


@pytest.mark.parametrize("group", ["gend_named", "gend_optimized"])
def test_gend_streams_equal_oracle(walked, oracle, group):
    """Gen D conversions of every third decodable fixture: status and records as oracle.walk_tile's."""
    n = 0
    for t, r in walked[group]:
        st, ss = oracle.walk_tile(t, oracle.FMT_GEND)
        assert st == 0 and r["status"] == 0
        assert r["s"] == _oracle_rows(ss)
        _assert_layers(ss, r)
        n += len(ss)
    assert len(walked[group]) == 42 and n > 0


def test_property_records_equal_oracle(walked, oracle):
    """Both formats: every PropRaw field as oracle.walk_properties' (localized string sub-columns among them)."""
    n_lang, n = 0, {}
    for group, fmt in (("genc", oracle.FMT_GENC), ("gend_named", oracle.FMT_GEND), ("gend_optimized", oracle.FMT_GEND)):
        n[group] = 0
        for t, r in walked[group]:
            st, ps = oracle.walk_properties(t, fmt)
            assert st == 0 and r["status"] == 0
            assert r["p"] == [_prop_row(p) for p in ps]
            n[group] += len(ps)
            n_lang += sum(1 for p in r["p"] if p[5] >= 0)
    assert all(v > 0 for v in n.values()), n
    assert n_lang > 0


def test_malformed_tiles_status_and_records(walked, oracle, decodable_tiles):
    """The malformed corpus: the grammar accepts exactly the tiles the oracle's walk accepts, with the oracle's
    records, and every tile's status is the one the host walkers gave before the shared grammar replaced them
    (tests/golden/container_walk_status.json, recorded from covt_plan_create)."""
    with open(os.path.join(GOLDEN, "container_walk_status.json")) as f:
        pinned = json.load(f)
    h = hashlib.sha256()
    for t, _ in walked["malformed"]:
        h.update(len(t).to_bytes(8, "little"))
        h.update(t)
    assert h.hexdigest() == pinned["corpus_sha256"]  # (the corpus the statuses were recorded for)
    assert len(walked["malformed"]) == len(pinned["status"]) == 184
    n_bad = 0
    for i, (t, r) in enumerate(walked["malformed"]):
        st, ss = oracle.walk_tile(t)
        assert (r["status"] == 0) == (st == 0), i
        assert r["status"] == pinned["status"][i], i
        if st == 0:
            assert r["s"] == _oracle_rows(ss), i
            _assert_layers(ss, r)
        n_bad += st != 0
    assert n_bad >= 60

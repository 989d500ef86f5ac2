"""The C MVT decoder behind the MVT-vs-COVT benchmark (oracle/mvt_decode.c) agrees
with the independent Python MVT reader of the parity tests (tests/covt_geom.mvt_layers) on every OMT
MVT fixture: feature and vertex totals per tile, and feature counts with tests/golden/mvt_digests.json.
The fixtures are tests/golden/mvt: the smallest of the reference's MVT originals at each of z10-z13
(byte-identical copies made by tests/golden/make_golden.py; the lower zooms' tiles are 0.3-1.5 MB each).  CPU."""
import glob
import json
import os

import covt_geom as G

HERE = os.path.dirname(os.path.abspath(__file__))
MVT_DIR = os.path.join(HERE, "golden", "mvt")


def _mvt_files():
    return sorted(glob.glob(os.path.join(MVT_DIR, "*.mvt")))


def test_mvt_decoder_matches_python_reader(oracle):
    digests = json.load(open(os.path.join(HERE, "golden", "mvt_digests.json")))
    files = _mvt_files()
    assert sorted(int(os.path.basename(f).split("_")[0]) for f in files) == [10, 11, 12, 13]
    for f in files:
        data = open(f, "rb").read()
        st, nf, nv, _, _, _ = oracle.mvt_decode(data)
        assert st == 0, f
        key = os.path.basename(f)[:-4]
        if key in digests:
            assert nf == sum(int(v["n_features"]) for v in digests[key].values()), f
        layers = G.mvt_layers(data)
        assert nf == sum(len(L["features"]) for L in layers.values())
        assert nv == sum(len(p) for L in layers.values() for _, _, parts in L["features"] for p in parts)
        st2, nf2, nv2, _, nval, _ = oracle.mvt_decode(data, with_props=True)
        assert (st2, nf2, nv2) == (0, nf, nv) and nval > 0


def test_mvt_decoder_rejects_truncation(oracle):
    files = _mvt_files()
    data = open(files[0], "rb").read() if files else bytes([0x1a, 0x05, 0x12, 0x03, 0x22, 0x01, 0x09])
    assert oracle.mvt_decode(data[: len(data) // 2])[0] == 1 or len(data) < 8
    assert oracle.mvt_decode(b"\x1a\x7f")[0] == 1  # a layer longer than the tile

"""The directed FastPFOR corpus (tests/covt_fpf.py) on the CPU: every case round-trips through the oracle and
through the plain Python reference, and the framing walker shows the frame each case is there for -- a corpus
that stops reaching a decoder path fails here, without a GPU."""
import numpy as np
import pytest

import covt_fpf as F
from oracle import pyref


@pytest.fixture(scope="module")
def corpus(oracle):
    return {name: (enc, v) for name, enc, v in F.cases(oracle)}


def test_cases_round_trip(oracle, corpus):
    for name, (enc, v) in corpus.items():
        st, out, dec = oracle.fastpfor_uncompress(enc, 0, len(enc), v.size)
        assert st == 0 and dec == v.size and np.array_equal(out, v), name
        raw, dec = pyref.fastpfor_uncompress(enc, 0, len(enc), v.size)
        assert dec == v.size and np.array_equal(np.asarray(raw, dtype=np.uint32), v), name


def _frame(enc):
    pages = F.walk(enc)
    assert pages[-1]["next"] <= len(enc) // 4
    return pages


def test_frames(corpus):
    pg = _frame(corpus["ce100"][0])
    assert len(pg) == 1 and pg[0]["blocks"] == [(3, 100, 17)] and pg[0]["sizes"][17][1] == 100  # the ce > 64 path

    enc = corpus["b32"][0]
    pg = _frame(enc)
    assert pg[0]["blocks"] == [(32, 0, 1)] and len(enc) == 1044  # stage's extra 16 bytes, a ring wrap

    (b, ce, idx), = _frame(corpus["idx1"][0])[0]["blocks"]
    assert idx == 1 and ce > 0 and b == 3  # the implicit 1 << b

    pg, = _frame(corpus["widths"][0])
    assert sorted(pg["sizes"]) == list(range(2, 32)) and all(s == 40 for _, s in pg["sizes"].values())
    assert sorted(i for _, _, i in pg["blocks"]) == list(range(1, 32))  # (the 2-bit block: b = 2, index 1)
    assert pg["meta_words"] == 985 > 255 and pg["container_bytes"] == 1292 > 1020  # xin false, chunk_load

    pg, = _frame(corpus["exc40"][0])
    assert pg["container_bytes"] == 2176 and pg["sizes"] == {17: (pg["sizes"][17][0], 2056)}
    assert (2056 * 17 + 31) // 32 == 1093 and max(ce for _, ce, _ in pg["blocks"]) == 69
    assert F.batch_exception_words(pg) > 224  # past kFpfXw: the gathered words and the memory path both run

    enc = corpus["small3"][0]
    pg, = _frame(enc)
    assert pg["meta_words"] == 61 <= 255 and len(enc) == 540 and len(pg["blocks"]) == 3  # xin true

    pg = _frame(corpus["pages2"][0])
    assert [len(p["blocks"]) for p in pg] == [256, 2]

    for k, n in (("small3", 768), ("b32", 256)):  # the VariableByte tails
        for extra in (1, 13, 255):
            enc, v = corpus["%s+%d" % (k, extra)]
            assert v.size == n + extra and F.words(enc)[0] == n and F.walk(enc)[-1]["next"] < len(enc) // 4


def test_malformed_set(oracle):
    bad = F.malformed(oracle)
    assert sum(name.startswith("trunc") for name, *_ in bad) == 135
    assert len(set(name for name, *_ in bad)) == len(bad) == 135 + 13
    base = oracle.encode_fastpfor(F.base_values()["small3"])
    for name, enc, n, good in bad:
        if not name.startswith("trunc"):  # a single field: one byte or one word differs
            assert len(enc) == len(base)
            diff = [i // 4 for i in range(len(enc)) if enc[i] != base[i]]
            assert len(set(diff)) == 1, name

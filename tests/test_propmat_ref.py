"""CPU: the plain reference of the property materialization (tests/covt_propmat.py prop_reference) held to the
C oracle (oracle/covt_oracle_props.c oracle_decode_property) on seeded Gen D layers and on hand-made columns
the Gen D writer never emits, plus known answers written out by hand.  The GPU tests of
tests/test_gpu_propmat.py compare the kernels with this reference."""
import numpy as np
import pytest

import covt_propmat as P
from oracle import gend as W

NS = [0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193]
DENSITIES = [0.0, 0.03, 0.5, 0.97, 1.0]
WORDS = ["Straße", "東京", "road", "", "ŻÓŁW", "x" * 40]


def column_from_tile(oracle, tile, p):
    """The column dict of an oracle_prop: its present / data / length streams decoded one by one by the oracle's
    stream decoders (format Id mode), flags by the plan's rule (covt_props_plan.h prop_streams)."""
    n, nb = p.n_features, (p.n_features + 7) // 8
    st = [0, 0, 0]

    def raw(role):
        return tile[p.s_off[role]:p.s_off[role] + p.s_bl[role]]

    present = None
    if p.s_off[0] >= 0:
        st[0], present, _, _ = oracle.decode_byte_rle(raw(0), nb, 0, p.s_bl[0])
    dn, enc, flags = p.s_nv[1], p.s_enc[1], 0
    lengths = dictionary = None
    if p.type == P.BOOLEAN:
        if present is not None:
            flags |= P.DENSE_BOOL
        st[1], data, _, _ = oracle.decode_byte_rle(raw(1), (dn + 7) // 8 if present is not None else nb, 0, p.s_bl[1])
    elif p.type == P.INT64:
        if enc == W.RLE:
            st[1], data, _, _ = oracle.decode_rle(raw(1), dn, 0, True)
        elif enc in (W.VARINT_ZIG_ZAG, W.VARINT_DELTA_ZIG_ZAG):
            st[1], u, _ = oracle.decode_varint_u64(raw(1), 0, dn)
            z = (u >> np.uint64(1)) ^ (np.uint64(0) - (u & np.uint64(1)))
            data = (np.cumsum(z, dtype=np.uint64) if enc == W.VARINT_DELTA_ZIG_ZAG else z).view(np.int64)
        else:
            flags, data = P.UNSUPPORTED_LATE, np.zeros(0, np.int64)
    elif p.type == P.FLOAT:
        if dn * 4 > p.s_bl[1]:
            flags |= P.DATA_SHORT
        data = np.frombuffer(raw(1)[:4 * dn], dtype="<u4")
    else:
        st[1], idx, _, _ = oracle.decode_rle(raw(1), dn, 0, False)
        st[2], lens, _, _ = oracle.decode_rle(raw(2), p.s_nv[3], 0, False)
        data, lengths, dictionary = idx.astype(np.int32), lens.astype(np.int32), raw(3)  # the (int) casts
    return P.column(p.type, n, present, data, dn, lengths, dictionary, flags, st)


def _compare(oracle, tile, fmt=1):
    """Every property column of the tile: prop_reference equals oracle.decode_property.  -> the statuses."""
    ost, props = oracle.walk_properties(tile, fmt)
    assert ost == 0
    out = []
    for k, p in enumerate(props):
        o = oracle.decode_property(tile, p, 0)
        r = P.prop_reference(column_from_tile(oracle, tile, p))
        assert r[0] == o[0], (k, r[0], o[0])
        out.append(o[0])
        if o[0]:
            continue
        assert r[5] == o[5], k
        assert r[1].tobytes() == o[1].tobytes() and r[2].tobytes() == np.asarray(o[2]).tobytes(), k
        if p.type == P.STRING:
            assert r[3].tobytes() == o[3].tobytes() and r[4].tobytes() == o[4].tobytes(), k
    return out


def _layer(rng, n, columns, L=0):
    xy = rng.integers(-200, 8400, size=(n, 2))
    cols = [W.id_column(rng.integers(0, 1 << 40, size=n).astype(np.uint64)),
            W.geometry_column(np.zeros(n, np.uint8), vertices=xy, column_type=W.CT_PLAIN, num_bits=14)]
    return W.layer("L%d" % L, 8192, n, cols + columns, optimized=bool(L & 1), layer_id=L)


@pytest.mark.parametrize("n", NS)
def test_reference_equals_oracle_on_gend_layers(oracle, n):
    rng = np.random.default_rng(7000 + n)
    cols = []
    for di, dens in enumerate(DENSITIES):
        pres = rng.random(n) < dens if 0.0 < dens < 1.0 else np.full(n, dens == 1.0)
        opt = lambda vals: [v if p else None for v, p in zip(vals, pres)]  # noqa: E731
        ints = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64)
        cols += [W.property_column("i%d" % di, opt([int(v) for v in ints])),
                 W.property_column("m%d" % di, opt([int(v) for v in np.cumsum(rng.integers(0, 1 << 20, size=n))])),
                 W.property_column("f%d" % di, opt([float(v) for v in rng.normal(size=n) * 1e3])),
                 W.property_column("s%d" % di, opt([WORDS[int(i)] for i in rng.integers(0, len(WORDS), size=n)])),
                 W.property_column("b%d" % di, opt([bool(b) for b in rng.random(n) < 0.5]))]
    statuses = _compare(oracle, W.tile([_layer(rng, n, cols)]))
    assert statuses == [0] * (5 * len(DENSITIES))


def _string(name, present, idx, lengths, raw):
    u = lambda a: np.asarray(a, dtype=np.int64) & 0xFFFFFFFF  # noqa: E731
    return {"name": name, "dtype": W.DT_STRING, "ctype": W.CT_DICTIONARY, "prefix": W.booleans(present),
            "streams": [(W.DATA, W.RLE, len(idx), W.encode_rle(u(idx), False)),
                        (W.LENGTH, W.RLE, len(lengths), W.encode_rle(u(lengths), False)),
                        (W.DICTIONARY, W.PLAIN, len(lengths), bytes(raw))]}


def _ints(name, present, dense):
    d = np.asarray(dense, dtype=np.int64)
    return {"name": name, "dtype": W.DT_INT_64, "ctype": W.CT_PLAIN, "prefix": W.booleans(present),
            "streams": [(W.DATA, W.VARINT_ZIG_ZAG, d.size, W.varints(d, zigzag=True))]}


def _floats(name, present, dense):
    return {"name": name, "dtype": W.DT_FLOAT, "ctype": W.CT_PLAIN, "prefix": W.booleans(present),
            "streams": [(W.DATA, W.PLAIN, len(dense), np.asarray(dense, dtype="<f4").tobytes())]}


def test_reference_equals_oracle_on_columns_the_writer_never_emits(oracle):
    rng = np.random.default_rng(7100)
    n = 300
    full = np.ones(n, bool)
    half = rng.random(n) < 0.5
    k = int(half.sum())
    lens, raw = [3, 0, 5, 2], b"abcdefghij"
    idx = rng.integers(0, 4, size=n)

    def at(a, i, v):
        a = np.array(a, dtype=np.int64)
        a[i] = v
        return a

    cases = [
        ("index == n_dict", _string("a", full, at(idx, 200, 4), lens, raw), P.ERR_COUNT),
        ("index negative as an int", _string("b", full, at(idx, 7, 0xFFFFFFFF), lens, raw), P.ERR_COUNT),
        ("bad index past the present count", _string("c", half, at(idx, n - 1, 4), lens, raw), P.OK),
        ("length -1", _string("d", full, idx, [3, 0xFFFFFFFF, 5, 2], raw), P.ERR_COUNT),
        ("lengths sum to dict_bytes + 1", _string("e", full, idx, [3, 0, 5, 3], raw), P.ERR_TRUNCATED),
        ("lengths sum to dict_bytes", _string("f", full, idx, [3, 0, 5, 2], raw), P.OK),
        ("trailing dictionary bytes", _string("g", full, idx, [3, 0, 5, 1], raw), P.OK),
        ("one present bit too many, strings", _string("h", half, idx[:k - 1], lens, raw), P.ERR_COUNT),
        ("one present bit too many, ints", _ints("i", half, rng.integers(-9, 9, size=k - 1)), P.ERR_COUNT),
        ("one present bit too many, floats", _floats("j", half, rng.normal(size=k - 1)), P.ERR_COUNT),
        ("fewer present bits, strings", _string("k", half, idx[:k + 5], lens, raw), P.OK),
        ("fewer present bits, ints", _ints("l", half, rng.integers(-9, 9, size=k + 1)), P.OK),
        ("fewer present bits, floats", _floats("m", half, rng.normal(size=k + 9)), P.OK),
    ]
    assert 1 < k < n - 1  # (the bad index of case c lies past the present count)
    tile = W.tile([_layer(rng, n, [c for _, c, _ in cases])])
    statuses = _compare(oracle, tile)
    assert statuses == [want for _, _, want in cases], list(zip([w for w, _, _ in cases], statuses))


# ---- known answers ----------------------------------------------------------------------------------------
def _ref(*a, **k):
    st, validity, values, doffs, dbytes, nv = P.prop_reference(P.column(*a, **k))
    return (st, validity.tolist(), values.tolist(), None if doffs is None else doffs.tolist(),
            None if dbytes is None else dbytes.tobytes(), nv)


def test_known_answers_boolean():
    # one bit per feature, 10 features: tails beyond n are 0
    assert _ref(P.BOOLEAN, 10, None, [0b10110101, 0xFF]) == (0, [0xFF, 0x03], [0b10110101, 0x03], None, None, 10)
    # dense: features 1, 2, 5, 9 present, their values 1, 0, 1, 1
    assert _ref(P.BOOLEAN, 10, [0b00100110, 0b10], [0b1101], 4, flags=P.DENSE_BOOL) == \
        (0, [0b00100110, 0b10], [0b00100010, 0b10], None, None, 4)
    # dense, one value short
    assert _ref(P.BOOLEAN, 10, [0b00100110, 0b10], [0b101], 3, flags=P.DENSE_BOOL)[0] == P.ERR_COUNT
    assert _ref(P.BOOLEAN, 0, None, []) == (0, [], [], None, None, 0)


def test_known_answers_int64():
    lo, hi = -(1 << 63), (1 << 63) - 1
    assert _ref(P.INT64, 5, [0b10011], [lo, hi, -1]) == (0, [0b10011], [lo, hi, 0, 0, -1], None, None, 3)
    assert _ref(P.INT64, 3, [0b000], [7, 8]) == (0, [0], [0, 0, 0], None, None, 0)  # values left over: fine
    assert _ref(P.INT64, 3, [0b111], [7, 8])[0] == P.ERR_COUNT
    assert _ref(P.INT64, 3, [0b111], [7, 8, 9], st=(0, P.ERR_TRUNCATED, 0))[0] == P.ERR_TRUNCATED


def test_known_answers_float():
    nan = 0x7FC12345  # a NaN with a payload: words, not floats
    assert _ref(P.FLOAT, 4, [0b1010], [nan, 0x80000000]) == (0, [0b1010], [0, nan, 0, 0x80000000], None, None, 2)
    assert _ref(P.FLOAT, 4, [0b1010], [nan, 1], flags=P.DATA_SHORT)[0] == P.ERR_TRUNCATED
    assert _ref(P.FLOAT, 9, [0xFF, 0xFF], list(range(9)))[1:3] == ([0xFF, 0x01], list(range(9)))  # bits past n dropped


def test_known_answers_string():
    lens, raw = [2, 0, 3], b"abcdeZ"
    assert _ref(P.STRING, 4, [0b1101], [2, 1, 0], None, lens, raw) == \
        (0, [0b1101], [2, 0, 1, 0], [0, 2, 2, 5], b"abcdeZ", 3)
    assert _ref(P.STRING, 4, [0b1101], [2, 3, 0], None, lens, raw)[0] == P.ERR_COUNT
    assert _ref(P.STRING, 4, [0b0101], [2, 1, 3], None, lens, raw)[0] == P.OK  # the bad index is never read
    assert _ref(P.STRING, 4, [0b1101], [2, 1, 0], None, [2, 0, 5], raw)[0] == P.ERR_TRUNCATED
    assert _ref(P.STRING, 4, [0b1101], [2, 1, 0], None, [2, -1, 5], raw)[0] == P.ERR_COUNT  # before the overrun
    assert _ref(P.STRING, 0, [], [], None, [], b"") == (0, [], [], [0], b"", 0)
    # precedence: the present stream, UNSUPPORTED_LATE, data, length, the dictionary, the feature loop
    bad = dict(lengths=[2, -1, 5], dict=raw)
    assert _ref(P.STRING, 4, [0b1101], [9, 9, 9], **bad)[0] == P.ERR_COUNT
    assert _ref(P.STRING, 4, [0b1101], [9, 9, 9], st=(0, 0, P.ERR_TRUNCATED), **bad)[0] == P.ERR_TRUNCATED
    assert _ref(P.STRING, 4, [0b1101], [9, 9, 9], st=(0, -4, P.ERR_TRUNCATED), **bad)[0] == -4
    assert _ref(P.STRING, 4, [0b1101], [9], flags=P.UNSUPPORTED_LATE, st=(0, P.ERR_TRUNCATED, 0), **bad)[0] == P.ERR_UNSUPPORTED
    assert _ref(P.STRING, 4, [0b1101], [9], flags=P.UNSUPPORTED_LATE, st=(P.ERR_TRUNCATED, 0, 0), **bad)[0] == P.ERR_TRUNCATED
    assert _ref(P.STRING, 4, [0b1101], [9], flags=P.UNSUPPORTED, st=(P.ERR_TRUNCATED, 0, 0), **bad)[0] == P.ERR_UNSUPPORTED

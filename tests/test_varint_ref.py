"""The varint corpus of tests/covt_varint.py on the CPU: its plain reference equals the C oracle on every
descriptor the oracle has an entry point for (status, values, consumed; OP_VARINT_ZZ_DELTA_S64 through
oracle.decode_property on a one-column Gen D layer), and the corpus reaches what it aims at -- by the window model
for the kernel's step sizes, by the reference alone for the mix of statuses.  tests/test_gpu_varint.py runs the
same corpus on the device."""
import numpy as np

import covt_varint as CV

_CACHE = {}


def corpus(covt, oracle):
    """(corpus, the reference's (status, values, consumed) per row), built once and never changed."""
    if "corpus" not in _CACHE:
        c = CV.build_corpus(covt, oracle)
        _CACHE["corpus"] = (c, [c.expected(i) for i in range(len(c.rows))])
    return _CACHE["corpus"]


def _oracle_row(covt, oracle, c, r):
    """(status, values, consumed) from the oracle, or None where it has no call for the descriptor."""
    from oracle import gend as W

    op, n, av = r["op"], r["n"], r["avail"]
    if av < 0:
        return None  # (a buffer has no negative length)
    buf = bytes(c.blob[r["in_off"]:r["in_off"] + av])
    O = oracle
    if r["head"] is not None:
        if r["bl"] != av:
            return None
        f = {covt.OP_FPF_ZZ_DELTA_I32: lambda: O.decode_fastpfor_zigzag_delta(buf, n, av, 0),
             covt.OP_FPF_ZZ_DELTA_XY: lambda: O.decode_fastpfor_delta_coordinates(buf, n, av, 0),
             covt.OP_FPF_DELTA_MORTON: lambda: O.decode_fastpfor_delta_morton_codes(buf, n, av, 0, r["nb"])}[op]
        st, arr, pos = f()
        return st, np.asarray(arr, dtype=np.int32), pos
    if op == covt.OP_VARINT_ZZ_DELTA_S64:
        if n < 0:
            return None
        col = {"name": "v", "dtype": W.DT_INT_64, "ctype": W.CT_PLAIN, "prefix": W.booleans(np.ones(n, bool)),
               "streams": [(W.DATA, W.VARINT_DELTA_ZIG_ZAG, n, buf)]}
        tile = W.tile([W.layer("L", 4096, n, [W.id_column(np.zeros(n, np.uint64)), col])])
        st, props = O.walk_properties(tile, O.FMT_GEND)
        assert st == 0 and len(props) == 1
        o = O.decode_property(tile, props[0], O.ID_FORMAT)
        return o[0], np.asarray(o[2]).view(np.int64)[:max(n, 0)], None  # (a column reports no consumed bytes)
    if op in (covt.OP_VARINT_U64, covt.OP_VARINT_ZZ_S64):
        st, arr, pos = O.decode_varint_u64(buf, 0, n)
        if op == covt.OP_VARINT_ZZ_S64:
            u = arr.astype(np.uint64)
            arr = (u >> np.uint64(1)) ^ (np.uint64(0) - (u & np.uint64(1)))
        return st, arr.view(np.int64), pos
    if op in (covt.OP_VARINT_I32, covt.OP_VARINT_I32_AS_I64):
        st, arr, pos = O.decode_varint(buf, 0, n)
    elif op in (covt.OP_VARINT_ZZ_I32, covt.OP_VARINT_ZZ_I32_AS_I64):
        st, arr, pos = O.decode_zigzag_varint(buf, 0, n)
    elif op in (covt.OP_VARINT_ZZ_DELTA_I32, covt.OP_VARINT_ZZ_DELTA_I64):
        st, arr, pos = O.decode_zigzag_delta_varint(buf, 0, n)
    elif op == covt.OP_VARINT_ZZ_DELTA_XY:
        st, arr, pos = O.decode_zigzag_delta_varint_coordinates(buf, 0, n)
    else:
        st, arr, pos = O.decode_delta_varint_morton_codes(buf, 0, n, r["nb"])
    arr = np.asarray(arr, dtype=np.int32)
    if op in (covt.OP_VARINT_I32_AS_I64, covt.OP_VARINT_ZZ_I32_AS_I64, covt.OP_VARINT_ZZ_DELTA_I64):
        arr = arr.astype(np.int64)  # the widenings of CovtParser (mapToLong)
    return st, arr, pos


def test_reference_equals_the_oracle(covt, oracle):
    c, exp = corpus(covt, oracle)
    n_cmp = 0
    seen_ops = set()
    for r, (st, vals, cons) in zip(c.rows, exp):
        o = _oracle_row(covt, oracle, c, r)
        if o is None:
            assert st == covt.ERR_INVALID_ARG or r["bl"] != r["avail"], r
            continue
        tag = (r["group"], r["note"], r["op"], r["n"], r["avail"])
        assert o[0] == st, (tag, o[0], st)
        if st == 0:
            assert o[2] is None or o[2] == cons, (tag, o[2], cons)
            assert vals.dtype == o[1].dtype and vals.tobytes() == o[1].tobytes(), tag
        else:
            assert vals is None and cons == 0, tag
        seen_ops.add(r["op"])
        n_cmp += 1
    assert seen_ops == set(c.ref.java_ops + c.ref.u64_ops + c.ref.fpf_ops)
    assert n_cmp >= len(c.rows) - 60


def test_reference_pins():
    """A few values by hand, so the reference does not only agree with the oracle but with the grammars."""
    class K:  # the constants the reference reads
        (OP_VARINT_I32, OP_VARINT_ZZ_I32, OP_VARINT_ZZ_DELTA_I32, OP_VARINT_ZZ_DELTA_XY, OP_VARINT_DELTA_MORTON,
         OP_VARINT_I32_AS_I64, OP_VARINT_ZZ_I32_AS_I64, OP_VARINT_ZZ_DELTA_I64, OP_VARINT_U64, OP_VARINT_ZZ_S64,
         OP_VARINT_ZZ_DELTA_S64, OP_FPF_ZZ_DELTA_I32, OP_FPF_ZZ_DELTA_XY, OP_FPF_DELTA_MORTON) = range(14)
        ERR_TRUNCATED, ERR_COUNT_MISMATCH, ERR_BAD_HEADER, ERR_INVALID_ARG = -2, -3, -4, -6

    ref = CV.Reference(K)
    # four continuation bytes are a whole Java value: 0x7f from each, the next byte starts a new one
    st, v, cons = ref.varint(K.OP_VARINT_I32, b"\xff\xff\xff\xff\x05", 5, 2)
    assert (st, v.tolist(), cons) == (0, [0x0fffffff, 5], 5)
    st, v, cons = ref.varint(K.OP_VARINT_ZZ_DELTA_XY, bytes([2, 4, 1, 3]), 4, 4)
    assert (st, v.tolist(), cons) == (0, [1, 2, 0, 0], 4)
    assert ref.varint(K.OP_VARINT_ZZ_DELTA_XY, bytes([2, 4, 1, 3]), 4, 3)[0] == K.ERR_COUNT_MISMATCH
    assert ref.varint(K.OP_VARINT_ZZ_DELTA_XY, bytes([2, 4, 1]), 3, 3)[0] == K.ERR_TRUNCATED
    st, v, cons = ref.varint(K.OP_VARINT_U64, b"\xff" * 9 + b"\x7f", 10, 1)
    assert (st, int(v.view(np.uint64)[0]), cons) == (0, CV.M64, 10)  # bits above bit 0 of the tenth byte fall off
    assert ref.varint(K.OP_VARINT_U64, b"\x80" * 10 + b"\x00\x01", 12, 1)[0] == K.ERR_BAD_HEADER
    st, v, cons = ref.varint(K.OP_VARINT_U64, b"\x01" + b"\x80" * 10 + b"\x00", 12, 1)
    assert (st, v.tolist(), cons) == (0, [1], 1)  # an over-long value past num_values is never read
    assert ref.varint(K.OP_VARINT_U64, b"\x80" * 3000, 3000, 1)[0] == K.ERR_TRUNCATED
    st, v, cons = ref.varint(K.OP_VARINT_ZZ_DELTA_S64, CV.vu(CV.zz64((1 << 63) - 1)) + CV.vu(CV.zz64(1)), 11, 2)
    assert (st, v.tolist(), cons) == (0, [(1 << 63) - 1, -(1 << 63)], 11)
    assert ref.varint(K.OP_VARINT_U64, b"\x01", -1, 1)[0] == K.ERR_INVALID_ARG
    # VariableByte: bit 7 set ends a value; six bytes wrap the shift to 35 & 31 = 3
    data, first = CV.write_fpf(b"\x85" + b"\x01\x82" + b"\x00" * 5 + b"\x81" + b"\x07", header=0)
    assert first == 1 and len(data) == 16 and data[4:8] == b"\x00\x82\x01\x85"
    head = (np.zeros(0, np.uint32), first)
    st, v, cons = ref.fastpfor(K.OP_FPF_ZZ_DELTA_I32, data, 16, 4, 0, 16, head)
    raw = [5, 1 + (2 << 7), 1 << 3, 0]  # (the trailing 0x07 is a partial value; the fourth value is zero-filled)
    want = np.cumsum([(x >> 1) ^ -(x & 1) for x in raw])
    assert (st, v.tolist(), cons) == (0, want.tolist(), 16)
    assert ref.fastpfor(K.OP_FPF_ZZ_DELTA_I32, data, 16, 2, 0, 16, head)[0] == K.ERR_COUNT_MISMATCH


def test_corpus_covers_the_varint_engine(covt, oracle):
    c, exp = corpus(covt, oracle)
    ref = c.ref
    rows = c.rows
    vi, fi = c.varint_rows(), c.fpf_rows()
    assert len(vi) >= 2000 and len(fi) >= 300 and len(vi) + len(fi) == len(rows)
    assert len(c.blob) < (1 << 20)
    assert {r["group"] for r in rows} == {g for g, _ in CV.GROUPS}
    long_ok = ("counts", "overlong", "vbyte")  # the groups the corpus names as longer than 5 windows
    assert all(r["avail"] <= 5 * CV.WIN or r["group"] in long_ok for r in rows)
    st = np.array([e[0] for e in exp])
    ok = st == 0
    # conditions on the corpus, from the reference alone
    fail = 1.0 - ok.mean()
    assert 0.15 <= fail <= 0.50, fail
    for op in ref.java_ops + ref.u64_ops + ref.fpf_ops:
        assert sum(1 for r, e in zip(rows, exp) if r["op"] == op and e[0] == 0) >= 50, op
    for s in (covt.ERR_TRUNCATED, covt.ERR_BAD_HEADER, covt.ERR_COUNT_MISMATCH, covt.ERR_INVALID_ARG):
        assert (st == s).any(), s
    assert set(st.tolist()) <= {0, covt.ERR_TRUNCATED, covt.ERR_BAD_HEADER, covt.ERR_COUNT_MISMATCH,
                                covt.ERR_INVALID_ARG}
    assert all(e[2] == 0 and e[1] is None for e in exp if e[0] != 0)
    fams = {}
    for r, e in zip(rows, exp):
        if r["fam"] >= 0:
            fams.setdefault(r["fam"], set()).add(e[0] == 0)
    assert len(fams) >= 24 and all(v == {True, False} for v in fams.values())
    # over-long 64-bit values: an error only among the first num_values; a run to the end is TRUNCATED
    for r, e in zip(rows, exp):
        if r["group"] == "overlong":
            kind = r["note"][0] if r["note"][0] in ("run", "run_unread") else r["note"][1]
            want = {"first": covt.ERR_BAD_HEADER, "last": covt.ERR_BAD_HEADER, "at_n": 0, "later": 0,
                    "run": covt.ERR_TRUNCATED, "run_unread": 0}[kind]
            assert e[0] == want, (r["note"], e[0])
    # the delta sums of the 64-bit op pass 2^32 and 2^63, wrap, go negative and come back
    carry = [e[1] for r, e in zip(rows, exp) if r["note"] == "carry" and r["op"] == covt.OP_VARINT_ZZ_DELTA_S64]
    assert len(carry) >= 15
    for v in carry:
        assert v.max() > (1 << 62) and v.min() < -(1 << 62) and (np.abs(v[-100:]) < (1 << 50)).any()
        assert (np.diff(v.astype(np.float64)) < -1e19).any()  # a wrap past 2^63
    # the window model
    leads, residues = {}, {}
    cuts, tails, reloads, serial_at, runs_chunk, runs_window, wins = set(), set(), set(), set(), set(), set(), {}
    for r, e in zip(rows, exp):
        w = CV.window_walk(c, r)
        if e[0] != 0:
            continue
        g = ref.grammar(r["op"])
        odd_xy = False
        assert w is not None, r
        assert sum(x["take"] for x in w) == (r["n"] if g != "v" else sum(x["take"] for x in w))
        wins[r["op"]] = max(wins.get(r["op"], 0), len(w))
        for k, x in enumerate(w):
            leads.setdefault(g, set()).add(x["lead"])
            if k == 0:
                residues.setdefault(g, set()).add(r["in_off"] & 15)
            edge = 1 if k == 1 else 2
            if x["cut"]:
                cuts.add((g, x["line"]))
            if x["tail"]:
                tails.add((g, x["line"]))
            if x["reload"]:
                reloads.add((g,) + tuple(x["reload"]) + (edge,))
            if x["serial"] and len(w) >= 3:
                serial_at.add("first" if k == 0 else "last" if k == len(w) - 1 else "middle")
            for chunk_phase, win_phase in x["runs"]:
                if chunk_phase > 12:
                    runs_chunk.add(16 - chunk_phase)  # bytes of the run before the 16-byte chunk edge
        # a run of four continuation bytes across a window's end: the window sees only its first bytes
        if g == "j" and r["group"] == "serial" and r["note"][0] == "window":
            assert w[1]["serial"] and not w[0]["serial"] and len(w[1]["runs"]) == 1
            runs_window.add(w[0]["woff"] + CV.WIN - (w[1]["woff"] + w[1]["runs"][0][1]))
    # lead slots: a window's take ends on an output line (16 or 32 values) unless it is the stream's last, and a
    # window of >= 1009 bytes never holds less than a line of values of <= 10 bytes, so a one-wave decode starts
    # every group at a multiple of 4: leads 1..3 exist only in split chunks (out0 != 0, tests/test_gpu_split.py)
    assert leads == {"j": {0}, "u": {0}, "v": {0}}, leads
    assert all(residues[g] == set(range(16)) for g in ("j", "u")), residues
    assert residues["v"] == {0}  # FastPFOR streams are read as words: the plan aligns them
    # the output-line cut for 16 and 32 values a line; a restart at a line's tail needs a window that outlives its
    # take, which only the 64-bit grammar has (16 values a line)
    assert {("j", 16), ("j", 32), ("u", 16)} <= cuts and ("u", 16) in tails, (cuts, tails)
    for ln in (2, 3, 4):
        for k in range(1, ln):
            assert ("j", ln, k, 1) in reloads and ("j", ln, k, 2) in reloads, (ln, k)
    for k in range(1, 10):
        assert ("u", 10, k, 1) in reloads and ("u", 10, k, 2) in reloads, k
    for k in range(1, 5):
        assert ("v", 5, k, 1) in reloads and ("v", 5, k, 2) in reloads, k
    assert serial_at == {"first", "middle", "last"}
    assert runs_chunk == {1, 2, 3} and runs_window == {1, 2, 3}
    for op in ref.java_ops + ref.u64_ops:
        assert wins[op] >= 3, op
    assert max(wins[op] for op in ref.fpf_ops) >= 3
    # over-long VariableByte values (6..12 bytes) carry payload past the fifth byte: their value depends on the shift
    # being taken modulo 32.  (The check is on the CPU because a 32-bit shift of the GPU takes its count modulo 32
    # whatever the source says: a kernel that masked with 63 would compile to the same function.)
    for k in range(6, 13):
        hit = [r for r, e in zip(rows, exp) if r["note"] == ("overlong", k) and e[0] == 0]
        assert len(hit) >= 10, k
        for r in hit:
            data = memoryview(c.blob)[r["in_off"]:]
            assert ref.vbyte_tail(data, r["bl"], r["head"][1]) != ref.vbyte_tail(data, r["bl"], r["head"][1], mask=63), k
    # VariableByte values longer than a window: 0x00 bytes only advance the shift
    longs = {x["long"] for r, e in zip(rows, exp) if e[0] == 0 and r["head"] is not None
             for x in CV.window_walk(c, r) if x.get("long")}
    assert len(longs) >= 2 and max(longs) > 2 * CV.WIN, longs

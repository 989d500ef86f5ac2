"""GPU: the property materialization pass (covt_props.hip) at kernel level, through the C-ABI entry point
covt_materialize_properties_device on hand-made descriptors (tests/covt_propmat.py), against the plain
reference prop_reference (pinned to the C oracle by tests/test_propmat_ref.py): bytes, status and n_valid.

The property buffer is filled with 0x5A and the result rows with a pattern before every launch.  Every byte
outside the columns' slices (the 16-byte gap after each column included) must still hold the fill; for a
column that ended COVT_OK so must every byte between an array's exact end (ceil(n/8), the value bytes,
4 * (n_dict + 1), dict_bytes) and the 16-aligned end of its slice; a column flagged COVT_PROP_UNSUPPORTED
leaves its whole slice untouched.  The slices of a column that failed otherwise are unspecified.

Every batch runs twice: as built (at most 4,096 columns: prop_split_prep + prop_split_kernel, columns of 512
features or more in 4,096-feature chunks chained by the look-back, the rest as single waves, sixteen per
ticket) and padded with 1-feature columns to 4,097 (props_kernel: one wave per column, 256 features a step).
"""
import collections

import numpy as np
import pytest

import covt_propmat as P
from oracle import gend as W

pytestmark = pytest.mark.gpu

FILL = 0x5A
RES_FILL = 0x5A5A5A5A
NS = [0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 5]
N3 = 3 * 4096 + 5
BAD = -4  # a source stream's status no materialization step produces (COVT_ERR_BAD_HEADER)
PATTERNS = ["empty", "full", "r0.03", "r0.5", "r0.97", "absent4096_present4096", "present4096_absent4096",
            "bit0", "bit3", "bit4", "bit7", "bitlast"]
TINY = P.column(P.INT64, 1, P.bits([True]), [42])


# ---- running and checking ---------------------------------------------------------------------------------
def _upload(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")


def _run(covt, cols):
    """One launch over hand-made columns -> (property buffer, result rows, layouts)."""
    import torch

    inp, dec, rows, d, out_bytes, lays = P.pack_prop_columns(covt, cols, res_fill=RES_FILL)
    d_in, d_dec, d_rows, d_desc = _upload(inp), _upload(dec), _upload(rows), _upload(d)
    d_out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda:0")
    d_pres = torch.full((2 * len(cols),), RES_FILL, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    assert covt.lib().covt_materialize_properties_device(d_in.data_ptr(), d_dec.data_ptr(), d_rows.data_ptr(),
                                                         d_desc.data_ptr(), len(cols), d_out.data_ptr(),
                                                         d_pres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_pres.cpu().numpy().view(covt.PROP_RESULT_DTYPE), lays


def _reference(col, cache):
    if id(col) not in cache:
        cache[id(col)] = P.prop_reference(col)
    return cache[id(col)]


def _same(got, want, what):
    if got.tobytes() != want.tobytes():
        g, w = got.view(np.uint8), want.view(np.uint8)
        bad = np.nonzero(g != w)[0] if g.size == w.size else [-1]
        raise AssertionError("%s: %d of %d bytes differ, first at %d" % (what, len(bad), w.size, int(bad[0])))


def _check(cols, buf, pres, lays, cache, idx=None, window=None):
    """Columns `idx` (all) equal the reference, and every byte of `window` (the whole buffer) that no examined
    column may write holds FILL.  -> Counter of statuses."""
    lo, hi = window or (0, buf.size)
    untouched = np.ones(hi - lo, dtype=bool)

    def mark(lay, k, whole):
        o = lay["off"][k] - lo
        untouched[o:o + (lay["slice"][k] if whole else lay["size"][k])] = False

    tally = collections.Counter()
    for ci in (range(len(cols)) if idx is None else idx):
        col, lay = cols[ci], lays[ci]
        st, validity, values, doffs, dbytes, nv = _reference(col, cache)
        got = (int(pres["status"][ci]), int(pres["n_valid"][ci]))
        assert got == (st, nv), "column %d: (status, n_valid) %r, want %r" % (ci, got, (st, nv))
        tally[st] += 1
        if col["flags"] & P.UNSUPPORTED:
            continue  # nothing of it may be written
        if st == 0:
            g = P.unpack_prop_column(buf, lay, col)
            _same(g[0], validity, "column %d validity" % ci)
            _same(g[1], values, "column %d values" % ci)
            if col["type"] == P.STRING:
                _same(g[2], doffs, "column %d dictionary offsets" % ci)
                _same(g[3], dbytes, "column %d dictionary bytes" % ci)
        for k in (0, 1):
            mark(lay, k, whole=st != 0)
        if col["type"] == P.STRING and col["owner"] is None and col["st"][2] == 0:
            # the owner writes the dictionary whatever its present and data streams hold (a column flagged
            # UNSUPPORTED_LATE or DATA_SHORT has no promise either way: its dictionary slices are unspecified)
            dst, doffs, dbytes = P.dict_reference(col)
            if col["flags"] & (P.UNSUPPORTED_LATE | P.DATA_SHORT):
                dst = dst or 1
            if dst == 0:
                g = P.unpack_prop_column(buf, lay, col)
                _same(g[2], doffs, "column %d (status %d) dictionary offsets" % (ci, st))
                _same(g[3], dbytes, "column %d (status %d) dictionary bytes" % (ci, st))
            for k in (2, 3):
                mark(lay, k, whole=dst != 0)
    stray = np.nonzero(buf[lo:hi][untouched] != FILL)[0]
    assert stray.size == 0, "%d bytes outside the written arrays changed, first at %d" % (
        stray.size, lo + int(np.nonzero(untouched)[0][stray[0]]))
    return tally


def _both(covt, cols, cache=None, what=None):
    """The batch through the split kernel and, padded to 4,097 columns, through props_kernel."""
    cache = {} if cache is None else cache
    assert len(cols) <= P.COOP_MAX_COLUMNS
    split = P.split_plan(cols)
    t1 = _check(cols, *_run(covt, cols), cache)
    padded = cols + [TINY] * (P.COOP_MAX_COLUMNS + 1 - len(cols))
    assert P.split_plan(padded) is None
    t2 = _check(padded, *_run(covt, padded), cache)
    t2[0] -= len(padded) - len(cols)
    assert +t1 == +t2
    if what:
        print("propmat %s: split kernel %d columns (%d in chunks, %d single waves), wave kernel %d columns; statuses %s"
              % (what, len(cols), sum(split), len(cols) - sum(split), len(padded), dict(sorted(t1.items()))))
    return t1


# ---- building columns -------------------------------------------------------------------------------------
def _pattern(rng, name, n):
    m = np.zeros(n, dtype=bool)
    if name == "full":
        m[:] = True
    elif name.startswith("r"):
        m = rng.random(n) < float(name[1:])
    elif name == "absent4096_present4096":
        m = (np.arange(n) // 4096) % 2 == 1
    elif name == "present4096_absent4096":
        m = (np.arange(n) // 4096) % 2 == 0
    elif name.startswith("bit") and n:
        m[min(n - 1, n - 1 if name == "bitlast" else int(name[3:]))] = True
    return m


def _strings(rng, nd, dict_bytes=None, exact=True):
    """(lengths, bytes) of a dictionary of nd strings, empty ones among them, filling dict_bytes (a random total
    of up to 9 bytes a string when None) exactly or leaving trailing bytes."""
    if dict_bytes is None:
        lens = rng.integers(0, 10, size=nd)
        dict_bytes = int(lens.sum()) + (0 if exact else 5)
    else:
        total = dict_bytes if exact else int(rng.integers(0, dict_bytes + 1))
        cuts = np.sort(rng.integers(0, total + 1, size=nd)) if nd else np.zeros(0, np.int64)
        lens = np.diff(cuts, prepend=0)  # (the last string ends at its cut: bytes may be left over)
        if nd and exact:
            lens[-1] += total - int(lens.sum())
    return lens.astype(np.int32), rng.integers(0, 256, size=dict_bytes, dtype=np.uint8).tobytes()


def _mk(rng, kind, n, mask, extra=0, nd=7, owner=None, align=0, **kw):
    """A valid column.  kind: b BOOLEAN per feature, d BOOLEAN dense, i INT64, f FLOAT, s STRING; mask: the
    present features (None: no present stream); extra: data values beyond the present count."""
    dn = (n if mask is None else int(np.sum(mask))) + extra
    present = None if mask is None else P.bits(mask)
    if kind == "b":
        return P.column(P.BOOLEAN, n, present, rng.integers(0, 256, size=(n + 7) // 8, dtype=np.uint8), n, **kw)
    if kind == "d":
        return P.column(P.BOOLEAN, n, present, rng.integers(0, 256, size=(dn + 7) // 8, dtype=np.uint8), dn,
                        flags=P.DENSE_BOOL, **kw)
    if kind == "i":
        v = rng.integers(-(1 << 63), (1 << 63) - 1, size=dn, dtype=np.int64, endpoint=True)
        v[:4] = [-(1 << 63), (1 << 63) - 1, -1, 0][:min(dn, 4)]
        return P.column(P.INT64, n, present, v, **kw)
    if kind == "f":
        w = rng.integers(0, 1 << 32, size=dn, dtype=np.uint32)
        w[::5] |= 0x7F800001  # NaNs with payloads
        return P.column(P.FLOAT, n, present, w, align=align, **kw)
    if owner is not None:
        nd = len(owner["lengths"])
        lens = raw = None
    else:
        lens, raw = kw.pop("dictionary", None) or _strings(rng, nd)
        nd = len(lens)
    idx = rng.integers(0, max(nd, 1), size=dn).astype(np.int32)
    return P.column(P.STRING, n, present, idx, None, lens, raw, owner=owner, align=align, **kw)


# ---- 3a: feature-count steps ------------------------------------------------------------------------------
def test_feature_count_steps(covt, gpu_available):
    """Every n around the nibble / byte tails, the 256-feature wave step, kPropSplitMinFeatures and the
    4,096-feature chunk meets every type; every present pattern meets the multi-chunk sizes."""
    rng = np.random.default_rng(4100)
    cols, seen = [], set()
    for ni, n in enumerate(NS):
        for ki, kind in enumerate("bdifs"):
            pat = PATTERNS[(ni + 5 * ki) % len(PATTERNS)]
            mask = None if kind == "b" else _pattern(rng, pat, n)
            cols.append(_mk(rng, kind, n, mask, extra=(ni + ki) % 3))
            seen.add((n, kind))
    for ni, n in enumerate([8191, 8192, 8193, N3]):
        for pi, pat in enumerate(PATTERNS):
            kind = "difs"[(pi + ni) % 4]
            cols.append(_mk(rng, kind, n, _pattern(rng, pat, n), extra=pi % 2))
            seen.add((n, pat))
    assert len(seen) == 5 * len(NS) + 4 * len(PATTERNS)
    split = P.split_plan(cols)
    assert (sum(split), len(cols) - sum(split)) == (5 * 9 + 48, 5 * 12)
    tally = _both(covt, cols, what="3a")
    assert tally == {0: len(cols)}


# ---- 3b: batch-shape steps --------------------------------------------------------------------------------
def _handful(rng):
    owner = _mk(rng, "s", 513, _pattern(rng, "r0.5", 513), nd=300)
    return [_mk(rng, "i", 8193, _pattern(rng, "r0.5", 8193)), owner, _mk(rng, "f", 300, _pattern(rng, "r0.97", 300), align=1),
            _mk(rng, "s", 5000, _pattern(rng, "r0.03", 5000), owner=owner), _mk(rng, "d", 4097, _pattern(rng, "r0.5", 4097))]


@pytest.mark.parametrize("n_cols", [1, 3, 4, 5])
def test_few_columns(covt, gpu_available, n_cols):
    """Four columns per thread of prop_split_prep."""
    rng = np.random.default_rng(4200 + n_cols)
    cols = ([_mk(rng, "i", 2 * 4096 + 1, _pattern(rng, "r0.5", 2 * 4096 + 1))] +
            [_mk(rng, "ifds"[k % 4], [9, 600, 255, 4097][k % 4], _pattern(rng, "r0.5", [9, 600, 255, 4097][k % 4]))
             for k in range(4)])[:n_cols]
    assert _both(covt, cols, what="3b %d columns" % n_cols) == {0: n_cols}


@pytest.mark.parametrize("n_small", [15, 16, 17])
def test_small_columns_per_ticket(covt, gpu_available, n_small):
    """Sixteen single-wave columns per ticket, beside split ones."""
    rng = np.random.default_rng(4210 + n_small)
    small = [_mk(rng, "bdifs"[k % 5], [7, 255, 511, 64, 300][k % 5], None if k % 5 == 0 else _pattern(rng, "r0.5", [7, 255, 511, 64, 300][k % 5]))
             for k in range(n_small)]
    big = [_mk(rng, "s", 8192, _pattern(rng, "r0.97", 8192)), _mk(rng, "f", 512, _pattern(rng, "r0.5", 512), align=3)]
    cols = small[:5] + big[:1] + small[5:] + big[1:]
    split = P.split_plan(cols)
    assert (sum(split), len(cols) - sum(split)) == (2, n_small)
    assert _both(covt, cols, what="3b %d small" % n_small) == {0: len(cols)}


@pytest.mark.parametrize("n_cols", [4095, 4096, 4097])
def test_switch_between_kernels(covt, gpu_available, n_cols):
    """4,096 columns is the last batch of the split kernel, 4,097 the first of props_kernel: all tiny but a
    handful, which sit at the start, in the middle and at the very end of the batch."""
    rng = np.random.default_rng(4220)
    h = _handful(rng)
    cols = h[:2] + [TINY] * 2000 + h[2:4] + [TINY] * (n_cols - 2005) + h[4:]
    assert len(cols) == n_cols
    if n_cols <= P.COOP_MAX_COLUMNS:
        assert sum(P.split_plan(cols)) == 4
        assert _both(covt, cols, what="3b %d columns" % n_cols) == {0: n_cols}
    else:
        assert P.split_plan(cols) is None
        assert _check(cols, *_run(covt, cols), {}) == {0: n_cols}
        print("propmat 3b 4097 columns: wave kernel 4097 columns; statuses {0: 4097}")


# ---- 3c: the chunk budget ---------------------------------------------------------------------------------
@pytest.mark.parametrize("first_n", [65536, 65537], ids=["exactly_65536_chunks", "one_chunk_past"])
def test_chunk_budget(covt, gpu_available, first_n):
    """4,096 BOOLEAN columns of 65,536 features are 16 chunks each, 65,536 in all: exactly the budget, all
    split.  With column 0 one feature longer (17 chunks) the last prep thread's prefix passes the budget and
    its four columns fall back to single waves.  The columns share one present and one data array."""
    rng = np.random.default_rng(4300)
    n = 65536
    present = rng.integers(0, 256, size=8200, dtype=np.uint8)
    data = rng.integers(0, 256, size=8200, dtype=np.uint8)
    first = P.column(P.BOOLEAN, first_n, present, data, first_n)
    rest = P.column(P.BOOLEAN, n, present, data, n)
    cols = [first] + [rest] * 4095
    split = P.split_plan(cols)
    assert sum(split) == (4096 if first_n == n else 4092) and split[-4:] == [first_n == n] * 4
    cache = {}
    st, validity, values, _, _, nv = _reference(rest, cache)
    assert st == 0
    for batch in (cols, cols + [TINY]):
        buf, pres, lays = _run(covt, batch)
        start, stride = lays[1]["off"][0], 2 * 8192 + 16
        assert lays[4095]["off"][0] == start + 4094 * stride and buf.size >= 67_000_000
        assert _check(batch, buf, pres, lays, cache, idx=[0], window=(0, start)) == {0: 1}
        assert (pres["status"][1:4096] == 0).all() and (pres["n_valid"][1:4096] == nv).all()
        body = buf[start:start + 4095 * stride].reshape(4095, stride)
        assert (body[:, :8192] == validity).all() and (body[:, 8192:16384] == values).all()
        assert (body[:, 16384:] == FILL).all()
        if len(batch) > 4096:
            tail = start + 4095 * stride
            assert _check(batch, buf, pres, lays, cache, idx=[4096], window=(tail, buf.size)) == {0: 1}
    print("propmat 3c %s: split kernel 4096 columns (%d in chunks, %d single waves), wave kernel 4097 columns; "
          "statuses {0: 4096}" % (first_n, sum(split), 4096 - sum(split)))


# ---- 3d: dictionaries -------------------------------------------------------------------------------------
def test_dictionaries(covt, gpu_available):
    """Dictionary sizes around the owner's 256-length scan step, its 1,024-length batches, the int32x4 offset
    stores and the 16-byte copies, at every input alignment; every owner has sub-columns that only check it."""
    rng = np.random.default_rng(4400)
    cols, k = [], 0
    for nd in (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049):
        for db in (0, 1, 15, 16, 17, 1023, 1024, 1025, 5000):
            n = [0, 40, 600, 5000][(k + k // 4) % 4]  # (every alignment meets single waves and chunks)
            pat = "empty" if nd == 0 else ["r0.5", "full", "r0.97", "r0.03"][k % 4]
            dictionary = _strings(rng, nd, db, exact=(k // 3) % 2 == 0)
            owner = _mk(rng, "s", n, _pattern(rng, pat, n), dictionary=dictionary, align=k % 4)
            cols.append(owner)
            for j in range(1 + k % 2):  # (an owner without features has sub-columns with some)
                m = [700, 33, 0, 4097][(k + j) % 4] if n else 300 + 400 * j
                cols.append(_mk(rng, "s", m, _pattern(rng, "empty" if nd == 0 else "r0.5", m), owner=owner))
            k += 1
    for a in range(4):  # FLOAT data at every input alignment, single waves and chunks
        for n in (37, 4100):
            cols.append(_mk(rng, "f", n, _pattern(rng, "r0.5", n), align=a))
    for n in (50, 9000):  # an owner whose own data stream failed still writes the dictionary
        owner = _mk(rng, "s", n, _pattern(rng, "r0.5", n), nd=300, st=(0, P.ERR_TRUNCATED, 0), align=1)
        cols += [owner, _mk(rng, "s", n + 1, _pattern(rng, "r0.5", n + 1), owner=owner)]
    tally = _both(covt, cols, what="3d")
    assert tally == {0: len(cols) - 2, P.ERR_TRUNCATED: 2}
    assert len(cols) == 108 + 162 + 8 + 4


# ---- 3e: statuses -----------------------------------------------------------------------------------------
def _status_cases(rng):
    """[(what, column, wanted status)]: bad values in well-formed streams, each as a single wave (100 features)
    and in a column of four chunks (the fault in its last chunk where it has a position)."""
    out = []

    def add(what, col, want):
        out.append((what, col, want))
        return col

    for n in (100, N3):
        mask = rng.random(n) < 0.6
        mask[-1] = True
        k = int(mask.sum())
        nd = 2049
        ones = np.ones(nd, np.int32)
        raw = rng.integers(0, 256, size=nd, dtype=np.uint8).tobytes()

        def strings(idx=None, lengths=ones, raw=raw, m=mask, n_data=None, **kw):
            idx = rng.integers(0, len(lengths), size=int(m.sum())).astype(np.int32) if idx is None else idx
            return P.column(P.STRING, n, P.bits(m), idx, n_data, lengths, raw, **kw)

        def sub(owner, **kw):
            return P.column(P.STRING, n, P.bits(mask), rng.integers(0, 3, size=k).astype(np.int32), owner=owner, **kw)

        for pos in (0, 1023, 1024, nd - 1):  # a negative length: the owner and the sub-column that checks it
            lens = ones.copy()
            lens[pos] = -1 - pos
            owner = add("negative length at %d, owner" % pos, strings(lengths=lens), P.ERR_COUNT)
            add("negative length at %d, sub-column" % pos, sub(owner), P.ERR_COUNT)
            owner = add("owner beside a bad sub-column", strings(), P.OK)
            add("negative length at %d in the sub-column's own stream" % pos, sub(owner, lengths=lens), P.ERR_COUNT)
        owner = add("lengths sum to dict_bytes + 1, owner", strings(raw=raw[:-1]), P.ERR_TRUNCATED)
        add("lengths sum to dict_bytes + 1, sub-column", sub(owner), P.ERR_TRUNCATED)
        owner = add("lengths sum to dict_bytes, owner", strings(), P.OK)
        add("lengths sum to dict_bytes, sub-column", sub(owner), P.OK)
        for lens in ([0x7FFFFFFF] * 3, [0x40000000] * 4):  # 64-bit sums: the second wraps to 0 in 32 bits
            owner = add("huge lengths, owner", strings(lengths=np.array(lens, np.int32), raw=b"0123456789"), P.ERR_TRUNCATED)
            add("huge lengths, sub-column", sub(owner), P.ERR_TRUNCATED)
        for bad in (nd, -1):  # a dictionary index out of range at the first / the last present feature
            for pos in (0, k - 1):
                idx = rng.integers(0, nd, size=k).astype(np.int32)
                idx[pos] = bad
                add("index %d at rank %d" % (bad, pos), strings(idx), P.ERR_COUNT)
            idx = rng.integers(0, nd, size=k + 1).astype(np.int32)
            idx[k] = bad
            add("index %d past the present count" % bad, strings(idx), P.OK)
        early = np.zeros(n, bool)
        early[:min(n, 300):3] = True  # every present bit in the first chunk
        for kind in "difs":
            for m, where in ((mask, "last"), (early, "first")):
                c = _mk(rng, kind, n, m)
                short = dict(c, n_data=c["n_data"] - 1)
                add("one present bit too many, %s, the surplus in the %s chunk" % (kind, where), short, P.ERR_COUNT)
            add("fewer present bits than values, %s" % kind, _mk(rng, kind, n, mask, extra=2), P.OK)
        # precedence: pairs of simultaneous faults
        neg, over = ones.copy(), ones.copy()
        neg[7] = -1
        over[9] = 2
        bad_idx = np.full(k, nd, np.int32)
        L = P.UNSUPPORTED_LATE
        add("present stream before UNSUPPORTED_LATE", strings(st=(BAD, 0, 0), flags=L), BAD)
        add("UNSUPPORTED_LATE before the data stream", strings(st=(0, BAD, 0), flags=L), P.ERR_UNSUPPORTED)
        add("UNSUPPORTED_LATE before the length stream", strings(st=(0, 0, BAD), flags=L), P.ERR_UNSUPPORTED)
        add("data stream before length stream", strings(st=(0, BAD, P.ERR_TRUNCATED)), BAD)
        add("data stream before DATA_SHORT", strings(st=(0, BAD, 0), flags=P.DATA_SHORT), BAD)
        add("length stream before DATA_SHORT", strings(st=(0, 0, BAD), flags=P.DATA_SHORT), BAD)
        add("DATA_SHORT before a negative length", strings(lengths=neg, flags=P.DATA_SHORT), P.ERR_TRUNCATED)
        add("DATA_SHORT, FLOAT", dict(_mk(rng, "f", n, mask), flags=P.DATA_SHORT), P.ERR_TRUNCATED)
        add("negative length before overrun", strings(lengths=np.where(neg < 0, neg, 2).astype(np.int32)), P.ERR_COUNT)
        add("dictionary overrun before a bad index", strings(bad_idx, lengths=over), P.ERR_TRUNCATED)
        add("dictionary overrun before a missing value", strings(lengths=over, n_data=k - 1), P.ERR_TRUNCATED)
        add("UNSUPPORTED before everything", strings(bad_idx, lengths=neg, st=(BAD, BAD, BAD), flags=P.UNSUPPORTED | L | P.DATA_SHORT),
            P.ERR_UNSUPPORTED)
        add("UNSUPPORTED, INT64", dict(_mk(rng, "i", n, mask), flags=P.UNSUPPORTED, st=(BAD, 0, 0)), P.ERR_UNSUPPORTED)
        add("present stream failed, INT64", dict(_mk(rng, "i", n, mask), st=(P.ERR_TRUNCATED, 0, 0)), P.ERR_TRUNCATED)
        add("data stream failed, dense BOOLEAN", dict(_mk(rng, "d", n, mask), st=(0, P.ERR_COUNT, 0)), P.ERR_COUNT)
    return out


def test_statuses_and_their_order(covt, gpu_available):
    rng = np.random.default_rng(4500)
    cases = _status_cases(rng)
    cache = {}
    for what, col, want in cases:  # the table agrees with the reference before either meets the GPU
        assert _reference(col, cache)[0] == want, what
    cols = [c for _, c, _ in cases]
    n_fail = sum(want != 0 for _, _, want in cases)
    assert (n_fail, len(cols) - n_fail) == (2 * 45, 2 * 12)
    split = P.split_plan(cols)
    assert sum(split) == len(cols) // 2 - 2  # (the long UNSUPPORTED columns run as single waves)
    tally = _both(covt, cols, cache, what="3e")
    assert sum(v for s, v in tally.items() if s) == n_fail and tally[0] == len(cols) - n_fail
    assert set(tally) == {0, P.ERR_UNSUPPORTED, P.ERR_TRUNCATED, P.ERR_COUNT, BAD}


# ---- 3f: graph replay -------------------------------------------------------------------------------------
def test_split_kernel_replays_in_a_hip_graph(covt, gpu_available):
    """covt_materialize_properties_device alone, captured on a side stream after one warm-up launch on it and
    replayed three times; before each replay the output and the result rows are poisoned and the present
    bitsets in the decoded buffer overwritten.  A replay that accepted the previous replay's look-back records
    (an epoch frozen into the graph) would rank its values by the old bits' counts."""
    import torch

    rng = np.random.default_rng(4600)
    n = 5 * 4096 + 77
    base = [_mk(rng, kind, m, np.ones(m, bool)) for kind, m in
            (("i", n), ("s", n), ("f", n), ("d", n), ("i", 4 * 4096), ("s", 300), ("i", 511), ("f", 2 * 4096 + 1))]
    assert sum(P.split_plan(base)) == 6

    def with_bits(seed):
        r = np.random.default_rng(seed)
        return [dict(c, present=P.bits(r.random(c["n"]) < r.choice([0.1, 0.5, 0.9]))) for c in base]

    cols = with_bits(0)
    inp, dec, rows, d, out_bytes, lays = P.pack_prop_columns(covt, cols, res_fill=RES_FILL)
    d_in, d_dec, d_rows, d_desc = _upload(inp), _upload(dec), _upload(rows), _upload(d)
    d_out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda:0")
    d_pres = torch.full((2 * len(cols),), RES_FILL, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream("cuda:0")

    def launch():
        assert covt.lib().covt_materialize_properties_device(d_in.data_ptr(), d_dec.data_ptr(), d_rows.data_ptr(),
                                                             d_desc.data_ptr(), len(cols), d_out.data_ptr(),
                                                             d_pres.data_ptr(), s.cuda_stream) == 0

    def result():
        return d_out.cpu().numpy(), d_pres.cpu().numpy().view(covt.PROP_RESULT_DTYPE), lays

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        launch()  # the stream's scratch exists before the capture (an allocation cannot be captured)
    torch.cuda.synchronize()
    assert _check(cols, *result(), {}) == {0: len(cols)}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    counts = set()
    for r in range(1, 4):
        cols = with_bits(r)
        for c, row in zip(cols, d):
            o = int(row["present_off"])
            dec[o:o + c["present"].size] = c["present"]
        d_dec.copy_(torch.from_numpy(dec))
        d_out.fill_(FILL)
        d_pres.fill_(RES_FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        buf, pres, _ = result()
        assert _check(cols, buf, pres, lays, {}) == {0: len(cols)}
        counts.add(int(pres["n_valid"][0]))
    assert len(counts) == 3  # (three different sets of bits)
    del g
    torch.cuda.synchronize()
    assert covt.release_scratch(s) == 0  # pinned by the capture: kept unless asked
    assert covt.release_scratch(s, pinned=True) >= 1
    print("propmat 3f: split kernel %d columns (6 in chunks, 2 single waves), 1 eager launch and 3 replays; "
          "statuses {0: %d}" % (len(cols), len(cols)))


# ---- 3g: tile level ---------------------------------------------------------------------------------------
def _layer(rng, L, n):
    """tests/test_gpu_gend.py _synthetic_layer's recipe at a given feature count."""
    xy = rng.integers(-200, 8400, size=(n, 2))
    cols = [W.id_column(rng.integers(0, 1 << 40, size=n).astype(np.uint64)),
            W.geometry_column(np.zeros(n, np.uint8), vertices=xy, column_type=W.CT_PLAIN, num_bits=14)]
    pres = rng.random(n) < [0.3, 0.9, 1.0, 0.5][L % 4]
    opt = lambda vals: [v if p else None for v, p in zip(vals, pres)]  # noqa: E731
    words = ["Straße", "東京", "road", "", "ŻÓŁW", "x" * 40]
    for name, vals in (("big", [int(v) for v in rng.integers(-(1 << 45), 1 << 45, size=n)]),
                       ("small", [int(v) for v in rng.integers(-5, 6, size=n)]),
                       ("mono", [int(v) for v in np.cumsum(rng.integers(0, 1 << 20, size=n))]),
                       ("f", [float(v) for v in rng.normal(size=n) * 1e3]),
                       ("s", [words[int(i)] for i in rng.integers(0, len(words), size=n)]),
                       ("b", [bool(b) for b in rng.random(n) < 0.5])):
        cols.append(W.property_column(name, opt(vals)))
    return W.layer("L%d" % L, 8192, n, cols, optimized=bool(L & 1), layer_id=L)


@pytest.fixture(scope="module")
def chunk_edge_tile():
    rng = np.random.default_rng(4700)
    return W.tile([_layer(rng, L, n) for L, n in enumerate([4095, 4096, 4097, 20000])])


@pytest.mark.parametrize("mode", [0, 1], ids=["format", "java"])
def test_gend_layers_across_chunk_edges(covt, oracle, gpu_available, chunk_edge_tile, mode):
    """Decode and materialization together: Gen D layers of 4,095 / 4,096 / 4,097 / 20,000 features with every
    property type through Plan.from_tiles and properties_host, against the oracle's decode of the tile."""
    tile = chunk_edge_tile
    plan = covt.Plan.from_tiles([tile], covt.FORMAT_GEND, mode, covt.PLAN_PROPERTIES)
    assert (plan.tile_status == 0).all()
    buf, pres = plan.properties_host()
    ost, props = oracle.walk_properties(tile, oracle.FMT_GEND)
    assert ost == 0 and len(props) == plan.num_property_columns == 24
    tally = collections.Counter()
    for k, q in enumerate(props):
        o = oracle.decode_property(tile, q, mode)
        assert (int(pres["status"][k]), int(pres["n_valid"][k])) == (o[0], o[5] if o[0] == 0 else 0), k
        tally[o[0]] += 1
        if o[0]:
            continue
        col = plan.property_column(buf, pres, k)
        _same(col.validity, o[1], "column %d validity" % k)
        _same(col.values.view(np.uint8), np.asarray(o[2]).view(np.uint8), "column %d values" % k)
        if col.type == covt.PROP_STRING:
            _same(col.dict_offsets, o[3], "column %d dictionary offsets" % k)
            _same(col.dict_bytes, o[4], "column %d dictionary bytes" % k)
    if mode == 0:
        assert tally == {0: 24}
    print("propmat 3g %s: split kernel 24 columns (24 in chunks); statuses %s" % (["format", "java"][mode], dict(tally)))

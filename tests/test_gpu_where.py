"""GPU: the where pass (covt_where.hip, include/covt.h "Property predicates") against where_ref of
tests/covt_where.py, byte for byte: covt_select_where_device on hand-made property buffers (no decode), then
Plan.select_host(pred, where=...) on every fixture tile, the DeviceBatch / DevicePlan paths, a HIP-graph replay
and decode_covt(where=...).  Every synthetic buffer starts as a fill pattern; after each call every byte outside
the mask members and the status array still holds it, and the inputs are unchanged.

The kernel's steps the cases sit around: a lane takes four features, a workgroup of 256 lanes 1,024; a batch of
at most 4,096 columns gives a column min(64, 8192 / n_columns) workgroups, a larger one gives it one wave; a
STRING clause is answered from an LDS match bitmap up to covt.where_dict_bounds() dictionary entries (read from
the library, one bound per launch shape) and entry by entry beyond.
"""
import numpy as np
import pytest

import covt_geo as G
import covt_select as S
import covt_where as W
from conftest import tile_key, tile_paths

pytestmark = pytest.mark.gpu

FILL = 0x5A
SMALL = 4096
I64MIN, I64MAX = -2 ** 63, 2 ** 63 - 1
NM = W.NULL_MATCHES


# ---- synthetic property columns ---------------------------------------------------------------------------------
def _col(t, values, valid, status=0, entries=None, **kw):
    """A property column in where_ref's form.  entries: the dictionary of a STRING column (bytes each)."""
    n = len(valid)
    vals = W.pack(values) if t == W.T_BOOLEAN else np.asarray(
        values, {W.T_INT64: np.int64, W.T_FLOAT: np.float32, W.T_STRING: np.int32}[t])
    col = dict(type=t, n_features=n, status=status, validity=W.pack(valid), values=vals)
    if entries is not None:
        raw = b"".join(entries)
        col.update(n_dict=len(entries), dict_offsets=np.cumsum([0] + [len(e) for e in entries]).astype(np.int32),
                   dict_bytes=np.frombuffer(raw, np.uint8))
    col.update(kw)
    return col


def _garbage_tail(bitmap, n, rng):
    """The same bitmap with random bits past n in its last byte."""
    out = np.array(bitmap, np.uint8)
    if n % 8:
        out[-1] = (out[-1] & ((1 << (n % 8)) - 1)) | (int(rng.integers(0, 256)) & ~((1 << (n % 8)) - 1) & 0xFF)
    return out


def _geom(n, bind, mask_in=None, flags=0, rng=None):
    """A geometry column: its feature count, its bind row (padded with -1) and its incoming mask."""
    if mask_in is None:
        mask_in = (rng or np.random.default_rng(abs(n))).choice(np.array([0, 1, 0x80, 0xFF], np.uint8), max(n, 0))
    return dict(n=n, bind=list(bind) + [-1] * (8 - len(bind)), mask=np.asarray(mask_in, np.uint8), flags=flags)


def _run(covt, props, geoms, clauses, mode, with_status=True, blob=None):
    """covt_select_where_device over hand-made buffers -> (masks per geometry column, statuses).  The property
    buffer and the select buffer are laid out here, every member padded to 16 bytes as the plan's layout rule
    pads them, with a 16-byte gap after every column; everything starts as FILL.  Checks that nothing but the
    mask members and the status array changed."""
    import torch

    a16 = S.a16
    # the property buffer
    pd = np.zeros(max(len(props), 1), covt.PROP_DESC_DTYPE)
    pr = np.zeros(max(len(props), 1), covt.PROP_RESULT_DTYPE)
    off = 0
    place = []
    for ci, c in enumerate(props):
        n, t = int(c["n_features"]), c["type"]
        real_n = int(c.get("real_n", n))  # (the features the buffers were made for, if the descriptor lies)
        nb = (real_n + 7) // 8
        vbytes = {W.T_BOOLEAN: nb, W.T_INT64: 8 * real_n}.get(t, 4 * real_n)
        o = [off, off + a16(nb), -1, -1]
        end = o[1] + a16(vbytes)
        if "dict_of" in c:
            o[2], o[3] = place[c["dict_of"]][2], place[c["dict_of"]][3]
        elif "dict_offsets" in c:
            o[2] = end
            o[3] = o[2] + a16(4 * len(c["dict_offsets"]))
            end = o[3] + a16(len(c["dict_bytes"]))
        place.append(o)
        off = end + 16
        pd[ci]["out_off"] = o
        pd[ci]["present_off"] = pd[ci]["data_off"] = pd[ci]["length_off"] = pd[ci]["dict_in_off"] = -1
        pd[ci]["res"] = -1
        pd[ci]["n_features"], pd[ci]["type"] = n, t
        pd[ci]["n_dict"] = c.get("n_dict", 0)
        pd[ci]["dict_bytes"] = len(c["dict_bytes"]) if "dict_bytes" in c else 0
        pr[ci] = (c["status"], 0)
    pbuf = np.full(max(off, 16), FILL, np.uint8)
    for c, o in zip(props, place):
        pbuf[o[0]:o[0] + len(c["validity"])] = c["validity"]
        v = np.ascontiguousarray(c["values"]).view(np.uint8).reshape(-1)
        pbuf[o[1]:o[1] + v.size] = v
        if "dict_offsets" in c and "dict_of" not in c:
            d = np.ascontiguousarray(c["dict_offsets"], np.int32).view(np.uint8)
            pbuf[o[2]:o[2] + d.size] = d
            pbuf[o[3]:o[3] + len(c["dict_bytes"])] = c["dict_bytes"]
    # the select buffer: only the mask member matters here, the slices are whole
    nc = len(geoms)
    sd = np.zeros(nc, covt.SELECT_DESC_DTYPE)
    bind = np.zeros((nc, 8), np.int32)
    soff = 0
    for gi, g in enumerate(geoms):
        n = max(g["n"], 0)
        sd[gi] = (soff, 0, g["n"], g["flags"])
        bind[gi] = g["bind"]
        soff = a16(soff + S.member_offsets(n)[3]) + 16
    sel = np.full(max(soff, 16), FILL, np.uint8)
    for gi, g in enumerate(geoms):
        o = int(sd[gi]["off"])
        sel[o:o + g["mask"].size] = g["mask"]
    blob = W.make_blob(clauses) if blob is None else blob
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    host = [pd, pbuf, pr, sd, np.frombuffer(bytes(memoryview(blob)), np.uint8), bind]
    d_pd, d_pbuf, d_pr, d_sd, d_blob, d_bind = [up(a) for a in host]
    d_sel = up(sel)
    d_st = torch.full((nc + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    st = covt.lib().covt_select_where_device(d_pd.data_ptr(), d_pbuf.data_ptr(), d_pr.data_ptr(), len(props),
                                             d_sd.data_ptr(), nc, d_blob.data_ptr(), d_bind.data_ptr(), mode,
                                             d_sel.data_ptr(), d_st.data_ptr() if with_status else None, s)
    assert st == 0
    torch.cuda.synchronize()
    for a, d in zip(host, (d_pd, d_pbuf, d_pr, d_sd, d_blob, d_bind)):  # (the inputs are read only)
        assert d.cpu().numpy().tobytes() == np.ascontiguousarray(a).view(np.uint8).tobytes()
    out = d_sel.cpu().numpy()
    status = d_st.cpu().numpy()
    assert (status[nc:] == 0x5A5A5A5A).all() and (with_status or (status == 0x5A5A5A5A).all())
    untouched = np.ones(out.size, bool)
    masks = []
    for gi, g in enumerate(geoms):
        o = int(sd[gi]["off"])
        masks.append(out[o:o + max(g["n"], 0)].copy())
        untouched[o:o + max(g["n"], 0)] = False
    assert (out[untouched] == FILL).all(), np.nonzero(untouched & (out != FILL))[0][:8]
    return masks, status[:nc]


def _check(covt, props, geoms, clauses, modes=(W.WRITE, W.AND)):
    """Both modes against where_ref: masks and statuses.  Returns the WRITE-mode masks."""
    ref_clauses = [(op, flags, lits) for _, op, flags, lits in clauses]
    first = None
    for mode in modes:
        masks, status = _run(covt, props, geoms, clauses, mode)
        for gi, g in enumerate(geoms):
            if (g["flags"] & covt.SELECT_TOO_LARGE) or g["n"] <= 0:  # nothing written, status OK
                assert masks[gi].tobytes() == g["mask"][:max(g["n"], 0)].tobytes() and status[gi] == 0, gi
                continue
            want, st = W.where_ref(props, g["n"], ref_clauses, g["bind"], g["mask"], mode)
            assert status[gi] == st, (gi, mode, status[gi], st)
            if masks[gi].tobytes() != want.tobytes():
                bad = np.nonzero(masks[gi] != want)[0]
                raise AssertionError("column %d mode %d: %d of %d differ, first at %d: %d, want %d" % (
                    gi, mode, bad.size, g["n"], bad[0], masks[gi][bad[0]], want[bad[0]]))
        first = masks if first is None else first
    return first


def _one_clause_each(covt, col, tests, n_extra_props=0):
    """Clauses tested one at a time: up to eight per launch, geometry column k bound to clause k only; the
    others are unbound there and carry NULL_MATCHES so that they hold."""
    n = int(col["n_features"])
    chunks = [[]]
    for t in tests:  # (a blob holds eight clauses and 32 values)
        if len(chunks[-1]) == 8 or sum(len(x[2]) for x in chunks[-1]) + len(t[2]) > W.MAX_VALUES:
            chunks.append([])
        chunks[-1].append(t)
    for i, chunk in enumerate(chunks):
        clauses = [("c%d" % k, op, flags | NM, lits) for k, (op, flags, lits) in enumerate(chunk)]
        geoms = [_geom(n, [0 if j == k else -1 for j in range(len(chunk))], rng=np.random.default_rng(i + k))
                 for k in range(len(chunk))]
        _check(covt, [col], geoms, clauses)


def _typed_columns(n, rng):
    """One column of each type over n features, random validity with garbage bits past n."""
    nb = (n + 7) // 8
    valid = lambda: _garbage_tail(rng.integers(0, 256, nb, dtype=np.uint8), n, rng)  # noqa: E731
    entries = [b"aa", b"b", b"", b"aa", b"ccc"]
    cols = [
        dict(type=W.T_BOOLEAN, n_features=n, status=0, validity=valid(),
             values=_garbage_tail(rng.integers(0, 256, nb, dtype=np.uint8), n, rng)),
        dict(type=W.T_INT64, n_features=n, status=0, validity=valid(), values=rng.integers(-3, 4, n).astype(np.int64)),
        dict(type=W.T_FLOAT, n_features=n, status=0, validity=valid(),
             values=rng.choice(np.array([0.25, 0.5, 0.75, np.nan, -0.0], np.float32), n)),
        _col(W.T_STRING, rng.integers(-1, 7, n), [0] * n, entries=entries),
    ]
    cols[3]["validity"] = valid()
    return cols


TYPED_CLAUSES = [("b", W.EQ, NM, [W.lit(True)]), ("i", W.GE, NM, [W.lit(0)]), ("f", W.LT, NM, [W.lit(0.5)]),
                 ("s", W.IN, NM, [W.lit("aa"), W.lit("b")])]
TYPED_BINDS = [[0, 1, 2, 3], [0, -1, -1, -1], [-1, 1, -1, -1], [-1, -1, 2, -1], [-1, -1, -1, 3]]


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_feature_counts(covt, gpu_available, n):
    """Feature counts around the lane's four, the wave, the workgroup's step and the vector tails, for every
    column type alone and all four together, with garbage validity bits past n."""
    rng = np.random.default_rng(1000 + n)
    props = _typed_columns(n, rng)
    geoms = [_geom(n, b, rng=rng) for b in TYPED_BINDS]
    masks = _check(covt, props, geoms, TYPED_CLAUSES)
    if n >= 63:
        assert all(0 < int(m.sum()) < n for m in masks)


def test_batch_sizes_give_the_same_masks(covt, gpu_available):
    """The same columns alone, in a batch of 4,096 (two workgroups a column) and of 4,097 (a wave a column): the
    same masks each time."""
    rng = np.random.default_rng(7)
    props, shared = [], []
    for n in (1, 5, 64, 257, 1500, 4097):
        base = len(props)
        props += _typed_columns(n, rng)
        shared += [_geom(n, [base + b if b >= 0 else -1 for b in row], rng=rng) for row in TYPED_BINDS[:2]]
        shared.append(_geom(n, [-1, -1, -1, base + 3], rng=rng))
    tiny = _geom(3, [-1, 1, -1, -1], mask_in=[1, 0x80, 0])  # (bound to a column of another feature count: status -6)
    outs = []
    for total in (len(shared), SMALL, SMALL + 1):
        geoms = shared + [tiny] * (total - len(shared))
        outs.append([m.tobytes() for m in _check(covt, props, geoms, TYPED_CLAUSES)[:len(shared)]])
    assert outs[0] == outs[1] == outs[2]
    one = _check(covt, props[:4], [_geom(1, [0, 1, 2, 3], mask_in=[0xFF])], TYPED_CLAUSES)  # a batch of one column
    assert len(one) == 1


def test_int64_comparisons(covt, gpu_available):
    """INT64_MIN / -1 / 0 / 1 / INT64_MAX and their neighbours around each literal, all six comparisons, IN."""
    vals = [I64MIN, I64MIN + 1, -1, 0, 1, I64MAX - 1, I64MAX, 0, 5]
    col = _col(W.T_INT64, vals, [1, 1, 1, 1, 1, 1, 1, 0, 1])
    tests = [(op, 0, [W.lit(kinds=W.INT, i=x)]) for x in (I64MIN, -1, 0, 1, I64MAX) for op in range(6)]
    tests += [(W.IN, 0, [W.lit(kinds=W.INT, i=x) for x in (I64MIN, 1, I64MAX)]),
              (W.NOT_IN, 0, [W.lit(kinds=W.INT, i=x) for x in (I64MIN + 1, 0)]), (W.IS_NULL, 0, []), (W.NOT_NULL, 0, [])]
    _one_clause_each(covt, col, tests)


def test_float_comparisons(covt, gpu_available):
    """+-0.0, NaN, +-inf, a subnormal and 0.1f against 0.1: plain IEEE comparisons on the exactly widened value."""
    sub = np.float32(1e-45)
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, sub, 0.1, -0.1, 0.0, 3.0], np.float32)
    col = _col(W.T_FLOAT, vals, [1, 1, 1, 1, 1, 1, 1, 1, 0, 1])
    lits = [0.0, -0.0, 0.1, float(np.float32(0.1)), float("inf"), float("-inf"), float(sub), 5e-324, 3.0]
    tests = [(op, 0, [W.lit(kinds=W.REAL, d=x)]) for x in lits for op in range(6)]
    tests += [(W.IN, 0, [W.lit(kinds=W.REAL, d=x) for x in (0.1, float("inf"), 3.0)]),
              (W.NOT_IN, 0, [W.lit(kinds=W.REAL, d=x) for x in (0.0, float(np.float32(0.1)))])]
    _one_clause_each(covt, col, tests)


def test_boolean_at_every_bit_position(covt, gpu_available):
    """A set value bit, a clear one and a clear validity bit at each of the eight positions of a byte."""
    for n in (8, 13, 24):
        for k in range(8):
            values = [(f % 8 == k) for f in range(n)]
            valid = [(f % 8 != (k + 3) % 8) for f in range(n)]
            col = _col(W.T_BOOLEAN, values, valid)
            _one_clause_each(covt, col, [(W.EQ, 0, [W.lit(True)]), (W.EQ, 0, [W.lit(False)]), (W.NE, 0, [W.lit(True)]),
                                         (W.IN, 0, [W.lit(False), W.lit(True)]), (W.LE, 0, [W.lit(True)]),
                                         (W.EQ, 0, [W.lit(kinds=W.BOOL, b=0x100)]), (W.IS_NULL, 0, []), (W.LT, 0, [W.lit(True)])])


def test_kind_mismatches(covt, gpu_available):
    """A literal compares only with a column of one of its kinds: EQ, the orders and IN are false, NE and NOT_IN
    true, whatever the value; a literal of several kinds serves each of them."""
    rng = np.random.default_rng(5)
    cols = _typed_columns(37, rng)
    every = {W.T_BOOLEAN: W.lit(True), W.T_INT64: W.lit(kinds=W.INT, i=1), W.T_FLOAT: W.lit(kinds=W.REAL, d=0.5),
             W.T_STRING: W.lit("aa")}
    for t, col in enumerate(cols):
        tests = []
        for u, L in every.items():
            if u != t:
                tests += [(op, 0, [L]) for op in (W.EQ, W.NE, W.LT, W.LE, W.GT, W.GE, W.IN, W.NOT_IN)]
        both = W.lit(kinds=W.BOOL | W.INT | W.REAL | W.STRING, b=1, i=1, d=0.5, s=b"aa")
        tests += [(W.EQ, 0, [both]), (W.NE, 0, [both]), (W.IN, 0, [every[(t + 1) % 4], both])]
        _one_clause_each(covt, col, tests)
    # the binding's numeric literals: 1 is INT and REAL, 0.5 REAL only, 2^53 + 1 INT only
    _one_clause_each(covt, cols[1], [(W.EQ, 0, [W.lit(1)]), (W.EQ, 0, [W.lit(1.0)]), (W.LT, 0, [W.lit(0.5)])])
    _one_clause_each(covt, cols[2], [(W.GE, 0, [W.lit(0)]), (W.LT, 0, [W.lit(2 ** 53 + 1)]), (W.EQ, 0, [W.lit(0.5)])])


# ---- strings ----------------------------------------------------------------------------------------------------
def _dictionary(n_dict, rng):
    """n_dict entries of 0 .. 5 bytes over a small alphabet (many duplicates, some empty)."""
    return [bytes(rng.choice(np.frombuffer(b"abc", np.uint8), int(rng.integers(0, 6)))) for _ in range(n_dict)]


def test_string_cases(covt, gpu_available):
    """Small dictionaries: none, one entry, duplicates, an empty entry and an empty literal, literals of 1, 15,
    16, 17 and 64 bytes, prefixes both ways, indices out of range, garbage offsets, 16 literals in one IN."""
    long_ = [b"x", b"y" * 15, b"z" * 16, b"w" * 17, b"v" * 64]
    entries = [b"trunk", b"", b"trunk_link", b"trunk", b"tru", b"motorway"] + long_ + [e[:-1] + b"!" for e in long_]
    idx = list(range(len(entries))) + [-1, len(entries), 2 ** 31 - 1, -2 ** 31, 0, 3]
    valid = [1] * len(idx)
    valid[4] = 0
    col = _col(W.T_STRING, idx, valid, entries=entries)
    tests = [(W.EQ, 0, [W.lit("trunk")]), (W.NE, 0, [W.lit("trunk")]), (W.EQ, 0, [W.lit("")]),
             (W.EQ, 0, [W.lit("trunk_")]), (W.EQ, 0, [W.lit("trunk_link")]), (W.EQ, 0, [W.lit("tr")]),
             (W.IN, 0, [W.lit(e) for e in long_]), (W.NOT_IN, 0, [W.lit(e) for e in long_ + [b""]]),
             (W.IN, 0, [W.lit(e + b"?") for e in long_]), (W.LT, 0, [W.lit("zzz")]), (W.GE, 0, [W.lit("trunk")]),
             (W.IN, 0, [W.lit("q%d" % k) for k in range(15)] + [W.lit("motorway")]),
             (W.IN, 0, [W.lit("q%d" % k) for k in range(16)]), (W.IS_NULL, 0, []), (W.NOT_NULL, 0, []),
             (W.IN, 0, [W.lit(7), W.lit("tru"), W.lit(True)])]
    _one_clause_each(covt, col, tests)
    # no dictionary at all, and one entry
    none = _col(W.T_STRING, [0, -1, 1, 0], [1, 1, 1, 0], entries=[])
    one = _col(W.T_STRING, [0, 1, -1, 0, 0], [1, 1, 1, 0, 1], entries=[b"only"])
    for c in (none, one):
        _one_clause_each(covt, c, [(W.EQ, 0, [W.lit("only")]), (W.NE, 0, [W.lit("only")]), (W.EQ, 0, [W.lit("")]),
                                   (W.NOT_IN, 0, [W.lit(""), W.lit("only")])])
    # offsets no materialization writes: negative, past the bytes, decreasing -- read clamped to the bytes
    raw = np.frombuffer(b"trunkmotorwayxx", np.uint8)
    wild = dict(type=W.T_STRING, n_features=8, status=0, validity=W.pack([1] * 8),
                values=np.array([0, 1, 2, 3, 4, 5, 6, 7], np.int32), n_dict=7,
                dict_offsets=np.array([-7, 5, 13, 2 ** 31 - 1, 5, 0, -2 ** 31, 13], np.int32), dict_bytes=raw)
    _one_clause_each(covt, wild, [(W.EQ, 0, [W.lit("trunk")]), (W.EQ, 0, [W.lit("motorway")]), (W.EQ, 0, [W.lit("xx")]),
                                  (W.EQ, 0, [W.lit("")]), (W.IN, 0, [W.lit("trunkmotorwayxx"), W.lit("trunkmotorway")])])
    # a dictionary whose bytes end before its offsets do
    cut = dict(col, dict_bytes=col["dict_bytes"][:9])
    _one_clause_each(covt, cut, [(W.EQ, 0, [W.lit("trunk")]), (W.EQ, 0, [W.lit("trun")]), (W.EQ, 0, [W.lit("")])])


def _string_bound_case(covt, n_dict, n, total, rng):
    entries = _dictionary(n_dict, rng)
    entries[-1] = b"last!"
    entries[0] = b"first"
    idx = rng.integers(-2, n_dict + 2, n)
    idx[:4] = [0, n_dict - 1, n_dict, -1]
    valid = rng.integers(0, 8, n) > 0
    valid[:4] = True
    col = _col(W.T_STRING, idx, valid, entries=entries)
    clauses = [("s", W.IN, 0, [W.lit("last!"), W.lit("abc"), W.lit("")]), ("s", W.NE, NM, [W.lit("first")])]
    geoms = [_geom(n, [0, 0], rng=rng), _geom(n, [0, -1], rng=rng), _geom(n, [-1, 0], rng=rng)]
    tiny = _geom(2, [-1, -1], mask_in=[1, 0])
    masks = _check(covt, [col], geoms + [tiny] * (total - 3), clauses)
    assert 0 < int(masks[1].sum()) < n and masks[1][1] == (idx[1] == n_dict - 1) and masks[1][2] == 0
    return [m.tobytes() for m in masks[:3]]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_string_dictionary_at_the_lds_bounds(covt, gpu_available, delta):
    """Dictionaries of bound - 1, bound and bound + 1 entries for both launch shapes (the bitmap's last word, and
    the entry-by-entry path just past it); a dictionary much longer than a wave's column (entry by entry)."""
    group, wave = covt.where_dict_bounds()
    rng = np.random.default_rng(40 + delta)
    a = _string_bound_case(covt, group + delta, 4200, 3, np.random.default_rng(50 + delta))
    b = _string_bound_case(covt, group + delta, 4200, SMALL + 1, np.random.default_rng(50 + delta))
    assert a == b  # (above the wave's bound: the same masks from the other path)
    _string_bound_case(covt, wave + delta, wave // 4 + 100, SMALL + 1, rng)
    _string_bound_case(covt, wave + delta, 9, SMALL + 1, rng)  # n_dict > 4 n: entry by entry
    _string_bound_case(covt, 63 + delta, 300, 3, rng)
    _string_bound_case(covt, 64 + delta, 300, SMALL + 1, rng)


def test_shared_dictionary_and_eight_clauses(covt, gpu_available):
    """Eight clauses at once over four columns, two of them STRING sub-columns sharing one dictionary, with and
    without NULL_MATCHES, one clause unbound; then the blob's limits: 32 values."""
    rng = np.random.default_rng(11)
    n = 777
    props = _typed_columns(n, rng)
    props.append(dict(props[3], values=rng.integers(0, 5, n).astype(np.int32),
                      validity=rng.integers(0, 256, (n + 7) // 8, dtype=np.uint8), dict_of=3))
    clauses = [("b", W.NE, NM, [W.lit(False)]), ("i", W.IN, 0, [W.lit(x) for x in (-3, -1, 0, 1, 2, 3)]),
               ("f", W.NOT_IN, NM, [W.lit(0.75)]), ("s", W.NE, 0, [W.lit("ccc")]), ("s2", W.IN, NM, [W.lit("aa"), W.lit("")]),
               ("none", W.IS_NULL, 0, []), ("i", W.NOT_NULL, 0, []), ("f", W.GE, NM, [W.lit(-1.0)])]
    geoms = [_geom(n, [0, 1, 2, 3, 4, -1, 1, 2], rng=rng), _geom(n, [0, 1, 2, 4, 3, -1, 1, 2], rng=rng),
             _geom(n, [-1, -1, -1, -1, -1, -1, 1, -1], rng=rng), _geom(n, [0, 1, 2, 3, 4, 1, 1, 2], rng=rng),
             _geom(n, [-1] * 8, rng=rng)]
    masks = _check(covt, props, geoms, clauses)
    assert 0 < int(masks[0].sum()) < n and int(masks[4].sum()) == 0  # (all unbound: "i in (...)" without NM is false)
    # an unbound clause: absent for every feature
    for flags, op, want in ((0, W.EQ, 0), (NM, W.EQ, 1), (0, W.IS_NULL, 1), (NM, W.NOT_NULL, 0), (NM, W.NOT_IN, 1)):
        m = _check(covt, props, [_geom(50, [-1], mask_in=np.ones(50, np.uint8))],
                   [("x", op, flags, [] if op >= W.IS_NULL else [W.lit(1)])])[0]
        assert m.tolist() == [want] * 50
    # no clause: everything holds; WRITE gives ones, AND normalises the incoming bytes
    m = _run(covt, props, [_geom(9, [], mask_in=[0, 1, 0x80, 0xFF, 0, 2, 0, 0, 7])], [], W.AND)[0][0]
    assert m.tolist() == [0, 1, 1, 1, 0, 1, 0, 0, 1]
    assert _run(covt, props, [_geom(9, [], mask_in=[0] * 9)], [], W.WRITE, with_status=False)[0][0].tolist() == [1] * 9
    # 32 values: two INs of 16
    many = [("i", W.IN, 0, [W.lit(x) for x in range(100, 116)]), ("i", W.NOT_IN, NM, [W.lit(x) for x in range(-2, 14)])]
    _check(covt, props, [_geom(n, [1, 1], rng=rng)], many)


def test_blob_read_clamped(covt, gpu_available):
    """A blob no covt_where_add_clause builds (counts and ranges past its arrays) is read clamped to them: the
    call completes, writes only mask bytes 0 / 1 and leaves everything else alone."""
    rng = np.random.default_rng(12)
    n = 100
    props = _typed_columns(n, rng)

    blob = W.make_blob(TYPED_CLAUSES)
    blob.n_clauses = 0xFFFFFFFF
    blob.clauses[0].first_value, blob.clauses[0].n_values = -5, 2 ** 31 - 1
    blob.clauses[3].first_value, blob.clauses[3].n_values = 31, 40
    blob.values[3].str_off, blob.values[3].str_len = 1020, 2 ** 31 - 1
    blob.values[4].str_off, blob.values[4].str_len = -9, 77
    for k in range(4, 8):
        blob.clauses[k].op, blob.clauses[k].first_value, blob.clauses[k].n_values = 77 + k, 2 ** 31 - 1, -3
    masks, status = _run(covt, props, [_geom(n, [0, 1, 2, 3, 0, 1, 2, 3], rng=rng), _geom(n, [3, 2, 1, 0], rng=rng)],
                         TYPED_CLAUSES, W.AND, blob=blob)
    assert all(set(m.tolist()) <= {0, 1} for m in masks) and status.tolist() == [0, 0]


def test_column_rule_and_statuses(covt, gpu_available):
    """A failed property column, a feature count that differs, a bind entry out of range: an all-zero mask in
    both modes and the cause in the status array, the lowest clause winning; TOO_LARGE and empty columns are
    left alone with status OK; the status array may be null."""
    rng = np.random.default_rng(13)
    n = 300
    props = _typed_columns(n, rng)
    props.append(dict(props[1], status=covt.ERR_TRUNCATED))        # 4: failed
    props.append(dict(props[2], status=covt.ERR_COUNT_MISMATCH))   # 5: failed
    props.append(dict(props[1], n_features=n - 1, real_n=n))       # 6: another feature count
    ones = np.ones(n, np.uint8)
    geoms = [_geom(n, [0, 1, 2, 3], mask_in=ones), _geom(n, [0, 4, 2, 3], mask_in=ones), _geom(n, [0, 1, 5, 3], mask_in=ones),
             _geom(n, [0, 4, 5, 3], mask_in=ones), _geom(n, [0, 6, 5, 3], mask_in=ones), _geom(n, [0, 1, 2, 7], mask_in=ones),
             _geom(n, [-2, 4, 2, 3], mask_in=ones), _geom(n, [0, 1, 2, 3], mask_in=ones, flags=covt.SELECT_TOO_LARGE),
             _geom(0, [0, 1, 2, 3]), _geom(-4, [0, 1, 2, 3]), _geom(n, [0, 1, 2, 2 ** 31 - 1], mask_in=ones),
             _geom(n, [0, 1, 2, 3, 99], mask_in=ones)]  # (slot 4 is past n_clauses: not read)
    for mode in (W.WRITE, W.AND):
        masks, status = _run(covt, props, geoms, TYPED_CLAUSES, mode)
        assert status.tolist() == [0, covt.ERR_TRUNCATED, covt.ERR_COUNT_MISMATCH, covt.ERR_TRUNCATED,
                                   covt.ERR_INVALID_ARG, covt.ERR_INVALID_ARG, covt.ERR_INVALID_ARG, 0, 0, 0,
                                   covt.ERR_INVALID_ARG, 0]
        for gi in (1, 2, 3, 4, 5, 6, 10):
            assert not masks[gi].any(), gi
        assert masks[7].tobytes() == ones.tobytes() and masks[0].any() and masks[0].tobytes() == masks[11].tobytes()
    _check(covt, props, geoms, TYPED_CLAUSES)
    # in a wave-per-column batch too, and without a status array
    many = geoms + [_geom(2, [-1, -1, -1, -1], mask_in=[1, 1])] * (SMALL + 1 - len(geoms))
    _check(covt, props, many, TYPED_CLAUSES, modes=(W.AND,))
    masks, _ = _run(covt, props, geoms, TYPED_CLAUSES, W.WRITE, with_status=False)
    assert not masks[1].any() and masks[0].any()


# ---- fixture tiles ------------------------------------------------------------------------------------------------
PREDICATES = {
    "class_in": (("class", "in", ["motorway", "trunk"]),),
    "rank_le": (("rank", "<=", 3),),
    "name_de_null": (("name:de", "is null"),),
    "text_width": (("max-text-width", "==", 100.0),),
    "class_ne": (("class", "!=", "motorway", True),),
}


def _ref_clauses(where):
    """A covt.Where as where_ref's clause list, read back from the blob's bytes."""
    blob = W.Blob.from_buffer_copy(where.tobytes())
    text = bytes(blob.text)
    out = []
    for k in range(blob.n_clauses):
        c = blob.clauses[k]
        lits = []
        for j in range(c.first_value, c.first_value + c.n_values):
            v = blob.values[j]
            lits.append(W.lit(kinds=v.kinds, b=v.b, i=v.i, d=v.d, s=text[v.str_off:v.str_off + v.str_len]))
        out.append((c.op, c.flags, lits))
    return out


class _Fixtures:
    """Every fixture tile in one plan made with properties; the references' inputs computed once."""

    def __init__(self, covt):
        paths = tile_paths()
        self.covt = covt
        self.plan = plan = covt.Plan.from_tiles([open(p, "rb").read() for p in paths], flags=covt.PLAN_PROPERTIES)
        self.zxy = [list(G.zxy_of_key(tile_key(p))) for p in paths]
        self.pbuf, self.pres = plan.properties_host()
        self.measures = plan.measures_host()
        self.geo = {}
        self.by_desc = np.zeros(plan.num_property_columns, np.int64)  # descriptor -> record
        self.by_desc[plan.props["desc_index"]] = np.arange(plan.num_property_columns)
        self._cols = {}
        self._where = {}

    def products(self, crs):
        if crs not in self.geo:
            self.geo[crs] = (self.plan.wkb_host(crs, self.zxy), self.plan.bbox_host(crs, self.zxy))
        return self.geo[crs]

    def column(self, desc):
        """Property descriptor `desc` in where_ref's form, from the host copy of the property buffer."""
        if desc not in self._cols:
            c = int(self.by_desc[desc])
            p = self.plan.props[c]
            n, t = max(int(p["n_features"]), 0), int(p["type"])
            nb = (n + 7) // 8
            seg = lambda k, size: self.pbuf[int(p["out_off"][k]):int(p["out_off"][k]) + size]  # noqa: E731
            col = dict(type=t, n_features=int(p["n_features"]), status=int(self.pres["status"][c]), validity=seg(0, nb))
            if col["status"] == 0:
                col["values"] = {W.T_BOOLEAN: lambda: seg(1, nb), W.T_INT64: lambda: seg(1, 8 * n).view(np.int64),
                                 W.T_FLOAT: lambda: seg(1, 4 * n).view(np.float32),
                                 W.T_STRING: lambda: seg(1, 4 * n).view(np.int32)}[t]()
                if t == W.T_STRING and p["out_off"][2] >= 0:
                    col.update(n_dict=int(p["n_dict"]), dict_offsets=seg(2, 4 * (int(p["n_dict"]) + 1)).view(np.int32),
                               dict_bytes=seg(3, int(p["dict_bytes"])))
            self._cols[desc] = col
        return self._cols[desc]

    def where_masks(self, name):
        """(Where, per geometry column in tile order: the WRITE-mode mask and status of where_ref)."""
        if name not in self._where:
            plan = self.plan
            where = self.covt.Where(*PREDICATES[name])
            bind = plan.where_bind(where)
            clauses = _ref_clauses(where)
            out = []
            for c in range(plan.num_geometry_columns):
                row = bind[int(plan.geom["desc_index"][c])]
                n = int(plan.select["n_features"][c])
                cols = _Lazy(self, plan.num_property_columns)
                out.append(W.where_ref(cols, n, clauses, row, np.ones(max(n, 0), np.uint8), W.WRITE) if n > 0 and not
                           int(plan.select["flags"][c]) else (np.zeros(0, np.uint8), 0))
            self._where[name] = (where, out)
        return self._where[name]


class _Lazy:
    """The property columns by descriptor index, built on first use."""

    def __init__(self, fx, n):
        self.fx, self.n = fx, n

    def __len__(self):
        return self.n

    def __getitem__(self, desc):
        return self.fx.column(desc)


@pytest.fixture(scope="module")
def fixtures(covt, gpu_available):
    return _Fixtures(covt)


# each predicate in tile pixels with a window; one in CRS84; one without a window; one without a geometric predicate
FIXTURE_CASES = [(name, "CRS_TILE", "window") for name in PREDICATES] + [
    ("class_ne", "CRS_CRS84", "window"), ("rank_le", "CRS_TILE", "plain"), ("class_in", "CRS_TILE", "none")]


@pytest.mark.parametrize("name,crs_name,geometric", FIXTURE_CASES)
def test_fixture_tiles_select_where_host(covt, fixtures, name, crs_name, geometric):
    """Plan.select_host(pred, where=...) on every fixture tile: the mask is predicate_ref AND where_ref over the
    plan's own boxes, measures and property columns, sel / offsets / bytes are select_ref over its own WKB
    column, and the where statuses are the reference's.  Over the fixture set the property predicate alone keeps
    at least one feature and drops at least one."""
    crs = getattr(covt, crs_name)
    plan, zxy = fixtures.plan, fixtures.zxy
    (wbuf, wres), (bbuf, bres) = fixtures.products(crs)
    mbuf, mres = fixtures.measures
    window = (0.0, 0.0, 2048.0, 2048.0) if crs == covt.CRS_TILE else (-20.0, -10.0, 60.0, 50.0)
    pred = {"window": covt.SelectPred(window=window, min_area=4.0, min_length=8.0), "plain": covt.SelectPred(),
            "none": None}[geometric]
    where, ref = fixtures.where_masks(name)
    kept_by_where = sum(int(m.sum()) for m, _ in ref)
    total = sum(m.size for m, _ in ref)
    assert 0 < kept_by_where < total, (name, kept_by_where, total)
    sbuf, sres = plan.select_host(pred, crs, zxy, where=where)
    assert np.array_equal(sres["status"], wres["status"])
    n_ok = n_kept = n_dropped = 0
    for c in range(plan.num_geometry_columns):
        n, o = int(plan.select["n_features"][c]), int(plan.select["off"][c])
        if n > 0 and not int(plan.select["flags"][c]):
            assert int(plan.where_status[c]) == ref[c][1], c
        if int(sres["status"][c]):
            assert int(sres["n_selected"][c]) == 0 and int(sres["n_bytes"][c]) == 0
            continue
        w = plan.wkb_column(wbuf, wres, c)
        assert len(w) == n
        want = ref[c][0].copy()
        if pred is not None:
            size = bool(pred.flags & covt.SELECT_MIN_SIZE)
            if int(bres["status"][c]) == 0 and (not size or int(mres["status"][c]) == 0):
                b, m = plan.bbox_column(bbuf, bres, c), plan.measures_column(mbuf, mres, c)
                want &= S.predicate_ref(b.xmin, b.ymin, b.xmax, b.ymax, m.area, m.length, pred)
            else:
                want[:] = 0
        mask = sbuf[o:o + n]
        assert mask.tobytes() == want.tobytes(), (c, np.nonzero(mask != want)[0][:5])
        sel, offs, data = S.select_ref(w.offsets, w.data, mask)
        col = plan.select_column(sbuf, sres, c)
        assert (int(sres["n_selected"][c]), int(sres["n_bytes"][c])) == (sel.size, data.size), c
        assert col.index.tobytes() == sel.tobytes() and col.wkb.offsets.tobytes() == offs.tobytes(), c
        assert col.wkb.data.tobytes() == data.tobytes(), c
        n_ok += 1
        n_kept += sel.size
        n_dropped += n - sel.size
    assert n_ok >= 700 and n_kept > 0 and n_dropped > 0, (n_ok, n_kept, n_dropped)


def test_where_none_is_the_existing_entry(covt, fixtures):
    """select_host without `where` is covt_plan_select_host as before, on a plan made with properties too."""
    plan = fixtures.plan
    pred = covt.SelectPred(window=(0.0, 0.0, 2048.0, 2048.0))
    a, ra = plan.select_host(pred)
    b, rb = covt.Plan.from_tiles([open(p, "rb").read() for p in tile_paths()]).select_host(pred)
    assert ra.tobytes() == rb.tobytes()
    for c in range(plan.num_geometry_columns):
        o, n = int(plan.select["off"][c]), int(plan.select["n_features"][c])
        if int(ra["status"][c]) == 0:
            assert a[o:o + n].tobytes() == b[o:o + n].tobytes()


# ---- DeviceBatch / DevicePlan, graph replay, decode_covt ------------------------------------------------------------
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
    paths = sorted(tile_paths(("omt",)), key=lambda p: tile_key(p) != "omt/5_16_20")[:n_tiles]  # (that tile first)
    plan = covt.Plan.from_tiles([open(p, "rb").read() for p in paths], flags=covt.PLAN_PROPERTIES)
    return plan, covt.DeviceBatch(plan, "cuda:0")


WHERE = (("class", "in", ["motorway", "trunk", "primary", "ocean", "lake"]), ("name:xx", "is null"),
         ("rank", "<=", 10, True))


@pytest.mark.parametrize("n_tiles", [1, 12])
def test_device_paths_match_host_path(covt, gpu_available, n_tiles):
    """DeviceBatch: decode -> assemble -> wkb / bbox / measures -> materialize -> select_predicate ->
    select_where(AND) -> select equals the host path; the same through DevicePlan with where_bind(where, blob)."""
    import torch

    plan, b = _batch(covt, n_tiles)
    pred = covt.SelectPred(window=(0.0, 0.0, 3072.0, 3072.0), min_area=4.0, min_length=8.0)
    where = covt.Where(*WHERE)
    buf_h, sres_h = plan.select_host(pred, where=where)
    wst_h = plan.where_status.copy()
    assert (sres_h["status"] == 0).any() and 0 < int(sres_h["n_selected"].sum()) < int(plan.select["n_features"].sum())
    for step in (b.decode, b.assemble, b.wkb, b.bbox, b.measures, b.materialize_properties):
        step()
    b.select_predicate(pred)
    b.select_where(where, covt.WHERE_AND)
    b.select()
    torch.cuda.synchronize()
    buf_d, sres_d = b.select_results()
    assert sres_h.tobytes() == sres_d.tobytes() and np.array_equal(b.where_status(), wst_h)
    assert _columns_equal(plan, sres_h, buf_h, buf_d) > 0
    # WRITE mode alone is the host path without a geometric predicate
    buf_w, sres_w = plan.select_host(None, where=where)
    b.select_where(where)
    b.select()
    torch.cuda.synchronize()
    buf_d, sres_d = b.select_results()
    assert sres_w.tobytes() == sres_d.tobytes() and _columns_equal(plan, sres_w, buf_w, buf_d) > 0
    # the device plan: the same bind table from its record copies, the same bytes
    opts = covt.PlanOptions(flags=covt.PLAN_PROPERTIES)
    dp = covt.DevicePlan(b.d_in, plan.offsets.astype(np.int64), plan.sizes.astype(np.int64), options=opts)
    bind = dp.where_bind(where, plan.blob)
    assert np.array_equal(bind, plan.where_bind(where))
    d_out, d_res = dp.alloc()
    d_asm, d_gres = dp.alloc_assembly()
    d_wkb, d_wres = dp.alloc_wkb()
    d_props, d_pres = dp.alloc_properties()
    d_sel, d_sres = dp.alloc_select()
    d_sel.fill_(FILL)
    d_where = torch.from_numpy(np.frombuffer(where.tobytes(), np.uint8).copy()).to(b.device)
    d_bind = torch.from_numpy(bind.reshape(-1).copy()).to(b.device)
    d_st = torch.full((max(plan.num_geometry_columns, 1),), 77, dtype=torch.int32, device=b.device)
    dp.decode(d_out, d_res)
    dp.assemble(d_out, d_res, d_asm, d_gres)
    dp.wkb(d_out, d_res, d_asm, d_gres, d_wkb, d_wres)
    dp.materialize(d_out, d_res, d_props, d_pres)
    dp.select_where(d_props, d_pres, d_where, d_bind, d_sel, covt.WHERE_WRITE, d_st)
    dp.select(d_wkb, d_wres, d_sel, d_sres)
    torch.cuda.synchronize()
    sres_p = d_sres.cpu().numpy().view(covt.SELECT_RESULT_DTYPE)[:plan.num_geometry_columns][plan.select["desc_index"]]
    assert sres_p.tobytes() == sres_w.tobytes()
    assert _columns_equal(plan, sres_w, buf_w, d_sel.cpu().numpy()[:plan.select_bytes]) > 0
    assert np.array_equal(d_st.cpu().numpy()[:plan.num_geometry_columns][plan.select["desc_index"]], plan.where_status)


@pytest.mark.parametrize("n_tiles", [1, 12])
def test_predicate_where_and_select_replay_in_a_hip_graph(covt, gpu_available, n_tiles):
    """predicate + where + select captured in one HIP graph, the blob and the bind table uploaded before the
    capture, replayed twice on its capture stream into poisoned buffers: the bytes of the eager run each time."""
    import torch

    plan, b = _batch(covt, n_tiles)
    pred = covt.SelectPred(window=(1024.0, 1024.0, 4096.0, 4096.0), keep_empty=True)
    where = covt.Where(*WHERE)
    s = torch.cuda.Stream(b.device)
    with torch.cuda.stream(s):
        for step in (b.decode, b.assemble, b.wkb, b.bbox, b.measures, b.materialize_properties):
            step(s)
        b.select_predicate(pred, s)
        b.select_where(where, covt.WHERE_AND, s)
        b.select(s)
    torch.cuda.synchronize()
    buf_e, sres_e = b.select_results()
    buf_e, sres_e, wst_e = buf_e.copy(), sres_e.copy(), b.where_status().copy()
    assert (sres_e["status"] == 0).any() and int(sres_e["n_selected"].sum()) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.select_predicate(pred, s)
        b.select_where(where, covt.WHERE_AND, s)
        b.select(s)
    for _ in range(2):
        b.d_select.fill_(FILL)
        b.d_sres.fill_(0x5A5A5A5A5A5A5A5A)
        b.d_where_status.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        buf, sres = b.select_results()
        assert sres.tobytes() == sres_e.tobytes() and np.array_equal(b.where_status(), wst_e)
        assert _columns_equal(plan, sres_e, buf_e, buf) == int((sres_e["status"] == 0).sum())
    del g
    torch.cuda.synchronize()
    covt.release_scratch(s, pinned=True)


def test_decode_covt_where(covt, gpu_available, decodable_tiles):
    """decode_covt(properties=True, select=..., where=...) on one tile: every layer's selected features are the
    ones its own properties, boxes and measures give; a layer without the named column sees the clause absent."""
    pred = covt.SelectPred(window=(0.0, 0.0, 4096.0, 4096.0))
    where = covt.Where(("class", "in", ["motorway", "trunk", "primary", "ocean", "lake"]))
    lenient = covt.Where(("class", "in", ["motorway", "trunk", "primary", "ocean", "lake"], True))
    tile = dict(decodable_tiles)["omt/5_16_20"]
    layers = covt.CovtParser.decode_covt(tile, properties=True, select=pred, where=where)
    loose = covt.CovtParser.decode_covt(tile, properties=True, select=pred, where=lenient)
    alone = covt.CovtParser.decode_covt(tile, where=where)
    with_col = without_col = kept = 0
    clauses, lenient_clauses = _ref_clauses(where), _ref_clauses(lenient)
    assert [x.layer for x in layers] == [x.layer for x in loose]
    for lc, ll in zip(layers, loose):
        la = {x.layer: x for x in alone}.get(lc.layer)
        if lc.wkb is None:
            assert lc.selected is None
            continue
        n = len(lc.wkb)
        geo = S.predicate_ref(lc.bbox.xmin, lc.bbox.ymin, lc.bbox.xmax, lc.bbox.ymax, lc.measures.area,
                              lc.measures.length, pred)
        pc = (lc.properties or {}).get("class")
        if pc is None:
            cols, row = [], [-1]
            without_col += 1
        else:
            cols = [dict(type=pc.type, n_features=pc.n_features, status=0, validity=pc.validity, values=pc.values,
                         n_dict=len(pc.dict_offsets) - 1, dict_offsets=pc.dict_offsets, dict_bytes=pc.dict_bytes)]
            row = [0]
            with_col += 1
        for got, cl, g in ((lc, clauses, geo), (ll, lenient_clauses, geo), (la, clauses, np.ones(n, np.uint8))):
            want, st = W.where_ref(cols, n, cl, row, g, W.AND)
            sel, offs, data = S.select_ref(lc.wkb.offsets, lc.wkb.data, want)
            assert st == 0 and got.selected.index.tobytes() == sel.tobytes()
            assert got.selected.wkb.offsets.tobytes() == offs.tobytes() and got.selected.wkb.data.tobytes() == data.tobytes()
        if pc is None:
            assert len(lc.selected) == 0 and len(ll.selected) == int(geo.sum())
        assert la.properties is None  # (where= implies the plan's property columns, not LayerColumns.properties)
        kept += len(lc.selected)
    assert with_col > 0 and without_col > 0 and kept > 0

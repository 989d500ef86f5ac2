"""Test helpers for the property materialization pass (covt_props.hip, include/covt.h "Property columns").

* ``prop_reference``: CovtParser.decodePropertyColumn over already-decoded arrays, as nested loops, to be
  read against oracle/covt_oracle_props.c (oracle_decode_property) and the status order of the header;
* ``dict_reference``: getStringDictionary (Arrow offsets of the int32 lengths, and the bytes);
* ``pack_prop_columns`` / ``unpack_prop_column``: the device buffers (batch input, decoded-stream buffer,
  stream-result rows, covt_prop_desc table, output layout) to run hand-made columns directly through
  ``covt_materialize_properties_device``, and the way back;
* ``split_plan``: which columns of a batch prop_split_prep cuts into chunks (the rule restated).

A column is a dict (``column`` fills the defaults):
  type     BOOLEAN / INT64 / FLOAT / STRING
  n        features
  present  uint8 bitset of ceil(n/8) bytes, LSB first, or None (every feature has a value)
  data     the dense values: BOOLEAN a uint8 bitset, INT64 int64, FLOAT uint32 words, STRING int32 indices
  n_data   values the data stream holds (BOOLEAN with DENSE_BOOL: bits)
  lengths  STRING: int32 dictionary lengths (n_dict of them);  dict: the dictionary stream's bytes
  flags    COVT_PROP_* flags
  st       statuses of the present, data and length streams' decode
  owner    STRING: the column dict whose dictionary output this sub-column shares (None: its own)
  align    FLOAT data / dictionary bytes: their input offset modulo 4
"""
from __future__ import annotations

import numpy as np

BOOLEAN, INT64, FLOAT, STRING = range(4)
DICT_OWNER, DENSE_BOOL, UNSUPPORTED, DATA_SHORT, UNSUPPORTED_LATE = 0x1, 0x2, 0x4, 0x8, 0x10
OK, ERR_UNSUPPORTED, ERR_TRUNCATED, ERR_COUNT = 0, -1, -2, -3
# covt_props.hip: kPropSplitMinFeatures, kPropSplitK, kPropSplitMaxChunks, kPropCoopMaxColumns
SPLIT_MIN, SPLIT_K, SPLIT_MAX_CHUNKS, COOP_MAX_COLUMNS = 512, 4096, 65536, 4096
_VALUE_DTYPE = {BOOLEAN: np.uint8, INT64: np.int64, FLOAT: np.uint32, STRING: np.int32}


def column(type, n, present, data, n_data=None, lengths=None, dict=None, flags=0, st=(0, 0, 0), owner=None, align=0):
    data = np.ascontiguousarray(data, dtype=_VALUE_DTYPE[type])
    if type == STRING:
        if owner is None:
            flags |= DICT_OWNER
            dict = bytes(dict)
        else:  # the owner's dictionary stream; a length stream of its own only when given
            dict = owner["dict"]
            lengths = owner["lengths"] if lengths is None else lengths
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    if present is not None:
        present = np.ascontiguousarray(present, dtype=np.uint8)
        assert present.size >= (n + 7) // 8
    n_data = int(data.size if n_data is None else n_data)
    # well-formed: the arrays hold what the sizes promise (only the values in them may be bad)
    if type == BOOLEAN:
        assert data.size >= ((n_data if flags & DENSE_BOOL else n) + 7) // 8
    else:
        assert 0 <= n_data <= data.size
    return {"type": type, "n": n, "present": present, "data": data, "n_data": n_data, "lengths": lengths,
            "dict": dict, "flags": flags, "st": tuple(st), "owner": owner, "align": align}


def bits(mask) -> np.ndarray:
    """bool[n] -> LSB-first uint8 bitset of ceil(n/8) bytes."""
    mask = np.asarray(mask, dtype=bool)
    return np.packbits(mask, bitorder="little") if mask.size else np.zeros(0, np.uint8)


def _bit(b, i):
    return (int(b[i >> 3]) >> (i & 7)) & 1


def value_bytes(type, n):
    return (n + 7) // 8 if type == BOOLEAN else 8 * n if type == INT64 else 4 * n


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def dict_reference(col):
    """(status, int32 offsets[n_dict + 1], uint8 bytes[dict_bytes]) of a STRING column's dictionary: a negative
    length anywhere -> COUNT_MISMATCH, then strings past the dictionary stream -> TRUNCATED (the trailing bytes
    no string covers are copied)."""
    lens, raw = col["lengths"], col["dict"]
    nd = len(lens)
    for i in range(nd):
        if int(lens[i]) < 0:  # (int) length: decodeString fails
            return ERR_COUNT, None, None
    acc = 0
    for i in range(nd):
        acc += int(lens[i])
    if acc > len(raw):
        return ERR_TRUNCATED, None, None
    offs = np.zeros(nd + 1, dtype=np.int32)
    acc = 0
    for i in range(nd):
        acc += int(lens[i])
        offs[i + 1] = acc
    return OK, offs, np.frombuffer(raw, dtype=np.uint8).copy()


def prop_reference(col):
    """-> (status, validity u8[ceil(n/8)], values, dict_offsets, dict_bytes, n_valid).  A column that fails has
    zeroed arrays and n_valid 0 (the header leaves its slices unspecified).  Order: UNSUPPORTED, the present
    stream, UNSUPPORTED_LATE, the data stream, the length stream, DATA_SHORT, the dictionary (negative length,
    then overrun), the feature loop (a present bit without a value, a dictionary index out of range)."""
    t, n, flags = col["type"], col["n"], col["flags"]
    nb = (n + 7) // 8
    validity = np.zeros(nb, dtype=np.uint8)
    values = np.zeros(nb if t == BOOLEAN else n, dtype=_VALUE_DTYPE[t])
    doffs = dbytes = None

    def fail(st):
        return st, np.zeros_like(validity), np.zeros_like(values), None, None, 0

    if flags & UNSUPPORTED:
        return fail(ERR_UNSUPPORTED)
    if col["st"][0]:
        return fail(col["st"][0])
    if flags & UNSUPPORTED_LATE:
        return fail(ERR_UNSUPPORTED)
    if col["st"][1]:
        return fail(col["st"][1])
    if col["st"][2]:
        return fail(col["st"][2])
    if flags & DATA_SHORT:
        return fail(ERR_TRUNCATED)
    if t == STRING:
        dst, doffs, dbytes = dict_reference(col)
        if dst:
            return fail(dst)
    present, data, dn = col["present"], col["data"], col["n_data"]
    nd = len(col["lengths"]) if t == STRING else 0
    j = n_valid = 0
    for i in range(n):
        if present is not None and not _bit(present, i):
            continue  # absent: the slot holds 0
        validity[i >> 3] |= 1 << (i & 7)
        n_valid += 1
        if t == BOOLEAN and not flags & DENSE_BOOL:  # one bit per feature
            values[i >> 3] |= _bit(data, i) << (i & 7)
            continue
        if j >= dn:  # decodedDataColumn[j++] past its end
            return fail(ERR_COUNT)
        if t == BOOLEAN:
            values[i >> 3] |= _bit(data, j) << (i & 7)
        elif t == STRING:
            k = int(data[j])
            if k < 0 or k >= nd:  # dictionaryData[index]
                return fail(ERR_COUNT)
            values[i] = k
        else:
            values[i] = data[j]
        j += 1
    return OK, validity, values, doffs, dbytes, n_valid


# ---------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------
def _a16(x):
    return (x + 15) & ~15


def _a128(x):
    return (x + 127) & ~127


def layout_sizes(col):
    """Exact bytes of validity, values, dictionary offsets, dictionary bytes (prop_layout_sizes before its
    16-byte rounding; the dictionary only for its owner)."""
    n = col["n"]
    own = col["type"] == STRING and col["owner"] is None
    return [(n + 7) // 8, value_bytes(col["type"], n), 4 * (len(col["lengths"]) + 1) if own else 0,
            len(col["dict"]) if own else 0]


def pack_prop_columns(covt, cols, gap=16, res_fill=0x5A5A5A5A):
    """-> (input u8, decoded u8, stream-result rows int32[rows, 2], PROP_DESC_DTYPE array, output bytes,
    layouts).  layouts[c] = dict(off=[4 offsets], size=[4 exact sizes], slice=[4 aligned sizes]); every
    column's slices are followed by `gap` bytes nothing may write.  Arrays that are the same object are stored
    once (many columns may share a present or data array)."""
    d = np.zeros(len(cols), dtype=covt.PROP_DESC_DTYPE)
    in_parts, dec_parts, rows = [], [], [(0, res_fill)]
    in_seen, dec_seen = {}, {}
    in_off, dec_off = 16, 0

    def put_in(key, raw, align):
        nonlocal in_off
        if key in in_seen:
            return in_seen[key]
        o = _a16(in_off) + 4 + (align & 3)
        in_parts.append((o, np.frombuffer(bytes(raw), dtype=np.uint8)))
        in_off = o + len(in_parts[-1][1]) + 3
        in_seen[key] = o
        return o

    def put_dec(arr):
        nonlocal dec_off
        if id(arr) in dec_seen:
            return dec_seen[id(arr)]
        o = _a128(dec_off)
        dec_parts.append((o, arr.view(np.uint8).reshape(-1)))
        dec_off = o + max(arr.nbytes, 1)
        dec_seen[id(arr)] = o
        return o

    def row(st):
        rows.append((st, res_fill))
        return len(rows) - 1

    layouts, out = [], 0
    for ci, col in enumerate(cols):
        t, r = col["type"], d[ci]
        r["type"], r["flags"], r["n_features"], r["n_data"] = t, col["flags"], col["n"], col["n_data"]
        r["present_off"] = r["length_off"] = r["dict_in_off"] = -1
        r["res"] = -1
        if col["present"] is not None:
            r["present_off"] = put_dec(col["present"])
            r["res"][0] = row(col["st"][0])
        if t == FLOAT:  # read in place from the input: no decode stream
            r["data_off"] = put_in(id(col["data"]), col["data"], col["align"])
        else:
            r["data_off"] = put_dec(col["data"])
            r["res"][1] = row(col["st"][1])
        if t == STRING:
            r["length_off"] = put_dec(col["lengths"])
            r["res"][2] = row(col["st"][2])
            r["n_dict"], r["dict_bytes"] = len(col["lengths"]), len(col["dict"])
            own = col if col["owner"] is None else col["owner"]  # (stored once, at the owner's alignment)
            r["dict_in_off"] = put_in(("dict", id(own)), own["dict"], own["align"])
        size = layout_sizes(col)
        lay = {"off": [0] * 4, "size": size, "slice": [_a16(s) for s in size]}
        for k in range(4):
            lay["off"][k] = out
            out += lay["slice"][k]
        out += gap
        layouts.append(lay)
    by_id = {id(c): i for i, c in enumerate(cols)}
    for ci, col in enumerate(cols):  # a sub-column that shares a dictionary points at its owner's
        if col["type"] == STRING and col["owner"] is not None:
            own = layouts[by_id[id(col["owner"])]]
            layouts[ci]["off"][2:] = own["off"][2:]
        d[ci]["out_off"] = layouts[ci]["off"]
    inp = np.full(_a16(in_off) + covt.INPUT_PADDING, 0xA5, dtype=np.uint8)
    for o, b in in_parts:
        inp[o:o + b.size] = b
    dec = np.full(_a128(dec_off) + 128, 0xC3, dtype=np.uint8)
    for o, b in dec_parts:
        dec[o:o + b.size] = b
    return inp, dec, np.asarray(rows, dtype=np.int64).astype(np.int32), d, max(out, 16), layouts


def unpack_prop_column(buf, lay, col):
    """-> (validity, values, dict_offsets, dict_bytes) of a column: the exact arrays inside its slices (the
    dictionary those of its owner; None for the other types)."""
    def seg(k, nbytes):
        return buf[lay["off"][k]:lay["off"][k] + nbytes]

    t, n = col["type"], col["n"]
    values = seg(1, value_bytes(t, n)).view(_VALUE_DTYPE[t])
    if t != STRING:
        return seg(0, (n + 7) // 8), values, None, None
    return seg(0, (n + 7) // 8), values, seg(2, 4 * (len(col["lengths"]) + 1)).view(np.int32), seg(3, len(col["dict"]))


def split_plan(cols):
    """bool per column: prop_split_prep cuts it into chunks.  None for a batch of more than 4,096 columns
    (props_kernel: one wave per column).  A column wants chunks with 512 features or more unless flagged
    UNSUPPORTED; a prep thread holds four columns, and its columns split while the chunks up to and including
    its own stay within the budget of 65,536."""
    if len(cols) > COOP_MAX_COLUMNS:
        return None
    ch = [(c["n"] + SPLIT_K - 1) // SPLIT_K if c["n"] >= SPLIT_MIN and not c["flags"] & UNSUPPORTED else 0 for c in cols]
    out, before = [], 0
    for g in range(0, len(cols), 4):
        own = sum(ch[g:g + 4])
        fits = before + own <= SPLIT_MAX_CHUNKS
        out += [fits and x > 0 for x in ch[g:g + 4]]
        before += own
    return out

"""A directed FastPFOR corpus and a plain framing walker (FastPFOR.decodePage's layout, JavaFastPFOR 0.1.12).

The random FastPFOR streams of the other tests reach the decoders' rare branches only by chance; the cases
here reach each by construction: more than 64 exceptions in a block, 32-bit blocks, exceptions of index 1,
page metadata and byte containers past the 1 KiB windows, more exception words than a batch gathers, two
pages, VariableByte tails.  `walk` restates the framing in plain Python so that a CPU test can show that every
case still has the frame it is there for, and so that the malformed set can edit single fields by name.

A stream: W[0] = L (values in pages, whole blocks of 256); per page of up to 65536 values: the whereMeta
word, the blocks' packed words, then the metadata -- the bytesize word, the byte container (per block: b, ce
and, with exceptions, maxbits and ce positions), the bitmap word, and per set bit k - 1 array k's size word and
its values, 32 of them in k words; after the last page the VariableByte tail.  Container byte q is stream byte
4 bc + (q ^ 3).
"""
import numpy as np

BLOCK, PAGE = 256, 65536
BC_CAP = 3 * PAGE // BLOCK + PAGE  # JavaFastPFOR's byteContainer size (kFpfBcCap)
RESIDUES = (0, 4, 8, 12)           # stream address modulo 16


def words(enc: bytes):
    return [int.from_bytes(enc[4 * i:4 * i + 4], "big") for i in range(len(enc) // 4)]


def walk(enc: bytes):
    """Per page of a well-formed stream: where (the whereMeta word), meta (the bytesize word), meta_words
    (bytesize word .. end of the exception arrays), bc (the container's first word), container_bytes, bitmap
    (its word), sizes {k: (size word, size)}, blocks [(b, ce, idx)], headers [container offset], next."""
    W = words(enc)
    L = W[0] - W[0] % BLOCK
    pages, p, done = [], 1, 0
    while done < L:
        n = min(L - done, PAGE)
        meta = p + W[p]
        bc, bcw = meta + 1, (W[meta] + 3) // 4
        ie = bc + bcw
        bitmap, sizes = ie, {}
        ie += 1
        for k in range(2, 33):
            if W[bitmap] >> (k - 1) & 1:
                sizes[k] = (ie, W[ie])
                ie += 1 + (W[ie] * k + 31) // 32
        cb = lambda q: enc[4 * bc + (q ^ 3)]
        blocks, headers, cur = [], [], 0
        for _ in range(n // BLOCK):
            b, ce = cb(cur), cb(cur + 1)
            blocks.append((b, ce, cb(cur + 2) - b if ce else 1))
            headers.append(cur)
            cur += 3 + ce if ce else 2
        pages.append(dict(where=p, meta=meta, meta_words=ie - meta, bc=bc, container_bytes=4 * bcw, bitmap=bitmap,
                          sizes=sizes, blocks=blocks, headers=headers, next=ie))
        p, done = ie, done + n
    return pages


def batch_exception_words(page):
    """The most exception words one batch of up to 64 blocks gathers (run_fastpfor_stream: per block with an
    array, the words holding its values plus one)."""
    best, cur = 0, {}
    for j0 in range(0, len(page["blocks"]), 64):
        tot = 0
        for b, ce, idx in page["blocks"][j0:j0 + 64]:
            if ce and idx >= 2:
                c0 = cur.get(idx, 0)
                tot += ((c0 + ce) * idx + 31) // 32 - (c0 * idx) // 32 + 1
                cur[idx] = c0 + ce
        best = max(best, tot)
    return best


def _small(rng, n):
    return rng.integers(0, 8, size=n, dtype=np.uint32)


def _with_big(rng, v, count, bits=20):
    """`count` values of v replaced by values of exactly `bits` bits."""
    at = rng.choice(v.size, size=count, replace=False)
    v[at] = (rng.integers(0, 1 << (bits - 1), size=count, dtype=np.uint64) | (1 << (bits - 1))).astype(np.uint32)
    return v


def base_values():
    """{case: uint32 values}, whole blocks (the tails are added by `cases`)."""
    rng = np.random.default_rng(20260)
    out = {}
    out["ce100"] = _with_big(rng, _small(rng, BLOCK), 100)
    v = rng.integers(0, 1 << 32, size=BLOCK, dtype=np.uint64).astype(np.uint32)
    v[::7] |= 0x80000000
    out["b32"] = v
    v = _small(rng, BLOCK)
    v[rng.choice(BLOCK, size=10, replace=False)] |= 8
    out["idx1"] = v
    blocks = []
    for k in range(2, 33):
        v = rng.integers(0, 2, size=BLOCK, dtype=np.uint32)
        blocks.append(_with_big(rng, v, 40, bits=k))
    out["widths"] = np.concatenate(blocks)
    # (20 % and 10 % of the values, as counts per block: 2,056 and 70 exceptions in all)
    out["exc40"] = np.concatenate([_with_big(rng, _small(rng, BLOCK), ce) for ce in [69, 49] + [51] * 38])
    out["small3"] = np.concatenate([_with_big(rng, _small(rng, BLOCK), ce) for ce in (23, 23, 24)])
    out["pages2"] = _small(rng, PAGE + 2 * BLOCK)
    return out


def cases(oracle):
    """[(name, encoded bytes, raw values)]: the base cases, then small3 and b32 with VariableByte tails."""
    rng = np.random.default_rng(20261)
    base = base_values()
    out = [(k, oracle.encode_fastpfor(v), v) for k, v in base.items()]
    for k in ("small3", "b32"):
        for extra in (1, 13, 255):
            t = rng.integers(0, 1 << 28, size=extra, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 28, size=extra).astype(np.uint32)
            v = np.concatenate([base[k], t])
            out.append(("%s+%d" % (k, extra), oracle.encode_fastpfor(v), v))
    return out


def rows(covt, oracle):
    """Every case at every address residue with the three ops: dicts of name, enc, residue, op, nb, nv (the
    values asked for: the coded count, and 10 more for Java's zero fill; an odd count of the x,y op is its
    COUNT_MISMATCH row), ne (output elements) and the oracle's (status, array, consumed)."""
    ops = ((covt.OP_FPF_ZZ_DELTA_I32, 0), (covt.OP_FPF_ZZ_DELTA_XY, 0), (covt.OP_FPF_DELTA_MORTON, 14))
    out = []
    for name, enc, v in cases(oracle):
        for op, nb in ops:
            for nv in (v.size, v.size + 10):
                if op == covt.OP_FPF_ZZ_DELTA_I32:
                    o = oracle.decode_fastpfor_zigzag_delta(enc, nv, len(enc), 0)
                elif op == covt.OP_FPF_ZZ_DELTA_XY:
                    o = oracle.decode_fastpfor_delta_coordinates(enc, nv, len(enc), 0) if nv % 2 == 0 else \
                        (covt.ERR_COUNT_MISMATCH, np.zeros(0, dtype=np.int32), 0)
                else:
                    o = oracle.decode_fastpfor_delta_morton_codes(enc, nv, len(enc), 0, nb)
                for r in RESIDUES:
                    out.append(dict(name=name, enc=enc, residue=r, op=op, nb=nb, nv=nv, ne=2 * nv if nb else nv,
                                    oracle=o))
    return out


def _put(enc: bytes, word: int, value: int) -> bytes:
    return enc[:4 * word] + int(value & 0xffffffff).to_bytes(4, "big") + enc[4 * word + 4:]


def _put_cbyte(enc: bytes, bc: int, q: int, value: int) -> bytes:
    at = 4 * bc + (q ^ 3)
    return enc[:at] + bytes([value & 0xff]) + enc[at + 1:]


def malformed(oracle):
    """[(name, bytes, n, good)] from small3: every truncation to whole words, then single-field edits.  good:
    the blocks before the failing one when the edit fails a block (0 otherwise)."""
    enc = oracle.encode_fastpfor(base_values()["small3"])
    n = 3 * BLOCK
    pg = walk(enc)[0]
    out = [("trunc%03d" % w, enc[:4 * w], n, 0) for w in range(len(enc) // 4)]
    k, (sw, size) = sorted(pg["sizes"].items())[0]
    absent = next(a for a in range(2, 33) if a not in pg["sizes"])
    b0 = pg["blocks"][0][0]
    h0, h2 = pg["headers"][0], pg["headers"][2]
    out += [
        ("bytesize_negative", _put(enc, pg["meta"], -1), n, 0),
        ("bytesize_above_cap", _put(enc, pg["meta"], BC_CAP + 1), n, 0),
        ("wheremeta_past_stream", _put(enc, pg["where"], len(enc) // 4 + 5), n, 0),
        ("bitmap_absent_array", _put(enc, pg["bitmap"], words(enc)[pg["bitmap"]] | 1 << (absent - 1)), n, 0),
        ("size_negative", _put(enc, sw, 0x80000000), n, 0),
        ("size_too_small", _put(enc, sw, size - 1), n, 2),  # the last block's exceptions pass the array's end
        ("b_33", _put_cbyte(enc, pg["bc"], h0, 33), n, 0),
        ("idx_0", _put_cbyte(enc, pg["bc"], h0 + 2, b0), n, 0),
        ("idx_33", _put_cbyte(enc, pg["bc"], h0 + 2, b0 + 33), n, 0),
        ("idx_33_last_block", _put_cbyte(enc, pg["bc"], h2 + 2, pg["blocks"][2][0] + 33), n, 2),
        ("L_negative", _put(enc, 0, -BLOCK), n, 0),
        ("L_not_whole_blocks", _put(enc, 0, n + 5), n + 5, 0),
        ("L_above_n", _put(enc, 0, n + BLOCK), n, 0),
    ]
    return out

"""Descriptor-level corpus for tests/test_gpu_lane.py: hand-built ORC RLE v1 streams (RunLengthIntegerReader /
RunLengthByteReader, DecodingUtils.java:257-313) aimed at the lane-per-stream decoder's byte plumbing
(covt_decode.hip LaneBytes / Pack16 / lane_rle_int / lane_rle_byte), plus a plain model of that decoder's
68-byte sliding window, used only to prove on the CPU that the corpus reaches what it aims at.

The input blob holds the streams back to back (filler bytes, never zeros, where a stream needs a given address
residue), so a read past `avail` sees a neighbour's bytes.  Expected results come from the oracle alone."""
import numpy as np

WINDOW = 68          # bytes of a lane's LDS window (covt_decode.hip kLaneSlot * 4)
FILL = 0xC3          # filler between streams (a literal header as far as any stray read is concerned)
DELTAS = (-128, -1, 0, 1, 127)
M64 = (1 << 64) - 1


def align16(x):
    return (x + 15) // 16 * 16


def vu(v):
    """writeVulong: unsigned LEB128 of v mod 2^64 (1..10 bytes)."""
    v &= M64
    out = bytearray()
    while v >= 0x80:
        out.append(0x80 | (v & 0x7f))
        v >>= 7
    out.append(v)
    return bytes(out)


def vu_len(k, salt=0):
    """A value whose LEB128 form takes exactly k bytes (1..10)."""
    lo = 0 if k == 1 else 1 << (7 * (k - 1))
    hi = (1 << min(7 * k, 64)) - 1
    return lo + (salt * 0x9E3779B97F4A7C15 + 0x55) % (hi - lo + 1)


def overlong(k, salt=0):
    """An over-long varint of k > 10 bytes with payload in every byte: readVulong masks the shift to 6 bits,
    so bytes 10.. land on bits 6.., 13.. again."""
    body = bytes(0x80 | ((salt * 37 + 11 * i + 1) & 0x7f) for i in range(k - 1))
    return body + bytes([((salt * 5 + 3) & 0x7f) | 1])


def zz(v):
    return ((v << 1) ^ (v >> 63)) & M64


def int_run(control, delta, base_bytes):
    return bytes([control, delta & 0xff]) + base_bytes


def int_lits(varints):
    assert 1 <= len(varints) <= 128
    return bytes([0x100 - len(varints)]) + b"".join(varints)


def byte_run(control, b):
    return bytes([control, b])


def byte_lits(bs):
    assert 1 <= len(bs) <= 128
    return bytes([0x100 - len(bs)]) + bytes(bs)


class Corpus:
    """rows: one dict per descriptor (in_off, avail, n, op, group, fam: prefix family, lane_only, expect: a status
    the oracle has no call for, note: what a surplus case holds)."""

    def __init__(self, covt):
        self.covt = covt
        self.blob = bytearray()
        self.rows = []
        self.int_ops = (covt.OP_RLE_I32, covt.OP_RLE_U64, covt.OP_RLE_S64)
        self.byte_ops = (covt.OP_BYTE_RLE_U8, covt.OP_BYTE_RLE_RAW)
        self.elem = {covt.OP_RLE_I32: 4, covt.OP_RLE_U64: 8, covt.OP_RLE_S64: 8, covt.OP_BYTE_RLE_U8: 1,
                     covt.OP_BYTE_RLE_RAW: 1}
        self._fam = 0

    def place(self, data, residue=None):
        if residue is not None:
            while len(self.blob) % 16 != residue % 16:
                self.blob.append(FILL)
        off = len(self.blob)
        self.blob += data
        return off

    def desc(self, off, avail, n, op, group, fam=-1, lane_only=False, expect=None, note=None):
        self.rows.append(dict(in_off=off, avail=avail, n=n, op=op, group=group, fam=fam, lane_only=lane_only,
                              expect=expect, note=note))

    def stream(self, data, n, op, group, residue=None, avail=None, **kw):
        off = self.place(data, residue)
        self.desc(off, len(data) if avail is None else avail, n, op, group, **kw)
        return off

    def new_family(self):
        self._fam += 1
        return self._fam


# ---------------------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------------------
def add_runs(c, rng):
    """Run placement (Pack16::put_run / put_bytes): every control, every delta, the run starting in every packet
    slot, num_values ending 1, 2 and PER values into the run, at its end and past it; bases of 1..10 bytes."""
    covt = c.covt
    for op in c.int_ops:
        per = 16 // c.elem[op]
        for control in range(128):
            cnt = control + 3
            pre = (control + control // per) % per
            delta = DELTAS[(control + control // 5) % 5]
            k = control % 10 + 1
            head = int_lits([vu(vu_len((control + i) % 5 + 1, control + i)) for i in range(pre)]) if pre else b""
            tail = int_lits([vu(7), vu(300), vu(1 << 40)])
            data = head + int_run(control, delta, vu(vu_len(k, control))) + tail
            off = c.place(data, residue=int(rng.integers(0, 16)))
            for into in sorted({1, 2, per, cnt, cnt + 2}):
                c.desc(off, len(data), pre + into, op, "runs")
    for op in c.byte_ops:
        for control in range(128):
            cnt = control + 3
            pre = (control + control // 16) % 16
            b = control % 6 if op == covt.OP_BYTE_RLE_U8 else (control * 29 + 7) & 0xff
            head = byte_lits([(control + i) % 6 for i in range(pre)]) if pre else b""
            data = head + byte_run(control, b) + byte_lits([1, 2, 3])
            off = c.place(data, residue=int(rng.integers(0, 16)))
            for into in sorted({1, 2, 16, cnt, cnt + 2}):
                c.desc(off, len(data), pre + into, op, "runs")
    # wrap-around: bases at 2^31 - 1, 2^32 - 1, 2^63 - 1 with a positive delta; negative zigzag bases
    for op in c.int_ops:
        per = 16 // c.elem[op]
        signed = op == covt.OP_RLE_S64
        bases = [(1 << 31) - 1, (1 << 32) - 1, (1 << 63) - 1]
        if signed:
            bases += [-1, -(1 << 31), -(1 << 62) - 12345, -(1 << 63)]
        for bi, base in enumerate(bases):
            for delta in DELTAS:
                for pre in range(per):
                    control = (17 * bi + 5 * pre + delta) % 128
                    head = int_lits([vu(9)] * pre) if pre else b""
                    data = head + int_run(control, delta, vu(zz(base) if signed else base))
                    c.stream(data, pre + control + 3, op, "runs", residue=int(rng.integers(0, 16)))


def add_literals(c, rng):
    """Literal groups of 1..128 values, varints of 1..10 bytes at every position; over-long varints (11 and 12
    bytes: the masked shift) as literals and as a run base; byte literal groups at every output offset mod 16
    and every input address mod 4 (LaneBytes::at4, Pack16::put4 and its carry over a packet edge)."""
    covt = c.covt
    for op in c.int_ops:
        for cnt in range(1, 129):
            vs = [vu(vu_len((cnt + i) % 10 + 1, cnt * 131 + i)) for i in range(cnt)]
            c.stream(int_lits(vs), cnt, op, "literals", residue=int(rng.integers(0, 16)))
        for k in (11, 12):
            for pos in range(4):
                vs = [vu(vu_len(i % 10 + 1, i)) for i in range(5)]
                vs[pos] = overlong(k, pos)
                c.stream(int_lits(vs), 5, op, "literals", residue=int(rng.integers(0, 16)))
                data = int_lits(vs[:pos]) if pos else b""
                data += int_run(4 + pos, DELTAS[pos], overlong(k, pos + 9)) + int_lits([vu(1), vu(2)])
                c.stream(data, pos + 7 + pos + 2, op, "literals", residue=int(rng.integers(0, 16)))
    for op in c.byte_ops:
        hi = 6 if op == covt.OP_BYTE_RLE_U8 else 256
        for o in range(16):
            for r in range(4):
                for ln in (8, 17, 29):
                    if o == 0:
                        head = b""
                    elif o < 3:
                        head = byte_lits([3] * o)
                    else:
                        head = byte_run(o - 3, 4)
                    body = [int(x) for x in rng.integers(0, hi, size=ln)]
                    data = head + byte_lits(body) + byte_run(2, 5)
                    # the literal bytes start at stream byte len(head) + 1: residue picks their address mod 4
                    res = (r - len(head) - 1) % 4 + 4 * int(rng.integers(0, 4))
                    c.stream(data, o + ln + 5, op, "literals", residue=res)


def add_surplus(c, rng):
    """The last literal group holds more values than num_values takes: complete (consumed covers the whole
    group) and cut by avail (the integer reader reads every literal of a group it enters; the byte reader
    needs the whole group present); GeometryType bytes above 5 among the surplus, as the last value taken
    and in a run entered for one value."""
    covt = c.covt
    for op in c.int_ops:
        for cnt in (2, 3, 5, 16, 40, 128):
            for k0 in range(4):
                vs = [vu(vu_len((k0 + 3 * i) % 10 + 1, cnt + i)) for i in range(cnt)]
                head = int_run(k0, DELTAS[k0], vu(1000 + k0))
                data = head + int_lits(vs)
                off = c.place(data, residue=int(rng.integers(0, 16)))
                pre = k0 + 3
                for take in sorted({1, cnt // 2, cnt - 1} - {0, cnt}):
                    c.desc(off, len(data), pre + take, op, "surplus", note="complete")
                    end_taken = len(head) + 1 + sum(len(v) for v in vs[:take])
                    cuts = {len(data) - 1, end_taken, end_taken + 1, (end_taken + len(data)) // 2}
                    for av in sorted(cuts):
                        if end_taken <= av < len(data):
                            c.desc(off, av, pre + take, op, "surplus")  # cut inside the surplus
    for op in c.byte_ops:
        for cnt in (2, 5, 16, 33, 128):
            for o in range(0, 16, 3):
                head = byte_run(o, 2)
                pre = o + 3
                for take in sorted({1, cnt // 2, cnt - 1} - {0, cnt}):
                    clean = [int(x) for x in rng.integers(0, 6, size=cnt)]
                    for variant in ("clean", "bad_surplus", "bad_last_taken"):
                        body = list(clean)
                        if variant == "bad_surplus":
                            for i in range(take, cnt):
                                body[i] = 6 + (i * 41) % 250
                        elif variant == "bad_last_taken":
                            body[take - 1] = 6 + (take * 17) % 250
                        data = head + byte_lits(body)
                        off = c.place(data, residue=int(rng.integers(0, 16)))
                        c.desc(off, len(data), pre + take, op, "surplus", note=variant)
                        for av in sorted({len(data) - 1, len(head) + 1 + take}):
                            if av < len(data):
                                c.desc(off, av, pre + take, op, "surplus")  # the group itself is cut
        # a run above 5 entered for its first value only / never entered
        for o in range(0, 16, 5):
            data = byte_lits([1] * (o + 1)) + byte_run(7, 200) + byte_lits([0, 1])
            off = c.place(data, residue=int(rng.integers(0, 16)))
            c.desc(off, len(data), o + 1, op, "surplus", note="bad_run_unread")  # ends before the run
            c.desc(off, len(data), o + 2, op, "surplus", note="bad_run_first")   # the run's first value is taken
            c.desc(off, len(data), o + 1 + 10 + 2, op, "surplus")


def _trailer_int(i):
    return int_run(i % 50, DELTAS[i % 5], vu(1 << (i % 40))) + int_lits([vu(vu_len(j % 3 + 1, i + j)) for j in range(40)])


def _trailer_byte(i, hi):
    return byte_run(i % 50, i % hi) + byte_lits([(i * 7 + j * 3) % hi for j in range(60)]) + byte_run(1, (i + 1) % hi)


def add_window(c, rng):
    """p one-byte literal values, then a 10-byte varint / a run header / a byte literal group, the stream at every
    address residue: every field straddles the first window edge (stream byte 68 - (address & 3)) at every
    split; p + 68 puts it across the second edge."""
    covt = c.covt
    pads = list(range(0, 71)) + [p + WINDOW for p in range(56, 71)]
    i = 0
    for p in pads:
        for r in range(4):
            res = r + 4 * ((p + r) % 4)
            for op in c.int_ops:
                i += 1
                # (i) the 10-byte varint closes the padding's literal group
                ones = [bytes([(p + j) & 0x7f]) for j in range(p)]
                groups, cnt = b"", 0
                rest = ones + [vu(vu_len(10, p + r))]
                while rest:
                    groups += int_lits(rest[:128])
                    cnt += len(rest[:128])
                    rest = rest[128:]
                tr = _trailer_int(i)
                c.stream(groups + tr, cnt + i % 50 + 3 + 40, op, "window", residue=res)
                # (ii) a run header with a 3-byte base after the padding
                groups, cnt = b"", 0
                rest = ones
                while rest:
                    groups += int_lits(rest[:128])
                    cnt += len(rest[:128])
                    rest = rest[128:]
                run = int_run(5 + i % 20, DELTAS[i % 5], vu(vu_len(3, i)))
                c.stream(groups + run + tr, cnt + 8 + i % 20 + i % 50 + 3 + 40, op, "window", residue=res)
            for op in c.byte_ops:
                i += 1
                hi = 6 if op == covt.OP_BYTE_RLE_U8 else 256
                groups, cnt = b"", 0
                rest = [(p + j) % hi for j in range(p)]
                while rest:
                    groups += byte_lits(rest[:128])
                    cnt += len(rest[:128])
                    rest = rest[128:]
                tr = _trailer_byte(i, hi)
                ntr = i % 50 + 3 + 60 + 4
                lit = byte_lits([(i + 5 * j) % hi for j in range(12)])
                c.stream(groups + lit + tr, cnt + 12 + ntr, op, "window", residue=res)
                c.stream(groups + byte_run(9, i % hi) + tr, cnt + 12 + ntr, op, "window", residue=res)


def random_stream(c, rng, op, length, max_lit=128):
    """(bytes, values) of a well-formed stream of exactly `length` bytes (>= 4) mixing runs and literal groups."""
    covt = c.covt
    is_byte = op in c.byte_ops
    hi = 6 if op == covt.OP_BYTE_RLE_U8 else 256
    data, n = bytearray(), 0
    while True:
        left = length - len(data)
        if left <= 24:
            break
        if rng.random() < 0.3:
            ctl = int(rng.integers(0, 128))
            g = byte_run(ctl, int(rng.integers(0, hi))) if is_byte else \
                int_run(ctl, int(rng.integers(-128, 128)), vu(vu_len(int(rng.integers(1, 11)), int(rng.integers(0, 999)))))
            k = ctl + 3
        else:
            k = int(rng.integers(1, max_lit + 1))
            if is_byte:
                g = byte_lits([int(x) for x in rng.integers(0, hi, size=k)])
            else:
                k = min(k, 12)
                g = int_lits([vu(vu_len(int(rng.integers(1, 11)), int(rng.integers(0, 999)))) for _ in range(k)])
        if len(g) > left - 4:
            continue
        data += g
        n += k
    left = length - len(data)
    while left > 0:  # close with literal groups of one-byte values (k + 1 bytes each) to the exact length
        assert left >= 2
        k = min(left - 1, 100)
        if left - (k + 1) == 1:
            k -= 1
        data += byte_lits([(j + left) % hi for j in range(k)]) if is_byte else \
            int_lits([bytes([(j * 5 + left) & 0x7f]) for j in range(k)])
        n += k
        left = length - len(data)
    assert len(data) == length
    return bytes(data), n


def add_lengths(c, rng):
    """Stream lengths 1, 2, 3, 63..73, 127..137, 508..516, about 1,000 and about 4,000 bytes, every op."""
    ops = c.int_ops + c.byte_ops
    for op in ops:
        for data in (b"\x05", b"\x05\x01", b"\x05\x01\x07"):
            c.stream(data, 8, op, "lengths", residue=int(rng.integers(0, 16)))
    lens = list(range(63, 74)) + list(range(127, 138)) + list(range(508, 517)) + [1000, 1003, 4000, 4001]
    for ln in lens:
        for op in ops:
            data, n = random_stream(c, rng, op, ln)
            c.stream(data, n, op, "lengths", residue=int(rng.integers(0, 16)))


def add_prefixes(c, rng):
    """A dozen streams of at most 160 bytes mixing all group kinds; one descriptor per avail in 0..length, all
    over the same input bytes (num_values: every value, or about half of them)."""
    ops = c.int_ops + c.byte_ops
    for k in range(12):
        op = ops[k % 5]
        ln = int(rng.integers(100, 161))
        data, n = random_stream(c, rng, op, ln, max_lit=20)
        if k >= 5:
            n = max(n // 2, 1)
        off = c.place(data, residue=int(rng.integers(0, 16)))
        fam = c.new_family()
        for av in range(ln + 1):
            c.desc(off, av, n, op, "prefix", fam=fam)


def add_degenerate(c, rng):
    covt = c.covt
    ops = c.int_ops + c.byte_ops
    for op in ops:
        data, n = random_stream(c, rng, op, 40, max_lit=10)
        off = c.place(data, residue=int(rng.integers(0, 16)))
        c.desc(off, len(data), 0, op, "degenerate")      # nothing asked for
        c.desc(off, 0, 0, op, "degenerate")
        c.desc(off, 0, n, op, "degenerate")              # nothing to read
        c.desc(off, len(data), -1, op, "degenerate", expect=covt.ERR_INVALID_ARG)
        c.desc(off, -1, n, op, "degenerate", expect=covt.ERR_INVALID_ARG)
    for op in (covt.OP_VARINT_I32, covt.OP_VARINT_ZZ_DELTA_I32, covt.OP_VARINT_U64):
        off = c.place(bytes([1, 2, 3, 4, 5, 6, 7, 8]))
        c.desc(off, 8, 4, op, "degenerate", lane_only=True, expect=covt.ERR_UNSUPPORTED_ENCODING)


GROUPS = (("runs", add_runs), ("literals", add_literals), ("surplus", add_surplus), ("window", add_window),
          ("lengths", add_lengths), ("prefix", add_prefixes), ("degenerate", add_degenerate))


def build_corpus(covt, seed=20240607):
    rng = np.random.default_rng(seed)
    c = Corpus(covt)
    for _, add in GROUPS:
        add(c, rng)
    return c


# ---------------------------------------------------------------------------------------------------------
# expected results (the oracle) and the window model (coverage only)
# ---------------------------------------------------------------------------------------------------------
def expected(c, oracle, row):
    """(status, values as the op's output dtype or None, consumed) of one descriptor, from the oracle."""
    covt = c.covt
    if row["expect"] is not None:
        return row["expect"], None, 0
    op, n, av = row["op"], row["n"], row["avail"]
    buf = bytes(c.blob[row["in_off"]:row["in_off"] + av])
    if op in c.byte_ops:
        st, arr, _, cons = oracle.decode_byte_rle(buf, n, 0, len(buf))
        if op == covt.OP_BYTE_RLE_U8 and st == 0 and (np.asarray(arr) > 5).any():
            st = covt.ERR_BAD_HEADER  # GeometryType.values()[b]
        vals = np.asarray(arr, dtype=np.uint8)
    else:
        st, arr, _, cons = oracle.decode_rle(buf, n, 0, op == covt.OP_RLE_S64)
        vals = np.asarray(arr, dtype=np.int64)
        if op == covt.OP_RLE_I32:
            vals = vals.astype(np.int32)  # the (int) cast of CovtParser
    if st != 0:
        return st, None, 0
    return 0, vals, cons


def window_walk(c, row):
    """The lane decoder's reads of one descriptor through its sliding window: run starts (packet slot), byte
    literal starts (output offset mod 16, address of the first literal byte mod 4) and the fields that
    straddle a window edge (kind, edge number: 1 = the first).  Returns None where the stream does not decode
    (the statuses are the oracle's business; this only locates fields)."""
    covt = c.covt
    op, n, avail, addr = row["op"], row["n"], row["avail"], row["in_off"]
    d = c.blob
    if op not in c.elem:
        return None
    is_byte = op in c.byte_ops
    raw4 = op == covt.OP_BYTE_RLE_RAW
    per = 16 if is_byte else 16 // c.elem[op]
    st = dict(w0=-(addr & 3), edges=0)
    runs, lits, straddles = [], [], []

    def touch(p, span=1):  # LaneBytes::at (span 1) / at4 (span 4)
        if p + span - st["w0"] > WINDOW:
            st["w0"] = p - ((addr + p) & 3)
            st["edges"] += 1
            return True
        return False

    def field(kind, positions):  # positions: (p, span) reads of one field, in order
        first = True
        for p, span in positions:
            if p >= avail:
                return False
            if touch(p, span) and not first:
                straddles.append((kind, st["edges"]))
            first = False
        return True

    def varint_end(p):
        while p < avail and d[addr + p] & 0x80:
            p += 1
        return p + 1  # one past the terminator (> avail: cut)

    o = done = 0
    while done < n:
        if o >= avail:
            return None
        ctl = d[addr + o]
        if ctl < 0x80:
            cnt = ctl + 3
            e = o + 2 if is_byte else varint_end(o + 2)
            if not field("run", [(p, 1) for p in range(o, e)]) or e > avail:
                return None
            runs.append(done % per)
            done += min(cnt, n - done)
            o = e
        else:
            cnt = 0x100 - ctl
            if is_byte:
                if o + 1 + cnt > avail:
                    return None
                take = min(cnt, n - done)
                reads = [(o, 1)]
                p = o + 1
                i = 0
                if raw4:
                    while i + 4 <= take:
                        reads.append((p, 4))
                        p += 4
                        i += 4
                reads += [(q, 1) for q in range(p, o + 1 + take)]
                field("bytelit", reads)
                lits.append((done % 16, (addr + o + 1) & 3, cnt))
                done += take
                o += 1 + cnt
            else:
                if not field("ctl", [(o, 1)]):
                    return None
                o += 1
                for _ in range(cnt):
                    e = varint_end(o)
                    if not field("varint", [(p, 1) for p in range(o, min(e, avail + 1))]) or e > avail:
                        return None
                    o = e
                done += min(cnt, n - done)
    return dict(runs=runs, lits=lits, straddles=straddles, consumed=o)

"""Descriptor-level corpus for tests/test_gpu_varint.py and tests/test_varint_ref.py: hand-built streams aimed at
the varint engine's own step sizes (covt_decode.hip win_load / win_value / varint_take / sink_u64: the 1 KiB window
16-byte aligned to the absolute address, groups of 256 slots, the output-line cut, the lead slots, the serial
parse of Java's capped grammar) in its three grammars -- Java's 4-byte-capped varints (DecodingUtils.java:157-186),
64-bit LEB128 and the VariableByte tail of a FastPFOR stream in word-reversed byte order -- plus

* a plain reference of the eleven varint ops and of the three FastPFOR ops over a crafted tail: pure Python and
  numpy, no ctypes; tests/test_varint_ref.py pins it to the C oracle on every descriptor the oracle has a call for;
* a model of the window sequence of a descriptor (window_walk), used only to prove on the CPU that the corpus
  reaches what it aims at.

The input blob holds the streams back to back (filler bytes where a stream needs a given address residue), so a
read past `avail` sees a neighbour's bytes."""
import numpy as np

WIN = 1024            # bytes of a window (covt_decode.hip kWin)
FILL = 0xC3           # filler between streams
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MORTON_BITS = 14


def align(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------------
# byte builders
# ---------------------------------------------------------------------------------------------------------
def vu(v):
    """Unsigned LEB128 of v mod 2^64 (1..10 bytes)."""
    v &= M64
    out = bytearray()
    while v >= 0x80:
        out.append(0x80 | (v & 0x7f))
        v >>= 7
    out.append(v)
    return bytes(out)


def zz64(v):
    return ((v << 1) ^ (v >> 63)) & M64


def jbytes(k, rng):
    """A Java-capped varint of exactly k bytes (1..4); the fourth byte ends the value whatever its bit 7."""
    body = bytes(0x80 | int(x) for x in rng.integers(0, 128, size=k - 1))
    last = int(rng.integers(0, 256)) if k == 4 else int(rng.integers(0, 128))
    return body + bytes([last])


def ubytes(k, rng):
    """A 64-bit LEB128 value of exactly k bytes (1..10; the tenth byte with bits above bit 0 half the time)."""
    body = bytes(0x80 | int(x) for x in rng.integers(0, 128, size=k - 1))
    last = int(rng.integers(0, 128))
    if k == 10 and rng.random() < 0.5:
        last &= 1
    return body + bytes([last])


def vbytes(v, k=None):
    """VariableByte form of uint32 v in k bytes (default: the shortest, 1..5): 7 bits per byte, low first, the last
    byte with bit 7 set."""
    v &= M32
    if k is None:
        k = max(1, (v.bit_length() + 6) // 7)
    return bytes((v >> (7 * i)) & 0x7f for i in range(k - 1)) + bytes([((v >> (7 * (k - 1))) & 0x7f) | 0x80])


def overlong_u64(k, salt=0):
    """A terminated 64-bit varint of k > 10 bytes with payload in every byte."""
    return bytes(0x80 | ((salt * 37 + 11 * i + 1) & 0x7f) for i in range(k - 1)) + bytes([((salt * 5 + 3) & 0x7f) | 1])


def profile_values(grammar, profile, nbytes, rng, count=None):
    """Values (bytes each) of one width profile -- "one": 1 byte, "max": 4 (Java) / 10 (64-bit), "mixed" -- filling
    about nbytes bytes, or exactly `count` values."""
    mk, top = (jbytes, 4) if grammar == "j" else (ubytes, 10)
    out, size = [], 0
    while (len(out) < count) if count is not None else (size < nbytes):
        k = 1 if profile == "one" else top if profile == "max" else int(rng.integers(1, top + 1))
        v = mk(k, rng)
        if grammar == "j" and profile == "mixed" and k == 4 and v[3] & 0x80 and rng.random() < 0.5:
            v = v[:3] + bytes([v[3] & 0x7f])
        out.append(v)
        size += len(v)
    return out


def fill_values(nbytes, count_mod, mod, rng, grammar):
    """One- and two-byte values of exactly nbytes bytes whose count is count_mod modulo mod (mod <= 32 < nbytes)."""
    f = nbytes
    while f % mod != count_mod % mod:
        f -= 1
    two = nbytes - f
    assert 0 <= two <= f
    mk = jbytes if grammar == "j" else ubytes
    vals = [mk(2, rng) if i < two else mk(1, rng) for i in range(f)]
    order = rng.permutation(f)
    return [vals[i] for i in order]


# ---------------------------------------------------------------------------------------------------------
# the plain reference
# ---------------------------------------------------------------------------------------------------------
def parse_j4(data, avail, want):
    """(raw values, end position, status) of `want` Java-capped varints from data[:avail]; status 0 or "T"."""
    vals, o = [], 0
    for _ in range(want):
        v = 0
        for i in range(4):
            if o >= avail:
                return vals, o, "T"
            b = data[o]
            o += 1
            v |= (b & 0x7f) << (7 * i)
            if i < 3 and not b & 0x80:
                break
        vals.append(v)
    return vals, o, 0


def parse_u64(data, avail, want):
    """The same for 64-bit LEB128: a terminated value of more than 10 bytes is "H", one cut by the end "T"."""
    vals, o = [], 0
    for _ in range(want):
        v, k = 0, 0
        while True:
            if o >= avail:
                return vals, o, "T"
            b = data[o]
            o += 1
            if k < 10:
                v |= (b & 0x7f) << (7 * k)
            k += 1
            if not b & 0x80:
                break
        if k > 10:
            return vals, o, "H"
        vals.append(v & M64)
    return vals, o, 0


def _zz32(u):
    u = np.asarray(u, dtype=np.uint32)
    return (u >> np.uint32(1)) ^ (np.uint32(0) - (u & np.uint32(1)))


def _zz64(u):
    u = np.asarray(u, dtype=np.uint64)
    return (u >> np.uint64(1)) ^ (np.uint64(0) - (u & np.uint64(1)))


def _sum32(u):
    return np.cumsum(np.asarray(u, dtype=np.uint32), dtype=np.uint32)


def _xy_sums(z):
    out = np.empty(z.size, dtype=np.uint32)
    out[0::2] = _sum32(z[0::2])
    out[1::2] = _sum32(z[1::2])
    return out.view(np.int32)


def morton_xy(codes, nb):
    """GeometryUtils.decodeMorton (GeometryUtils.java:34-47) on Java ints -> int32 [n, 2]."""
    c = np.asarray(codes, dtype=np.uint32).view(np.int32).astype(np.int64)  # int promoted to long
    half = np.int64(((2 << ((nb - 2) & 31)) & M32) // 2)

    def axis(c):
        r = np.zeros(c.shape, dtype=np.int64)
        for i in range(nb):
            bit = c & (np.int64(1) << np.int64((2 * i) & 63))
            r = (r | (bit >> np.int64(i & 63))).astype(np.int32).astype(np.int64)
        return r

    cy = (c.astype(np.int32) >> np.int32(1)).astype(np.int64)
    xy = np.stack([axis(c) - half, axis(cy) - half], axis=1)
    return xy.astype(np.int32)


class Reference:
    """(status, values in the op's output dtype or None, consumed) of one descriptor."""

    def __init__(self, covt):
        self.covt = covt
        c = covt
        self.java_ops = (c.OP_VARINT_I32, c.OP_VARINT_ZZ_I32, c.OP_VARINT_ZZ_DELTA_I32, c.OP_VARINT_ZZ_DELTA_XY,
                         c.OP_VARINT_DELTA_MORTON, c.OP_VARINT_I32_AS_I64, c.OP_VARINT_ZZ_I32_AS_I64,
                         c.OP_VARINT_ZZ_DELTA_I64)
        self.u64_ops = (c.OP_VARINT_U64, c.OP_VARINT_ZZ_S64, c.OP_VARINT_ZZ_DELTA_S64)
        self.fpf_ops = (c.OP_FPF_ZZ_DELTA_I32, c.OP_FPF_ZZ_DELTA_XY, c.OP_FPF_DELTA_MORTON)
        self.elem = {op: 4 for op in self.java_ops + self.fpf_ops}
        for op in (c.OP_VARINT_I32_AS_I64, c.OP_VARINT_ZZ_I32_AS_I64, c.OP_VARINT_ZZ_DELTA_I64, c.OP_VARINT_DELTA_MORTON,
                   c.OP_FPF_DELTA_MORTON) + self.u64_ops:
            self.elem[op] = 8  # bytes per value (a Morton vertex: two int32)
        # values per 128-byte output line (covt_decode.hip run_varint_stream kLine)
        self.line = {op: 128 // self.elem[op] for op in self.java_ops + self.u64_ops}
        self._parsed = {}

    def grammar(self, op):
        return "j" if op in self.java_ops else "u" if op in self.u64_ops else "v"

    def _status(self, s):
        return {0: 0, "T": self.covt.ERR_TRUNCATED, "H": self.covt.ERR_BAD_HEADER}[s]

    def varint(self, op, data, avail, n, nb=0, key=None):
        """data: the bytes at the descriptor's in_off (at least avail of them)."""
        c = self.covt
        if n < 0 or avail < 0:
            return c.ERR_INVALID_ARG, None, 0
        java = op in self.java_ops
        # Java reads the x,y pair of an odd last value before values[i + 1] overruns (DecodingUtils.java:99-105)
        want = n + (n & 1) if op == c.OP_VARINT_ZZ_DELTA_XY else n
        k = (key, java, avail, want)
        if key is None or k not in self._parsed:
            got = (parse_j4 if java else parse_u64)(data, avail, want)
            if key is None:
                return self._varint_out(op, got, n, nb)
            self._parsed[k] = got
        return self._varint_out(op, self._parsed[k], n, nb)

    def _varint_out(self, op, parsed, n, nb):
        c = self.covt
        vals, end, st = parsed
        if st:
            return self._status(st), None, 0
        if op == c.OP_VARINT_ZZ_DELTA_XY and n & 1:
            return c.ERR_COUNT_MISMATCH, None, 0
        if op in self.u64_ops:
            u = np.array(vals, dtype=np.uint64)
            if op != c.OP_VARINT_U64:
                u = _zz64(u)
            if op == c.OP_VARINT_ZZ_DELTA_S64:
                u = np.cumsum(u, dtype=np.uint64)
            return 0, u.view(np.int64), end
        u = np.array(vals, dtype=np.uint32)
        if op in (c.OP_VARINT_I32, c.OP_VARINT_I32_AS_I64):
            r = u.view(np.int32)
        elif op in (c.OP_VARINT_ZZ_I32, c.OP_VARINT_ZZ_I32_AS_I64):
            r = _zz32(u).view(np.int32)
        elif op in (c.OP_VARINT_ZZ_DELTA_I32, c.OP_VARINT_ZZ_DELTA_I64):
            r = _sum32(_zz32(u)).view(np.int32)
        elif op == c.OP_VARINT_ZZ_DELTA_XY:
            r = _xy_sums(_zz32(u))
        else:  # Morton: no zigzag
            r = morton_xy(_sum32(u), nb).reshape(-1)
        if self.elem[op] == 8 and op != c.OP_VARINT_DELTA_MORTON:
            r = r.astype(np.int64)
        return 0, np.ascontiguousarray(r), end

    def vbyte_tail(self, data, byte_length, first_word, mask=31):
        """VariableByte.uncompress over words [first_word, byte_length / 4) of a FastPFOR stream: the logical bytes
        are the LE bytes of the big-endian words; a byte with bit 7 set ends a value; int32 arithmetic with the
        shift masked to 5 bits (`mask`: for the coverage test, what another mask would give); a trailing partial value
        is dropped."""
        out, v, shift = [], 0, 0
        for q in range(first_word, byte_length // 4):
            for b in data[4 * q + 3], data[4 * q + 2], data[4 * q + 1], data[4 * q]:
                v = (v + ((b & 127) << (shift & mask))) & M32
                if b & 128:
                    out.append(v)
                    v, shift = 0, 0
                else:
                    shift += 7
        return out

    def fastpfor(self, op, data, avail, n, nb, byte_length, head):
        """A crafted-tail stream (write_fpf): `head` = the raw values of its FastPFOR pages, the VariableByte tail
        in the words after them."""
        c = self.covt
        if n < 0 or avail < 0 or byte_length < 0:
            return c.ERR_INVALID_ARG, None, 0
        raw = np.zeros(n, dtype=np.uint32)
        if byte_length // 4 > 0:
            L = len(head[0])
            if L > n:
                return c.ERR_COUNT_MISMATCH, None, 0
            raw[:L] = head[0]
            tail = self.vbyte_tail(data, byte_length, head[1])
            if L + len(tail) > n:
                return c.ERR_COUNT_MISMATCH, None, 0  # one value too many
            raw[L:L + len(tail)] = tail
        if op == c.OP_FPF_ZZ_DELTA_I32:
            r = _sum32(_zz32(raw)).view(np.int32)
        elif op == c.OP_FPF_ZZ_DELTA_XY:
            if n & 1:
                return c.ERR_COUNT_MISMATCH, None, 0
            r = _xy_sums(_zz32(raw))
        else:
            r = morton_xy(_sum32(raw), nb).reshape(-1)
        return 0, np.ascontiguousarray(r), byte_length


def write_fpf(logical, header=None, head=None, extra=0):
    """A FastPFOR stream whose VariableByte tail is `logical` (padded with 0x00 -- a partial value -- to whole
    words, each stored big-endian).  header: the count word h < 256 of a stream without a page; head: an encoded
    stream of whole 256-value blocks (it ends with no tail).  extra (0..3): bytes past the last word, which
    byte_length / 4 leaves out.  -> (stream bytes, first tail word)."""
    lg = bytes(logical) + b"\x00" * (-len(logical) % 4)
    words = b"".join(lg[i:i + 4][::-1] for i in range(0, len(lg), 4))
    pre = int(header).to_bytes(4, "big") if head is None else bytes(head)
    assert len(pre) % 4 == 0
    return pre + words + b"\xff" * extra, len(pre) // 4


# ---------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------
class Corpus:
    """rows: one dict per descriptor (in_off, avail, n, op, nb, bl: byte_length, group, fam: prefix family,
    head: (raw head values, first tail word) of a FastPFOR row, note)."""

    def __init__(self, covt):
        self.covt = covt
        self.ref = Reference(covt)
        self.blob = bytearray()
        self.rows = []
        self._fam = 0

    def place(self, data, residue=None):
        if residue is not None:
            while len(self.blob) % 16 != residue % 16:
                self.blob.append(FILL)
        off = len(self.blob)
        self.blob += data
        return off

    def desc(self, off, avail, n, op, group, fam=-1, bl=None, head=None, note=None):
        nb = MORTON_BITS if op in (self.covt.OP_VARINT_DELTA_MORTON, self.covt.OP_FPF_DELTA_MORTON) else 0
        self.rows.append(dict(in_off=off, avail=avail, n=n, op=op, nb=nb, bl=avail if bl is None else bl, group=group,
                              fam=fam, head=head, note=note))

    def ops_of(self, grammar):
        return self.ref.java_ops if grammar == "j" else self.ref.u64_ops

    def all_ops(self, off, avail, n, grammar, group, **kw):
        for op in self.ops_of(grammar):
            self.desc(off, avail, n, op, group, **kw)

    def new_family(self):
        self._fam += 1
        return self._fam

    def varint_rows(self):
        return [i for i, r in enumerate(self.rows) if r["head"] is None]

    def fpf_rows(self):
        return [i for i, r in enumerate(self.rows) if r["head"] is not None]

    def expected(self, i):
        r = self.rows[i]
        data = memoryview(self.blob)[r["in_off"]:]
        if r["head"] is not None:
            return self.ref.fastpfor(r["op"], data, r["avail"], r["n"], r["nb"], r["bl"], r["head"])
        return self.ref.varint(r["op"], data, r["avail"], r["n"], r["nb"], key=r["in_off"])


def add_counts(c, rng):
    """Every op x num_values around the lane (4), wave (256 slots) and 1024 steps x three width profiles; avail ends
    with the last value, so the stream's end is the window's valid end."""
    xy = c.covt.OP_VARINT_ZZ_DELTA_XY
    for g in ("j", "u"):
        for prof in ("one", "max", "mixed"):
            vals = profile_values(g, prof, 0, rng, count=COUNTS[-1] + 1)
            ends = np.concatenate(([0], np.cumsum([len(v) for v in vals])))
            off = c.place(b"".join(vals), residue=int(rng.integers(0, 16)))
            for n in COUNTS:
                for op in c.ops_of(g):
                    c.desc(off, int(ends[n]), n, op, "counts", note=prof)
                    if op == xy and n & 1:  # the pair is there: COUNT_MISMATCH, not TRUNCATED
                        c.desc(off, int(ends[n + 1]), n, op, "counts", note=prof)


def add_residues(c, rng):
    """All 16 address residues over a 3-window stream: the first window holds 1024 - r bytes, and the line cut and
    the lead slots take every phase."""
    for g in ("j", "u"):
        for prof in ("one", "max", "mixed"):
            for r in range(16):
                vals = profile_values(g, prof, 3 * WIN - 40 - r, rng)
                data = b"".join(vals)
                off = c.place(data, residue=r)
                c.all_ops(off, len(data), len(vals), g, "residues", note=prof)


def add_straddles(c, rng):
    """A value across the first and across a later window edge, with every split of its bytes.  64-bit: the value
    follows a whole number of output lines, so the window is left through the straddle reload and not through the
    line cut.  (Java windows always restart at the next value: there a straddling value only leaves the window's
    last bytes without a terminator.)"""
    for g, lens in (("j", (2, 3, 4)), ("u", (10,))):
        mk = jbytes if g == "j" else ubytes
        for ln in lens:
            for k in range(1, ln):
                for line in ((16, 32) if g == "j" else (16,)):
                    r = int(rng.integers(0, 16))
                    # first window: stream bytes [0, 1024 - r)
                    vals = fill_values(WIN - r - k, 0, line, rng, g) + [mk(ln, rng)]
                    p1 = WIN - r - k  # the straddler's start; the next window is aligned to its address
                    a = (r + p1) & 15
                    vals += fill_values(WIN - a - ln - k, -1, line, rng, g) + [mk(ln, rng)]
                    vals += profile_values(g, "mixed", 300, rng)
                    data = b"".join(vals)
                    off = c.place(data, residue=r)
                    c.all_ops(off, len(data), len(vals), g, "straddles", note=(ln, k))


def _cont4(rng):
    """Exactly four continuation bytes: Java's capped value, then a one-byte value so the run stays four long."""
    return bytes(0x80 | int(x) for x in rng.integers(0, 128, size=4)) + bytes([int(rng.integers(0, 128))])


def add_serial(c, rng):
    """Java ops: windows that hold four continuation bytes in a row are parsed serially."""
    def ones(nb):
        return bytes(int(x) for x in rng.integers(0, 128, size=nb))

    for k in (1, 2, 3):  # the run across a 16-byte chunk edge / across the first window edge as k | 4 - k
        for r in (0, 5, 11):
            data = ones(16 * 7 - r - k) + _cont4(rng) + ones(200)
            off = c.place(data, residue=r)
            c.all_ops(off, len(data), len(data) - 4, "j", "serial", note=("chunk", k))
            data = ones(WIN - r - k) + _cont4(rng) + ones(700)
            off = c.place(data, residue=r)
            c.all_ops(off, len(data), len(data) - 4, "j", "serial", note=("window", k))
    for where in (0, 1, 2):  # the only run of a 3-window stream in its first, a middle, the last window
        for r in (0, 9):
            data = bytearray(ones(3 * WIN - 50))
            at = where * WIN + 400
            data[at:at + 5] = _cont4(rng)
            off = c.place(bytes(data), residue=r)
            c.all_ops(off, len(data), len(data) - 4, "j", "serial", note=("pos", where))
    for k in (3, 4, 5, 7, 8, 1023, 1024, 1025, 2047, 2048, 2049):
        data = b"\x80" * k
        off = c.place(data, residue=int(rng.integers(0, 16)))
        for n in sorted({k // 4, k // 4 + 1, max(k // 4 - 1, 0)}):
            c.all_ops(off, k, n, "j", "serial", note="x80")
    # biased-random byte strings (as test_gpu_split._streams): runs of continuation bytes, capped values sprinkled in
    for p_cont in (0.5, 0.8, 0.97):
        b = rng.random(3000) < p_cont
        raw = (rng.integers(0, 128, size=b.size).astype(np.uint8) | (b.astype(np.uint8) << 7)).tobytes()
        total = len(parse_j4(raw, len(raw), 1 << 30)[0])
        off = c.place(raw, residue=int(rng.integers(0, 16)))
        for n in (total, total - 37, total + 1):
            c.all_ops(off, len(raw), n, "j", "serial", note="rand")
    z = bytearray(ones(2500))
    for k in range(0, len(z) - 8, 97):
        z[k:k + 4] = b"\xff\x81\x80\x80"
    total = len(parse_j4(z, len(z), 1 << 30)[0])
    off = c.place(bytes(z), residue=int(rng.integers(0, 16)))
    for n in (total, total // 2):
        c.all_ops(off, len(z), n, "j", "serial", note="sprinkled")


def add_u64_values(c, rng):
    """64-bit values: every length, the tenth byte with bits above bit 0, all-ones, zigzag of INT64_MIN / MAX; for
    the delta op sums that pass 2^32 and 2^63, wrap, go negative and come back, the large deltas placed so that the
    carry crosses a lane edge (4 slots), a group edge (256 slots) and a window edge."""
    edge = [vu(0), vu(1), vu(127), vu(128), vu(M64), vu(zz64(-(1 << 63))), vu(zz64((1 << 63) - 1)), vu(1 << 63),
            vu((1 << 63) - 1), vu(1 << 32), vu((1 << 32) - 1), b"\xff" * 9 + b"\x7f", b"\x80" * 9 + b"\x7e",
            b"\x80" * 9 + b"\x01", b"\x80" * 9 + b"\x02", b"\x80\x80\x00", b"\x80\x00"]
    vals = edge + [ubytes(k, rng) for k in range(1, 11) for _ in range(3)]
    for rep in range(4):
        order = rng.permutation(len(vals))
        data = b"".join(vals[i] for i in order)
        off = c.place(data, residue=int(rng.integers(0, 16)))
        c.all_ops(off, len(data), len(vals), "u", "u64values")
    big = [(1 << 32) + 12345, (1 << 62), (1 << 62), -(1 << 63) + 5, (1 << 63) - 1, -(1 << 33), -(1 << 62) - 7,
           (1 << 40), -1, 1, -(1 << 32), (1 << 63) - 1, (1 << 63) - 1, 2]
    back = -sum(big) & M64  # ... and the delta that brings the sum back
    big.append(back - (1 << 64) if back >> 63 else back)
    for at in (3, 4, 255, 256, 257, 259, 260):  # the large deltas from value `at` on: lane and group edges
        d = [int(x) for x in rng.integers(-50, 50, size=at)] + big + [int(x) for x in rng.integers(-50, 50, size=300)]
        data = b"".join(vu(zz64(x)) for x in d)
        off = c.place(data, residue=int(rng.integers(0, 16)))
        c.all_ops(off, len(data), len(d), "u", "u64values", note="carry")
    for r in (0, 7):  # ... and around the first window edge: one-byte deltas up to it
        for back in (0, 1, 3, 16, 17):
            d = [int(x) for x in rng.integers(-50, 50, size=WIN - r - back)] + big + \
                [int(x) for x in rng.integers(-50, 50, size=200)]
            data = b"".join(vu(zz64(x)) for x in d)
            off = c.place(data, residue=r)
            c.all_ops(off, len(data), len(d), "u", "u64values", note="carry")


def add_u64_overlong(c, rng):
    """One terminated value of more than 10 bytes at index 0, num_values - 1, num_values and later (an error only
    in the first two places); a run of continuation bytes to the end of the stream (the oracle runs off the end:
    TRUNCATED, however long the run)."""
    for bad in (11, 12, 40, 1000, 1024, 1025, 2100):
        for where in ("first", "last", "at_n", "later"):
            pre = [ubytes(int(rng.integers(1, 11)), rng) for _ in range(0 if where == "first" else 37)]
            post = [ubytes(int(rng.integers(1, 11)), rng) for _ in range(20)]
            data = b"".join(pre) + overlong_u64(bad, bad) + b"".join(post)
            n = {"first": 5, "last": 38, "at_n": 37, "later": 30}[where]
            off = c.place(data, residue=int(rng.integers(0, 16)))
            c.all_ops(off, len(data), n, "u", "overlong", note=(bad, where))
    for run in (5, 1000, 1024, 3000):
        for npre in (0, 37):
            pre = [ubytes(int(rng.integers(1, 11)), rng) for _ in range(npre)]
            data = b"".join(pre) + bytes(0x80 | int(x) for x in rng.integers(0, 128, size=run))
            off = c.place(data, residue=int(rng.integers(0, 16)))
            c.all_ops(off, len(data), npre + 1, "u", "overlong", note=("run", run))
            if npre:
                c.all_ops(off, len(data), npre, "u", "overlong", note=("run_unread", run))


def add_prefixes(c, rng):
    """A dozen streams of 100-160 bytes per grammar, one descriptor per avail in 0..length over the same bytes; and
    avail around the first window edge of a 3-window stream."""
    for g in ("j", "u"):
        ops = c.ops_of(g)
        for k in range(12):
            ln = int(rng.integers(100, 161))
            vals = profile_values(g, "mixed", ln, rng)
            data = b"".join(vals)
            n = len(vals) if k < 6 else max(len(vals) // 2, 1)
            if ops[k % len(ops)] == c.covt.OP_VARINT_ZZ_DELTA_XY:
                n &= ~1
            off = c.place(data, residue=int(rng.integers(0, 16)))
            fam = c.new_family()
            for av in range(len(data) + 1):
                c.desc(off, av, n, ops[k % len(ops)], "prefix", fam=fam)
        for prof in ("one", "mixed"):
            r = int(rng.integers(1, 16))
            vals = profile_values(g, prof, 3 * WIN - 100, rng)
            data = b"".join(vals)
            off = c.place(data, residue=r)
            ends = np.cumsum([len(v) for v in vals])
            for av in range(WIN - r - 2, WIN - r + 3):
                n = int(np.searchsorted(ends, av, side="right"))  # the values that end within avail
                c.all_ops(off, av, n, g, "prefix", note="edge")
                c.all_ops(off, av, n + 1, g, "prefix", note="edge")


def add_degenerate(c, rng):
    for g in ("j", "u"):
        vals = profile_values(g, "mixed", 60, rng)
        data = b"".join(vals)
        off = c.place(data, residue=int(rng.integers(0, 16)))
        n = len(vals)
        c.all_ops(off, 0, n, g, "degenerate")            # nothing to read
        c.all_ops(off, len(data), 0, g, "degenerate")    # nothing asked for
        c.all_ops(off, 0, 0, g, "degenerate")
        c.all_ops(off, -1, n, g, "degenerate")           # INVALID_ARG
        c.all_ops(off, len(data), -1, g, "degenerate")
        c.all_ops(off, len(data), n - 5, g, "degenerate")  # trailing bytes after the last value
        c.all_ops(off, len(data), n - 4, g, "degenerate")


def _vb_mixed(rng, nbytes):
    out, size = [], 0
    while size < nbytes:
        k = int(rng.integers(1, 6))
        v = int(rng.integers(0, 1 << min(7 * k, 32)))
        out.append(vbytes(v, k))
        size += k
    return out


def _vb_overlong(k, rng):
    return bytes(int(x) for x in rng.integers(1, 128, size=k - 1)) + bytes([0x80 | int(rng.integers(0, 128))])


def add_vbyte(c, rng, oracle):
    """VariableByte tails, each as a pure tail under the headers 0, 1 and 255 and after a 256- and a 512-value
    FastPFOR head."""
    covt = c.covt
    heads = []
    for nh in (256, 512):
        raw = (rng.integers(0, 1 << 20, size=nh, dtype=np.uint32) >> rng.integers(0, 20, size=nh).astype(np.uint32))
        raw[rng.integers(0, nh, size=9)] = rng.integers(1 << 24, 1 << 31, size=9, dtype=np.uint32)  # exceptions
        heads.append((raw.astype(np.uint32), oracle.encode_fastpfor(raw)))
    containers = [dict(header=h) for h in (0, 1, 255)] + [dict(head=enc, raw=raw) for raw, enc in heads]

    def emit(logical, coded, note, counts=(0,), extra=0):
        """One stream per container; num_values = head + coded + d for d in counts."""
        for ct in containers:
            raw = ct.get("raw", np.zeros(0, np.uint32))
            data, first = write_fpf(logical, header=ct.get("header"), head=ct.get("head"), extra=extra)
            off = c.place(data, residue=0)  # (the plan aligns every stream to 16 bytes: FastPFOR reads whole words)
            for op in c.ref.fpf_ops:
                for d in counts:
                    n = len(raw) + coded + d
                    if op == covt.OP_FPF_ZZ_DELTA_XY and n & 1 and d == 0:
                        n += 1  # (zero-filled by one: an even count)
                    if n >= 0:
                        c.desc(off, len(data), n, op, "vbyte", head=(raw, first), note=note)

    for cnt in (0, 1, 255, 256, 257, 1023, 1024, 1025, 3000):
        vals = [vbytes(int(x)) for x in rng.integers(0, 128, size=cnt)]
        emit(b"".join(vals), cnt, ("ones", cnt), counts=(0,) if cnt not in (257, 1025) else (0, -1, 10))
    vals = _vb_mixed(rng, 3 * WIN - 60)
    emit(b"".join(vals), len(vals), "mixed", counts=(0, -1, 10))
    for k in range(6, 13):  # over-long values: the shift masked to 5 bits
        vals = _vb_mixed(rng, 40) + [_vb_overlong(k, rng)] + _vb_mixed(rng, 40) + [_vb_overlong(k, rng)]
        emit(b"".join(vals), len(vals), ("overlong", k))
    for run in (1, 4, 5, 31, 200, 1000, 1100, 2500):  # 0x00 bytes: continuation bytes that only advance the shift
        vals = _vb_mixed(rng, 30) + [b"\x00" * run + vbytes(int(rng.integers(1, 128)), 1)] + _vb_mixed(rng, 30)
        emit(b"".join(vals), len(vals), ("zeros", run))
    vals = _vb_mixed(rng, 50)
    emit(b"".join(vals) + b"\x05\x7f\x01", len(vals), "partial")  # a trailing partial value is dropped
    vals = _vb_mixed(rng, WIN + 300)
    emit(b"".join(vals) + b"\x11" * 7, len(vals), "partial")
    for extra in (1, 2, 3):  # byte_length = 1, 2, 3 mod 4
        vals = _vb_mixed(rng, 90)
        emit(b"".join(vals), len(vals), ("extra", extra), extra=extra)
    # num_values one below the coded count with the surplus value in the second window
    vals = [vbytes(int(x)) for x in rng.integers(0, 128, size=WIN + 40)]
    emit(b"".join(vals), len(vals), "surplus2", counts=(-1, 0))
    # a 5-byte value across the first and a later window edge, 1..4 bytes before it (window byte 0 = logical byte
    # 4 * first_word & ~15 of the stream)
    for k in range(1, 5):
        for ct in containers:
            raw = ct.get("raw", np.zeros(0, np.uint32))
            first = write_fpf(b"", header=ct.get("header"), head=ct.get("head"))[1]
            vpos = 4 * first
            e1 = (vpos & ~15) + WIN
            lg = bytearray()
            cnt = 0
            for edge_no in (1, 2):
                fill = e1 - k - (vpos + len(lg)) if edge_no == 1 else None
                if edge_no == 2:
                    p1 = vpos + len(lg) - 5  # the reload put the window at the first straddler
                    fill = (p1 & ~15) + WIN - k - (vpos + len(lg))
                lg += b"".join(vbytes(int(x)) for x in rng.integers(0, 128, size=fill))
                lg += vbytes(int(rng.integers(1 << 28, 1 << 32)), 5)
                cnt += fill + 1
            tail = _vb_mixed(rng, 100)
            lg += b"".join(tail)
            cnt += len(tail)
            data, first = write_fpf(bytes(lg), header=ct.get("header"), head=ct.get("head"))
            off = c.place(data, residue=0)
            for op in c.ref.fpf_ops:
                n = len(raw) + cnt
                c.desc(off, len(data), n + (n & 1 if op == covt.OP_FPF_ZZ_DELTA_XY else 0), op, "vbyte",
                       head=(raw, first), note=("straddle", k))
    # degenerate descriptors
    data, first = write_fpf(b"".join(_vb_mixed(rng, 20)), header=0)
    off = c.place(data, residue=0)
    for op in c.ref.fpf_ops:
        c.desc(off, len(data), -1, op, "vbyte", head=(np.zeros(0, np.uint32), first), note="invalid")
        c.desc(off, 3, 4, op, "vbyte", bl=3, head=(np.zeros(0, np.uint32), first), note="nowords")
        c.desc(off, 0, 0, op, "vbyte", bl=0, head=(np.zeros(0, np.uint32), first), note="nowords")


GROUPS = (("counts", add_counts), ("residues", add_residues), ("straddles", add_straddles), ("serial", add_serial),
          ("u64values", add_u64_values), ("overlong", add_u64_overlong), ("prefix", add_prefixes),
          ("degenerate", add_degenerate), ("vbyte", add_vbyte))


def build_corpus(covt, oracle, seed=20250314):
    """oracle: only its FastPFOR encoder, for the heads of the VariableByte streams."""
    rng = np.random.default_rng(seed)
    c = Corpus(covt)
    for name, add in GROUPS:
        if name == "vbyte":
            add(c, rng, oracle)
        else:
            add(c, rng)
    return c


# ---------------------------------------------------------------------------------------------------------
# the window model (coverage only)
# ---------------------------------------------------------------------------------------------------------
def window_walk(c, row):
    """The window sequence of one descriptor as varint_take steps through it (covt_decode.hip): a list of dicts

      start   stream position the window's values start at        take    values taken from it
      serial  Java: the window holds four continuation bytes in a row and was parsed serially
      lead    slots before the first value of its first group ((out0 + got) & 3; VariableByte: 0)
      reload  (value bytes, bytes before the edge): the previous window ended inside this value and was reloaded
              at it (Java windows always start at the next value, so there it only marks the cut value)
      cut     the previous window stopped at an output line and left the line's tail to this one
      tail    only a line's tail was left in the previous window, which was restarted at it (64-bit only: Java
              windows always start at the next value)
      long    VariableByte: bytes of a value longer than the window, read on to its terminator outside the window
      runs    Java serial windows: (16-byte chunk phase, window phase) of each run of exactly four continuation bytes

    or None where the stream does not decode (statuses are the reference's business)."""
    covt, ref = c.covt, c.ref
    op, n, addr = row["op"], row["n"], row["in_off"]
    g = ref.grammar(op)
    d = c.blob
    if n < 0 or row["avail"] < 0:
        return None
    if g == "v":
        first = row["head"][1]
        end = 4 * (row["bl"] // 4)
        pos, want, line, lead_k = 4 * first, n - len(row["head"][0]), 0, 1

        def byte(q):  # logical byte q of the stream
            return d[addr + (q & ~3) + 3 - (q & 3)]

        def aligned(q):
            return q & ~15
        term = lambda b: bool(b & 0x80)
    else:
        end = row["avail"]
        pos, line, lead_k = 0, ref.line[op], 4
        want = n - (n & 1) if op == covt.OP_VARINT_ZZ_DELTA_XY else n

        def byte(q):
            return d[addr + q]

        def aligned(q):
            return ((addr + q) & ~15) - addr
        term = lambda b: not b & 0x80
    out = []
    got = 0
    woff = None
    ends = []       # positions of the terminators the window indexes
    pending = {}    # what the next window record carries
    until_end = g == "v"
    while (pos < end) if until_end else (got < want):
        if woff is None or pos < woff or pos >= woff + WIN or g == "j":
            woff, ends, serial, runs = _load(byte, term, g, aligned(pos), pos, end, addr)
        have = [e for e in ends if e >= pos]
        if not have:
            if woff != aligned(pos):
                ln = _value_len(byte, term, g, pos, end)
                pending["reload"] = (ln, woff + WIN - pos)
                woff, ends, serial, runs = _load(byte, term, g, aligned(pos), pos, end, addr)
                continue
            if until_end:
                q = pos  # a VariableByte value longer than the window is read on to its terminator
                while woff + WIN < end and q < end and not term(byte(q)):
                    q += 1
                if woff + WIN < end and q < end:
                    if got >= want:
                        return None
                    out.append(dict(start=pos, take=1, serial=False, lead=0, runs=[], woff=woff, reload=None, cut=False,
                                    tail=False, line=0, long=q - pos + 1))
                    pos, got = q + 1, got + 1
                    continue
                break
            return None
        take = len(have)
        if until_end:
            if got + take > want:
                return None
        else:
            take = min(take, want - got)
        cut = 0
        if line and not until_end and got + take < want:
            cut = (got + take) & (line - 1)
            if cut < take:
                take -= cut
            else:
                cut = 0
                if woff != aligned(pos):
                    pending["tail"] = True
                    woff, ends, serial, runs = _load(byte, term, g, aligned(pos), pos, end, addr)
                    continue
        rec = dict(start=pos, take=take, serial=serial, lead=(got & (lead_k - 1)), runs=runs, woff=woff,
                   reload=pending.pop("reload", None), cut=pending.pop("cut", False), tail=pending.pop("tail", False),
                   line=line)
        out.append(rec)
        pos = have[take - 1] + 1
        got += take
        if cut:
            pending["cut"] = True
        if g == "j" and got < want and take == len(have) and woff + WIN <= end:
            # the window ran out inside a value: the next one starts at it
            k = woff + WIN - pos
            if k > 0:
                pending["reload"] = (_value_len(byte, term, g, pos, end), k)
    if until_end and got > want:
        return None
    return out


def _value_len(byte, term, g, pos, end):
    q = pos
    while q < end and not term(byte(q)) and not (g == "j" and q - pos == 3):
        q += 1
    return q - pos + 1


def _load(byte, term, g, woff, p, end, addr):
    """win_load: -> (woff, positions of the indexed terminators, serial, runs)."""
    lim = min(end, woff + WIN)
    lo = p if g == "j" else max(woff, 0)
    bs = [byte(q) for q in range(lo, lim)]
    runs = []
    serial = False
    if g == "j":
        q = 0
        while q < len(bs):
            if bs[q] & 0x80:
                e = q
                while e < len(bs) and bs[e] & 0x80:
                    e += 1
                if e - q >= 4:
                    serial = True
                    if e - q == 4:
                        runs.append(((addr + lo + q) & 15, lo + q - woff))
                q = e
            else:
                q += 1
        ends, q = [], 0
        while q < len(bs):  # DecodingUtils.java:157-186 (the indexed parse finds the same ends without such runs)
            k = 0
            while k < 3 and q + k < len(bs) and bs[q + k] & 0x80:
                k += 1
            if q + k >= len(bs):
                break
            ends.append(lo + q + k)
            q += k + 1
        return woff, ends, serial, runs
    return woff, [lo + i for i, b in enumerate(bs) if term(b)], False, runs

// covt_split_plan.h -- split chunks: the descriptor layout of a chunk group, the rules that decide which
// streams split, and the FastPFOR framing the planners walk for the chunks' start states.  The one statement
// of the contract between the host plan (covt_host.cpp), the device plan (covt_plan_device.hip) and the
// chunk kernels (covt_decode.hip); include/covt.h describes it for callers.  Plain arithmetic, no HIP calls,
// so a host-only program can include it (tests/split_plan).
#ifndef COVT_SPLIT_PLAN_H
#define COVT_SPLIT_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "covt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_SPLIT_HD __host__ __device__
#else
#define COVT_SPLIT_HD
#endif

// ---- The layout --------------------------------------------------------------------------------------
// A chunk is a group of COVT_SPLIT_SLOTS consecutive descriptors: the head (the stream's descriptor with
// flags COVT_DESC_SPLIT | kind and avail = the chunk's index) and seven pads (COVT_DESC_SPLIT_PAD | kind),
// which reuse the descriptor's fields by position and are zero elsewhere:
//   pad 1      in_off / out_off: the chunk's range [s, e), stream-relative bytes (values for FastPFOR)
//   pad 2, 3   ORC RLE: (first value, values) and the bytes the whole stream consumes
//   pads 2..7  FastPFOR: kFpfStateSlots int32 start-state slots, seven per pad (fpf_state_slot)
enum : int {
    kSplitPadRange = 1,
    kSplitPadRleValues = 2,
    kSplitPadRleConsumed = 3,
    kSplitPadFpfState = 2,  // the first of the state pads
};
// A FastPFOR chunk's start state, as the planner's walk of the headers before the chunk leaves it; all
// slots zero: no state, the chunk walks the headers itself.
enum : int {
    kFpfStPresent = 0,  // 1: the state is there
    kFpfStPage = 1,     // the first value of the chunk's page
    kFpfStHeader = 2,   // container offset of the chunk's first block header
    kFpfStWord = 3,     // stream word of its packed data
    kFpfStCursor = 4,   // + k: the exception cursor of dataTobePacked array k, k = 0..32
    kFpfStUsed = kFpfStCursor + 33,
};
constexpr int kFpfStatePerPad = 7;  // every field but op / num_bits / flags
constexpr int kFpfStateSlots = 42;
COVT_SPLIT_HD constexpr int covt_fpf_state_byte(int k) { return k < 6 ? 4 * k : 28; }

static_assert(COVT_SPLIT_SLOTS == 8, "a chunk group: the head and seven pads");
static_assert(sizeof(covt_stream_desc) == 32 && kFpfStateSlots == (COVT_SPLIT_SLOTS - kSplitPadFpfState) * kFpfStatePerPad &&
                  kFpfStUsed <= kFpfStateSlots,
              "the FastPFOR state fits pads 2..7");
// every slot of a pad lies inside the descriptor and clear of the field at [lo, lo + size)
constexpr bool fpf_state_clear_of(size_t lo, size_t size) {
    for (int k = 0; k < kFpfStatePerPad; ++k) {
        const size_t b = (size_t)covt_fpf_state_byte(k);
        if (b + 4 > sizeof(covt_stream_desc) || (b < lo + size && lo < b + 4)) return false;
    }
    return true;
}
static_assert(fpf_state_clear_of(offsetof(covt_stream_desc, op), sizeof(uint8_t)) &&
                  fpf_state_clear_of(offsetof(covt_stream_desc, num_bits), sizeof(uint8_t)) &&
                  fpf_state_clear_of(offsetof(covt_stream_desc, flags), sizeof(uint16_t)),
              "no state slot overlaps op / num_bits / flags");

// state slot m of the chunk whose head is group[0]
COVT_SPLIT_HD inline int32_t* fpf_state_slot(covt_stream_desc* group, int m) {
    return (int32_t*)((uint8_t*)(group + kSplitPadFpfState + m / kFpfStatePerPad) + covt_fpf_state_byte(m % kFpfStatePerPad));
}
COVT_SPLIT_HD inline const int32_t* fpf_state_slot(const covt_stream_desc* group, int m) {
    return (const int32_t*)((const uint8_t*)(group + kSplitPadFpfState + m / kFpfStatePerPad) +
                            covt_fpf_state_byte(m % kFpfStatePerPad));
}

// One chunk: its range [s, e) and, for ORC RLE, its values [v0, v0 + nv)
struct SplitChunk {
    int32_t s, e, v0, nv;
};
// chunk c of a varint (unit: bytes, total: byte_length) or FastPFOR (values, num_values) stream
COVT_SPLIT_HD inline SplitChunk split_unit_chunk(int64_t c, int64_t unit, int64_t total) {
    return SplitChunk{(int32_t)(c * unit), (int32_t)((c + 1) * unit < total ? (c + 1) * unit : total), 0, 0};
}
COVT_SPLIT_HD inline int64_t split_unit_chunks(int64_t unit, int64_t total) { return (total + unit - 1) / unit; }

COVT_SPLIT_HD inline bool split_family(int fam) {
    return fam == COVT_FAMILY_SPLIT || fam == COVT_FAMILY_SPLIT_FPF || fam == COVT_FAMILY_SPLIT_RLE;
}
COVT_SPLIT_HD inline uint16_t split_kind_flag(int fam) {
    return fam == COVT_FAMILY_SPLIT_FPF ? COVT_DESC_SPLIT_FPF : fam == COVT_FAMILY_SPLIT_RLE ? COVT_DESC_SPLIT_RLE : 0;
}

// The writer: descriptor `slot` of chunk c of the stream with descriptor `stream`, split as family fam.
// rle_consumed counts only for COVT_FAMILY_SPLIT_RLE; a FastPFOR chunk's state pads start zero (no state).
COVT_SPLIT_HD inline covt_stream_desc split_slot_desc(const covt_stream_desc& stream, int fam, int64_t c, int slot,
                                                      const SplitChunk& ch, int32_t rle_consumed) {
    const uint16_t kind = split_kind_flag(fam);
    if (slot == 0) {
        covt_stream_desc head = stream;
        head.flags = COVT_DESC_SPLIT | kind;
        head.avail = (int32_t)c;
        return head;
    }
    covt_stream_desc pad{};
    pad.flags = COVT_DESC_SPLIT_PAD | kind;
    if (slot == kSplitPadRange) pad.in_off = (uint64_t)ch.s, pad.out_off = (uint64_t)ch.e;
    if (fam == COVT_FAMILY_SPLIT_RLE) {
        if (slot == kSplitPadRleValues) pad.in_off = (uint64_t)ch.v0, pad.out_off = (uint64_t)ch.nv;
        if (slot == kSplitPadRleConsumed) pad.in_off = (uint64_t)rle_consumed;
    }
    return pad;
}

// The readers (group: the chunk's head)
COVT_SPLIT_HD inline bool split_is_pad(const covt_stream_desc& d) { return (d.flags & COVT_DESC_SPLIT_PAD) != 0; }
COVT_SPLIT_HD inline int32_t split_chunk_index(const covt_stream_desc& head) { return head.avail; }
// the chunk's range, from its range pad group[kSplitPadRange]
COVT_SPLIT_HD inline SplitChunk split_range(const covt_stream_desc& range_pad) {
    return SplitChunk{(int32_t)range_pad.in_off, (int32_t)range_pad.out_off, 0, 0};
}
COVT_SPLIT_HD inline SplitChunk split_rle_chunk(const covt_stream_desc* group) {
    return SplitChunk{(int32_t)group[kSplitPadRange].in_off, (int32_t)group[kSplitPadRange].out_off,
                      (int32_t)group[kSplitPadRleValues].in_off, (int32_t)group[kSplitPadRleValues].out_off};
}
COVT_SPLIT_HD inline uint32_t split_rle_consumed(const covt_stream_desc* group) {
    return (uint32_t)group[kSplitPadRleConsumed].in_off;
}

// ---- The rules ---------------------------------------------------------------------------------------
// A stream's cost: its bytes + output bytes / 4 (the launch-order key and the split threshold's measure;
// FastPFOR and RLE time follows the values as much as the bytes)
COVT_SPLIT_HD inline int64_t stream_cost(int64_t byte_length, int64_t out_elems, int64_t elem_bytes) {
    return byte_length + out_elems * elem_bytes / 4;
}
COVT_SPLIT_HD inline int64_t stream_cost(const covt_stream_info& s) {
    return stream_cost(s.byte_length, s.out_elems, s.elem_bytes);
}

// Plan rule for split streams: the Java-capped int32 varint ops (value ends are local: every byte
// with bit 7 clear ends a value, DecodingUtils.java:157-186), longer than split_min bytes.
COVT_SPLIT_HD inline bool split_op(int op) {
    return op == COVT_OP_VARINT_I32 || op == COVT_OP_VARINT_ZZ_I32 || op == COVT_OP_VARINT_ZZ_DELTA_I32 ||
           op == COVT_OP_VARINT_ZZ_DELTA_XY || op == COVT_OP_VARINT_DELTA_MORTON || op == COVT_OP_VARINT_I32_AS_I64 ||
           op == COVT_OP_VARINT_ZZ_I32_AS_I64 || op == COVT_OP_VARINT_ZZ_DELTA_I64 || op == COVT_OP_VARINT_U64 ||
           op == COVT_OP_VARINT_ZZ_S64;
}
// FastPFOR ops whose long streams split into value chunks.  The chunk kernel (covt_decode.hip
// run_fastpfor_chunk) adds a chunk's carry in place for the linear int32 ops (ZZ_DELTA_I32, ZZ_DELTA_XY) and
// decodes Morton twice; an op added here needs a carry rule there (static_asserts guard it).
COVT_SPLIT_HD inline bool split_fpf_op(int op) {
    return op == COVT_OP_FPF_ZZ_DELTA_I32 || op == COVT_OP_FPF_ZZ_DELTA_XY || op == COVT_OP_FPF_DELTA_MORTON;
}
COVT_SPLIT_HD inline bool split_rle_op(int op) {
    return op == COVT_OP_RLE_U64 || op == COVT_OP_RLE_I32 || op == COVT_OP_RLE_S64 || op == COVT_OP_BYTE_RLE_U8 ||
           op == COVT_OP_BYTE_RLE_RAW;
}
// The cost the split threshold sees: a FastPFOR wave's time follows the blocks, i.e. the values, so their
// output counts fpf_w times (covt_plan_options.fpf_split_weight)
COVT_SPLIT_HD inline int64_t split_cost(int op, int64_t byte_length, int64_t out_elems, int64_t elem_bytes, int64_t fpf_w) {
    const int64_t c = stream_cost(byte_length, out_elems, elem_bytes);
    return split_fpf_op(op) ? c + (fpf_w - 1) * (out_elems * elem_bytes / 4) : c;
}
// FastPFOR streams split by values into chunks of whole blocks (their own headers and page directories
// locate every block), at least two chunks
// cost: the stream's split_cost
COVT_SPLIT_HD inline bool split_stream(int op, int32_t num_values, int64_t cost, int64_t split_min, int64_t split_values) {
    if (split_min < 0 || num_values <= 0 || cost <= split_min) return false;
    if (split_fpf_op(op)) return num_values > split_values && !(op == COVT_OP_FPF_ZZ_DELTA_XY && (num_values & 1));
    return split_op(op) && !(op == COVT_OP_VARINT_ZZ_DELTA_XY && (num_values & 1));
}
// ORC RLE streams split where the planner's walk of their groups frames them in two chunks or more: the
// streams worth that walk
COVT_SPLIT_HD inline bool split_rle_candidate(int op, int32_t num_values, int64_t cost, int64_t split_min) {
    return split_min >= 0 && split_rle_op(op) && cost > split_min && num_values > 0;
}

// The batch's split parameters (options and totals resolved): threshold, chunk units, FastPFOR weight
struct SplitRule {
    int64_t split_min, chunk_bytes, chunk_values, fpf_w;
};
// A stream's family and descriptor count before the RLE walk (which turns a candidate it frames into
// COVT_FAMILY_SPLIT_RLE, COVT_SPLIT_SLOTS descriptors per chunk).  num_values: the values to decode (a plan
// under construction keeps them beside the entry); fam: the stream's family when not split
struct SplitChoice {
    int32_t fam;
    int64_t ndesc;
};
COVT_SPLIT_HD inline SplitChoice split_choice(const covt_stream_info& s, int32_t num_values, int fam, const SplitRule& r) {
    const int64_t sc = split_cost(s.op, s.byte_length, s.out_elems, s.elem_bytes, r.fpf_w);
    if (!split_stream(s.op, num_values, sc, r.split_min, r.chunk_values)) return SplitChoice{fam, 1};
    const bool fpf = split_fpf_op(s.op);
    const int64_t nch = fpf ? split_unit_chunks(r.chunk_values, num_values) : split_unit_chunks(r.chunk_bytes, s.byte_length);
    return SplitChoice{fpf ? COVT_FAMILY_SPLIT_FPF : COVT_FAMILY_SPLIT, nch * COVT_SPLIT_SLOTS};
}

// covt_plan_options.split_grow: chunks (split_chunk bytes, split_values values) doubled for plans of >= 4 MiB of
// cost and quadrupled from 48 MiB.  In a plan whose streams fill the chip a chunk wave shares its SIMD with
// the crowd, and its fixed costs (start state, look-back) weigh more than a longer body
// (profiles/r05/shard_sizes.txt: 2 KiB chunks best for one tile, 4 KiB for 8-30 MiB plans, 8 KiB above)
COVT_SPLIT_HD inline int64_t split_grow_factor(int64_t total_cost, int32_t grow) {
    if (!grow) return 1;
    return total_cost >= (48ll << 20) ? 4 : total_cost >= (4ll << 20) ? 2 : 1;
}

// ---- The FastPFOR framing (JavaFastPFOR FastPFOR.decodePage, read exactly as run_fastpfor's pre-walk does) ----
// Both planners walk a split stream's page directories and block headers for the chunks' start states and
// must agree byte for byte with each other and with the kernels.  The page grammar is stated once, here:
// fpf_page_container and fpf_directory are the functions the two FastPFOR decoders of covt_decode.hip parse
// a page with (their word reader: the LDS windows; their array callback: lane k's start and size), and
// fpf_page_dir is the same two with no callback.  The planners keep their own loops and cursor storage over
// fpf_page_dir and fpf_block_step, templates over a reader R of the stream's nw = byte_length / 4 words:
//   uint32_t R::word(int64_t i)     big-endian word i
//   uint64_t R::bytes8(int64_t i)   stream bytes [4 i, 4 i + 8), byte m in bits [8 m, 8 m + 8)
// Nothing here reads a word outside [0, nw) (tests/split_plan feeds it every prefix of random words).
constexpr int kFpfBlock = 256;
constexpr int kFpfPage = 65536;
constexpr int kFpfBcCap = 3 * kFpfPage / kFpfBlock + kFpfPage;  // JavaFastPFOR byteContainer size

// the values held in pages (whole blocks) of a stream of n values; 0: none, or a stream (or chunk unit)
// the walk does not follow
template <class R>
COVT_SPLIT_HD inline int32_t fpf_paged_values(R& rd, int64_t nw, int32_t n, int64_t unit) {
    if (nw <= 0 || unit % kFpfBlock) return 0;
    int32_t L = (int32_t)rd.word(0);
    if (L < 0) return 0;
    L -= L % kFpfBlock;
    return L > n ? 0 : L;
}

// One page's directory: the byte container (block headers and exception bytes), where its packed words
// start and where the next page does
struct FpfPage {
    int64_t bc;     // the container's first word
    int32_t bclen;  // its bytes (whole words)
    int64_t pk;     // the first block's packed word
    int64_t next;   // the word after the page's exception arrays
};
// The byte container of the page whose bytesize word reads `bytesize` and is followed by word `at`.
// Returns COVT_OK, COVT_ERR_BAD_HEADER (a size outside [0, kFpfBcCap]) or COVT_ERR_TRUNCATED (the container
// and the bitmap word after it do not fit the stream).
struct FpfContainer {
    int64_t bc;     // the container's first word
    int32_t bclen;  // its bytes (whole words); the directory's bitmap word: bc + bclen / 4
};
COVT_SPLIT_HD inline int32_t fpf_page_container(int32_t bytesize, int64_t at, int64_t nw, FpfContainer& ct) {
    if (bytesize < 0 || bytesize > kFpfBcCap) return COVT_ERR_BAD_HEADER;
    const int64_t bcw = (bytesize + 3) / 4;
    if (at + bcw >= nw) return COVT_ERR_TRUNCATED;
    ct.bc = at;
    ct.bclen = (int32_t)(bcw * 4);
    return COVT_OK;
}
// The exception-array directory from its bitmap word ie (< nw) on: bit k - 1 set: dataTobePacked[k] present
// (k >= 2), as its size word and then its values, 32 of them packed into k words.  word(i): big-endian word
// i < nw; array(k, start, size): array k's first word and its values.  ie: left after the last array (it may
// lie far past nw).  Returns COVT_OK, COVT_ERR_TRUNCATED (a size word at or past nw) or COVT_ERR_BAD_HEADER
// (a negative size).
template <class Word, class Array>
COVT_SPLIT_HD inline int32_t fpf_directory(Word&& word, int64_t nw, int64_t& ie, Array&& array) {
    uint32_t bm = word(ie++) & ~1u;
    while (bm) {
        const int32_t k = __builtin_ctz(bm) + 1;
        bm &= bm - 1;
        if (ie >= nw) return COVT_ERR_TRUNCATED;
        const int32_t size = (int32_t)word(ie++);
        if (size < 0) return COVT_ERR_BAD_HEADER;
        const int64_t groups = ((int64_t)size + 31) / 32;
        array(k, ie, size);
        ie += groups * k - ((groups * 32 - size) * k) / 32;
    }
    return COVT_OK;
}
// the page whose whereMeta word is p0; false: the framing cannot be followed
template <class R>
COVT_SPLIT_HD inline bool fpf_page_dir(R& rd, int64_t nw, int64_t p0, FpfPage& pg) {
    if (p0 >= nw) return false;
    int64_t ie = p0 + (int32_t)rd.word(p0);
    if (ie < 0 || ie >= nw) return false;
    FpfContainer ct;
    if (fpf_page_container((int32_t)rd.word(ie), ie + 1, nw, ct) != COVT_OK) return false;
    ie = ct.bc + ct.bclen / 4;
    if (fpf_directory([&](int64_t i) { return rd.word(i); }, nw, ie, [](int32_t, int64_t, int32_t) {}) != COVT_OK) return false;
    pg.bc = ct.bc;
    pg.bclen = ct.bclen;
    pg.pk = p0 + 1;
    pg.next = ie;
    return true;
}

// One block header at container offset cur: advances cur to the next header and pk past the block's
// packed words; the block adds cnt exceptions to array arr (arr = cnt = 0: none the walk tracks).
// false: the framing cannot be followed.  Container byte q is stream byte 4 bc + (q ^ 3); bytes cur,
// cur + 1, cur + 2 come from one read of the two words holding them (both inside the stream: the
// container is followed by the bitmap word).
template <class R>
COVT_SPLIT_HD inline bool fpf_block_step(R& rd, const FpfPage& pg, int32_t& cur, int64_t& pk, int32_t& arr, int32_t& cnt) {
    if (cur + 3 > pg.bclen + 1) return false;  // (the device reads the header word through its window)
    const int32_t w = cur >> 2;
    const uint64_t x = rd.bytes8(pg.bc + w);
    auto cb = [&](int32_t q) -> uint32_t { return (uint32_t)(x >> (8 * (4 * ((q >> 2) - w) + ((q & 3) ^ 3)))) & 0xffu; };
    const int32_t hb = (int32_t)(int8_t)cb(cur), ce = (int32_t)cb(cur + 1);
    const int32_t idx = ce > 0 && cur + 2 < pg.bclen ? (int32_t)(int8_t)cb(cur + 2) - hb : 0;
    const bool tracked = ce > 0 && idx >= 2 && idx <= 32;
    arr = tracked ? idx : 0;
    cnt = tracked ? ce : 0;
    pk += 8 * hb;
    cur += ce > 0 ? 3 + ce : 2;
    return cur <= pg.bclen;
}

#endif

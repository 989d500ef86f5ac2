// split_plan_check.cc -- TEST INFRASTRUCTURE: the split-chunk contract of cov-tiles_amd/csrc/covt_split_plan.h
// run on the CPU in a stand-alone program, built by tests/test_split_plan.py with -fsanitize=address,undefined.
//   round trip  the writer's eight slots of a chunk group against the layout as include/covt.h documents it
//               (stated here by position, independently of the header's names), and the readers on them
//   bounds      the shared FastPFOR page-directory parse and block-header step over every prefix of random
//               and of framed streams, through a reader that aborts on a word outside [0, nw)
// Prints "ok <groups checked> <walks> <block steps>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "covt_split_plan.h"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
            return 1;                                                 \
        }                                                             \
    } while (0)

static std::mt19937_64 rng(0x5eed5eedull);
static int64_t rnd(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }

static bool same(const covt_stream_desc& a, const covt_stream_desc& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// one group of each kind per call
static int round_trip(int fam, uint16_t kind) {
    covt_stream_desc base;
    base.in_off = rng();
    base.out_off = rng() & ~127ull;
    base.avail = base.byte_length = (int32_t)rnd(1, INT32_MAX);
    base.num_values = (int32_t)rnd(1, INT32_MAX);
    base.op = (uint8_t)rnd(0, 255);
    base.num_bits = (uint8_t)rnd(0, 255);
    base.flags = (uint16_t)(rnd(0, 1) ? COVT_DESC_LANE : 0);
    const bool rle = fam == COVT_FAMILY_SPLIT_RLE, fpf = fam == COVT_FAMILY_SPLIT_FPF;
    SplitChunk ch;
    int64_t c;
    const int32_t consumed = (int32_t)rnd(0, INT32_MAX);
    if (rle) {
        c = rnd(0, 1 << 20);
        ch.s = (int32_t)rnd(0, INT32_MAX);
        ch.e = (int32_t)rnd(ch.s, INT32_MAX);
        ch.v0 = (int32_t)rnd(0, INT32_MAX);
        ch.nv = (int32_t)rnd(0, INT32_MAX - ch.v0);
    } else {
        const int64_t total = fpf ? base.num_values : base.byte_length, unit = rnd(64, 1 << 16);
        const int64_t nch = split_unit_chunks(unit, total);
        REQUIRE(nch >= 1 && (nch - 1) * unit < total && nch * unit >= total);
        c = rnd(0, 3) ? rnd(0, nch - 1) : nch - 1;
        ch = split_unit_chunk(c, unit, total);
        REQUIRE(ch.s == c * unit && ch.e > ch.s && ch.e <= total && (ch.e == ch.s + unit || (c == nch - 1 && ch.e == total)));
        REQUIRE(ch.v0 == 0 && ch.nv == 0);
    }
    // exactly COVT_SPLIT_SLOTS descriptors on the heap: an accessor that strays is AddressSanitizer's
    std::vector<covt_stream_desc> g(COVT_SPLIT_SLOTS);
    for (int q = 0; q < COVT_SPLIT_SLOTS; ++q) g[(size_t)q] = split_slot_desc(base, fam, c, q, ch, consumed);

    covt_stream_desc head = base;  // the stream's descriptor but for the chunk index and the flags
    head.avail = (int32_t)c;
    head.flags = (uint16_t)(COVT_DESC_SPLIT | kind);
    REQUIRE(same(g[0], head));
    for (int q = 1; q < 8; ++q) {  // pads: the flags, the documented fields, zero elsewhere
        covt_stream_desc pad;
        std::memset(&pad, 0, sizeof pad);
        pad.flags = (uint16_t)(COVT_DESC_SPLIT_PAD | kind);
        if (q == 1) pad.in_off = (uint64_t)ch.s, pad.out_off = (uint64_t)ch.e;
        if (rle && q == 2) pad.in_off = (uint64_t)ch.v0, pad.out_off = (uint64_t)ch.nv;
        if (rle && q == 3) pad.in_off = (uint64_t)consumed;
        REQUIRE(same(g[(size_t)q], pad));
    }
    // the readers
    REQUIRE(!split_is_pad(g[0]) && split_chunk_index(g[0]) == c);
    for (int q = 1; q < 8; ++q) REQUIRE(split_is_pad(g[(size_t)q]));
    const SplitChunk rg = split_range(g[1]);
    REQUIRE(rg.s == ch.s && rg.e == ch.e);
    if (rle) {
        const SplitChunk r = split_rle_chunk(g.data());
        REQUIRE(r.s == ch.s && r.e == ch.e && r.v0 == ch.v0 && r.nv == ch.nv);
        REQUIRE(split_rle_consumed(g.data()) == (uint32_t)consumed);
    }
    if (fpf) {  // 42 state slots: distinct aligned words of pads 2..7, clear of op / num_bits / flags and of pad 1
        std::set<size_t> seen;
        int32_t val[42];
        for (int m = 0; m < 42; ++m) {
            const size_t off = (size_t)((uint8_t*)fpf_state_slot(g.data(), m) - (uint8_t*)g.data());
            REQUIRE(off % 4 == 0 && off >= 2 * sizeof(covt_stream_desc) && off + 4 <= 8 * sizeof(covt_stream_desc));
            REQUIRE(off / sizeof(covt_stream_desc) == (size_t)(2 + m / 7));
            REQUIRE(seen.insert(off).second);
            REQUIRE((const uint8_t*)fpf_state_slot((const covt_stream_desc*)g.data(), m) == (uint8_t*)g.data() + off);
            val[m] = (int32_t)rng();
            std::memcpy(fpf_state_slot(g.data(), m), &val[m], 4);
        }
        REQUIRE(kFpfStateSlots == 42 && seen.size() == 42);
        for (int m = 0; m < 42; ++m) {
            int32_t v;
            std::memcpy(&v, fpf_state_slot((const covt_stream_desc*)g.data(), m), 4);
            REQUIRE(v == val[m]);
        }
        REQUIRE(same(g[0], head) && split_range(g[1]).s == ch.s && split_range(g[1]).e == ch.e);
        for (int q = 2; q < 8; ++q)
            REQUIRE(g[(size_t)q].flags == (COVT_DESC_SPLIT_PAD | kind) && g[(size_t)q].op == 0 && g[(size_t)q].num_bits == 0);
    }
    return 0;
}

// the framing's reader over nw words; a read outside them ends the program
struct CheckedWords {
    const uint32_t* w;
    int64_t nw;
    uint32_t word(int64_t i) const {
        if (i < 0 || i >= nw) {
            std::fprintf(stderr, "word %lld outside [0, %lld)\n", (long long)i, (long long)nw);
            std::abort();
        }
        return w[i];
    }
    uint64_t bytes8(int64_t i) const {
        return (uint64_t)__builtin_bswap32(word(i)) | ((uint64_t)__builtin_bswap32(word(i + 1)) << 32);
    }
};

// the planners' walk (fpf_chunk_states, fpf_states_walk) without the state records; the block steps taken
static int64_t walk(const CheckedWords& rd, int32_t n, int64_t unit) {
    int64_t steps = 0, p = 1;
    const int32_t L = fpf_paged_values(rd, rd.nw, n, unit);
    int32_t done = 0;
    FpfPage pg;
    while (done < L && fpf_page_dir(rd, rd.nw, p, pg)) {
        const int32_t thissize = L - done < kFpfPage ? L - done : kFpfPage, nblk = thissize / kFpfBlock;
        int32_t cur = 0, arr = -1, cnt = -1;
        int64_t pk = pg.pk;
        if (pg.bc <= 0 || pg.bc + pg.bclen / 4 >= rd.nw || pg.bclen % 4) std::abort();
        for (int32_t j = 0; j < nblk; ++j) {
            if (!fpf_block_step(rd, pg, cur, pk, arr, cnt)) return steps;
            if (arr < 0 || arr > 32 || arr == 1 || cnt < 0 || cnt > 255 || (arr == 0) != (cnt == 0)) std::abort();
            ++steps;
        }
        done += thissize;
        p = pg.next;
    }
    return steps;
}

// a stream of n words: random, or pages framed as FastPFOR writes them (directory offsets, container of
// small header bytes, bitmap, array sizes) with random words between
static std::vector<uint32_t> make_stream(size_t n, bool framed) {
    std::vector<uint32_t> w(n);
    for (auto& x : w) x = (uint32_t)rng();
    if (!framed) return w;
    const int64_t pages = rnd(1, 3);
    w[0] = (uint32_t)((pages - 1) * 65536 + 256 * rnd(1, 256) + rnd(0, 255));
    size_t p = 1;
    for (int64_t pg = 0; pg < pages && p < n; ++pg) {
        const size_t meta = (size_t)rnd(1, 24), ie = p + meta;
        w[p] = (uint32_t)meta;
        if (ie >= n) break;
        const size_t bytesize = (size_t)rnd(0, 1000), bcw = (bytesize + 3) / 4;
        w[ie] = (uint32_t)bytesize;
        for (size_t k = ie + 1; k < n && k <= ie + bcw; ++k) {  // header bytes: b, exceptions, max bits
            uint32_t x = 0;
            for (int b = 0; b < 4; ++b) x = (x << 8) | (uint32_t)(rnd(0, 9) < 7 ? 0 : rnd(0, 5) ? rnd(1, 3) : rnd(0, 40));
            w[k] = x;
        }
        size_t q = ie + 1 + bcw;
        if (q >= n) break;
        const uint32_t bm = (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng();
        w[q++] = bm;
        for (int k = 1; k <= 32 && q < n; ++k) {
            if (!((bm & ~1u) >> (k - 1) & 1u)) continue;
            const int64_t size = rnd(0, 40), groups = (size + 31) / 32;
            w[q++] = (uint32_t)size;
            q += (size_t)(groups * k - ((groups * 32 - size) * k) / 32);
        }
        p = q;
    }
    return w;
}

int main() {
    long groups = 0;
    for (int it = 0; it < 20000; ++it) {
        if (round_trip(COVT_FAMILY_SPLIT, 0)) return 1;
        if (round_trip(COVT_FAMILY_SPLIT_FPF, COVT_DESC_SPLIT_FPF)) return 1;
        if (round_trip(COVT_FAMILY_SPLIT_RLE, COVT_DESC_SPLIT_RLE)) return 1;
        groups += 3;
    }
    long walks = 0;
    int64_t steps = 0, deepest = 0;
    for (int it = 0; it < 120; ++it) {
        const std::vector<uint32_t> full = make_stream(640, it % 4 != 0);
        for (size_t nw = 0; nw <= full.size(); ++nw) {
            // the prefix in a buffer of its own size: a stray read is AddressSanitizer's as well as the reader's
            const std::vector<uint32_t> w(full.begin(), full.begin() + (long)nw);
            const CheckedWords rd{w.data(), (int64_t)nw};
            const int64_t s = walk(rd, INT32_MAX, 256 << (it % 3));
            steps += s;
            deepest = s > deepest ? s : deepest;
            ++walks;
        }
    }
    REQUIRE(walk(CheckedWords{nullptr, 0}, INT32_MAX, 2048) == 0);
    // the framed streams reach the block steps and a second page, or the sweep proves little
    REQUIRE(steps > 100000 && deepest > 256);
    std::printf("ok %ld %ld %lld\n", groups, walks, (long long)steps);
    return 0;
}

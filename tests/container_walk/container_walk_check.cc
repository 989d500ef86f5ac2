// container_walk_check.cc -- the container grammars of cov-tiles_amd/csrc/covt_container.h (the ones the
// host plan and the device plan's serial walkers instantiate) compiled by g++ alone and run over tiles
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_container_walk.py).
//
// Input (argv[1]): per tile an int32 format (0 Gen C, 1 Gen D), an int64 size and the bytes.  Every tile is
// served from a heap copy of exactly its size; peek8 aborts on an offset outside [0, size) and returns poison
// for the bytes past the end.  Each tile is walked with 32-bit and with 64-bit cursors, each with two poison
// patterns, by a visitor taking stream and property records in one pass; and with the first pair again by a
// streams-only and a properties-only visitor (the compiled-away branches), and with a table that reads a
// geometry column's metadata again instead of keeping it (the device plan's lane layout).  All of them must agree, or the
// program aborts.  Output: per tile "t index status streams props layers", then its records:
//   l extent n_features
//   s layer kind type encoding column_type num_values byte_length num_bits offset
//   p layer column type ctype nf lang name_len lang_len name_off lang_off s_off[4] s_nv[4] s_bl[4] s_enc[4]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "covt_container.h"

template <class OffT>
struct PoisonWindow {
    using Off = OffT;
    const uint8_t* t;  // a heap block of exactly len bytes
    int64_t len;
    uint8_t poison;
    uint64_t peek8(Off i) {
        if (i < 0 || (int64_t)i >= len) {
            std::fprintf(stderr, "peek8(%lld) outside a tile of %lld bytes\n", (long long)i, (long long)len);
            std::abort();
        }
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) {
            const int64_t j = (int64_t)i + k;
            v |= (uint64_t)(j < len ? t[j] : (uint8_t)(poison + 29 * k)) << (8 * k);
        }
        return v;
    }
};

struct Layer {
    int32_t extent, nfeat;
};
template <bool kS, bool kP>
struct Collect {
    static constexpr bool kStreams = kS, kProps = kP;
    std::vector<RawStream> ss;
    std::vector<PropRaw> ps;
    std::vector<Layer> ls;
    size_t s0 = 0, p0 = 0;
    void layer_begin(int32_t extent, int32_t nfeat) {
        ls.push_back(Layer{extent, nfeat});
        s0 = ss.size();
        p0 = ps.size();
    }
    void operator()(const RawStream& s) { ss.push_back(s); }
    void operator()(const PropRaw& p) { ps.push_back(p); }
    void layer_end(int64_t data_start) {
        for (size_t i = s0; i < ss.size(); ++i) ss[i].off += data_start;
        for (size_t i = p0; i < ps.size(); ++i)
            for (int r = 0; r < 4; ++r)
                if (ps[i].s_off[r] >= 0) ps[i].s_off[r] += data_start;
    }
};

// the plain-array table, but with the geometry streams read again from the metadata (the lane layout's table)
template <class Off>
struct RereadTab : ArrayTab {
    static constexpr bool kKeepsGeo = false;
    GeoReread<Off> again;
    void geo_set(uint32_t, const GeoSm&) {}
    void geo_rewind(Off s0) { again.geo_rewind(s0); }
    template <class R>
    GeoSm geo_get(R& r, uint32_t s) { return again.geo_get(r, s); }
};

template <class Off, bool kReread = false, bool kS, bool kP>
int walk(const uint8_t* t, int64_t len, int fmt, uint8_t poison, Collect<kS, kP>& c) {
    ContainerRd<PoisonWindow<Off>> r;
    r.t = t;
    r.len = len;
    r.poison = poison;
    if (fmt != 0) return walk_gend(r, c);
    typename std::conditional<kReread, RereadTab<Off>, ArrayTab>::type tab;
    std::memset((void*)&tab, 0xa5, sizeof tab);
    return walk_genc(r, c, tab);
}

static bool same_stream(const RawStream& a, const RawStream& b) {
    return a.layer == b.layer && a.kind == b.kind && a.type == b.type && a.enc == b.enc && a.ctype == b.ctype &&
           a.nv == b.nv && a.bl == b.bl && a.nb == b.nb && a.off == b.off;
}
static bool same_prop(const PropRaw& a, const PropRaw& b) {
    bool ok = a.layer == b.layer && a.column == b.column && a.type == b.type && a.ctype == b.ctype && a.nf == b.nf &&
              a.lang == b.lang && a.name_len == b.name_len && a.lang_len == b.lang_len && a.name_off == b.name_off &&
              a.lang_off == b.lang_off;
    for (int r = 0; r < 4; ++r)
        ok = ok && a.s_off[r] == b.s_off[r] && a.s_nv[r] == b.s_nv[r] && a.s_bl[r] == b.s_bl[r] && a.s_enc[r] == b.s_enc[r];
    return ok;
}
template <class A, class B>
void must_agree(int64_t tile, const char* what, int sa, const A& a, int sb, const B& b) {
    bool ok = sa == sb;
    if (ok && sa == 0) {
        if (A::kStreams && B::kStreams) {
            ok = ok && a.ss.size() == b.ss.size();
            for (size_t i = 0; ok && i < a.ss.size(); ++i) ok = same_stream(a.ss[i], b.ss[i]);
        }
        if (A::kProps && B::kProps) {
            ok = ok && a.ps.size() == b.ps.size();
            for (size_t i = 0; ok && i < a.ps.size(); ++i) ok = same_prop(a.ps[i], b.ps[i]);
        }
        ok = ok && a.ls.size() == b.ls.size();
        for (size_t i = 0; ok && i < a.ls.size(); ++i) ok = a.ls[i].extent == b.ls[i].extent && a.ls[i].nfeat == b.ls[i].nfeat;
    }
    if (!ok) {
        std::fprintf(stderr, "tile %lld: %s disagree (status %d vs %d)\n", (long long)tile, what, sa, sb);
        std::abort();
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t fmt;
    int64_t len, tile = 0, n_streams = 0, n_props = 0;
    while (std::fread(&fmt, sizeof fmt, 1, f) == 1) {
        if (std::fread(&len, sizeof len, 1, f) != 1 || len < 0) return 2;
        uint8_t* t = (uint8_t*)std::malloc((size_t)len);  // exactly the tile: one byte more is an ASan report
        if (len && (!t || std::fread(t, 1, (size_t)len, f) != (size_t)len)) return 2;
        Collect<true, true> a, b, c, d;
        const int sa = walk<int32_t>(t, len, fmt, 0x00, a), sb = walk<int32_t>(t, len, fmt, 0xff, b);
        const int sc = walk<int64_t>(t, len, fmt, 0x80, c), sd = walk<int64_t>(t, len, fmt, 0x7f, d);
        must_agree(tile, "poison patterns", sa, a, sb, b);
        must_agree(tile, "cursor widths", sa, a, sc, c);
        must_agree(tile, "poison patterns (64-bit cursors)", sc, c, sd, d);
        Collect<true, false> so;
        Collect<false, true> po;
        const int sso = walk<int32_t>(t, len, fmt, 0x00, so), spo = walk<int32_t>(t, len, fmt, 0xff, po);
        must_agree(tile, "the streams-only visitor", sa, a, sso, so);
        must_agree(tile, "the properties-only visitor", sa, a, spo, po);
        Collect<true, true> e;
        const int se = walk<int32_t, true>(t, len, fmt, 0xff, e);
        must_agree(tile, "the re-reading geometry table", sa, a, se, e);
        if (!so.ps.empty() || !po.ss.empty()) std::abort();
        std::free(t);
        if (sa) a = Collect<true, true>();  // a failed tile contributes nothing
        std::printf("t %lld %d %zu %zu %zu\n", (long long)tile, sa, a.ss.size(), a.ps.size(), a.ls.size());
        for (const Layer& l : a.ls) std::printf("l %d %d\n", l.extent, l.nfeat);
        for (const RawStream& s : a.ss)
            std::printf("s %d %d %d %d %d %d %d %d %lld\n", s.layer, s.kind, s.type, s.enc, s.ctype, s.nv, s.bl, s.nb,
                        (long long)s.off);
        for (const PropRaw& p : a.ps) {
            std::printf("p %d %d %d %d %d %d %d %d %lld %lld", p.layer, p.column, p.type, p.ctype, p.nf, p.lang, p.name_len,
                        p.lang_len, (long long)p.name_off, (long long)p.lang_off);
            for (int r = 0; r < 4; ++r) std::printf(" %lld", (long long)p.s_off[r]);
            for (int r = 0; r < 4; ++r) std::printf(" %d", p.s_nv[r]);
            for (int r = 0; r < 4; ++r) std::printf(" %d", p.s_bl[r]);
            for (int r = 0; r < 4; ++r) std::printf(" %d", p.s_enc[r]);
            std::printf("\n");
        }
        n_streams += (int64_t)a.ss.size();
        n_props += (int64_t)a.ps.size();
        ++tile;
    }
    std::fclose(f);
    std::printf("ok %lld %lld %lld\n", (long long)tile, (long long)n_streams, (long long)n_props);
    return 0;
}
